// scripted_loop.h -- one call of a scripted closed-loop entry (mpc_closed_loop_traffic, _convoy, _noisy, _traced,
// _warm) as the request both backends take: the entry fills by name the fields it has and leaves the others at
// their defaults (no script, no worlds, no noise, no trace, no warm start, no optional output); mpcqp.hip's
// scripted_loop() hands it to the kernels, Backend::closed_loop_scripted (cpu_backend.h) runs it on the host.  What
// follows from the fields is stated once, below them.  Plain C++17: tools/*_host_check.cpp fill one too.
#pragma once
#include "../../include/mpcqp.h"
#include <math.h>

struct ScriptedLoop {
    const char* label = "scripted-loop";    // names the entry in the messages of device and allocation failures
    int B = 0;
    const double* x_init = nullptr;         // [B][5]
    int max_steps = 0;
    double s_stop = 0.0;
    // the scripts [n_scripts][A]; with_slab: the solver runs with max_obs = A + K
    const mpc_actor* actors = nullptr;
    int A = 0, n_scripts = 0;
    bool with_slab = false;
    // worlds: the egos [w*W, (w+1)*W) see each other, up to K leaders closer than lead_range per ego.  Off: the
    // traffic entry (W = 1, K = 0; the device launches no cv_* kernel and keeps A-wide slab histories)
    bool worlds = false;
    int W = 1, K = 0;
    double lead_range = INFINITY;
    // noisy: the measure / plant steps draw with (seed, ego_offset + b); noise [n_noise] (1 or B), NULL: all zero
    bool noisy = false;
    const mpc_noise* noise = nullptr;
    int n_noise = 0;
    unsigned long long seed = 0;
    long long ego_offset = 0;
    // outputs; quant is required, histories are [n_hist] rows for the egos hist_egos names
    double *quant = nullptr, *extra = nullptr;
    int n_hist = 0;
    const int* hist_egos = nullptr;
    double *hist_x = nullptr, *hist_u = nullptr, *hist_ua = nullptr, *hist_xm = nullptr, *hist_car_s = nullptr;
    int *hist_tl = nullptr, *hist_status = nullptr, *hist_nobs = nullptr;
    double* hist_slab = nullptr;
    int* hist_lead = nullptr;
    int* n_steps = nullptr;
    double* step_ms = nullptr;
    // traces: gapq [B][n_look][MPC_TG_NQ] for the stages lookahead [n_look], the solver's Xpred / U of every step
    const int* lookahead = nullptr;
    int n_look = 0;
    double *gapq = nullptr, *hist_pred = nullptr, *hist_plan = nullptr;
    // warm: set when the solver is to be handed a ubar (a carried plan, or the reference one for a warm output)
    const mpc_warm* warm = nullptr;
    double *warmq = nullptr, *hist_ubar = nullptr;

    // ---- what follows from the fields ----
    bool per_ego() const { return n_scripts == B && B > 1; }         // n_scripts == B == 1 is the shared case
    int nsc() const { return per_ego() ? B : (actors ? 1 : 0); }     // the scripts there are to read
    const mpc_actor* script(int b) const { return actors + (per_ego() ? (size_t)b * (size_t)A : 0); }
    bool nz_per_ego() const { return noisy && n_noise == B && B > 1; }
    const mpc_noise& noise_of(int b) const { return noise ? noise[nz_per_ego() ? b : 0] : quiet; }
    bool traced() const { return n_look > 0 || hist_pred || hist_plan; }
    int nx() const { return noisy ? MPC_NZ_NX : (worlds ? MPC_CV_NX : MPC_TR_NX); }    // the width of extra
    mpc_noise quiet = {};                   // noise == NULL: every ego draws with this all-zero struct
};
