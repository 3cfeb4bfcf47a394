// evaluator_common.h -- the phase the tracker's batched evaluators share (evaluate_kernel.h, gradient_kernel.h,
// multiplier_kernel.h, hessvec_kernel.h): how an instance is read, rolled out and linearised.  Each kernel carves its
// own LDS and keeps what only it computes; what is stated here is stated once for all of them, and for the host
// backend's twins in cpu_backend.h (evaluator_instance, linearise_one).
//
// An instance runs on a group of lanes gl = 0, 1, ... (a lane group of the solver's layout, or a whole wavefront):
// lane j = 0..N-1 owns control j and the coefficients of A_j, lane j = 1..N owns stage j.  Three steps, in this order:
//
//   evc_instance   x0, the obstacle slab and the obstacle count of instance b, as every evaluator reads them.
//   evc_rollout    the lane's roles and its control; predict_grp rolls the instance out into L.Xr / L.kap and leaves
//                  lane j <= N the reference state at s_j (with its slopes when SLOPES).  U is staged for lane 0 in
//                  a buffer of 2 N doubles the caller names: any part of its LDS that is dead until the rollout is
//                  over (lane 0 has read it before predict_grp's first barrier, so it is free on return).  The
//                  function begins with LDS writes and ends behind predict_grp's last barrier: Xr and kap are
//                  readable by every lane on return.
//   evc_linearise  control gl: its cost terms (ev_control, with CT) and A_gl (stage_A); stage gl: its cost terms and
//                  rows (ev_stage; the rows go to `rows` [N][rw] when given) and its stage gradients q_gl and c_gl
//                  (gr_stage, c weighted by the batch's `lamg` [B][N][rw]; without CS the zero c is dropped).  With CT the lane also
//                  zeroes kap[gl - 1], ev_sums' L1 partial, which only the evaluator kernel fills.  No barrier: the
//                  caller may go on with the lane's own rows (the multiplier kernel counts them).
//   evc_sweeps     a barrier, then the reverse sweeps in place: lane 0 the cost's over L.qs, lane 1 the rows' over
//                  L.cs when has_lam.  Lane 0 stores g0 = A_0' p_1 of the cost to gx0 [5] when given.  The costates
//                  are readable by the other lanes after the caller's next barrier.
//
// The LDS contract (doubles): Xr [N+1][5] and kap [N+1] for the rollout; As [N][5] and qs [N][5] for the linearisation,
// ct [N][5] with CT and cs [N][5] with CS (null otherwise: the multiplier kernel has neither).  Where they lie is the
// kernel's business: each header states its own carving.
#pragma once
#include "device_common.h"

struct EvcLds {
    double* Xr;     // the rollout
    double* kap;    // k_ref of the rollout; with ct, zero afterwards
    double* ct;     // the evaluator's cost terms, or null
    double* As;     // stage_A at x_0..x_N-1
    double* qs;     // the cost's stage gradients, then its costates p_1..p_N
    double* cs;     // the rows' weighted gradients, then their costates p'_1..p'_N, or null
};

// what a lane holds of its instance
struct EvcInst {
    double x0[5];
    const double* obs;      // the instance's obstacle slab [max_obs][2], null without OBS
    int nobs;
    bool ctrl, stage;       // this lane owns control gl and A_gl / stage gl
    double u1, u2;          // control gl
    double st[5], sl[4];    // the reference state at s_gl and its slopes
};

template <bool OBS>
__device__ __forceinline__ void evc_instance(const KParams& Pr, int b, const double* __restrict__ x0g,
                                             const double* __restrict__ obsg, const int* __restrict__ nobsg,
                                             EvcInst& I) {
#pragma unroll
    for (int j = 0; j < 5; ++j) I.x0[j] = x0g[5 * (size_t)b + j];
    // the obstacle count as the solver reads it: NULL = all max_obs rows, clamped to [0, max_obs]
    I.nobs = 0;
    I.obs = nullptr;
    if (OBS) {
        int nobs = nobsg ? nobsg[b] : Pr.max_obs;
        nobs = nobs < 0 ? 0 : (nobs > Pr.max_obs ? Pr.max_obs : nobs);
        I.nobs = nobs;
        I.obs = obsg + (size_t)b * Pr.max_obs * 2;
    }
}

template <bool SLOPES>
__device__ __forceinline__ void evc_rollout(const DevTable& tab, const KParams& Pr, int b, int gl,
                                            const double* __restrict__ Ug, double* ustage, const EvcLds& L,
                                            EvcInst& I) {
    const int N = Pr.N;
    I.ctrl = gl < N;
    I.stage = gl >= 1 && gl <= N;
    I.u1 = 0.0;
    I.u2 = 0.0;
    if (I.ctrl) {
        I.u1 = Ug[(size_t)b * 2 * N + 2 * gl];
        I.u2 = Ug[(size_t)b * 2 * N + 2 * gl + 1];
        ustage[2 * gl] = I.u1;
        ustage[2 * gl + 1] = I.u2;
    }
    wave_sync();
#pragma unroll
    for (int a = 0; a < 5; ++a) I.st[a] = 0.0;
#pragma unroll
    for (int a = 0; a < 4; ++a) I.sl[a] = 0.0;
    predict_grp(tab, N, Pr.dt, I.x0, ustage, L.Xr, L.kap, gl, I.st, SLOPES ? I.sl : nullptr);
}

template <bool CT, bool CS>
__device__ __forceinline__ void evc_linearise(const KParams& Pr, int b, int rw, int gl, const EvcLds& L,
                                              const EvcInst& I, const double* __restrict__ lamg, double* rows,
                                              EvRun& run, GrRun& gr) {
    if (I.ctrl) {
        if (CT) ev_control(Pr, I.u1, I.u2, L.ct + 5 * gl, run);
        stage_A(L.Xr + 5 * gl, Pr.dt, I.st[3], I.sl[2], L.As + 5 * gl);
    }
    if (I.stage) {
        EvStage S = ev_stage_begin();
        double ct3[3], cd[5];
        ev_stage(Pr, gl, L.Xr + 5 * gl, I.st, I.obs, I.nobs, rw, CT ? L.ct + 5 * (gl - 1) : ct3,
                 rows ? rows + (gl - 1) * rw : nullptr, S, run);
        const double* lam = lamg ? lamg + ((size_t)b * Pr.N + (gl - 1)) * rw : nullptr;
        gr_stage(Pr, gl, L.Xr + 5 * gl, I.st, I.sl, I.obs, I.nobs, lam, L.qs + 5 * (gl - 1),
                 CS ? L.cs + 5 * (gl - 1) : cd, gr);
        if (CT) L.kap[gl - 1] = 0.0;
    }
}

__device__ __forceinline__ void evc_sweeps(int N, double dt, int gl, const EvcLds& L, bool has_lam, double* gx0) {
    wave_sync();
    if (gl == 0 || (gl == 1 && has_lam)) {
        double g0[5];
        gr_sweep(N, dt, L.As, gl == 0 ? L.qs : L.cs, g0);
        if (gl == 0 && gx0) {
#pragma unroll
            for (int a = 0; a < 5; ++a) gx0[a] = g0[a];
        }
    }
}
