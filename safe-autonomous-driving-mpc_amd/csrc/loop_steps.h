// loop_steps.h -- what one ego (or one actor) does in one step of the closed loops, stated once for the kernels
// (closed_loop / sweep / traffic / convoy / noise _kernels.h) and for the host backend (cpu_backend.h).  Both sides
// keep their own storage and loops and hand single values in: references into it, or for the quantity columns an
// accessor q with `double& operator[](int col)` (a pointer to the ego's row on the host, a field-major view on the
// device).  Single rounded FP64 operations, integer arithmetic, fabs and comparisons only, and the build has
// -ffp-contract=off, so the device pass, the host pass and a plain C++ compiler produce the same bits.  A store
// happens only where a value changes: the kernels' memory traffic is what is written here.
#pragma once
#include "../../include/mpcqp.h"
#include <math.h>

#ifdef __HIPCC__
#define LOOP_STEP __host__ __device__
#define LOOP_UNROLL _Pragma("unroll")
#else
#define LOOP_STEP
#define LOOP_UNROLL
#endif

// ------------------------------------------------------------------------------------------
// running extremes
// ------------------------------------------------------------------------------------------
// m <- min / max(m, a) with numpy's NaN rule: a NaN a enters the extreme, and a NaN m fails both tests for every
// later a, so it stays.  True if a replaced m
LOOP_STEP inline bool keep_min(double& m, double a) {
    if (!(a < m || a != a)) return false;
    m = a;
    return true;
}
LOOP_STEP inline bool keep_max(double& m, double a) {
    if (!(a > m || a != a)) return false;
    m = a;
    return true;
}

// the running minimum m of a gap that may not have been seen yet (bit 0 of flags: it has): the first gap seeds
// it, the later ones enter by keep_min.  True if g replaced m
LOOP_STEP inline bool min_gap(double& m, int& flags, double g) {
    if (flags & 1) return keep_min(m, g);
    flags |= 1;
    m = g;
    return true;
}

// the extremes of a control pair in the columns c0 .. c0 + 3 (u1 min, u1 max, u2 min, u2 max): step 0, which every
// ego that runs at all runs, seeds them
template <typename Q>
LOOP_STEP inline void extremes4(Q q, int c0, int step, double u1, double u2) {
    if (step == 0) {
        q[c0] = u1;
        q[c0 + 1] = u1;
        q[c0 + 2] = u2;
        q[c0 + 3] = u2;
        return;
    }
    double m[4] = {q[c0], q[c0 + 1], q[c0 + 2], q[c0 + 3]};
    if (keep_min(m[0], u1)) q[c0] = u1;
    if (keep_max(m[1], u1)) q[c0 + 1] = u1;
    if (keep_min(m[2], u2)) q[c0 + 2] = u2;
    if (keep_max(m[3], u2)) q[c0 + 3] = u2;
}

// ------------------------------------------------------------------------------------------
// ObstaclesFSM (trajectory_tracking.py:266-374)
// ------------------------------------------------------------------------------------------
// ObstaclesFSM.update (:335-372) of one ego on its state before the step.  fl: car active, car triggered, light
// green, waiting.  Writes the slab entries to o (the car first) and returns their number; car_s is the car's
// position while it is on the road, else NaN
LOOP_STEP inline int fsm_step(const mpc_fsm& F, double dt, double s, double v, int* fl, double& car, double& timer,
                              double* o, double& car_s) {
    int n = 0;
    car_s = NAN;
    if (F.dynamic_obstacle) {                        // :335-349
        if (!fl[1] && s >= F.obs_trigger_s) { fl[1] = 1; fl[0] = 1; }
        if (fl[0]) {
            const double os = car + F.obs_v * dt;
            car = os;
            if (os > F.obs_end_s) {
                fl[0] = 0;
            } else {
                o[0] = os;
                o[1] = F.obs_v;
                n = 1;
                car_s = os;
            }
        }
    }
    if (F.traffic_light && !fl[2]) {                 // :351-372
        const double dist = F.tl_pos - s;
        if (0.0 < dist && dist < F.tl_trigger_s) {
            o[2 * n] = F.tl_pos;
            o[2 * n + 1] = 0.0;
            ++n;
            if (v < 0.1 && dist < 10.0) fl[3] = 1;
        }
        if (fl[3]) {
            const double t = timer + dt;
            timer = t;
            if (t >= F.tl_stop_duration) { fl[2] = 1; fl[3] = 0; }
        }
    }
    return n;
}

// the sweep's red-pass question, decided once (bit 1 of qflags) at the first state past the light
template <typename Q>
LOOP_STEP inline void red_pass_step(const mpc_fsm& F, double s, int green, Q q, int& qflags) {
    if (F.traffic_light && !(qflags & 2) && s > F.tl_pos) {
        qflags |= 2;
        if (!green) q[MPC_CLQ_RED_PASS] = 1.0;
    }
}

// per-actor flag bits of a script
enum {
    ACT_CAR_ACTIVE = 1,      // car: on the road (obs_active)
    ACT_CAR_TRIGGERED = 2,   // car: has been spawned once (obs_has_triggered)
    ACT_TL_GREEN = 4,        // light: GREEN
    ACT_TL_WAITING = 8,      // light: the ego stands in front of it (tl_waiting)
    ACT_PASS_DECIDED = 16    // light: the red-pass question is decided
};
// what actor_step reports
enum {
    ACTOR_EMITS = 1,         // (os, ov) is this actor's slab entry of the step
    ACTOR_GREEN = 2,         // a light that is GREEN after the step
    ACTOR_RAN_RED = 4        // a light whose red-pass question was decided at this step, and it was RED
};

// One actor M of a script (not MPC_ACTOR_NONE) for one step: ObstaclesFSM's per-obstacle transitions on its own
// state (fl: ACT_* bits; val: a car's position, a light's timer) and the ego's state before the step.  Returns
// ACTOR_* bits, with the slab entry in (os, ov) if it emits one
LOOP_STEP inline int actor_step(const mpc_actor& M, double dt, double s, double v, int& fl, double& val, double& os,
                                double& ov) {
    int out = 0;
    os = 0.0;
    ov = 0.0;
    if (M.kind == MPC_ACTOR_CAR) {                   // :335-349, this car's state
        if (!(fl & ACT_CAR_TRIGGERED) && s >= M.trigger_s) fl |= ACT_CAR_TRIGGERED | ACT_CAR_ACTIVE;
        if (fl & ACT_CAR_ACTIVE) {
            ov = M.v;
            os = val + ov * dt;
            val = os;
            if (os > M.end_s) fl &= ~ACT_CAR_ACTIVE;
            else out = ACTOR_EMITS;
        }
        return out;
    }
    const double tl_pos = M.pos_s;                   // :351-372, this light's state
    if (!(fl & ACT_TL_GREEN)) {
        const double dist = tl_pos - s;
        if (0.0 < dist && dist < M.trigger_s) {
            out = ACTOR_EMITS;
            os = tl_pos;
            if (v < 0.1 && dist < 10.0) fl |= ACT_TL_WAITING;
        }
        if (fl & ACT_TL_WAITING) {
            const double t = val + dt;
            val = t;
            if (t >= M.stop_duration) fl = (fl | ACT_TL_GREEN) & ~ACT_TL_WAITING;
        }
    }
    if (fl & ACT_TL_GREEN) out |= ACTOR_GREEN;
    if (!(fl & ACT_PASS_DECIDED) && s > tl_pos) {    // the first state past this light
        fl |= ACT_PASS_DECIDED;
        if (!(fl & ACT_TL_GREEN)) out |= ACTOR_RAN_RED;
    }
    return out;
}

// ------------------------------------------------------------------------------------------
// the plant step and the quantities of an ego
// ------------------------------------------------------------------------------------------
// the row of an ego before its first step, which one that never runs keeps: its initial s and |d|, zeros, a NaN
// gap (closed_loop_quantities' n_steps == 0 row)
template <typename Q>
LOOP_STEP inline void quant_init(Q q, int b, double s0, double d0) {
    for (int k = 0; k < MPC_CL_NQ; ++k) q[k] = 0.0;
    q[MPC_CLQ_EGO] = (double)b;
    q[MPC_CLQ_S_FINAL] = s0;
    q[MPC_CLQ_MAX_DEV] = fabs(d0);
    q[MPC_CLQ_MIN_OBS_DIST] = NAN;
}

// x <- x + dt * dynamics(x, ua, k_ref) (:403-406) with the applied control ua = (ua1, ua2); k_ref is the reference
// curvature at x[0], entry 3 of the caller's state lookup
LOOP_STEP inline void plant_step(double* x, double dt, double ua1, double ua2, double k_ref) {
    const double xd[5] = {x[4], x[4] * x[2], x[4] * (x[3] - k_ref), ua1, ua2};
    LOOP_UNROLL
    for (int j = 0; j < 5; ++j) x[j] = x[j] + dt * xd[j];
}

// the plant-side quantities after step `step` left the ego at x: (u1, u2) is the commanded control, status the
// solver's
template <typename Q>
LOOP_STEP inline void plant_quant(Q q, int step, const double* x, double u1, double u2, int status) {
    q[MPC_CLQ_N_STEPS] = (double)(step + 1);
    q[MPC_CLQ_S_FINAL] = x[0];
    keep_max(q[MPC_CLQ_MAX_DEV], fabs(x[1]));
    extremes4(q, MPC_CLQ_U1_MIN, step, u1, u2);
    const int code = status & MPC_STATUS_MASK;
    if (code == MPC_INFEASIBLE) q[MPC_CLQ_N_INFEASIBLE] += 1.0;
    if (code != MPC_OK) q[MPC_CLQ_N_NOT_OK] += 1.0;
}

// ------------------------------------------------------------------------------------------
// the plan-vs-outcome gaps of mpc_closed_loop_traced (include/mpcqp.h, MPC_TG_*)
// ------------------------------------------------------------------------------------------
// Lookahead j keeps the (s, d, v) of stage j of the last j predictions in a ring of j slots: the prediction made
// at step t takes slot t mod j
LOOP_STEP inline int trace_slot(int t, int j) { return t % j; }

// the state after step t is row t + 1 of the ego: it pairs with the prediction made at step t + 1 - j, if any
LOOP_STEP inline bool trace_pair(int t, int j) { return t + 1 >= j; }

// the row of an ego and a lookahead before the first pair, which one without pairs keeps
template <typename Q>
LOOP_STEP inline void trace_init(Q g) {
    g[MPC_TG_N_CMP] = 0.0;
    g[MPC_TG_MAX_DS] = NAN;
    g[MPC_TG_MAX_DD] = NAN;
    g[MPC_TG_MAX_DV] = NAN;
    g[MPC_TG_STEP_DD] = -1.0;
}

// One pair: (ps, pd, pv) predicted at step t0 against the true (xs, xd, xv).  The first pair seeds the maxima, the
// later ones enter by keep_max; MAX_DD's step moves only when the maximum grows or turns NaN, so ties and later
// NaNs leave it at the earliest (numpy's argmax)
template <typename Q>
LOOP_STEP inline void trace_gap(Q g, int t0, double ps, double pd, double pv, double xs, double xd, double xv) {
    const double ds = fabs(ps - xs), dd = fabs(pd - xd), dv = fabs(pv - xv);
    const double n = g[MPC_TG_N_CMP];
    g[MPC_TG_N_CMP] = n + 1.0;
    if (n == 0.0) {
        g[MPC_TG_MAX_DS] = ds;
        g[MPC_TG_MAX_DD] = dd;
        g[MPC_TG_MAX_DV] = dv;
        g[MPC_TG_STEP_DD] = (double)t0;
        return;
    }
    double ms = g[MPC_TG_MAX_DS], mv = g[MPC_TG_MAX_DV];
    const double md = g[MPC_TG_MAX_DD];
    if (keep_max(ms, ds)) g[MPC_TG_MAX_DS] = ds;
    if (keep_max(mv, dv)) g[MPC_TG_MAX_DV] = dv;
    if (dd > md || (dd != dd && md == md)) {
        g[MPC_TG_MAX_DD] = dd;
        g[MPC_TG_STEP_DD] = (double)t0;
    }
}

// ------------------------------------------------------------------------------------------
// the noise source of mpc_closed_loop_noisy (include/mpcqp.h): stateless Philox4x32-10, one block per variate
// ------------------------------------------------------------------------------------------
#define NZ_M0 0xD2511F53u
#define NZ_M1 0xCD9E8D57u
#define NZ_W0 0x9E3779B9u
#define NZ_W1 0xBB67AE85u
#define NZ_C (1.7320508075688772 * 0x1p-32)    // the double nearest sqrt(3), scaled exactly

// the block of counter (c0 .. c3) under key (k0, k1); the high halves come from 64-bit products
LOOP_STEP inline void noise_words(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1,
                                  unsigned w[4]) {
    LOOP_UNROLL
    for (int r = 0; r < 10; ++r) {
        const unsigned long long p0 = (unsigned long long)NZ_M0 * c0, p1 = (unsigned long long)NZ_M1 * c2;
        c0 = (unsigned)(p1 >> 32) ^ c1 ^ k0;
        c1 = (unsigned)p1;
        c2 = (unsigned)(p0 >> 32) ^ c3 ^ k1;
        c3 = (unsigned)p0;
        k0 += NZ_W0;
        k1 += NZ_W1;
    }
    w[0] = c0; w[1] = c1; w[2] = c2; w[3] = c3;
}

// the variate of four words: the sum is an exact integer below 2^34, the subtraction is exact, one rounding
LOOP_STEP inline double noise_variate(const unsigned w[4]) {
    const unsigned long long s = (unsigned long long)w[0] + w[1] + w[2] + w[3];
    return ((double)s - 8589934590.0) * NZ_C;
}

// who draws: the key (the seed's halves), the global ego and the step
struct NoiseAt {
    unsigned k0, k1;
    unsigned long long g;
    int step;
};

LOOP_STEP inline double noise_z(const NoiseAt& at, int channel) {
    unsigned w[4];
    noise_words((unsigned)at.g, (unsigned)(at.g >> 32), (unsigned)at.step, (unsigned)channel, at.k0, at.k1, w);
    return noise_variate(w);
}

// x + (scale * sigma) * z of `channel`; a channel whose sigma is 0 draws nothing and leaves x as it is
LOOP_STEP inline double noise_add(double x, double sigma, const NoiseAt& at, int channel, double scale = 1.0) {
    return sigma != 0.0 ? x + (scale * sigma) * noise_z(at, channel) : x;
}

// the actuation clamp of one component
LOOP_STEP inline double clamp_control(double t, double lo, double hi) { return t < lo ? lo : (t > hi ? hi : t); }

// the applied control of one channel: the commanded u plus its draw, clamped to [lo, hi]; clamped is set if the
// clamp changed it.  Sigma 0: u as it is, unclamped
LOOP_STEP inline double apply_actuation(double u, double sigma, const NoiseAt& at, int channel, double lo, double hi,
                                        bool& clamped) {
    if (sigma == 0.0) return u;
    const double t = noise_add(u, sigma, at, channel);
    clamped = clamped || t < lo || t > hi;
    return clamp_control(t, lo, hi);
}

// ------------------------------------------------------------------------------------------
// the warm starts of mpc_closed_loop_warm (include/mpcqp.h, MPC_WARM_*, MPC_WQ_*)
// ------------------------------------------------------------------------------------------
// The reference warm start (trajectory_tracking.py:224-246) one stage after the other, the arithmetic the solver
// runs for itself without a ubar: s advances by repeated addition of v * dt, the brake flag is sticky once a slab
// position is within brake_distance of s, the reference control is looked up at s.  The stages are walked in order
// (warm_ref_advance) and the control is looked up at those that need it (warm_ref_control); ctl(s, ur) is the
// caller's get_control on its own table
struct WarmRef {
    double s, v;
    bool brake;
};
LOOP_STEP inline WarmRef warm_ref_begin(const double* xm) { return WarmRef{xm[0], xm[4], false}; }

// stage k's s and brake flag from stage k - 1's (k = 0: from warm_ref_begin's)
LOOP_STEP inline void warm_ref_advance(WarmRef& w, int k, double dt, const double* obs, int nobs,
                                       double brake_distance) {
    if (k > 0) w.s += w.v * dt;
    for (int i = 0; i < nobs; ++i)
        if ((obs[2 * i] - w.s) < brake_distance) w.brake = true;
}

// the warm start's control of the stage w stands at
template <typename Ctl>
LOOP_STEP inline void warm_ref_control(const WarmRef& w, double brake_accel, Ctl ctl, double& u1, double& u2) {
    double ur[2];
    ctl(w.s, ur);
    u1 = ur[0];
    u2 = w.brake ? brake_accel : ur[1];
}

// an element of a kept plan that may be carried
LOOP_STEP inline bool warm_finite(double u) { return u - u == 0.0; }

// Does this step start from the reference warm start?  kept_status: the status of the ego's last solve, -1 before
// its first; plan_finite: every element of the kept plan is; kept_nobs / nobs: the n_obs the solver was handed at
// the last step and is handed now
LOOP_STEP inline bool warm_reset(const mpc_warm& w, int kept_status, bool plan_finite, int kept_nobs, int nobs) {
    if (w.mode != MPC_WARM_CARRY || kept_status < 0 || !plan_finite) return true;
    const int code = kept_status & MPC_STATUS_MASK;
    if (code == MPC_NUMERICAL) return true;
    if ((w.reset & MPC_WRESET_NOBS) && nobs != kept_nobs) return true;
    if ((w.reset & MPC_WRESET_INFEASIBLE) && code == MPC_INFEASIBLE) return true;
    return (w.reset & MPC_WRESET_MAX_ITER) && code == MPC_MAX_ITER;
}

// the stage of the kept plan that stage k of a carried ubar takes (clamped), -1: the reference warm start's stage k
LOOP_STEP inline int warm_source(int k, int N, int tail) {
    return k < N - 1 ? k + 1 : (tail == MPC_WTAIL_HOLD ? N - 1 : -1);
}

// the row of an ego before its first step, which one that never runs keeps
template <typename Q>
LOOP_STEP inline void warm_init(Q w) {
    w[MPC_WQ_N_RESET] = 0.0;
    w[MPC_WQ_MAX_MOVE] = NAN;
    w[MPC_WQ_STEP_MAX_MOVE] = -1.0;
    w[MPC_WQ_SUM_MOVE] = 0.0;
}

// move <- max(move, |u - ub|) over the elements of a plan, from 0.0: a NaN enters and stays
LOOP_STEP inline void warm_move_element(double& move, double u, double ub) { keep_max(move, fabs(u - ub)); }

// Step `step` moved the plan by `move` from its ubar.  Step 0, which every ego that runs at all runs, seeds the
// maximum; its step moves only when the maximum grows or turns NaN (trace_gap's rule for MAX_DD)
template <typename Q>
LOOP_STEP inline void warm_move(Q w, int step, double move) {
    const double m = w[MPC_WQ_MAX_MOVE];
    if (step == 0 || move > m || (move != move && m == m)) {
        w[MPC_WQ_MAX_MOVE] = move;
        w[MPC_WQ_STEP_MAX_MOVE] = (double)step;
    }
    w[MPC_WQ_SUM_MOVE] = w[MPC_WQ_SUM_MOVE] + move;
}
