// evaluate_kernel.h -- the batched evaluator (mpc_evaluate_batch, include/mpcqp.h): for any control sequence U the
// nonlinear rollout predict(x0, U) (trajectory_tracking.py:87-114), the reference's cost (:116-152), its constraint
// rows (:155-211) and a per-instance summary of them.  No QP, no solver state.
//
// The solver's layout: one lane group of GL lanes per instance (GL = 16, 32, 64 by N + 1, 64 / GL instances per
// wavefront).  The instance is read and rolled out by the shared phase (evaluator_common.h): predict_grp rolls it out
// (lane 0 rolls s, k, v; lane j looks the table up at s_j; lane 0 rolls d, o) and leaves lane j the whole reference
// state at s_j, so no table is searched twice.  Lane j = 1..N then
// owns stage j (its three cost terms, its 7 + n_obs rows, written straight to its slice of `rows`) and lane
// j = 0..N-1 owns control j (its two cost terms, its box excess).  Minima and counts go through Grp<GL>; the two
// sums whose bits must not depend on GL, the running cost and the L1 violation, are added by lane 0 from LDS in the
// order the header states.  The steps of a control and of a stage and the sums are tracker_model.h's, which the
// host backend's evaluate_one (cpu_backend.h) folds sequentially: the two agree bit for bit.
//
// Per-instance LDS (doubles): the rollout Xr [N+1][5], kap [N+1] (k_ref of the rollout; once the rollout is done,
// the L1 partial of stage j at kap[j-1]) and ct [N][5]: the cost terms (d, o, v) of stage j+1 and (u1, u2) of
// control j.  Until the rollout's first phase is over ct also stages U for lane 0.  The array is static, sized for
// the longest horizon of the lane group (N = GL - 1): 5.4 - 5.5 KB per wavefront for every GL.
#pragma once
#include "evaluator_common.h"

__host__ __device__ constexpr int ev_lds_doubles(int N) { return (11 * N + 6 + 1) & ~1; }

template <int GL, bool OBS>
__global__ void __launch_bounds__(WAVE)
mpc_evaluate_kernel(DevTable tab, KParams Pr, int B, int rw, const double* __restrict__ x0g,
                    const double* __restrict__ obsg, const int* __restrict__ nobsg, const double* __restrict__ Ug,
                    double* __restrict__ Xg, double* __restrict__ sumg, double* __restrict__ termg,
                    double* __restrict__ rowg) {
    constexpr int G = WAVE / GL;
    constexpr int LD = ev_lds_doubles(GL - 1);
    __shared__ __attribute__((aligned(16))) double smem[G * LD];
    const int ln = threadIdx.x;
    const int grp = ln / GL, gl = ln % GL;
    int b = blockIdx.x * G + grp;
    const bool bvalid = b < B;
    if (!bvalid) b = B - 1;          // a spare group repeats the last instance (every lane reaches every
                                     // wave_sync); it writes nothing
    const Grp<GL> Q{grp * GL};
    const int N = Pr.N, NP = N + 1;
    double* Xr = smem + grp * LD;
    double* kap = Xr + 5 * NP;
    double* ct = kap + NP;
    const double inf = __builtin_inf(), qnan = __builtin_nan("");

    // ---- the shared phase (evaluator_common.h): the instance and its rollout; U is staged in ct ----
    const EvcLds L{Xr, kap, ct, nullptr, nullptr, nullptr};
    EvcInst I;
    evc_instance<OBS>(Pr, b, x0g, obsg, nobsg, I);
    evc_rollout<false>(tab, Pr, b, gl, Ug, ct, L, I);
    const bool stage = I.stage;
    const int nobs = I.nobs;

    // ---- control gl (cost terms, box excess), then stage gl (cost terms and rows): tracker_model.h's steps ----
    EvRun run = ev_run_begin();
    if (I.ctrl) ev_control(Pr, I.u1, I.u2, ct + 5 * gl, run);
    EvStage S = ev_stage_begin();
    if (stage) {
        double* ro = bvalid && rowg ? rowg + ((size_t)b * N + (gl - 1)) * rw : nullptr;
        ev_stage(Pr, gl, Xr + 5 * gl, I.st, I.obs, nobs, rw, ct + 5 * (gl - 1), ro, S, run);
        kap[gl - 1] = S.p1;
    }

    // ---- group summary -------------------------------------------------------------------------
    const int myflags = ev_flags(run, S.snan);
    const int flags = (int)__double_as_longlong(Q.reduce(__longlong_as_double((long long)myflags), [](double a, double c) {
        return __longlong_as_double(__double_as_longlong(a) | __double_as_longlong(c));
    }));
    const bool anyn = (flags & EV_NAN_ROW) != 0;
    const double m = Q.min(stage && !S.snan ? S.smin : inf);
    // np.argmin: the first NaN row if there is one, else the first row equal to the minimum
    const bool mine = stage && (anyn ? S.snan : (!S.snan && S.smin == m));
    const int astage = (int)Q.min(mine ? (double)gl : 1e9);
    const double mfirst = Q.get(S.smin, astage);                // the first minimum's own bits
    const int akind = __shfl(S.skind, Q.base + astage, WAVE);
    const double cnt = Q.sum((double)S.nneg);
    const double mlane = Q.min(run.fl), mobs = Q.min(run.fo), mv = Q.min(run.fv), mbox = Q.max(run.bx);
    wave_sync();

    // lane 0 adds the cost terms and the L1 partials in the stated order and writes the summary
    if (bvalid && gl == 0) {
        const EvSums Z = ev_sums(N, ct, kap);
        if (sumg)
            ev_summary(sumg + (size_t)b * MPC_EV_NQ, Z, anyn ? qnan : mfirst, astage, akind, cnt, mlane, mobs, mv, mbox,
                       flags, nobs);
        if (termg) {
#pragma unroll
            for (int a = 0; a < 5; ++a) termg[(size_t)b * 5 + a] = Z.t[a];
        }
    }
    if (bvalid && Xg)
        for (int i = gl; i < 5 * NP; i += GL) Xg[(size_t)b * 5 * NP + i] = Xr[i];
}
