// gradient_kernel.h -- the batched gradients (mpc_gradient_batch, include/mpcqp.h): for any control sequence U the
// gradient of the reference's cost in U and x0 and J' lam of its constraint rows, by reverse (adjoint) sweeps over
// the rollout predict(x0, U).  No QP, no solver state.
//
// The evaluator's layout (evaluate_kernel.h): one lane group of GL lanes per instance (GL = 16, 32, 64 by N + 1,
// 64 / GL instances per wavefront).  Everything up to the costates is the shared phase (evaluator_common.h):
// predict_grp rolls the instance out and leaves lane j the reference state at s_j and its slopes.  Lane j = 0..N-1
// then owns control j and the coefficients of A_j (stage_A), lane j = 1..N owns stage j: its cost terms, its stage
// gradient q_j and its weighted row gradient c_j, parked in LDS.  The two reverse recursions are sequential chains
// of N short steps: lane 0 runs the cost's and lane 1 the rows' in lock step, in place in LDS (q becomes the
// costate p, c becomes p'), which fixes the order of every addition.  Lane j
// then reads p_j+1 and p'_j+1 and writes grad[j] and jtl[j]; the extremes go through Grp<GL>, and the cost is
// added by lane 0 from LDS in the evaluator's order (ev_sums).  The steps are tracker_model.h's, which the host
// backend's gradient_one (cpu_backend.h) folds sequentially: the two agree bit for bit.
//
// Per-instance LDS (doubles): the rollout Xr [N+1][5], kap [N+1] (k_ref of the rollout; zero once the rollout is
// done: ev_sums' L1 partials, which nobody reads here), ct [N][5] (the evaluator's cost terms; until the rollout's
// first phase is over it also stages U for lane 0), A [N][5], q [N][5] and c [N][5].  The array is static, sized
// for the longest horizon of the lane group (N = GL - 1): 12.4 - 12.9 KB per wavefront for every GL.
#pragma once
#include "evaluator_common.h"

__host__ __device__ constexpr int gr_lds_doubles(int N) { return (26 * N + 6 + 1) & ~1; }

enum { GR_NAN_GRAD = 1, GR_NAN_LAG = 2, GR_NAN_PG = 4, GR_NAN_COMPL = 8, GR_NAN_LAM = 16 };

template <int GL, bool OBS>
__global__ void __launch_bounds__(WAVE)
mpc_gradient_kernel(DevTable tab, KParams Pr, int B, int rw, const double* __restrict__ x0g,
                    const double* __restrict__ obsg, const int* __restrict__ nobsg, const double* __restrict__ Ug,
                    const double* __restrict__ lamg, double* __restrict__ gradg, double* __restrict__ jtlg,
                    double* __restrict__ gx0g, double* __restrict__ cosg, double* __restrict__ sumg) {
    constexpr int G = WAVE / GL;
    constexpr int LD = gr_lds_doubles(GL - 1);
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
    double* As = ct + 5 * N;
    double* qs = As + 5 * N;
    double* cs = qs + 5 * N;
    const double qnan = __builtin_nan("");
    const bool has_lam = lamg != nullptr;

    // ---- the shared phase (evaluator_common.h): the instance, its rollout (U is staged in ct), the linearisation
    // (cost terms, A, q, c) and the reverse sweeps, lane 0 the cost's and lane 1 the rows', in place ----
    const EvcLds L{Xr, kap, ct, As, qs, cs};
    EvcInst I;
    evc_instance<OBS>(Pr, b, x0g, obsg, nobsg, I);
    evc_rollout<true>(tab, Pr, b, gl, Ug, ct, L, I);
    EvRun run = ev_run_begin();
    GrRun gr = gr_run_begin();
    evc_linearise<true, true>(Pr, b, rw, gl, L, I, lamg, nullptr, run, gr);
    evc_sweeps(N, Pr.dt, gl, L, has_lam, bvalid && gx0g ? gx0g + (size_t)b * 5 : nullptr);
    wave_sync();

    // ---- control gl: its gradient and J' lam from p_gl+1, p'_gl+1 ----
    if (I.ctrl) {
        double g[2], jt[2];
        gr_control(Pr, I.u1, I.u2, qs + 5 * gl, has_lam ? cs + 5 * gl : nullptr, g, jt, gr);
        if (bvalid && gradg) {
            gradg[(size_t)b * 2 * N + 2 * gl] = g[0];
            gradg[(size_t)b * 2 * N + 2 * gl + 1] = g[1];
        }
        if (bvalid && jtlg) {
            jtlg[(size_t)b * 2 * N + 2 * gl] = jt[0];
            jtlg[(size_t)b * 2 * N + 2 * gl + 1] = jt[1];
        }
    }
    if (bvalid && cosg)
        for (int i = gl; i < 5 * N; i += GL) cosg[(size_t)b * 5 * N + i] = qs[i];

    // ---- group summary: vmax / vmin drop a NaN, so which extremes met one is reduced beside them ----
    if (sumg) {
        const int myflags = (gr.ginf != gr.ginf ? GR_NAN_GRAD : 0) | (gr.linf != gr.linf ? GR_NAN_LAG : 0) |
                            (gr.pginf != gr.pginf ? GR_NAN_PG : 0) | (gr.compl_ != gr.compl_ ? GR_NAN_COMPL : 0) |
                            (gr.minlam != gr.minlam ? GR_NAN_LAM : 0);
        const int flags = (int)__double_as_longlong(Q.reduce(__longlong_as_double((long long)myflags), [](double a, double c) {
            return __longlong_as_double(__double_as_longlong(a) | __double_as_longlong(c));
        }));
        GrRun T;
        T.ginf = Q.max(gr.ginf != gr.ginf ? 0.0 : gr.ginf);
        T.linf = Q.max(gr.linf != gr.linf ? 0.0 : gr.linf);
        T.pginf = Q.max(gr.pginf != gr.pginf ? 0.0 : gr.pginf);
        T.compl_ = Q.max(gr.compl_ != gr.compl_ ? 0.0 : gr.compl_);
        T.minlam = Q.min(gr.minlam != gr.minlam ? __builtin_inf() : gr.minlam);
        if (flags & GR_NAN_GRAD) T.ginf = qnan;
        if (flags & GR_NAN_LAG) T.linf = qnan;
        if (flags & GR_NAN_PG) T.pginf = qnan;
        if (flags & GR_NAN_COMPL) T.compl_ = qnan;
        if (flags & GR_NAN_LAM) T.minlam = qnan;
        // lane 0 adds the cost terms in the evaluator's order and writes the summary
        if (bvalid && gl == 0) {
            const EvSums Z = ev_sums(N, ct, kap);
            gr_summary(sumg + (size_t)b * MPC_GR_NQ, Z.cost, T, has_lam);
        }
    }
}
