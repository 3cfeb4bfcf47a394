// hessvec_kernel.h -- the batched Hessian-vector products and row tangents (mpc_hessvec_batch, include/mpcqp.h): for
// any control sequence U and M directions v, (d2 L / dU2) v and J v, by one forward tangent chain and one second-order
// reverse chain per direction over the rollout predict(x0, U).  No QP, no solver state.
//
// One wavefront per instance.  Phase 1 is the shared phase (evaluator_common.h) on lanes 0..N, as in
// gradient_kernel.h with one group of 64 lanes: predict_grp rolls the instance out, lane j = 0..N-1 owns control j
// and A_j, lane j = 1..N owns stage j (cost terms, q_j, c_j), lanes 0 and 1 run the two reverse sweeps in place, and
// the Lagrangian costate pi = p - p' replaces q.  It leaves X, A, the slopes and pi in LDS.
//
// Phase 2 runs in passes of W = hv_pass_width(N) directions: lane m owns direction pass * W + m and runs its chains
// alone, so the order of every addition is the header's and does not depend on what the other lanes carry.  The
// forward chain parks dx_1..dx_N in LDS, laid out [stage][component][lane] with a component stride of W + 1 doubles:
// a wavefront's accesses are consecutive 8-byte words (conflict-free), and the odd stride also spreads the
// transposed reads of the copies below over the banks.  J v is then formed by all lanes together, element by element
// of the pass's contiguous block of JV (every element is a function of one dx_k alone: hv_row_tangent), so the stores
// are consecutive.  The reverse chain walks k = N..1 and leaves dpi_k[3], dpi_k[4] in the slot of dx_k, which is dead
// by then; the lane then forms H v and its curvature sums in increasing i and leaves H v in the first two
// components of the slots, from where all lanes copy the pass's contiguous block of HV out.  Lane 0 folds the
// summary over the instance's curvatures, kept in LDS across the passes.  The steps are tracker_model.h's, which the
// host backend's hessvec_one (cpu_backend.h) folds sequentially: the two agree bit for bit.
//
// LDS (doubles), dynamic, sized by the actual N: the rollout Xr [N+1][5], kap [N+1], ct [N][5], A [N][5], q / pi
// [N][5], c [N][5], the slopes [N+1][4], the curvatures [MPC_HV_MAX_DIRS][2], then dX [N][5][W + 1].  W = 64 for
// N <= MPC_HV_N64_MAX = 56, where that still fits the 160 KiB of a CU, and 32 beyond:
//   N = 20, W = 64:  58.9 KB (two workgroups per CU)     N = 56, W = 64: 161.2 KB     N = 63, W = 32: 100.4 KB
#pragma once
#include "evaluator_common.h"

__host__ __device__ constexpr int hv_inst_doubles(int N) { return 30 * N + 10 + 2 * MPC_HV_MAX_DIRS; }
__host__ __device__ constexpr int hv_lds_doubles(int N, int W) { return hv_inst_doubles(N) + 5 * N * (W + 1); }

template <int W, bool OBS>
__global__ void __launch_bounds__(WAVE)
mpc_hessvec_kernel(DevTable tab, KParams Pr, int B, int rw, const double* __restrict__ x0g,
                   const double* __restrict__ obsg, const int* __restrict__ nobsg, const double* __restrict__ Ug,
                   const double* __restrict__ lamg, int M, const double* __restrict__ Vg, int mode,
                   double* __restrict__ HVg, double* __restrict__ JVg, double* __restrict__ curvg,
                   double* __restrict__ sumg) {
    constexpr int PS = W + 1;            // the component stride of dX
    extern __shared__ __attribute__((aligned(16))) double hv_smem[];
    const int ln = threadIdx.x;
    const int b = blockIdx.x;
    if (b >= B) return;                  // wave-uniform; the grid has B workgroups
    const int N = Pr.N, NP = N + 1, n2 = 2 * N;
    const double dt = Pr.dt;
    double* Xr = hv_smem;
    double* kap = Xr + 5 * NP;
    double* ct = kap + NP;
    double* As = ct + 5 * N;
    double* qs = As + 5 * N;
    double* cs = qs + 5 * N;
    double* sls = cs + 5 * N;
    double* cvs = sls + 4 * NP;
    double* dX = cvs + 2 * MPC_HV_MAX_DIRS;
    const bool has_lam = lamg != nullptr;
    const bool exact = mode == MPC_HV_EXACT;

    // ---- phase 1: the shared phase (evaluator_common.h) on lanes 0..N, U staged in ct; the slopes are kept ----
    const EvcLds L{Xr, kap, ct, As, qs, cs};
    EvcInst I;
    evc_instance<OBS>(Pr, b, x0g, obsg, nobsg, I);
    evc_rollout<true>(tab, Pr, b, ln, Ug, ct, L, I);
    const int nobs = I.nobs;
    EvRun run = ev_run_begin();
    GrRun gr = gr_run_begin();
    if (ln <= N) {
#pragma unroll
        for (int a = 0; a < 4; ++a) sls[4 * ln + a] = I.sl[a];
    }
    evc_linearise<true, true>(Pr, b, rw, ln, L, I, lamg, nullptr, run, gr);
    evc_sweeps(N, dt, ln, L, has_lam, nullptr);
    wave_sync();
    if (has_lam)
        for (int i = ln; i < 5 * N; i += WAVE) qs[i] = qs[i] - cs[i];      // pi = p - p'
    wave_sync();

    // ---- phase 2: a lane per direction, W directions per pass ----
    const size_t jvn = (size_t)N * rw;         // JV's doubles per direction
    for (int m0 = 0; m0 < M; m0 += W) {
        const int dir = m0 + ln;
        const bool mine = ln < W && dir < M;
        const int nd = M - m0 < W ? M - m0 : W;                         // the directions of this pass
        const double* Vd = Vg ? Vg + ((size_t)b * M + dir) * n2 : nullptr;
        double* col = dX + ln;                 // this lane's column: element (k, a) at col[(5 * k + a) * PS]
        if (mine) {
            double dx[5] = {0.0, 0.0, 0.0, 0.0, 0.0}, y[5];
            for (int k = 0; k < N; ++k) {
                hv_tangent_step(As + 5 * k, dt, dx, hv_dir(Vd, dir, k, 0), hv_dir(Vd, dir, k, 1), y);
#pragma unroll
                for (int a = 0; a < 5; ++a) {
                    dx[a] = y[a];
                    col[(5 * k + a) * PS] = y[a];                       // slot k holds dx_k+1
                }
            }
        }
        wave_sync();
        if (JVg) {
            double* out = JVg + ((size_t)b * M + m0) * jvn;
            const int nj = N * rw;             // nd * nj <= 64 * 63 * 71
            for (int i = ln; i < nd * nj; i += WAVE) {
                const int m = i / nj, r = i % nj;
                const int k = r / rw, c = r % rw;                       // stage k + 1
                double dx[5];
#pragma unroll
                for (int a = 0; a < 5; ++a) dx[a] = dX[(5 * k + a) * PS + m];
                out[i] = hv_row_tangent(Pr, c, nobs, Xr + 5 * (k + 1), dx);
            }
            wave_sync();
        }
        if (mine && (HVg || curvg || sumg)) {
            double dp[5] = {0.0, 0.0, 0.0, 0.0, 0.0}, dx[5], qd[5], e[5] = {0.0, 0.0, 0.0, 0.0, 0.0}, y[5];
            for (int k = N; k >= 1; --k) {
#pragma unroll
                for (int a = 0; a < 5; ++a) dx[a] = col[(5 * (k - 1) + a) * PS];
                hv_stage(Pr, sls + 4 * k, dx, qd);
                if (k == N) {
#pragma unroll
                    for (int a = 0; a < 5; ++a) y[a] = qd[a];
                } else {
                    if (exact) hv_second_order(dt, sls[4 * k + 2], dx, qs + 5 * k, e);
                    hv_reverse_step(As + 5 * k, dt, qd, dp, exact, e, y);
                }
#pragma unroll
                for (int a = 0; a < 5; ++a) dp[a] = y[a];
                col[(5 * (k - 1) + 3) * PS] = y[3];
                col[(5 * (k - 1) + 4) * PS] = y[4];
            }
            double cv[2] = {0.0, 0.0}, hv[2];
            for (int k = 0; k < N; ++k) {
                const double v1 = hv_dir(Vd, dir, k, 0), v2 = hv_dir(Vd, dir, k, 1);
                dp[3] = col[(5 * k + 3) * PS];
                dp[4] = col[(5 * k + 4) * PS];
                hv_control(Pr, v1, v2, dp, hv);
                hv_curv(cv, v1, hv[0]);
                hv_curv(cv, v2, hv[1]);
                col[(5 * k) * PS] = hv[0];
                col[(5 * k + 1) * PS] = hv[1];
            }
            cvs[2 * dir] = cv[0];
            cvs[2 * dir + 1] = cv[1];
        }
        wave_sync();
        if (HVg) {
            double* out = HVg + ((size_t)b * M + m0) * n2;
            for (int i = ln; i < nd * n2; i += WAVE) {
                const int m = i / n2, r = i % n2;
                out[i] = dX[(5 * (r >> 1) + (r & 1)) * PS + m];
            }
        }
        wave_sync();
    }
    if (curvg)
        for (int i = ln; i < 2 * M; i += WAVE) curvg[(size_t)b * 2 * M + i] = cvs[i];
    // lane 0 adds the cost terms in the evaluator's order and folds the summary over the directions
    if (sumg && ln == 0) hv_summary(sumg + (size_t)b * MPC_HV_NQ, ev_sums(N, ct, kap).cost, M, cvs);
}
