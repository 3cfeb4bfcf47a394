// multiplier_kernel.h -- the batched multiplier estimates (mpc_multipliers_batch, include/mpcqp.h): for any control
// sequence U the least-squares lam of grad = J' lam over the active rows and the free controls.  No QP, no solver
// state.
//
// One wavefront per instance (the Gram matrix and the factorisation want a lane per active row, up to 64 of them).
// The first phase is the shared phase (evaluator_common.h) without cost terms and row weights: predict_grp rolls the
// instance out, lane j = 0..N-1 owns control j and A_j, lane j = 1..N owns stage j: its rows (ev_stage, parked in
// LDS), its stage gradient q_j; lane 0 runs the cost's reverse sweep in place and lane j forms grad[j].  The stage lanes count their active rows; a prefix over the counts
// gives every stage its place in the list, which it fills in the reference's order.  Lane a then owns active row a:
// it runs the row's own reverse chain over the LDS-resident A_k (mu_row_chain) and parks j_a in LDS, forms row a of
// the Gram matrix (columns b <= a) and r[a], and holds row a through the right-looking factorisation: after column c
// every later row takes L[a][c] L[b][c] off its entries, so an entry's terms are subtracted in increasing c, the
// order the header states.  The pivot test, the pivot and its square root are computed by every lane alike (the
// decisions are wave-uniform).  r turns into y during the factorisation; the back substitution walks the kept columns
// downwards.  The steps are tracker_model.h's, which the host backend's multipliers_one (cpu_backend.h) folds
// sequentially: the two agree bit for bit.
//
// LDS (doubles), static, sized for the longest horizon NM = GL - 1 of the lane-group class of N: the rollout Xr
// [NM+1][5], kap [NM+1], A [NM][5], q [NM][5], grad [2 NM] (it stages U for the rollout first), lam of the list [64],
// the free mask [2 NM], the list [64] and the stage counts [64] as ints, the row gradients J [2 NM][65] by component
// (lane a reads and writes column a: conflict-free; the stride of 65 keeps the transposed reads of the residual
// conflict-free too) and G / L [64][65] by column.  The rows [N][rw] live in J's space until the list is built, and
// the lam slab is assembled there at the end.  52.2 KB (GL = 16), 71.3 KB (GL = 32), 109.4 KB (GL = 64) per wavefront.
#pragma once
#include "evaluator_common.h"

#define MU_JS 65     // the lane stride of J's and G's columns (doubles)

__host__ __device__ constexpr int mu_lds_doubles(int NM) {
    return 6 * (NM + 1) + 12 * NM + MPC_MAX_ACTIVE + (NM + MPC_MAX_ACTIVE) + 2 * NM * MU_JS + MPC_MAX_ACTIVE * MU_JS;
}

template <int GL, bool OBS>
__global__ void __launch_bounds__(WAVE)
mpc_multipliers_kernel(DevTable tab, KParams Pr, int B, int rw, const double* __restrict__ x0g,
                       const double* __restrict__ obsg, const int* __restrict__ nobsg, const double* __restrict__ Ug,
                       double active_tol, double bound_tol, double rank_tol, double* __restrict__ lamg,
                       int* __restrict__ actg, double* __restrict__ sumg) {
    constexpr int NM = GL - 1, MA = MPC_MAX_ACTIVE, JS = MU_JS;
    static_assert(MA == WAVE, "a lane per active row");
    static_assert(7 + MPC_MAX_OBS <= 2 * JS, "the rows [N][rw] fit in J's space");
    __shared__ __attribute__((aligned(16))) double smem[mu_lds_doubles(NM)];
    const int ln = threadIdx.x;
    const int b = blockIdx.x;
    if (b >= B) return;              // wave-uniform; the grid has B workgroups
    const int N = Pr.N, n2 = 2 * N;
    const double dt = Pr.dt;
    double* Xr = smem;
    double* kap = Xr + 5 * (NM + 1);
    double* As = kap + (NM + 1);
    double* qs = As + 5 * NM;
    double* gradv = qs + 5 * NM;
    double* lamv = gradv + 2 * NM;
    int* freem = reinterpret_cast<int*>(lamv + MA);
    int* list = freem + 2 * NM;
    int* cnt = list + MA;
    double* J = lamv + MA + (NM + MA);
    double* W = J + 2 * NM * JS;
    double* rowsb = J;
    const double qnan = __builtin_nan("");

    // ---- the shared phase (evaluator_common.h): the instance, its rollout (U is staged in gradv) and the
    // linearisation without cost terms and without weighted rows: A_ln, then stage ln's rows (kept in LDS) and q ----
    const EvcLds L{Xr, kap, nullptr, As, qs, nullptr};
    EvcInst I;
    evc_instance<OBS>(Pr, b, x0g, obsg, nobsg, I);
    evc_rollout<true>(tab, Pr, b, ln, Ug, gradv, L, I);
    const bool ctrl = I.ctrl, stage = I.stage;
    const double u1 = I.u1, u2 = I.u2;
    const int nobs = I.nobs;
    EvRun run = ev_run_begin();
    GrRun gr = gr_run_begin();
    evc_linearise<false, false>(Pr, b, rw, ln, L, I, nullptr, rowsb, run, gr);

    // ---- the free test of control ln, and stage ln's count of active rows ----
    bool f0 = false, f1 = false;
    if (ctrl) {
        f0 = mu_free(u1, Pr.u_min0, Pr.u_max0, bound_tol);
        f1 = mu_free(u2, Pr.u_min1, Pr.u_max1, bound_tol);
        freem[2 * ln] = f0;
        freem[2 * ln + 1] = f1;
    }
    int mycnt = 0;
    bool rownan = false;             // a NaN row is never active, and it makes the instance MPC_MU_NONFINITE
    if (stage) {
        const double* ro = rowsb + (ln - 1) * rw;
        for (int i = 0; i < 7 + nobs; ++i) {
            const double g = ro[mu_list_col(i, nobs)];
            mycnt += mu_active(g, active_tol) ? 1 : 0;
            rownan = rownan || g != g;
        }
    }
    cnt[ln] = mycnt;

    // ---- the cost's reverse sweep (the shared phase's, lane 0), and the list: a prefix over the stage counts places
    // every stage ----
    evc_sweeps(N, dt, ln, L, false, nullptr);
    int off = 0, na = 0;
    for (int j = 1; j <= N; ++j) {
        const int cj = cnt[j];
        off += j < ln ? cj : 0;
        na += cj;
    }
    if (stage && na <= MA) {
        const double* ro = rowsb + (ln - 1) * rw;
        int pos = off;
        for (int i = 0; i < 7 + nobs; ++i) {
            const int col = mu_list_col(i, nobs);
            if (mu_active(ro[col], active_tol)) {
                list[pos] = (ln - 1) * rw + col;
                ++pos;
            }
        }
    }
    wave_sync();

    // ---- control ln: its gradient; the counts every lane decides by ----
    bool bad = rownan;
    if (ctrl) {
        double g[2], jt[2];
        gr_control(Pr, u1, u2, qs + 5 * ln, nullptr, g, jt, gr);
        gradv[2 * ln] = g[0];
        gradv[2 * ln + 1] = g[1];
        bad = bad || (f0 && !mu_finite(g[0])) || (f1 && !mu_finite(g[1]));
    }
    const int nf = __popcll(__ballot(f0)) + __popcll(__ballot(f1));
    const bool listed = na <= MA && na > 0 && nf > 0;
    const int mine = (listed && ln < na) ? list[ln] : -1;
    wave_sync();                     // the rows are dead from here: J takes their space

    // ---- lane a: the reverse chain of active row a ----
    if (mine >= 0) {
        const int t = mine / rw + 1;
        double c[5];
        mu_row_grad(Pr, mine % rw, Xr + 5 * t, c);
        for (int i = 2 * t; i < n2; ++i) J[i * JS + ln] = 0.0;
        mu_row_chain(t, dt, As, c, [&](int i, double v) {
            J[i * JS + ln] = v;
            if (freem[i] && !mu_finite(v)) bad = true;
        });
    }
    const int status = mu_status(na, nf, __ballot(bad) != 0);
    const int m = (status == MPC_MU_OK && listed) ? na : 0;
    wave_sync();

    // ---- the normal equations over the free components: row ln of G (columns <= ln) and r[ln] ----
    double r = 0.0, gd = 0.0;
    if (ln < m) {
        for (int c = 0; c <= ln; ++c) {
            double s = 0.0;
            for (int i = 0; i < n2; ++i)
                if (freem[i]) s = s + J[i * JS + ln] * J[i * JS + c];
            W[c * JS + ln] = s;
            gd = s;
        }
        double s = 0.0;
        for (int i = 0; i < n2; ++i)
            if (freem[i]) s = s + J[i * JS + ln] * gradv[i];
        r = s;
    }
    wave_sync();

    // ---- Cholesky in list order with the drop rule, right-looking; r becomes y ----
    unsigned long long keepm = 0ull;
    int nu = 0;
    double minpiv = INFINITY, ldiag = 0.0;
    for (int c = 0; c < m; ++c) {
        const double d = W[c * JS + c];
        const double g0c = __shfl(gd, c, WAVE);
        const double rc0 = __shfl(r, c, WAVE);
        if (mu_keep(d, g0c, rank_tol)) {       // wave-uniform
            keepm |= 1ull << c;
            ++nu;
            const double piv = d / g0c;
            if (piv < minpiv) minpiv = piv;
            const double lcc = sqrt(d);
            const double rc = rc0 / lcc;
            const bool below = ln > c && ln < m;
            double lac = 0.0;
            if (ln == c) {
                r = rc;
                ldiag = lcc;
            }
            if (below) {
                lac = W[c * JS + ln] / lcc;
                W[c * JS + ln] = lac;
                r = r - lac * rc;
            }
            wave_sync();
            if (below)
                for (int bb = c + 1; bb <= ln; ++bb) W[bb * JS + ln] = W[bb * JS + ln] - lac * W[c * JS + bb];
        }
        wave_sync();
    }
    double lam_mine = 0.0;
    for (int c = m - 1; c >= 0; --c) {
        const double yc = __shfl(r, c, WAVE), lcc = __shfl(ldiag, c, WAVE);
        if (!((keepm >> c) & 1ull)) continue;
        const double lc = yc / lcc;
        if (ln == c) lam_mine = lc;
        if (ln < c) r = r - W[ln * JS + c] * lc;
    }
    lamv[ln] = lam_mine;
    wave_sync();

    // ---- the residual over the free components, a lane per component ----
    double res = 0.0;
    if (status == MPC_MU_OK)
        for (int i = ln; i < n2; i += WAVE) {
            if (!freem[i]) continue;
            double s = 0.0;
            for (int a = 0; a < m; ++a)
                if ((keepm >> a) & 1ull) s = s + lamv[a] * J[i * JS + a];
            gr_nmax(res, fabs(gradv[i] - s));
        }
    const bool resnan = __ballot(res != res) != 0;
    double resid = wave_max(res != res ? 0.0 : res);
    if (resnan) resid = qnan;

    // ---- outputs: the lam slab is assembled in J's space (every element written once), then streamed out ----
    if (lamg) {
        wave_sync();
        double* slab = J;
        for (int i = ln; i < N * rw; i += WAVE) slab[i] = 0.0;
        wave_sync();
        if (ln < m && ((keepm >> ln) & 1ull)) slab[mine] = lam_mine;
        wave_sync();
        for (int i = ln; i < N * rw; i += WAVE) lamg[(size_t)b * N * rw + i] = slab[i];
    }
    if (actg) actg[(size_t)b * MA + ln] = (na <= MA && ln < na) ? list[ln] : -1;
    if (sumg && ln == 0) mu_summary(sumg + (size_t)b * MPC_MU_NQ, status, na, nf, nu, resid, minpiv);
}
