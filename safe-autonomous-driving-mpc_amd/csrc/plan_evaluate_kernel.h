// plan_evaluate_kernel.h -- the planner's batched evaluator (plan_evaluate_chunks, include/mpcplan_evaluate.h): for any
// z = [X, U, S] the reference NLP's cost (trajectory_planning.py:128-170), Hermite-Simpson defects (:181-210),
// inequality rows (:238-349) and a per-chunk summary of them.  No QP, no solver state; included by plan.hip after
// plan_kernel.h, whose route view and wave reductions it reuses.  What a stage contributes -- its defect, cost term,
// rows and their argmin / L1 / count update -- is plan_model.h's, shared with plan_host::evaluate_one
// (plan_evaluate_host.h); here are the mapping of stages to lanes, the ordered sums and the wave reductions.
//
// One 64-lane wavefront (one workgroup) per chunk, blockIdx.x the chunk.  The horizon is not bounded by
// PLAN_MAX_N: lane l owns stages l, l + 64, ... and the wave walks the chunk in passes of 64 stages.  For stage k
// a lane computes interval k's defect (three route_kappa searches, one dyn at the midpoint), the stage's rows
// (written straight to its slice of `rows`), its cost term and its partials of the reductions; nothing per stage
// is kept in LDS beyond one pass.  Minima, maxima and counts accumulate per lane and meet in wave shuffles at the
// end.  The three sums whose bits must not depend on the mapping (COST, L1_EQ, L1_INEQ) go through a static LDS
// tile of one pass: every lane stores its stage's terms, then lanes 0, 1 and 2 each add one of the three
// sequences in order of k, carrying their running sum from pass to pass (the orders: include/mpcplan_evaluate.h).
// Row kinds are visited in a fully unrolled loop (no per-lane array indexed at run time: no scratch memory).
#pragma once
#include "../../include/mpcplan_evaluate.h"
#include "plan_kernel.h"

namespace {

constexpr int EV_TC = 0;                  // tile: cost term of stage l
constexpr int EV_TE = WAVE;               //       |defect[l][0..4]| at EV_TE + 5 l + i
constexpr int EV_TI = 6 * WAVE;           //       the stage's L1 partial of the rows
constexpr int EV_TILE = 7 * WAVE;
static_assert(EV_TILE * sizeof(double) == PLAN_EV_LDS_BYTES, "mpcplan_evaluate.h states the evaluator's LDS");

struct EArgs {
    DevRoute R;
    plan_params P;
    int B, Nmax, Nfixed;
    const int* N;
    const double *x0, *st;
    const int* fin;
    const double *X, *U, *S;
    double *sum, *def, *rows;
};

__device__ __forceinline__ bool wany(bool f) { return __ballot(f) != 0ull; }

}  // namespace

__global__ void __launch_bounds__(WAVE) plan_evaluate_kernel(EArgs a) {
    __shared__ double tile[EV_TILE];
    const int b = blockIdx.x, ln = threadIdx.x;
    const int Nmax = a.Nmax;
    const int N = a.N ? a.N[b] : a.Nfixed;
    const double inf = __builtin_inf(), qnan = __builtin_nan("");
    double* so = a.sum ? a.sum + (size_t)b * PLAN_EV_NQ : nullptr;
    if (N < 1 || N > Nmax) {                         // wave-uniform: not evaluated, nothing but the summary written
        if (so && ln < PLAN_EV_NQ) so[ln] = qnan;
        return;
    }
    const plan_params& P = a.P;
    const int fin = a.fin ? (a.fin[b] != 0) : 0;
    const double starget = a.st[b];
    const double* Xb = a.X + (size_t)b * (Nmax + 1) * 5;
    const double* Ub = a.U + (size_t)b * Nmax * 2;
    const double* Sb = a.S ? a.S + (size_t)b * Nmax : nullptr;
    double* rowb = a.rows ? a.rows + (size_t)b * (Nmax + 1) * PLAN_EV_NR : nullptr;
    double* defb = a.def ? a.def + (size_t)b * Nmax * 5 : nullptr;
    const double s_total = a.R.s_total;
    const double cden = fmax(1.0, s_total - a.x0[5 * (size_t)b]);

    // per-lane accumulators over this lane's stages (ascending k, so "first" within a lane is the smallest k)
    double rmin = inf, dmax = 0.0, vmin = inf, latmax = 0.0, slmax = 0.0, u1lo = inf, u1hi = -inf, u2lo = inf, u2hi = -inf;
    bool rnan = false, dnan = false, vnan = false, latnan = false, slnan = false, u1nan = false, u2nan = false;
    int rstage = ln, rkind = 0, nneg = 0;           // a lane's first row: stage ln, column 0
    double acc = 0.0;                                // lanes 0, 1, 2: the running COST, L1_EQ, L1_INEQ

    for (int base = 0; base <= N; base += WAVE) {
        const int k = base + ln;
        double tcost = 0.0, p1 = 0.0, ad[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
        if (k <= N) {
            double x[5];
#pragma unroll
            for (int i = 0; i < 5; ++i) x[i] = Xb[5 * (size_t)k + i];
            const bool iv = k < N;
            double u1 = 0.0, u2 = 0.0, sl = 0.0;
            if (iv) {
                double xb[5], df[5];
#pragma unroll
                for (int i = 0; i < 5; ++i) xb[i] = Xb[5 * (size_t)(k + 1) + i];
                u1 = Ub[2 * (size_t)k];
                u2 = Ub[2 * (size_t)k + 1];
                sl = Sb ? Sb[k] : 0.0;
                defect(a.R, P, x, xb, u1, u2, df);
#pragma unroll
                for (int i = 0; i < 5; ++i) {
                    ad[i] = fabs(df[i]);
                    ev_max(dmax, dnan, ad[i]);
                    if (defb) defb[5 * (size_t)k + i] = df[i];
                }
                tcost = ev_stage_cost(P, x, u1, u2, sl, s_total, cden);
                ev_max(slmax, slnan, fabs(sl));
                ev_min(u1lo, u1nan, u1);
                ev_max(u1hi, u1nan, u1);
                ev_min(u2lo, u2nan, u2);
                ev_max(u2hi, u2nan, u2);
            }
            ev_min(vmin, vnan, x[4]);
            ev_max(latmax, latnan, fabs(x[1]));

            p1 = ev_stage_rows(a.R, P, k, x, u1, u2, sl, iv, !iv && !fin, starget, rowb, rmin, rnan, rstage, rkind, nneg);
        }
        tile[EV_TC + ln] = tcost;
#pragma unroll
        for (int i = 0; i < 5; ++i) tile[EV_TE + 5 * ln + i] = ad[i];
        tile[EV_TI + ln] = p1;
        __syncthreads();
        if (ln < 3) {
            const int ni = imin(WAVE, N - base), ns = imin(WAVE, N + 1 - base);   // intervals, stages of this pass
            const int n = ln == 0 ? ni : (ln == 1 ? 5 * ni : ns);
            const int off = ln == 0 ? EV_TC : (ln == 1 ? EV_TE : EV_TI);
            for (int i = 0; i < n; ++i) acc = acc + tile[off + i];
        }
        __syncthreads();
    }

    // stages and intervals past the horizon: NaN
    if (rowb)
        for (int i = (N + 1) * PLAN_EV_NR + ln; i < (Nmax + 1) * PLAN_EV_NR; i += WAVE) rowb[i] = qnan;
    if (defb)
        for (int i = N * 5 + ln; i < Nmax * 5; i += WAVE) defb[i] = qnan;
    if (!so) return;

    // the equality rows of x_0 and of the final chunk's end (every lane: uniform loads)
    double x0res = 0.0, e0[5];
    bool x0nan = false;
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        e0[i] = fabs(Xb[i] - a.x0[5 * (size_t)b + i]);
        ev_max(x0res, x0nan, e0[i]);
    }
    const double sN = Xb[5 * (size_t)N], vN = Xb[5 * (size_t)N + 4];
    if (ln == 1) {
#pragma unroll
        for (int i = 0; i < 5; ++i) acc = acc + e0[i];
        if (fin) {
            acc = acc + fabs(sN - starget);
            acc = acc + fabs(vN);
        }
    }
    const double cost = __shfl(acc, 0, WAVE), l1eq = __shfl(acc, 1, WAVE), l1in = __shfl(acc, 2, WAVE);

    // MIN_ROW: the first NaN row if there is one, else the first row equal to the minimum
    const bool anyn = wany(rnan);
    const double m = wmin(rnan ? inf : rmin);
    const bool mine = ln <= N && (anyn ? rnan : rmin == m);     // lanes past N own no stage
    const int astage = (int)wmin(mine ? (double)rstage : 1e18);
    const int owner = astage & (WAVE - 1);
    const double mfirst = __shfl(rmin, owner, WAVE);  // the first minimum's own bits (-0.0 against 0.0)
    const int akind = __shfl(rkind, owner, WAVE);
    const int cnt = wsumi(nneg);
    const bool f_d = wany(dnan), f_v = wany(vnan), f_lat = wany(latnan), f_sl = wany(slnan), f_u1 = wany(u1nan),
               f_u2 = wany(u2nan);
    const double r_d = wmax(dmax), r_v = wmin(vmin), r_lat = wmax(latmax), r_sl = wmax(slmax), r_u1lo = wmin(u1lo),
                 r_u1hi = wmax(u1hi), r_u2lo = wmin(u2lo), r_u2hi = wmax(u2hi);
    if (ln == 0) {
        so[PLAN_EVQ_COST] = cost;
        so[PLAN_EVQ_MAX_DEFECT] = f_d ? qnan : r_d;
        so[PLAN_EVQ_L1_EQ] = l1eq;
        so[PLAN_EVQ_X0_RES] = x0nan ? qnan : x0res;
        so[PLAN_EVQ_TERM_S] = fin ? sN - starget : qnan;
        so[PLAN_EVQ_TERM_V] = fin ? vN : qnan;
        so[PLAN_EVQ_MIN_ROW] = anyn ? qnan : mfirst;
        so[PLAN_EVQ_ARGMIN_STAGE] = (double)astage;
        so[PLAN_EVQ_ARGMIN_KIND] = (double)akind;
        so[PLAN_EVQ_L1_INEQ] = l1in;
        so[PLAN_EVQ_N_NEG] = (double)cnt;
        so[PLAN_EVQ_S_FINAL] = sN;
        so[PLAN_EVQ_S_TOTAL] = s_total;
        so[PLAN_EVQ_V_FINAL] = vN;
        // + 0.0: an extreme of -0.0 and 0.0 comes out as 0.0 whichever the reduction met first
        so[PLAN_EVQ_MIN_V] = f_v ? qnan : r_v + 0.0;
        so[PLAN_EVQ_MAX_ABS_D] = f_lat ? qnan : r_lat;
        so[PLAN_EVQ_MAX_ABS_SLACK] = f_sl ? qnan : r_sl;
        so[PLAN_EVQ_U1_MIN] = f_u1 ? qnan : r_u1lo + 0.0;
        so[PLAN_EVQ_U1_MAX] = f_u1 ? qnan : r_u1hi + 0.0;
        so[PLAN_EVQ_U2_MIN] = f_u2 ? qnan : r_u2lo + 0.0;
        so[PLAN_EVQ_U2_MAX] = f_u2 ? qnan : r_u2hi + 0.0;
    }
}
