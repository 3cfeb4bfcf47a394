// plan_evaluate_host.h -- the host backend's evaluator (plan_evaluate_chunks on a device = -1 context, and
// plan_check_verdicts): what plan_evaluate_kernel (plan_evaluate_kernel.h) computes, in IEEE double, one chunk per
// task on std::thread workers.  What a stage contributes is plan_model.h's, shared with the kernel; here are the
// sequential accumulation and the thread pool.  The sums run in the orders include/mpcplan_evaluate.h states, so a chunk's
// result does not depend on B, on Nmax or on the number of workers; the comparisons (min / max / abs columns, NaN
// placement, integer columns) equal the device's bit for bit, the arithmetic differs by libm's sin / cos.
#pragma once
#include "../../include/mpcplan_evaluate.h"
#include "plan_host.h"

namespace plan_host {

// one chunk; X [N+1][5], U [N][2], S [N] or NULL (this chunk's slices); sum [PLAN_EV_NQ], def [Nmax][5],
// rows [Nmax+1][PLAN_EV_NR], each may be NULL
inline void evaluate_one(const route* rt, const plan_params* p, int N, int Nmax, const double x0[5], double starget,
                         int fin, const double* X, const double* U, const double* S, double* sum, double* def,
                         double* rows) {
    const double inf = INFINITY, qnan = NAN;
    if (N < 1 || N > Nmax) {
        if (sum)
            for (int i = 0; i < PLAN_EV_NQ; ++i) sum[i] = qnan;
        return;
    }
    fin = fin != 0;
    const double s_total = route_s_total(rt);
    const double cden = fmax(1.0, s_total - x0[0]);
    double rmin = inf, dmax = 0.0, vmin = inf, latmax = 0.0, slmax = 0.0, u1lo = inf, u1hi = -inf, u2lo = inf, u2hi = -inf;
    bool rnan = false, dnan = false, vnan = false, latnan = false, slnan = false, u1nan = false, u2nan = false;
    int rstage = 0, rkind = 0, nneg = 0;
    double cost = 0.0, l1eq = 0.0, l1in = 0.0;
    for (int k = 0; k <= N; ++k) {
        const double* x = X + 5 * (size_t)k;
        const bool iv = k < N;
        double u1 = 0.0, u2 = 0.0, sl = 0.0;
        if (iv) {
            double df[5];
            u1 = U[2 * (size_t)k];
            u2 = U[2 * (size_t)k + 1];
            sl = S ? S[k] : 0.0;
            defect(*rt, *p, x, x + 5, u1, u2, df);
            for (int i = 0; i < 5; ++i) {
                const double ad = fabs(df[i]);
                ev_max(dmax, dnan, ad);
                l1eq = l1eq + ad;
                if (def) def[5 * (size_t)k + i] = df[i];
            }
            cost = cost + ev_stage_cost(*p, x, u1, u2, sl, s_total, cden);
            ev_max(slmax, slnan, fabs(sl));
            ev_min(u1lo, u1nan, u1);
            ev_max(u1hi, u1nan, u1);
            ev_min(u2lo, u2nan, u2);
            ev_max(u2hi, u2nan, u2);
        }
        ev_min(vmin, vnan, x[4]);
        ev_max(latmax, latnan, fabs(x[1]));
        l1in = l1in + ev_stage_rows(*rt, *p, k, x, u1, u2, sl, iv, !iv && !fin, starget, rows, rmin, rnan, rstage, rkind, nneg);
    }
    if (rows)
        for (size_t i = (size_t)(N + 1) * PLAN_EV_NR; i < (size_t)(Nmax + 1) * PLAN_EV_NR; ++i) rows[i] = qnan;
    if (def)
        for (size_t i = (size_t)N * 5; i < (size_t)Nmax * 5; ++i) def[i] = qnan;
    if (!sum) return;
    double x0res = 0.0;
    bool x0nan = false;
    for (int i = 0; i < 5; ++i) {
        const double e = fabs(X[i] - x0[i]);
        ev_max(x0res, x0nan, e);
        l1eq = l1eq + e;
    }
    const double sN = X[5 * (size_t)N], vN = X[5 * (size_t)N + 4];
    if (fin) {
        l1eq = l1eq + fabs(sN - starget);
        l1eq = l1eq + fabs(vN);
    }
    sum[PLAN_EVQ_COST] = cost;
    sum[PLAN_EVQ_MAX_DEFECT] = dnan ? qnan : dmax;
    sum[PLAN_EVQ_L1_EQ] = l1eq;
    sum[PLAN_EVQ_X0_RES] = x0nan ? qnan : x0res;
    sum[PLAN_EVQ_TERM_S] = fin ? sN - starget : qnan;
    sum[PLAN_EVQ_TERM_V] = fin ? vN : qnan;
    sum[PLAN_EVQ_MIN_ROW] = rnan ? qnan : rmin;
    sum[PLAN_EVQ_ARGMIN_STAGE] = (double)rstage;
    sum[PLAN_EVQ_ARGMIN_KIND] = (double)rkind;
    sum[PLAN_EVQ_L1_INEQ] = l1in;
    sum[PLAN_EVQ_N_NEG] = (double)nneg;
    sum[PLAN_EVQ_S_FINAL] = sN;
    sum[PLAN_EVQ_S_TOTAL] = s_total;
    sum[PLAN_EVQ_V_FINAL] = vN;
    sum[PLAN_EVQ_MIN_V] = vnan ? qnan : vmin + 0.0;     // + 0.0: as the device (plan_evaluate_kernel.h)
    sum[PLAN_EVQ_MAX_ABS_D] = latnan ? qnan : latmax;
    sum[PLAN_EVQ_MAX_ABS_SLACK] = slnan ? qnan : slmax;
    sum[PLAN_EVQ_U1_MIN] = u1nan ? qnan : u1lo + 0.0;
    sum[PLAN_EVQ_U1_MAX] = u1nan ? qnan : u1hi + 0.0;
    sum[PLAN_EVQ_U2_MIN] = u2nan ? qnan : u2lo + 0.0;
    sum[PLAN_EVQ_U2_MAX] = u2nan ? qnan : u2hi + 0.0;
}

// B chunks in plan_evaluate_chunks' layout (row stride Nmax), one chunk per task over `threads` workers
inline void evaluate_batch(const route* rt, const plan_params* p, int B, int Nmax, const int* N, const double* x0,
                           const double* s_target, const int* is_final, const double* X, const double* U,
                           const double* S, double* sum, double* def, double* rows, int threads) {
    std::atomic<int> next(0);
    auto work = [&]() {
        for (;;) {
            const int b = next.fetch_add(1);
            if (b >= B) return;
            evaluate_one(rt, p, N ? N[b] : p->N, Nmax, x0 + 5 * (size_t)b, s_target[b], is_final ? is_final[b] : 0,
                         X + (size_t)b * 5 * (Nmax + 1), U + (size_t)b * 2 * Nmax, S ? S + (size_t)b * Nmax : nullptr,
                         sum ? sum + (size_t)b * PLAN_EV_NQ : nullptr, def ? def + (size_t)b * 5 * Nmax : nullptr,
                         rows ? rows + (size_t)b * PLAN_EV_NR * (Nmax + 1) : nullptr);
        }
    };
    threads = std::max(1, std::min(threads, B));
    std::vector<std::thread> pool;
    for (int t = 1; t < threads; ++t) pool.emplace_back(work);
    work();
    for (auto& t : pool) t.join();
}

// sanity_checks.plan_check_summary's verdict bits (PLAN_CHKB_*) of one summary row
inline int check_verdict(const plan_params* p, const double* q) {
    const double error_s = fabs(q[PLAN_EVQ_S_FINAL] - q[PLAN_EVQ_S_TOTAL]);
    const bool destination = !(error_s > PLAN_CHK_DISTANCE_TOL);
    const bool full_stop = !(fabs(q[PLAN_EVQ_V_FINAL]) > PLAN_CHK_VELOCITY_TOL);
    const bool forward = !(q[PLAN_EVQ_MIN_V] < -PLAN_CHK_VELOCITY_TOL);
    const bool u1_ok = !(q[PLAN_EVQ_U1_MIN] < p->u_min[0] - PLAN_CHK_CONTROLS_TOL &&
                         q[PLAN_EVQ_U1_MAX] > p->u_max[0] + PLAN_CHK_CONTROLS_TOL);
    const bool u2_ok = !(q[PLAN_EVQ_U2_MIN] < p->u_min[1] - PLAN_CHK_CONTROLS_TOL &&
                         q[PLAN_EVQ_U2_MAX] > p->u_max[1] + PLAN_CHK_CONTROLS_TOL);
    const bool lateral_ok = !(q[PLAN_EVQ_MAX_ABS_D] > PLAN_CHK_LATERAL_DEV_TOL);
    const bool slack_ok = !(q[PLAN_EVQ_MAX_ABS_SLACK] > PLAN_CHK_SLACK_TOL);
    bool passed = destination && full_stop && forward;
    if (passed) passed = u1_ok;
    if (passed) passed = u2_ok;
    passed = passed && lateral_ok && slack_ok;
    return (destination << PLAN_CHKB_DESTINATION) | (full_stop << PLAN_CHKB_FULL_STOP) | (forward << PLAN_CHKB_FORWARD) |
           (u1_ok << PLAN_CHKB_U1_OK) | (u2_ok << PLAN_CHKB_U2_OK) | (lateral_ok << PLAN_CHKB_LATERAL_OK) |
           (slack_ok << PLAN_CHKB_SLACK_OK) | (passed << PLAN_CHKB_PASSED);
}

}  // namespace plan_host
