/* mpcplan_evaluate.h — C ABI of the planner's batched evaluator (libmpcplan.so), the companion of mpcplan.h.
 *
 * The entries below live in the same library as mpcplan.h's and take its plan_ctx; there is no version step
 * (MPCPLAN_VERSION is unchanged): callers detect them by the presence of the symbols, as mpcqp.h's callers do for
 * its evaluator.  They are kept in a header of their own so that mpcplan.h stays the solver's boundary as it was.
 */
#ifndef MPCPLAN_EVALUATE_H
#define MPCPLAN_EVALUATE_H

#include "mpcplan.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- the evaluator: the reference NLP's own functions at any z = [X, U, S] ------------------------------
 * plan_evaluate_chunks computes, for B given chunk plans (from plan_solve_chunks, plan_optimize, the reference's
 * SLSQP, a file, ...), the reference's cost (trajectory_planning.py:128-170), its Hermite-Simpson defects
 * (:181-210, with the context's defect_sign) and its inequality rows (:238-349), plus a per-chunk summary.  No
 * solve, no solver state: it reads the context's dt, weights, bounds, k_min / k_max, a_max, v_min, defect_sign
 * and the route, and ignores the solver knobs.  Unlike the solver's row set (see the top of mpcplan.h) this is
 * the reference's full set: the rows of x_0 and of a final chunk's last stage included, and v_max is
 * v_max_fun at the evaluated s_k, never a frozen limit.
 *
 * Inputs in plan_solve_chunks_device's layout, row stride Nmax: X[b][Nmax+1][5], U[b][Nmax][2], S[b][Nmax]
 * (NULL: every slack zero), x0[b][5], s_target[b], is_final[b] (NULL: all intermediate), N[b] (NULL: the
 * params' N).  N[b] is NOT limited by PLAN_MAX_N: any 1 <= N[b] <= Nmax, so a whole committed trajectory is
 * evaluated as one final chunk with x0 = X[0], s_target = s_total.  A chunk whose N[b] lies outside [1, Nmax]
 * gets an all-NaN summary and no rows or defects are written for it.  B == 0 succeeds; all three outputs NULL
 * is allowed (nothing runs); any single output may be NULL.
 *
 * Outputs:
 *   defects[b][Nmax][5]            interval k's defect x_{k+1} - (x_k + sign dt/6 (f_k + 4 f_mid + f_{k+1})); NaN past N[b]
 *   rows[b][Nmax+1][PLAN_EV_NR]    stage k's rows in the reference's >= 0 sense, columns PLAN_EVR_*; NaN where the
 *                                  reference has no row (columns 6..10 at k = N, column 11 except at k = N of an
 *                                  intermediate chunk) and on stages past N[b]
 *   summary[b][PLAN_EV_NQ]         columns PLAN_EVQ_*
 *
 * Summation orders (the same on every backend and for every B and Nmax):
 *   COST      c = 0; for k = 0..N-1: c = c + (((w_y (d^2 + o^2) + w_s (e e)) + w_u (u1^2 + u2^2)) + w_slack S^2),
 *             e = (s_total - s_k) / max(1, s_total - x0[0])  (x0 the argument)
 *   L1_EQ     one running sum from 0: |defect[k][i]| for k = 0..N-1, i = 0..4 (k-major), then |X_0[i] - x0[i]|,
 *             i = 0..4, then for a final chunk |s_N - s_target|, |v_N|
 *   L1_INEQ   per stage p_k = sum over the existing columns 0..11, in column order from 0, of max(-g, 0); then one
 *             running sum from 0 of p_k for k = 0..N
 * Extremes follow numpy's NaN rule (a NaN among the inputs of a min / max gives NaN); MIN_ROW with its ARGMIN_*
 * is the first minimum in (stage, column) order over the existing rows, a NaN row winning like np.argmin.  The
 * min / max / abs columns, the NaN placement and the integer columns are bit-equal on the device and the host
 * backend; the arithmetic columns (COST, L1_*, MAX_DEFECT, defects) differ by the device's sin / cos. */
#define PLAN_EV_NR 12
enum { PLAN_EVR_VMIN, PLAN_EVR_VMAX, PLAN_EVR_LATP, PLAN_EVR_LATM, PLAN_EVR_KMIN, PLAN_EVR_KMAX, PLAN_EVR_U1MIN,
       PLAN_EVR_U1MAX, PLAN_EVR_U2MIN, PLAN_EVR_U2MAX, PLAN_EVR_S, PLAN_EVR_STERM };
/*   0 v + S_k - v_min      1 v_max_fun(s_k) - (v + S_k)  (S_N = 0)      2 a_max - k v^2      3 a_max + k v^2
 *   4 k - k_min            5 k_max - k            6..9 u1 - u_min[0], u_max[0] - u1, u2 - u_min[1], u_max[1] - u2
 *   10 S_k                 11 s_N - s_target / 2  (stage N of an intermediate chunk) */
enum { PLAN_EVQ_COST,          /* the reference's cost                                                       */
       PLAN_EVQ_MAX_DEFECT,    /* max |defect| over intervals and components                                */
       PLAN_EVQ_L1_EQ,         /* sum of the equality rows' absolute values                                 */
       PLAN_EVQ_X0_RES,        /* max |X_0 - x0|                                                            */
       PLAN_EVQ_TERM_S,        /* s_N - s_target of a final chunk, else NaN                                 */
       PLAN_EVQ_TERM_V,        /* v_N of a final chunk, else NaN                                            */
       PLAN_EVQ_MIN_ROW, PLAN_EVQ_ARGMIN_STAGE, PLAN_EVQ_ARGMIN_KIND,
       PLAN_EVQ_L1_INEQ,       /* sum of max(-g, 0)                                                         */
       PLAN_EVQ_N_NEG,         /* rows < 0                                                                  */
       /* the quantities of sanity_checks.reference_trajectory_check (sanity_checks.py:3-75) */
       PLAN_EVQ_S_FINAL,       /* X[N][0]                                                                   */
       PLAN_EVQ_S_TOTAL,       /* the route's                                                               */
       PLAN_EVQ_V_FINAL,       /* X[N][4]                                                                   */
       PLAN_EVQ_MIN_V,         /* min over stages 0..N of v                                                 */
       PLAN_EVQ_MAX_ABS_D,     /* max over stages 0..N of |d|                                               */
       PLAN_EVQ_MAX_ABS_SLACK, /* max over k < N of |S_k|                                                   */
       PLAN_EVQ_U1_MIN, PLAN_EVQ_U1_MAX, PLAN_EVQ_U2_MIN, PLAN_EVQ_U2_MAX,
       PLAN_EV_NQ };
/* static LDS of the evaluation kernel (bytes): one 64-stage tile of the three order-fixed sums' terms (cost 1,
 * |defect| 5, stage L1 1 doubles per stage), independent of Nmax; the kernel uses no scratch memory */
#define PLAN_EV_LDS_BYTES 3584

/* Host buffers, synchronous (a device context stages the inputs and copies the outputs back, as plan_optimize
 * does).  Nmax is the row stride and bounds every N[b]; with N NULL, Nmax < params N is PLAN_E_ARG. */
int plan_evaluate_chunks(plan_ctx* c, int B, int Nmax, const int* N, const double* x0, const double* s_target,
                         const int* is_final, const double* X, const double* U, const double* S,
                         double* summary, double* defects, double* rows);

/* Device pointers, asynchronous on `stream`: one kernel, no host synchronisation, no allocation, capturable
 * into a HIP graph; it shares nothing with the order-buffer pool and may overlap a solve on another stream of
 * the same context.  One 64-lane wavefront per chunk, lane l on stages l, l + 64, ...
 * Exception to the other device-pointer entries: on a host context (device = -1) this entry does not fail with
 * PLAN_E_DEVICE; it takes HOST pointers and runs synchronously on the PLAN_CPU_THREADS workers (`stream` is
 * ignored), like mpc_evaluate_batch_device of mpcqp.h. */
int plan_evaluate_chunks_device(plan_ctx* c, int B, int Nmax, const int* N, const double* x0, const double* s_target,
                                const int* is_final, const double* X, const double* U, const double* S,
                                double* summary, double* defects, double* rows, void* stream);

/* sanity_checks.plan_check_summary's verdicts (reference_trajectory_check, sanity_checks.py:3-75) from summary
 * rows, on the host (summary is a host pointer on every context).  verdicts[b] has bit PLAN_CHKB_* set when that
 * check passes; the two control checks keep the reference's AND (:48 / :54: a control check fails only when both
 * of its limits are exceeded, with the context's u_min / u_max) and PASSED its `if passed:` chaining.
 * counts[k] = chunks with bit k set.  verdicts or counts may be NULL. */
#define PLAN_CHK_DISTANCE_TOL 0.5      /* m     (:19)  */
#define PLAN_CHK_VELOCITY_TOL 0.1      /* m/s   (:27, :35) */
#define PLAN_CHK_CONTROLS_TOL 0.1      /*       (:48, :54) */
#define PLAN_CHK_LATERAL_DEV_TOL 1.5   /* m     (:59)  */
#define PLAN_CHK_SLACK_TOL 0.1         /*       (:67)  */
enum { PLAN_CHKB_DESTINATION, PLAN_CHKB_FULL_STOP, PLAN_CHKB_FORWARD, PLAN_CHKB_U1_OK, PLAN_CHKB_U2_OK,
       PLAN_CHKB_LATERAL_OK, PLAN_CHKB_SLACK_OK, PLAN_CHKB_PASSED };
int plan_check_verdicts(const plan_ctx* c, int B, const double* summary, int* verdicts, int counts[8]);

#ifdef __cplusplus
}
#endif
#endif
