/*
 * mpcqp.h — C ABI of the MI355X batched tracking-MPC solver (libmpcqp.so).
 *
 * Drop-in boundary for the reference's hot path:
 *   TrajectoryTracker.solve(x0, obstacles) -> (u0, pred_X, solve_time)
 *       medinammartin3/Safe-Autonomous-Driving-MPC  trajectory_tracking.py:213-263
 *   with its read-only state: TrajectoryTracker.__init__ params  (trajectory_tracking.py:12-47)
 *   and the reference signal  TrajectoryLoader                  (trajectory_loader.py:13-102).
 *
 * A reference-side binding (ctypes) is shown in INTEGRATION.md; the package's
 * trajectory_tracking.py is that binding.
 *
 * Conventions
 *   - all arrays are plain row-major float64 / int32, caller-owned;
 *   - per-instance solver outcomes go to status[] and never fail the call
 *     (the reference ignores SLSQP's status, trajectory_tracking.py:260-263);
 *   - API misuse returns a negative MPC_E* code and sets mpc_last_error();
 *   - a context is bound to one HIP device, or to the host backend (device = -1), and is not re-entrant.
 *   - Without a GPU, mpc_create with a device index >= 0 fails loudly (MPC_E_DEVICE); device = -1 selects the
 *     host (CPU) backend explicitly (BASELINE config 1, the reference's CPU path): the same solver, outputs
 *     and status codes on host threads (csrc/cpu_backend.h; MPC_CPU_THREADS sets the thread count).
 */
#ifndef MPCQP_H
#define MPCQP_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: status[] / hist_status[] may carry the MPC_SQP_UNCONVERGED flag (16) OR-ed onto the code; mask with
 *    MPC_STATUS_MASK before comparing with MPC_OK .. MPC_NUMERICAL (version 1 returned 0-3 only).
 * 3: the ego-shard communicator (mpc_comm_*, mpc_gather*, MPC_E_COMM); nothing else changed.
 * 4: mpc_closed_loop_sweep, mpc_cl_verdicts; nothing else changed.
 * 5: mpc_closed_loop_traffic, mpc_actors_from_fsm (mpc_actor); nothing else changed.
 *    mpc_closed_loop_convoy was added later without a version step: detect it by the presence of its symbol.
 *    So were mpc_closed_loop_noisy / mpc_noise_draw, mpc_evaluate_batch / mpc_evaluate_batch_device,
 *    mpc_closed_loop_traced, mpc_closed_loop_warm / mpc_default_warm, mpc_gradient_batch /
 *    mpc_gradient_batch_device, mpc_multipliers_batch / mpc_multipliers_batch_device and mpc_hessvec_batch /
 *    mpc_hessvec_batch_device. */
#define MPCQP_VERSION 5
#define MPC_MAX_N 63          /* horizon limit (one lane per stage k=0..N in the kernel)   */
#define MPC_MAX_OBS 64        /* obstacle slab limit per instance                            */

/* status[] codes */
#define MPC_OK 0              /* QP solved to tolerance, hard constraints satisfied          */
#define MPC_MAX_ITER 1        /* iteration limit hit; best iterate returned                  */
#define MPC_INFEASIBLE 2      /* solved, but elastic slack active: hard QP(ubar) infeasible  */
#define MPC_NUMERICAL 3       /* numerical breakdown; best iterate returned                  */
/* flag OR-ed onto the last QP's code (status & MPC_STATUS_MASK) when sqp_iters > 1 and sqp_tol > 0 and the
 * SQP stopped without a QP moving U by <= sqp_tol: the sqp_iters cap, a 2-cycle or the elastic-QP streak */
#define MPC_SQP_UNCONVERGED 16
#define MPC_STATUS_MASK 15

/* return codes */
#define MPC_SUCCESS 0
#define MPC_E_ARG (-1)
#define MPC_E_DEVICE (-2)
#define MPC_E_ALLOC (-3)
#define MPC_E_LAUNCH (-4)
#define MPC_E_COMM (-5)       /* RCCL missing or a collective failed (mpc_comm_*, mpc_gather*)   */

/* Mirrors TrajectoryTracker.__init__ (trajectory_tracking.py:17-47) plus solver knobs.
 * Field names follow the reference attributes.  mpc_default_params() fills the reference values. */
typedef struct mpc_params {
    int N;                          /* horizon                      :18 (reference default 5)  */
    int max_obs;                    /* obstacle slab width per instance in the batch arrays    */
    double dt;                      /* control period               :17                        */
    double u_min[2], u_max[2];      /* (u1 curvature rate, u2 accel) bounds   :31-32           */
    double vehicle_radius;          /* :33 */
    double w_d, w_o, w_v, w_u1, w_u2;  /* :36-40 */
    double obstacle_safety_distance;   /* :43 */
    double max_time_2_obs;          /* :44 */
    double wheelbase;               /* :45 */
    double lane_width;              /* :46 */
    double safe_lane_margin;        /* :47 */
    double brake_distance;          /* warm start: obstacle closer than this -> brake (:232, 40.0)  */
    double brake_accel;             /* warm start braking control u2 (:240, -2.0)                    */
    /* solver */
    int linearization;              /* 1 = Gauss-Newton (reference slopes, default), 0 = frozen refs  */
    int sqp_iters;                  /* QP solves per call (at most, see sqp_tol): 1 = single QP at ubar
                                       (the tracking-QP parity gate); > 1 = Gauss-Newton SQP on the
                                       reference's nonlinear problem, re-linearised about each solution;
                                       0 = no solve: U = ubar, Xpred = predict(x0, ubar)              */
    int max_iter;                   /* PDIP iteration cap per QP                                     */
    int polish;                     /* 0 off; 1 active-set polish of the interior-point result;
                                       2 (default) crossover first: the active-set solve from the
                                       unconstrained optimum, the interior point only if it fails       */
    double tol;                     /* relative primal/dual residual tolerance                        */
    double tol_mu;                  /* absolute complementarity tolerance                             */
    double elastic_rho;             /* L1 penalty of the elastic (soft) state rows                    */
    double sqp_tol;                 /* SQP stops early once a re-linearised QP moves U by at most this
                                       (max-norm), and also (sqp_tol > 0) on a 2-cycle, i.e. a QP that
                                       returns U of two QPs back (|U_k - U_k-2| <= 1e-6 |U_k - U_k-1|),
                                       and after 5 elastic (infeasible) QPs in a row; 0 = always run
                                       sqp_iters QPs                                                  */
} mpc_params;

typedef struct mpc_ctx mpc_ctx;

/* Fill p with the reference values of trajectory_tracking.py:17-47 (N=5) and solver defaults. */
void mpc_default_params(mpc_params* p);

/* Create a context on HIP device `device` (>= 0), or on the host backend (device = -1).
 * X: T x 5 reference states (s,d,o,k,v), U: Tu x 2
 * reference controls, exactly the arrays of the trajectory JSON (trajectory_loader.py:22-24);
 * the strict-monotone s fix of trajectory_loader.py:26-30 is applied here.  The table is copied
 * to device memory (owned by the context).  Replaces TrajectoryLoader(...) + TrajectoryTracker(X_ref). */
int mpc_create(const double* X, int T, const double* U, int Tu, const mpc_params* p, int device,
               mpc_ctx** out);

/* Batched TrajectoryTracker.solve (trajectory_tracking.py:213-263), host buffers, synchronous.
 *   x0     [B][5]              current states
 *   obs    [B][max_obs][2]     (s, v) of each obstacle, or NULL (no obstacles).  Passing obs with
 *                              params.max_obs == 0 is an error (MPC_E_ARG): it would ignore them.
 *   n_obs  [B]                 obstacles used per instance (<= max_obs); NULL = all max_obs rows
 *   ubar   [B][N][2] or NULL   linearization point; NULL = the reference warm start (:224-246)
 * outputs (any may be NULL):
 *   u0 [B][2], U [B][N][2], Xpred [B][N+1][5] (nonlinear predict(x0,U*), :261),
 *   status [B], iters [B]  */
int mpc_solve_batch(mpc_ctx* c, int B, const double* x0, const double* obs, const int* n_obs,
                    const double* ubar, double* u0, double* U, double* Xpred, int* status, int* iters);

/* Same, with device pointers, launched asynchronously on `stream` (a hipStream_t; 0 = null stream).
 * On a host context (device = -1) the pointers are host memory and the call is synchronous.
 * Same argument contract as mpc_solve_batch (n_obs NULL = all max_obs rows; obs with max_obs == 0 is
 * MPC_E_ARG); the double arrays must be 8-byte aligned (MPC_E_ARG otherwise); u0 and U are written
 * with 16-byte stores when both are 16-byte aligned, else with 8-byte ones.  No host synchronisation and,
 * once warmed up, no allocation (graph-capturable): the
 * two-phase work list is allocated by mpc_create for up to 2^20 instances (a larger B runs the
 * single-kernel path, same results).  The two-phase launch keeps, per deferred instance, its linearisation
 * point, nominal rollout, the crossover's solve (the interior point's start) and the trajectory lookups at
 * its stages (21N+14 doubles for even N, 21N+13 for odd) in a stage cache that grows on the first eager call with a larger B (hipMalloc, which waits for the device; at most
 * 1 GiB, MPC_STAGE_CACHE=0 switches it off); a captured call never uses it (a later eager call may grow it,
 * which would leave the graph with a freed pointer) and recomputes the start bit for bit instead.  The work
 * list belongs to the context: consecutive eager calls on one context are ordered on the device even when
 * they use different streams (a call on a new stream waits for the previous
 * call's kernels), so their results never depend on the streams chosen.  A call made while `stream` is
 * being captured into a HIP graph records no such ordering (it would tie the graph to work outside
 * it): replays of that graph must not overlap eager calls, or replays of another graph, on the same
 * context -- run them on one stream, synchronise between them, or give the graph its own context. */
int mpc_solve_batch_device(mpc_ctx* c, int B, const double* x0, const double* obs, const int* n_obs,
                           const double* ubar, double* u0, double* U, double* Xpred, int* status,
                           int* iters, void* stream);

/* Batched evaluation of the reference's own measures for ANY control sequence U (it need not come from a solve):
 * the nonlinear rollout TrajectoryTracker.predict (trajectory_tracking.py:87-114), TrajectoryTracker.cost(U, x0)
 * (:116-152) and the rows of constraints(x0, obstacles) (:155-211), with a per-instance summary.  The evaluator
 * uses the context's N, dt, weights, u_min / u_max, wheelbase, lane_width, vehicle_radius, safe_lane_margin,
 * obstacle_safety_distance and max_time_2_obs, and ignores the solver knobs.  No version step: detect it by the
 * presence of its symbol.
 *   x0 [B][5], obs [B][max_obs][2] or NULL, n_obs [B] or NULL: mpc_solve_batch's contract (obs with
 *              max_obs == 0 is MPC_E_ARG; NULL n_obs = all max_obs rows; n_obs[b] is clamped to [0, max_obs])
 *   U  [B][N][2]   required (NULL is MPC_E_ARG)
 * outputs (any may be NULL; all NULL is allowed and launches nothing):
 *   Xpred   [B][N+1][5]      predict(x0, U): the bits a solve that returned this U wrote to its Xpred
 *   summary [B][MPC_EV_NQ]   the MPC_EVQ_* columns below
 *   terms   [B][5]           the cost shares (d, o, v, u1, u2), each summed over its stages in order; informative:
 *                            they need not add up to MPC_EVQ_COST bit for bit
 *   rows    [B][N][7 + max_obs]   stage k = 1..N is row k - 1; columns 0..5 the six lane rows in the reference's
 *                            order (sl - d, d + sl, sl - f, f + sl, sl - l, l + sl with f = d + (wheelbase / 2) o,
 *                            l = d + wheelbase o, sl = lane_width / 2 - vehicle_radius - safe_lane_margin);
 *                            column 6 is v; column 7 + i is obstacle i:
 *                            (s_obs + v_obs * (k * dt) - s) - max(obstacle_safety_distance, v * max_time_2_obs)
 *                            with the reference's max (the first argument unless the second is greater); NaN past
 *                            n_obs.  The reference's vector has, per stage, the lane rows, the obstacle rows, then v.
 * Summation orders (the results do not depend on the backend, the lane-group width or B):
 *   cost   one running sum from 0: for k = 1..N  + w_d (d - d_ref)^2, + w_o (o - o_ref)^2, + w_v (v - v_ref)^2
 *          with the references looked up at the rolled-out s_k; then for k = 0..N-1  + w_u1 u1^2, + w_u2 u2^2
 *   L1     per stage the sum of max(-g, 0) over its rows in the reference's order, from 0; the stage partials are
 *          then added for k = 1..N, from 0
 * Misuse is MPC_E_ARG with a message; B == 0 succeeds. */
#define MPC_EVQ_COST 0           /* TrajectoryTracker.cost(U, x0)                                              */
#define MPC_EVQ_MIN_ROW 1        /* np.min over the reference-order row vector (NaN if a row is NaN)           */
#define MPC_EVQ_ARGMIN_STAGE 2   /* its stage 1..N: np.argmin's row (the first minimum; the first NaN row)     */
#define MPC_EVQ_ARGMIN_KIND 3    /* its kind: 0..5 the lane rows, 6 the v >= 0 row, 7 + i obstacle i           */
#define MPC_EVQ_L1 4             /* sum of max(-g, 0) over all rows (NaN if a row is NaN)                      */
#define MPC_EVQ_N_NEG 5          /* rows with g < 0                                                            */
#define MPC_EVQ_MIN_LANE 6       /* minima per row family, numpy's min (NaN if a row of the family is NaN);    */
#define MPC_EVQ_MIN_OBS 7        /*   MIN_OBS is NaN when the instance has no obstacle                         */
#define MPC_EVQ_MIN_V 8
#define MPC_EVQ_BOX 9            /* max over k and component of max(u_min - u, u - u_max, 0): the excess over
                                    the bounds the reference hands SLSQP (:249-252); NaN if a control is NaN    */
#define MPC_EV_NQ 10
int mpc_evaluate_batch(mpc_ctx* c, int B, const double* x0, const double* obs, const int* n_obs, const double* U,
                       double* Xpred, double* summary, double* terms, double* rows);
/* Same, with device pointers, launched asynchronously on `stream` (a hipStream_t; 0 = null stream): one kernel,
 * no host synchronisation, no allocation, graph-capturable.  The double arrays must be 8-byte aligned (MPC_E_ARG
 * otherwise); n_obs without obs is MPC_E_ARG like mpc_solve_batch_device.  The call shares no state with the
 * solver's work list or stage cache, so it may overlap a solve on another stream of the same context.  On a host
 * context (device = -1) the pointers are host memory and the call is synchronous; every output equals the
 * device's bit for bit. */
int mpc_evaluate_batch_device(mpc_ctx* c, int B, const double* x0, const double* obs, const int* n_obs,
                              const double* U, double* Xpred, double* summary, double* terms, double* rows,
                              void* stream);

/* Batched gradients of what mpc_evaluate_batch computes, at ANY control sequence U: the gradient of
 * TrajectoryTracker.cost(U, x0) in U and in x0, and J' lam for the rows of constraints(x0, obstacles) weighted by
 * lam, by one reverse (adjoint) sweep each over the rollout predict(x0, U) -- exact, where the reference's SLSQP
 * differences 2N + 1 rollouts.  The function differentiated is the evaluator's: the table is piecewise linear and
 * its slope at s is that of the interval the lookup selects (the left one at a knot, 0 for s >= s_max); the safe
 * distance max(obstacle_safety_distance, v * max_time_2_obs) has slope max_time_2_obs in v only where
 * v * max_time_2_obs > obstacle_safety_distance (the reference's max).  The solver knobs (linearization too) are
 * ignored.  No version step: detect it by the presence of its symbol.
 *   x0, obs, n_obs, U   mpc_evaluate_batch's contract exactly
 *   lam [B][N][7 + max_obs] or NULL   row weights in the layout of `rows`; columns >= 7 + n_obs[b] are never read
 *                       (a `rows`-shaped array with NaN there is fine)
 * outputs (any may be NULL; all NULL is allowed and launches nothing; jtl without lam is MPC_E_ARG):
 *   grad    [B][N][2]   d cost / d u_k, k = 0..N-1
 *   jtl     [B][N][2]   sum over stages and rows of lam * d g / d u_k (J' lam)
 *   gx0     [B][5]      d cost / d x0
 *   costate [B][N][5]   p_1..p_N of the cost: p_k = d cost / d x_k with the later stages folded in
 *   summary [B][MPC_GR_NQ]   the MPC_GRQ_* columns below
 * With x_k = (s, d, o, k, v) the rollout, e_d = d - d_ref(s) (e_o, e_v alike) and d_ref' the table slope at s:
 *   q_k  (k = 1..N)  = (-((2 w_d e_d d_ref' + 2 w_o e_o o_ref') + 2 w_v e_v v_ref'), 2 w_d e_d, 2 w_o e_o, 0,
 *                      2 w_v e_v) with 2 w_d e_d = (2 w_d) * e_d
 *   p_N = q_N;  p_k = q_k + A_k' p_k+1 for k = N-1..1, each component one addition q_k[i] + (A_k' p_k+1)[i];
 *   A_k' p = (p_s + a20 p_o, p_d, p_o + a12 p_d, p_k + a23 p_o, ((p_v + dt p_s) + a14 p_d) + a24 p_o) with
 *        a12 = dt v, a14 = dt o, a20 = dt (-v k_ref'), a23 = dt v, a24 = dt (k - k_ref) at x_k
 *   grad[k] = ((2 w_u1) u1_k + dt p_k+1[3], (2 w_u2) u2_k + dt p_k+1[4]);   gx0 = A_0' p_1
 *   the row side repeats the sweep with q_k replaced by c_k = sum_r lam[k][r] grad_x g_k,r: per component one
 *        running sum from 0 over the rows in the reference's order (the six lane rows, the obstacles, v) that skips
 *        the rows whose coefficient in that component is structurally zero, adding lam * coefficient (lam itself
 *        where the coefficient is +-1); jtl[k] = dt (p'_k+1[3], p'_k+1[4])
 * The results do not depend on the backend, the lane-group width or B; a NaN in one instance's inputs stays in
 * that instance.  In the summary a NaN enters a maximum or minimum and stays (numpy's rule).
 * Misuse is MPC_E_ARG with a message; B == 0 succeeds. */
#define MPC_GRQ_COST 0           /* the same bits as MPC_EVQ_COST                                              */
#define MPC_GRQ_GRAD_INF 1       /* max |grad|                                                                 */
#define MPC_GRQ_LAG_INF 2        /* max |grad - jtl|; equals GRAD_INF when lam is NULL                         */
#define MPC_GRQ_PG_INF 3         /* max over components of |clamp(u - r, u_min, u_max) - u| with r = grad - jtl:
                                    the projected-gradient measure for the bounds handed to SLSQP              */
#define MPC_GRQ_COMPL 4          /* max |lam * g| over the rows read; NaN without lam                          */
#define MPC_GRQ_MIN_LAM 5        /* min lam over the rows read; NaN without lam                                */
#define MPC_GR_NQ 6
int mpc_gradient_batch(mpc_ctx* c, int B, const double* x0, const double* obs, const int* n_obs, const double* U,
                       const double* lam, double* grad, double* jtl, double* gx0, double* costate, double* summary);
/* Same, with device pointers, launched asynchronously on `stream`: one kernel, no host synchronisation, no
 * allocation, graph-capturable.  The double arrays must be 8-byte aligned (MPC_E_ARG otherwise).  The call shares
 * no state with the solver, so it may overlap a solve on another stream of the same context.  On a host context
 * (device = -1) the pointers are host memory and the call is synchronous; every output equals the device's bit for
 * bit. */
int mpc_gradient_batch_device(mpc_ctx* c, int B, const double* x0, const double* obs, const int* n_obs,
                              const double* U, const double* lam, double* grad, double* jtl, double* gx0,
                              double* costate, double* summary, void* stream);

/* Batched multiplier estimates for the rows of constraints(x0, obstacles) at ANY control sequence U: the least-squares
 * lam of  grad = J' lam  over the active rows and the controls off their bounds, where grad is mpc_gradient_batch's
 * cost gradient and J the Jacobian of the rows.  Only (x0, obs, U) enter: no solver state.  The output lam can be
 * handed to mpc_gradient_batch as it is.  No version step: detect it by the presence of its symbol.
 *   x0, obs, n_obs, U   mpc_evaluate_batch's contract exactly
 *   active_tol          a row is active when g <= active_tol (may be negative; NaN is MPC_E_ARG)
 *   bound_tol           component c of control k is free iff u_min[c] + bound_tol < u < u_max[c] - bound_tol
 *   rank_tol            the drop rule of the factorisation (below); bound_tol and rank_tol negative or NaN are MPC_E_ARG
 * outputs (any may be NULL; all NULL is allowed and launches nothing):
 *   lam     [B][N][7 + max_obs]   the layout of `rows`; every element is written, 0.0 wherever no multiplier is
 *                                 estimated (columns past n_obs too).  Either sign, as least squares gives it
 *   active  [B][MPC_MAX_ACTIVE]   the active rows in list order as (stage - 1) * (7 + max_obs) + column; -1 past
 *                                 N_ACTIVE; all -1 on MPC_MU_OVERFLOW
 *   summary [B][MPC_MU_NQ]        the MPC_MUQ_* columns below
 * Per instance, with every sum in the stated order (the results do not depend on the backend or on B; a NaN stays in
 * its instance; the host backend and the device agree bit for bit):
 *   1  the rollout, the rows and grad are mpc_evaluate_batch's and mpc_gradient_batch's, the same bits
 *   2  the active list takes the rows with g <= active_tol (a NaN row is never active) in the reference's order:
 *      stage 1..N, within a stage the six lane rows, obstacles 0..n_obs-1, then v.  N_ACTIVE is their number; with
 *      more than MPC_MAX_ACTIVE the status is MPC_MU_OVERFLOW and lam is zero
 *   3  N_FREE counts the free components i = 2k + c.  N_ACTIVE > 0 with N_FREE == 0 is MPC_MU_NO_FREE, lam zero
 *   4  j_a = J' e_a [2N] of active row a at stage t: p_t = grad_x g of that row alone (the coefficients of
 *      mpc_gradient_batch's c_k for a unit weight), p_k = A_k' p_k+1 for k = t-1..1, j_a[2k + c] = dt p_k+1[3 + c] for
 *      k < t and 0 for k >= t: jtl of a unit-lam call under ==.  If grad or a j_a is not finite on a free component,
 *      or a row of the instance is NaN, the status is MPC_MU_NONFINITE and lam is zero
 *   5  G[a][b] = sum_i j_a[i] j_b[i] and r[a] = sum_i j_a[i] grad[i], each one running sum from 0 over the free i
 *      in increasing order
 *   6  Cholesky in list order with a drop rule.  For c = 0, 1, ...: d = G[c][c] - sum L[c][e]^2 over the kept e < c,
 *      subtracted one by one in increasing e.  Row c is dropped (lam 0, no part in anything later) when
 *      !(d > rank_tol * G[c][c]) with the original diagonal; else L[c][c] = sqrt(d) and, for a > c,
 *      L[a][c] = (G[a][c] - sum L[a][e] L[c][e]) / L[c][c] with the same subtraction order.  Forward substitution
 *      y_c = (r[c] - sum L[c][e] y_e) / L[c][c], increasing e; back substitution lam_c = (y_c - sum L[e][c] lam_e)
 *      / L[c][c] over the kept e > c, subtracted in decreasing e.  This picks independent rows greedily in the
 *      reference's order; on a full-rank list it is the least-squares solution
 * Misuse is MPC_E_ARG with a message; B == 0 succeeds. */
#define MPC_MAX_ACTIVE 64
#define MPC_MU_OK 0              /* also an empty active list (lam zero)                                       */
#define MPC_MU_OVERFLOW 1        /* more than MPC_MAX_ACTIVE active rows; N_ACTIVE carries the true count      */
#define MPC_MU_NO_FREE 2         /* active rows but every control component on a bound                         */
#define MPC_MU_NONFINITE 3       /* grad or a row gradient is not finite on a free component, or a row is NaN  */
#define MPC_MUQ_STATUS 0
#define MPC_MUQ_N_ACTIVE 1
#define MPC_MUQ_N_FREE 2
#define MPC_MUQ_N_USED 3         /* the rows kept by the drop rule (0 unless the status is MPC_MU_OK)          */
#define MPC_MUQ_RESID 4          /* max over the free i of |grad[i] - sum_a lam_a j_a[i]|, the sum from 0 over the
                                    kept a in list order; NaN unless the status is OK; 0 with no free component */
#define MPC_MUQ_MIN_PIVOT 5      /* the least d / G[c][c] over the kept rows; NaN if none is kept              */
#define MPC_MU_NQ 6
int mpc_multipliers_batch(mpc_ctx* c, int B, const double* x0, const double* obs, const int* n_obs, const double* U,
                          double active_tol, double bound_tol, double rank_tol, double* lam, int* active,
                          double* summary);
/* Same, with device pointers, launched asynchronously on `stream`: one kernel (one wavefront per instance), no host
 * synchronisation, no allocation, graph-capturable.  The double arrays must be 8-byte aligned (MPC_E_ARG otherwise);
 * n_obs without obs is MPC_E_ARG.  The call shares no state with the solver, so it may overlap a solve on another
 * stream of the same context.  On a host context (device = -1) the pointers are host memory and the call is
 * synchronous; every output equals the device's bit for bit. */
int mpc_multipliers_batch_device(mpc_ctx* c, int B, const double* x0, const double* obs, const int* n_obs,
                                 const double* U, double active_tol, double bound_tol, double rank_tol, double* lam,
                                 int* active, double* summary, void* stream);

/* Batched Hessian-vector products and row tangents of what mpc_evaluate_batch computes, at ANY control sequence U:
 * for M directions v in U per instance, (d2 L / dU2) v with L = cost - lam . g (the sign convention of
 * MPC_GRQ_LAG_INF; L = cost when lam is NULL) and J v, the directional derivative of every row -- exact, by one
 * forward tangent chain and one second-order reverse chain per direction over the rollout predict(x0, U).  The function
 * differentiated is the evaluator's, as for mpc_gradient_batch: the table is piecewise linear with the lookup's
 * interval, and the obstacle max follows v only where v * max_time_2_obs > obstacle_safety_distance.  Hence every row
 * and every reference has zero second derivative, and H consists of the cost's own Hessian and of the bilinear dynamics
 * (v o, v (k - k_ref(s))) weighted by the costate.  No version step: detect it by the presence of its symbol.
 *   x0, obs, n_obs, U, lam   mpc_gradient_batch's contract exactly (lam may be NULL; columns >= 7 + n_obs[b] are never
 *                       read)
 *   M, V [B][M][N][2]   the directions, 1 <= M <= MPC_HV_MAX_DIRS.  V NULL: direction m is the unit vector e_m
 *                       (m = 2k + c) and M <= 2N is required; M = 2N then yields the dense Hessian (HV[b][m] is its
 *                       row and column m) and the dense row Jacobian (JV[b][m] is its column m) in one call
 *   mode                MPC_HV_EXACT or MPC_HV_GAUSS_NEWTON (anything else is MPC_E_ARG)
 * outputs (any may be NULL; all NULL is allowed and launches nothing):
 *   HV   [B][M][N][2]             H v
 *   JV   [B][M][N][7 + max_obs]   J v in the layout of `rows`, NaN past n_obs
 *   curv [B][M][2]                (v'Hv, v'v), each one running sum from 0 over i = 0..2N-1 (i = 2k + c): + v_i HV_i,
 *                                 + v_i v_i
 *   summary [B][MPC_HV_NQ]        the MPC_HVQ_* columns below
 * Per instance and direction, with x_k the rollout, a12..a24 mpc_gradient_batch's coefficients of A_k at x_k and
 * d_ref', o_ref', k_ref', v_ref' the table slopes at s_k:
 *   1  the rollout, A_k, q_k, c_k and both reverse sweeps are mpc_gradient_batch's, the same bits.  The Lagrangian
 *      costate is pi_k = p_k - p'_k for k = 1..N, one subtraction per component; without lam it is p_k
 *   2  tangent: dx_0 = 0; dx_k+1 = A_k dx_k + dt (0, 0, 0, v1_k, v2_k), by components
 *        ds + dt dv;  (dd + a12 do) + a14 dv;  ((do + a20 ds) + a23 dk) + a24 dv;  dk + dt v1;  dv + dt v2
 *   3  JV[m][k-1][col] = grad_x g_k,col . dx_k with the coefficients of mpc_multipliers_batch's step 4: the lane rows
 *      dd + c do (c = 0, wheelbase / 2, wheelbase per pair; c do is formed only where c is not 0), negated for the even
 *      columns; column 6 is dv; obstacle columns -ds, and (-ds) - max_time_2_obs dv where the max follows v
 *   4  second-order reverse sweep: dpi_N = Q_N dx_N; dpi_k = (Q_k dx_k + A_k' dpi_k+1) + E_k for k = N-1..1, one
 *      addition each per component, A_k' as in mpc_gradient_batch.  With t_d = (2 w_d) (dd - d_ref' ds), t_o and t_v
 *      alike:  Q_k dx = (-((t_d d_ref' + t_o o_ref') + t_v v_ref'), t_d, t_o, 0, t_v).
 *      E_k = (dA_k[dx_k])' pi_k+1 = (da20 pi[2], 0, da12 pi[1], da23 pi[2], da14 pi[1] + da24 pi[2]) with
 *      da12 = dt dv, da14 = dt do, da20 = dt (-dv k_ref'), da23 = dt dv, da24 = dt (dk - k_ref' ds) at x_k.
 *      In MPC_HV_GAUSS_NEWTON mode E_k is left out and lam does not enter HV: the curvature of the cost with the
 *      dynamics linearised.  JV does not depend on the mode
 *   5  HV[m][k] = ((2 w_u1) v1_k + dt dpi_k+1[3], (2 w_u2) v2_k + dt dpi_k+1[4])
 * The results do not depend on the backend, on B, on M or on which other directions are in the call; a NaN stays in
 * its instance and its direction.  Misuse is MPC_E_ARG with a message; B == 0 succeeds. */
#define MPC_HV_MAX_DIRS 128
#define MPC_HV_EXACT 0
#define MPC_HV_GAUSS_NEWTON 1
/* The device kernel carries 64 directions per pass of a wavefront for N <= MPC_HV_N64_MAX and 32 beyond; its LDS in
 * doubles is 30 N + 10 + 2 MPC_HV_MAX_DIRS for the instance and 5 N (W + 1) for the W directions of a pass:
 *   N = 20, W = 64:  58.9 KB (two workgroups per CU)     N = 56, W = 64: 161.2 KB     N = 63, W = 32: 100.4 KB
 * The results do not depend on the pass width. */
#define MPC_HV_N64_MAX 56
#define MPC_HVQ_COST 0           /* the same bits as MPC_EVQ_COST                                              */
#define MPC_HVQ_MIN_RAYLEIGH 1   /* min over m of v'Hv / v'v; numpy's rule: a NaN enters and stays, 0 / 0 is NaN */
#define MPC_HVQ_MAX_RAYLEIGH 2   /* max over m of the same                                                     */
#define MPC_HVQ_ARGMIN_DIR 3     /* np.argmin's direction: the first minimising m, or the first NaN one        */
#define MPC_HVQ_N_NEG 4          /* the number of directions with v'Hv < 0                                     */
#define MPC_HV_NQ 5
int mpc_hessvec_batch(mpc_ctx* c, int B, const double* x0, const double* obs, const int* n_obs, const double* U,
                      const double* lam, int M, const double* V, int mode, double* HV, double* JV, double* curv,
                      double* summary);
/* Same, with device pointers, launched asynchronously on `stream`: one kernel (one wavefront per instance), no host
 * synchronisation, no allocation, graph-capturable.  The double arrays must be 8-byte aligned (MPC_E_ARG otherwise);
 * n_obs without obs is MPC_E_ARG.  The call shares no state with the solver, so it may overlap a solve on another
 * stream of the same context.  On a host context (device = -1) the pointers are host memory and the call is
 * synchronous; every output equals the device's bit for bit. */
int mpc_hessvec_batch_device(mpc_ctx* c, int B, const double* x0, const double* obs, const int* n_obs,
                             const double* U, const double* lam, int M, const double* V, int mode, double* HV,
                             double* JV, double* curv, double* summary, void* stream);

/* Reference-signal service on the device table: TrajectoryLoader.get_state / get_control
 * (trajectory_loader.py:86-102), batched. Host buffers, synchronous.  out_state [n][5], out_control [n][2]. */
int mpc_lookup(mpc_ctx* c, int n, const double* s, double* out_state, double* out_control);

/* TrajectoryLoader.get_global_pose(s, d) (trajectory_loader.py:104-116), batched: Frenet (s, d) ->
 * global (x, y, psi) of the reference line built at mpc_create (trajectory_loader.py:32-62).
 * Host buffers, synchronous.  out [n][3]. */
int mpc_global_pose(mpc_ctx* c, int n, const double* s, const double* d, double* out);

/* Read a trajectory JSON in the reference's format ({"X": [[s,d,o,k,v],...], "U": [[u1,u2],...]},
 * trajectory_loader.py:13-24; other keys ignored).  Two-call pattern: with X == U == NULL only the
 * sizes T, Tu are returned; then X [T][5] and U [Tu][2] (capacities maxT, maxTu rows) are filled.
 * Host only, no device needed.  A missing file is MPC_E_ARG ("File not found : <path>."). */
int mpc_read_trajectory_json(const char* path, double* X, int maxT, double* U, int maxTu, int* T, int* Tu);

/* mpc_read_trajectory_json + mpc_create: replaces TrajectoryLoader(json_file) + TrajectoryTracker(X_ref). */
int mpc_create_from_json(const char* path, const mpc_params* p, int device, mpc_ctx** out);

/* Change parameters of an existing context (e.g. TrajectoryTracker.N = 20 after construction). */
int mpc_set_params(mpc_ctx* c, const mpc_params* p);
int mpc_get_params(const mpc_ctx* c, mpc_params* p);

/* ObstaclesFSM (trajectory_tracking.py:266-374): one dynamic car and one traffic light per ego.
 * mpc_default_fsm() fills the trajectory2.json preset (:292-308) with both scenarios off. */
typedef struct mpc_fsm {
    int dynamic_obstacle, traffic_light;                        /* :286-288                   */
    double obs_trigger_s, obs_start_s, obs_v, obs_end_s;        /* dynamic obstacle, :293-297 */
    double tl_pos, tl_trigger_s, tl_stop_duration;              /* traffic light, :302-304    */
} mpc_fsm;

void mpc_default_fsm(mpc_fsm* f);

/* Batched closed loop: run_simulation (trajectory_tracking.py:377-443) for B independent egos on the
 * device.  Per step: ObstaclesFSM.update(dt, s, v) per ego, one batched solve, the Euler plant step
 * x <- x + dt*dynamics(x, u0, k_ref(s)) (:403-406).  An ego leaves the loop once s > s_stop (the
 * reference runs while s <= s_max - 1, :395); the call returns when every ego has left or after
 * max_steps.  fsm may be NULL (no obstacles).  Host buffers (any history may be NULL):
 *   x_init [B][5]; hist_x [B][max_steps+1][5] (row 0 = x_init); hist_u [B][max_steps][2];
 *   hist_obs_s [B][max_steps] (car position, NaN if none); hist_tl [B][max_steps] (0 RED, 1 GREEN);
 *   hist_status [B][max_steps] (solver status); n_steps [B] (steps each ego ran; required);
 *   step_ms [max_steps] (wall time of each batched step on the device, NaN for steps not run).
 * Entries past an ego's n_steps are NaN (doubles) / -1 (ints). */
int mpc_closed_loop(mpc_ctx* c, int B, const double* x_init, const mpc_fsm* fsm, int max_steps, double s_stop,
                    double* hist_x, double* hist_u, double* hist_obs_s, int* hist_tl, int* hist_status,
                    int* n_steps, double* step_ms);

/* Closed-loop scenario sweep: mpc_closed_loop with a scenario per ego, the acceptance-check quantities
 * accumulated while the loop runs, and histories only for the egos the caller names.  Ego b's loop is
 * exactly mpc_closed_loop's loop with scenario fsm[b] (same FSM transitions, slab order, solver launch,
 * Euler plant, arithmetic order and exit test); nothing the call allocates grows with B * max_steps.
 *
 * Columns of the per-ego summary quant [B][MPC_CL_NQ]; 0..10 are shard.CL_FIELDS in its order, and every
 * row equals shard.closed_loop_quantities on that ego's full histories (a NaN state or control propagates
 * into the extreme like numpy's max / min; an ego that never ran has its initial s and |d|, zeros and a NaN
 * gap). */
#define MPC_CLQ_EGO 0            /* b (the caller adds its shard offset)                                  */
#define MPC_CLQ_N_STEPS 1
#define MPC_CLQ_S_FINAL 2
#define MPC_CLQ_MAX_DEV 3        /* max |d| over the initial state and every state reached                */
#define MPC_CLQ_U1_MIN 4
#define MPC_CLQ_U1_MAX 5
#define MPC_CLQ_U2_MIN 6
#define MPC_CLQ_U2_MAX 7
#define MPC_CLQ_MAX_STEP_MS 8    /* max of step_ms over the steps this ego ran (0 if none)                */
#define MPC_CLQ_MIN_OBS_DIST 9   /* min (car_s - s) over steps with a car, s the state before the step;
                                    NaN if never                                                          */
#define MPC_CLQ_RED_PASS 10      /* 1.0: the first state with s > tl_pos was reached while RED (decided at
                                    the first step that starts from such a state, with that step's light
                                    after the FSM update; a first crossing at the final state does not
                                    count)                                                                */
#define MPC_CLQ_N_INFEASIBLE 11  /* steps whose (status & MPC_STATUS_MASK) == MPC_INFEASIBLE              */
#define MPC_CLQ_N_NOT_OK 12      /* steps whose masked status != MPC_OK                                   */
#define MPC_CL_NQ 13

/*   fsm, n_fsm   n_fsm == B: fsm[b] is ego b's scenario; n_fsm == 1: one scenario shared by all; fsm NULL
 *                with n_fsm == 0: none.  The solver runs with an obstacle slab of 2 when any ego's scenario
 *                has a switch on; an ego whose own scenario has both off gets no obstacle, records NaN for
 *                the car and 0 (RED) for the light, like mpc_closed_loop without scenarios.
 *   quant        [B][MPC_CL_NQ], required.
 *   hist_egos    [n_hist] egos whose histories are kept: distinct, in [0, B).  hist_x .. hist_status are
 *                [n_hist][...] with mpc_closed_loop's per-ego layout, row k for ego hist_egos[k]; any may be
 *                NULL, all must be NULL when n_hist == 0.
 *   n_steps [B], step_ms [max_steps]: optional here.  Step times are always taken (a small ring of events
 *                read at the every-8-steps host sync); MPC_CLQ_MAX_STEP_MS is max(step_ms[:n_steps[b]]).
 * Misuse (n_fsm not in {0 with NULL, 1, B}, quant NULL, n_hist < 0, a history pointer with n_hist == 0, an
 * index out of range or repeated) is MPC_E_ARG. */
int mpc_closed_loop_sweep(mpc_ctx* c, int B, const double* x_init, const mpc_fsm* fsm, int n_fsm, int max_steps,
                          double s_stop, double* quant, int n_hist, const int* hist_egos, double* hist_x,
                          double* hist_u, double* hist_obs_s, int* hist_tl, int* hist_status, int* n_steps,
                          double* step_ms);

/* The verdicts of the restated acceptance check (the package's sanity_checks.py, check_verdicts, which
 * restates the reference's sanity_checks.py:79-184) from the sweep's quantities.  The constants are those of
 * sanity_checks.py: LATERAL_LIMIT, CONTROLS_TOL, CPU_LIMIT, SAFETY_DIST, and the 1 m of the destination
 * check (:97-103). */
#define MPC_CL_DEST_TOL 1.0          /* destination: not (s_final < s_total - 1.0)            */
#define MPC_CL_LATERAL_LIMIT 1.5     /* on road: not (max |d| > 1.5 m)                        */
#define MPC_CL_CONTROLS_TOL 0.1      /* controls within the context's u_min / u_max -+ 0.1    */
#define MPC_CL_STEP_MS_LIMIT 150.0   /* real time: not (max step time > 150 ms)               */
#define MPC_CL_SAFETY_DIST 1.0       /* car: no gap, or not (min gap < 1.0 m)                 */
/* verdict bits, in check_verdicts' order */
#define MPC_CLV_DESTINATION 1
#define MPC_CLV_ON_ROAD 2
#define MPC_CLV_STEER_OK 4
#define MPC_CLV_ACCEL_OK 8
#define MPC_CLV_REALTIME 16
#define MPC_CLV_OBSTACLE_OK 32
#define MPC_CLV_LIGHT_OK 64
#define MPC_CLV_PASSED 128           /* all of the above                                      */
/* Host only.  quant [B][MPC_CL_NQ]; verdicts [B] bitmask (may be NULL); counts[k] = egos with bit 1 << k set
 * (may be NULL).  The control bounds are the context's u_min / u_max. */
int mpc_cl_verdicts(const mpc_ctx* c, int B, const double* quant, double s_total, int* verdicts, int counts[8]);

/* Closed-loop traffic scripts: mpc_closed_loop_sweep with up to MPC_MAX_ACTORS obstacles per ego.  Each ego
 * runs a script of A actors; an actor is a car or a light with the per-obstacle state machine of ObstaclesFSM
 * (trajectory_tracking.py:338-372: "each obstacle has its own FSM") and its own state.  MPC_ACTOR_NONE is a
 * placeholder that emits nothing and has no state. */
#define MPC_ACTOR_NONE 0
#define MPC_ACTOR_CAR 1
#define MPC_ACTOR_LIGHT 2
#define MPC_MAX_ACTORS 16
typedef struct mpc_actor {
    int kind;
    double trigger_s;      /* car: obs_trigger_s (ego position that spawns it); light: tl_trigger_s (distance) */
    double pos_s;          /* car: obs_start_s; light: tl_pos                                                   */
    double v;              /* car: obs_v                                                                        */
    double end_s;          /* car: obs_end_s                                                                    */
    double stop_duration;  /* light: tl_stop_duration                                                           */
} mpc_actor;

/* The two actors that restate an mpc_fsm: out[0] the car (NONE if dynamic_obstacle is off), out[1] the light
 * (NONE if traffic_light is off).  Fields an actor kind does not use are 0. */
void mpc_actors_from_fsm(const mpc_fsm* f, mpc_actor out[2]);

/* Columns of the optional per-ego extra [B][MPC_TR_NX] of mpc_closed_loop_traffic. */
#define MPC_TRX_MAX_NOBS 0        /* largest slab count the ego saw                                          */
#define MPC_TRX_N_RED_PASS 1      /* lights passed on red                                                    */
#define MPC_TRX_MIN_GAP_ACTOR 2   /* index of the actor behind MPC_CLQ_MIN_OBS_DIST (-1.0: no car ever
                                     emitted); on ties the earliest step, then the lowest index              */
#define MPC_TR_NX 3

/* Per step, for an ego still in the loop, the actors are visited in index order on the state before the step
 * (s, v), with the arithmetic and tests of ObstaclesFSM.update applied to that actor's own state:
 *   car    triggers once, when s >= trigger_s; while active its position advances by v * dt from pos_s; past
 *          end_s it goes inactive for good, otherwise it appends (position, v) to the slab;
 *   light  while RED and 0 < pos_s - s < trigger_s it appends (pos_s, 0) and sets its waiting flag when
 *          v < 0.1 and the distance is < 10; while waiting its timer advances by dt; GREEN at
 *          timer >= stop_duration.
 * The slab holds the emitted entries in actor order and n_obs is their count.  When any actor of any script is
 * not NONE the solver runs with max_obs = A on the obstacle kernels, otherwise with no slab (like the sweep
 * without scenarios); an ego whose own actors are all NONE gets n_obs = 0.  The plant, the exit test, the list
 * compaction every 8 steps and the step timing are mpc_closed_loop_sweep's.
 *   actors, A, n_scripts   [n_scripts][A], 0 <= A <= MPC_MAX_ACTORS; n_scripts == B: a script per ego;
 *                n_scripts == 1: one shared script; actors NULL with A == 0 and n_scripts == 0: none.
 *   quant        [B][MPC_CL_NQ], required; the sweep's columns (mpc_cl_verdicts reads it unchanged).
 *                MPC_CLQ_MIN_OBS_DIST is the running minimum of position - s over every step and every car
 *                that emitted at that step (actor order within a step; the sweep's NaN rule; NaN if never);
 *                MPC_CLQ_RED_PASS is 1.0 if any light was passed on red, each light decided once, at the first
 *                step that starts with s > pos_s, with that light's colour after this step's update.
 *   extra        [B][MPC_TR_NX], optional.
 *   hist_egos .. as in the sweep.  hist_car_s [n_hist][max_steps]: the first car in the slab, NaN if none;
 *                hist_tl [n_hist][max_steps]: bit a is set when actor a is a light that is GREEN after this
 *                step's update; hist_nobs [n_hist][max_steps]; hist_slab [n_hist][max_steps][A][2]: this
 *                step's slab, NaN past n_obs.  Tails are NaN / -1.  n_steps, step_ms: optional.
 * Misuse (A out of range, n_scripts not in {0 with NULL, 1, B}, a kind outside 0..2, quant NULL, n_hist < 0,
 * a history pointer with n_hist == 0, hist_slab with A == 0, an index out of range or repeated) is MPC_E_ARG.
 * Device memory is O(B * A) + O(n_hist * max_steps * A). */
int mpc_closed_loop_traffic(mpc_ctx* c, int B, const double* x_init, const mpc_actor* actors, int A, int n_scripts,
                            int max_steps, double s_stop, double* quant, double* extra, int n_hist,
                            const int* hist_egos, double* hist_x, double* hist_u, double* hist_car_s, int* hist_tl,
                            int* hist_status, int* hist_nobs, double* hist_slab, int* n_steps, double* step_ms);

/* Closed-loop convoys: mpc_closed_loop_traffic in which the egos of one world see each other.  Egos
 * [w*W, (w+1)*W) form world w; every world drives the context's one reference line and egos of different worlds
 * never see each other.  A world with fewer cars is made by starting the spare egos past s_stop.
 *   ahead-of   within a world ego j is ahead of ego i iff s_j > s_i, or s_j == s_i and j < i, on the states
 *              before the step: a strict total order.
 *   leaders    per step, for an ego still in the loop: the egos of its world that are ahead of it and still in
 *              the loop (an ego that passed s_stop or went NaN is gone from the next step on), nearest first in
 *              that order, at most K, cut at the first one with s_j - s_i >= lead_range.  Each appends
 *              (s_j, v_j), the leader's state before the step (v_j as it is, NaN included), to the slab after
 *              the ego's script entries; n_obs counts both.  Followers are invisible to leaders.
 *   actors, A, n_scripts   mpc_closed_loop_traffic's, the same state machines in the same order.
 *   W, K, lead_range   1 <= W <= MPC_MAX_WORLD, B a multiple of W; 0 <= K, A + K <= MPC_MAX_ACTORS;
 *              lead_range > 0 (+inf allowed).
 * The solver runs with max_obs = A + K when any actor is not NONE or when K > 0 and W > 1, otherwise with no
 * slab.  With W == 1 or K == 0 every output the traffic entry has equals mpc_closed_loop_traffic's bit for bit.
 *   quant      [B][MPC_CL_NQ], required.  MPC_CLQ_MIN_OBS_DIST is the running minimum over scripted cars and
 *              leaders (within a step the cars in actor order, then the leaders in slab order; strict <, the
 *              sweep's NaN rule): a leader is a car for the obstacle verdict.
 *   extra      [B][MPC_CV_NX], optional.  Columns 0..2 are the traffic extras, MPC_TRX_MAX_NOBS over the whole
 *              slab and MPC_TRX_MIN_GAP_ACTOR -1.0 also when a leader holds the minimum.
 *   hist_*     the traffic entry's, with hist_slab [n_hist][max_steps][A+K][2] and
 *              hist_lead [n_hist][max_steps][K]: the leaders' batch indices in slab order, -1 past them and
 *              past n_steps.  hist_car_s stays the first scripted car.
 * Misuse: the traffic entry's cases, W out of range, B % W != 0, K out of range, A + K > MPC_MAX_ACTORS,
 * lead_range <= 0 or NaN, hist_lead with K == 0 or n_hist == 0, hist_slab with A + K == 0: MPC_E_ARG.
 * Device memory is O(B * (A + K)) + O(n_hist * max_steps * (A + K)). */
#define MPC_MAX_WORLD 256
#define MPC_CVX_MIN_LEAD_GAP 3    /* min (s_j - s_i) over leaders only; NaN if the ego never had a leader     */
#define MPC_CVX_MIN_LEAD_EGO 4    /* batch index of the leader behind it (earliest step, then slab order); -1 */
#define MPC_CVX_MAX_LEADERS 5     /* largest number of leaders in one step                                    */
#define MPC_CV_NX 6
int mpc_closed_loop_convoy(mpc_ctx* c, int B, int W, int K, double lead_range, const double* x_init,
                           const mpc_actor* actors, int A, int n_scripts, int max_steps, double s_stop,
                           double* quant, double* extra, int n_hist, const int* hist_egos, double* hist_x,
                           double* hist_u, double* hist_car_s, int* hist_tl, int* hist_status, int* hist_nobs,
                           double* hist_slab, int* hist_lead, int* n_steps, double* step_ms);

/* Closed-loop disturbance sweeps: mpc_closed_loop_convoy with seeded, reproducible noise between the world and
 * the solver.  The world keeps the truth: the actors' state machines, the leader ranking, the exit test, every
 * MPC_CLQ_* quantity, the slab of hist_slab and the gap quantities use the true states exactly as in the convoy
 * entry.  Only the state and the slab copy handed to the solver are perturbed, and the control the plant
 * integrates.
 *
 * Noise source: counter-based Philox4x32-10 (multipliers 0xD2511F53, 0xCD9E8D57; Weyl key increments 0x9E3779B9,
 * 0xBB67AE85), no generator state.  One draw:
 *   key     = (seed & 0xffffffff, seed >> 32)
 *   counter = (g & 0xffffffff, g >> 32, (unsigned)step, channel), g = ego_offset + b as a 64-bit integer
 *   words   w0..w3 of that one block; S = w0 + w1 + w2 + w3 (exact, < 2^34)
 *   z       = ((double)S - 8589934590.0) * c, c = 1.7320508075688772 * 2^-32: mean 0, variance 1,
 *             |z| <= 2 sqrt(3) (Irwin-Hall of four uniforms); the multiply is the only rounding
 * so an ego's noise depends on (seed, global ego index, step, channel) only: not on B, on the compaction of the
 * solver's list, on the backend or on the shard.  Channels: j = 0..4 measurement noise of state component j;
 * 5, 6 actuation noise of u1, u2; 7 + j process noise of state component j; 16 + 2j, 17 + 2j perception noise
 * of (s, v) of slab entry j < MPC_MAX_ACTORS.  A channel whose sigma is 0 draws nothing and leaves its value
 * untouched (no + 0 * z, no clamp).
 *
 * Per step, for an ego still in the loop, with x the true state before the step and (u1, u2) the solver's
 * first control:
 *   measure  the solver receives xm[j] = x[j] + meas_sigma[j] * z(j), and of slab entry j the pair
 *            (s + perc_sigma[0] * z(16 + 2j), v + perc_sigma[1] * z(17 + 2j)); zeros past n_obs as before
 *   actuate  ua[k] = clamp(u[k] + act_sigma[k] * z(5 + k), u_min[k], u_max[k]) with the context's bounds
 *            (t < u_min ? u_min : t > u_max ? u_max : t: a NaN stays)
 *   plant    x_next[j] = (x[j] + dt * xd[j]) + (dt * proc_sigma[j]) * z(7 + j), xd the convoy's with (ua1, ua2)
 *            for (u1, u2) and k_ref looked up at the true s
 * MPC_CLQ_U* and hist_u stay the commanded controls: the controls verdict judges the solver, not the actuator.
 *   noise, n_noise   n_noise == B: noise[b] is ego b's; n_noise == 1: one struct shared by all; noise NULL with
 *                n_noise == 0: no noise (every sigma 0)
 *   seed, ego_offset   ego_offset >= 0 is the global index of ego 0 (a shard's offset)
 *   extra        [B][MPC_NZ_NX], optional: columns 0..5 the convoy's, then the MPC_NZX_* columns
 *   hist_ua      [n_hist][max_steps][2] applied controls; hist_xm [n_hist][max_steps][5] the state the solver was
 *                given; NaN past n_steps.  Every other argument is mpc_closed_loop_convoy's.
 * With every sigma 0 every output the convoy entry has equals mpc_closed_loop_convoy's bit for bit, hist_ua equals
 * hist_u, hist_xm the states before the steps, the applied extremes the commanded ones and N_CLAMPED is 0.
 * Misuse: the convoy entry's cases, a sigma that is negative or NaN, n_noise not in {0 with NULL, 1, B},
 * ego_offset < 0, hist_ua or hist_xm with n_hist == 0: MPC_E_ARG.
 * Device memory is O(B * (A + K)) + O(n_hist * max_steps * (A + K)). */
typedef struct mpc_noise {
    double meas_sigma[5];   /* the solver sees x + sigma*z per component (s, d, o, k, v)         */
    double act_sigma[2];    /* the plant applies clamp(u0 + sigma*z, u_min, u_max) per component */
    double proc_sigma[5];   /* x_next[j] = (x[j] + dt*xd[j]) + (dt*sigma[j])*z                   */
    double perc_sigma[2];   /* every slab entry handed to the solver: (s + sigma0*z, v + sigma1*z') */
} mpc_noise;
void mpc_default_noise(mpc_noise* n);           /* all zero */
#define MPC_NZ_CH_MEAS 0          /* + j, j < 5                                                              */
#define MPC_NZ_CH_ACT 5           /* + k, k < 2                                                              */
#define MPC_NZ_CH_PROC 7          /* + j, j < 5                                                              */
#define MPC_NZ_CH_PERC 16         /* + 2 * entry (s), + 2 * entry + 1 (v)                                    */
#define MPC_NZ_CHANNELS 48
#define MPC_NZX_U1A_MIN 6         /* extremes of the applied controls, the sweep's NaN rule                  */
#define MPC_NZX_U1A_MAX 7
#define MPC_NZX_U2A_MIN 8
#define MPC_NZX_U2A_MAX 9
#define MPC_NZX_N_CLAMPED 10      /* steps at which the clamp changed a component                            */
#define MPC_NZ_NX 11
int mpc_closed_loop_noisy(mpc_ctx* c, int B, int W, int K, double lead_range, const double* x_init,
                          const mpc_actor* actors, int A, int n_scripts, const mpc_noise* noise, int n_noise,
                          unsigned long long seed, long long ego_offset, int max_steps, double s_stop, double* quant,
                          double* extra, int n_hist, const int* hist_egos, double* hist_x, double* hist_u,
                          double* hist_ua, double* hist_xm, double* hist_car_s, int* hist_tl, int* hist_status,
                          int* hist_nobs, double* hist_slab, int* hist_lead, int* n_steps, double* step_ms);
/* The draws themselves, on the context's backend: words [n][4] (may be NULL) and z [n] (may be NULL) of
 * (seed, ego[i], step[i], channel[i]).  The public way to regenerate or audit the noise of a run offline.
 * n < 0, a NULL index array with n > 0, ego[i] < 0, or a channel outside 0 .. MPC_NZ_CHANNELS - 1: MPC_E_ARG. */
int mpc_noise_draw(mpc_ctx* c, unsigned long long seed, int n, const long long* ego, const int* step,
                   const int* channel, unsigned* words, double* z);

/* Closed-loop plan traces: mpc_closed_loop_noisy that also keeps the plan behind each applied control, the sixth
 * return value of the reference's run_simulation (hist_preds, trajectory_tracking.py:389, :416), and accumulates
 * on the device how far every ego ended up from what it planned.  The arguments are mpc_closed_loop_noisy's, in
 * its order, followed by the trace outputs.
 *   hist_pred    [n_hist][max_steps][N+1][5]: for named ego hist_egos[k] at step t exactly what the solver
 *                returned as Xpred for the inputs it was handed at that step (the measured state hist_xm[k][t]
 *                and the perceived slab), so stage 0 is the measured state.  NaN past n_steps.
 *   hist_plan    [n_hist][max_steps][N][2]: the solver's U of that step; hist_plan[k][t][0] is hist_u[k][t].
 *                NaN past n_steps.
 *   lookahead, n_look   0 <= n_look <= MPC_MAX_LOOK; each 1 <= lookahead[i] <= N, distinct.
 *   gapq         [B][n_look][MPC_TG_NQ], required iff n_look > 0: plan-vs-outcome gaps of every ego.  With x_r the
 *                true state row r of the ego (row 0 is x_init, row r the state after step r - 1: hist_x's rows)
 *                and P_t[j] stage j of the prediction made at step t, lookahead j = lookahead[i] compares the
 *                pairs (P_t[j], x_{t+j}) for t = 0 .. n_steps - 1 with t + j <= n_steps: the final state is
 *                compared, predictions that reach past the ego's exit are not.  The truth is compared, not the
 *                measurement: like every MPC_CLQ_* quantity of the noisy entry the gap judges the world.
 * With n_look == 0 and hist_pred == hist_plan == NULL the call launches exactly the noisy entry's kernels and every
 * output equals mpc_closed_loop_noisy's bit for bit.  With any trace output requested the solver is also asked for
 * its U and Xpred, two more kernels run per step, and every output the noisy entry has still equals the noisy
 * entry's bit for bit.
 * Misuse: the noisy entry's cases, n_look out of range, a lookahead outside 1 .. N or repeated, lookahead NULL with
 * n_look > 0, gapq NULL with n_look > 0 or given with n_look == 0, hist_pred or hist_plan with n_hist == 0:
 * MPC_E_ARG.
 * Device memory is the noisy entry's, O(B * (A + K)) + O(n_hist * max_steps * (A + K)), plus, only when a trace
 * output is requested, O(B * N) for the solver's U and Xpred of the listed egos, O(B * sum(lookahead) * 3) for the
 * prediction rings, O(B * n_look) for the gaps and O(n_hist * max_steps * N) for the two histories. */
#define MPC_MAX_LOOK 4
#define MPC_TG_N_CMP 0            /* number of pairs, max(0, n_steps - j + 1)                                  */
#define MPC_TG_MAX_DS 1           /* max over the pairs of |P_t[j].c - x_{t+j}.c| for c = s, d, v: the sweep's   */
#define MPC_TG_MAX_DD 2           /* NaN rule (a NaN difference enters and stays); NaN when there is no pair     */
#define MPC_TG_MAX_DV 3
#define MPC_TG_STEP_DD 4          /* the t of the pair that holds MAX_DD: the earliest on ties, the first NaN
                                     pair if there is one; -1.0 when there is no pair                          */
#define MPC_TG_NQ 5
int mpc_closed_loop_traced(mpc_ctx* c, int B, int W, int K, double lead_range, const double* x_init,
                           const mpc_actor* actors, int A, int n_scripts, const mpc_noise* noise, int n_noise,
                           unsigned long long seed, long long ego_offset, int max_steps, double s_stop, double* quant,
                           double* extra, int n_hist, const int* hist_egos, double* hist_x, double* hist_u,
                           double* hist_ua, double* hist_xm, double* hist_car_s, int* hist_tl, int* hist_status,
                           int* hist_nobs, double* hist_slab, int* hist_lead, int* n_steps, double* step_ms,
                           const int* lookahead, int n_look, double* gapq, double* hist_pred, double* hist_plan);

/* Closed-loop warm starts: mpc_closed_loop_traced whose steps may linearise about the ego's own previous plan, the
 * real-time iteration: one QP per step that follows the nonlinear optimum across steps.  The arguments are
 * mpc_closed_loop_traced's, in its order, followed by `warm` (NULL: mpc_default_warm) and the warm outputs.  No
 * version step: the entry is detected by the presence of the symbol.
 * Per step and ego still in the loop, with xm the state and (slab, n_obs) the slab copy the solver is handed (after
 * the noisy entry's measure step):
 *   ref[k], k = 0 .. N-1   the reference warm start of (xm[0], xm[4], the slab positions, brake_distance,
 *                brake_accel): the bits the solver computes for itself when ubar == NULL.
 *   reset        the ego has no kept plan (its first step), the kept plan has a non-finite element, the kept status
 *                (masked with MPC_STATUS_MASK: MPC_SQP_UNCONVERGED never resets) is MPC_NUMERICAL, or the condition
 *                of a bit of warm->reset holds.  MPC_WARM_REFERENCE: always.
 *   ubar[k]      ref[k] if reset; else clamp(Uprev[k+1]) for k < N-1, and for k == N-1 ref[N-1]
 *                (MPC_WTAIL_REFERENCE) or clamp(Uprev[N-1]) (MPC_WTAIL_HOLD); clamp is per component to the context's
 *                u_min / u_max.  ubar is the solver's linearisation point (with sqp_iters > 1: the first QP's).
 *   after the solve the ego's U (exactly as returned), its status and this step's n_obs are kept, and
 *                move_t = max over k, c of |U[k][c] - ubar[k][c]| (the sweep's NaN rule) enters warmq.
 *   warmq        [B][MPC_WQ_NQ], optional: the MPC_WQ_* columns of every ego.
 *   hist_ubar    [n_hist][max_steps][N][2], optional: the ubar the solver was handed.  NaN past n_steps.
 * MPC_WARM_REFERENCE with warmq == hist_ubar == NULL: the call launches exactly the traced entry's kernels, ubar stays
 * NULL, and every output equals mpc_closed_loop_traced's bit for bit.  MPC_WARM_REFERENCE with either output
 * requested: ref is handed to the solver as an explicit ubar every step (MPC_WQ_N_RESET == n_steps), and every
 * output the traced entry has still equals the traced entry's bit for bit.
 * Misuse: the traced entry's cases, mode or tail outside their values, unknown bits in reset, hist_ubar with
 * n_hist == 0, sqp_iters == 0 with MPC_WARM_CARRY: MPC_E_ARG.
 * Device memory is the traced entry's plus, only when carrying or when a warm output is requested, O(B * N) for the
 * kept plans, the packed ubar and the solver's U, and O(n_hist * max_steps * N) for hist_ubar. */
#define MPC_WARM_REFERENCE 0      /* ubar = the reference warm start every step (the other entries' behaviour)    */
#define MPC_WARM_CARRY 1          /* ubar = the ego's previous plan shifted by one stage                          */
#define MPC_WTAIL_REFERENCE 0     /* last stage of a carried ubar: the reference warm start's stage N-1           */
#define MPC_WTAIL_HOLD 1          /* ... : the kept plan's last control again                                     */
#define MPC_WRESET_NOBS 1         /* optional reset: n_obs handed to the solver differs from the last step's      */
#define MPC_WRESET_INFEASIBLE 2   /* optional reset: last masked status == MPC_INFEASIBLE                         */
#define MPC_WRESET_MAX_ITER 4     /* optional reset: last masked status == MPC_MAX_ITER                           */
typedef struct mpc_warm {
    int mode, tail, reset;
} mpc_warm;
void mpc_default_warm(mpc_warm* w);             /* MPC_WARM_REFERENCE, MPC_WTAIL_REFERENCE, 0 */
#define MPC_WQ_N_RESET 0          /* steps whose ubar was the reference warm start (the first step included)      */
#define MPC_WQ_MAX_MOVE 1         /* max over steps of move_t (the sweep's NaN rule); NaN if the ego never ran    */
#define MPC_WQ_STEP_MAX_MOVE 2    /* its step: the earliest on ties, the first NaN step if any; -1.0 if never ran */
#define MPC_WQ_SUM_MOVE 3         /* running sum from 0 of move_t in step order                                   */
#define MPC_WQ_NQ 4
int mpc_closed_loop_warm(mpc_ctx* c, int B, int W, int K, double lead_range, const double* x_init,
                         const mpc_actor* actors, int A, int n_scripts, const mpc_noise* noise, int n_noise,
                         unsigned long long seed, long long ego_offset, int max_steps, double s_stop, double* quant,
                         double* extra, int n_hist, const int* hist_egos, double* hist_x, double* hist_u,
                         double* hist_ua, double* hist_xm, double* hist_car_s, int* hist_tl, int* hist_status,
                         int* hist_nobs, double* hist_slab, int* hist_lead, int* n_steps, double* step_ms,
                         const int* lookahead, int n_look, double* gapq, double* hist_pred, double* hist_plan,
                         const mpc_warm* warm, double* warmq, double* hist_ubar);

/* ---- Multi-GPU: ego shards, one gather ----------------------------------------------------
 * Every ego is independent; a batch splits into contiguous per-rank shards (one process per GPU) with no
 * per-step exchange.  The one collective returns what the reference's run_simulation returns
 * (trajectory_tracking.py:443: the closed-loop histories) to rank 0: ncclGather (RCCL over xGMI,
 * rccl.h:745) of a fixed-size payload per rank.  RCCL is loaded (dlopen librccl.so.1) by the first
 * mpc_comm_unique_id / mpc_comm_create; without it they fail with MPC_E_COMM.
 *   - rank 0 calls mpc_comm_unique_id and hands the MPC_COMM_UID_BYTES bytes to every rank out of band (the
 *     package's shard.py uses a TCP rendezvous on MASTER_ADDR); every rank then calls mpc_comm_create
 *     (collective: it returns once all nranks ranks joined);
 *   - mpc_gather: device buffers, asynchronous on `stream` (hipStream_t, 0 = null stream): rank i's `bytes`
 *     land at recv + i*bytes on the root (recv holds nranks*bytes there; may be NULL elsewhere);
 *   - mpc_gather_host: the same from host buffers, staged through the communicator's device buffer on its
 *     own stream, synchronous (returns when the root's recv is filled);
 *   - mpc_comm_allreduce_max: in-place max of one double over all ranks (the measurement's max-over-ranks
 *     time), synchronous; mpc_comm_barrier: returns on every rank once all ranks entered it;
 *   - one communicator per process and device; not re-entrant. */
#define MPC_COMM_UID_BYTES 128
typedef struct mpc_comm mpc_comm;
int mpc_comm_unique_id(char* uid /* [MPC_COMM_UID_BYTES] */);
int mpc_comm_create(const char* uid, int nranks, int rank, int device, mpc_comm** out);
int mpc_comm_info(const mpc_comm* c, int* nranks, int* rank, int* device);
int mpc_gather(mpc_comm* c, const void* send, size_t bytes, void* recv, int root, void* stream);
int mpc_gather_host(mpc_comm* c, const void* send, size_t bytes, void* recv, int root);
int mpc_comm_allreduce_max(mpc_comm* c, double* value);
int mpc_comm_barrier(mpc_comm* c);
void mpc_comm_destroy(mpc_comm* c);

/* Thread-local description of the last API error on this thread. */
const char* mpc_last_error(void);
int mpc_version(void);
void mpc_destroy(mpc_ctx* c);

#ifdef __cplusplus
}
#endif
#endif /* MPCQP_H */
