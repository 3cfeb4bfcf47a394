// solve_kernel.h -- the solver kernel mpc_solve_kernel<GL, OBS, MODE, NT> (setup, crossover, interior point,
// polish, outputs), its launch modes, and the table lookup kernel.  Its constants are tracker_model.h's.
#pragma once
#include "../../include/mpcqp.h"
#include "riccati_lanes.h"

// phase-cycle instrumentation of a diagnostic build (-DMPC_PROF, tools/phase_probe.py); compiled
// out of the product library
#ifdef MPC_PROF
__device__ unsigned long long g_prof[16];
#define PROF_DECL                                \
    unsigned long long prof_acc[12];             \
    for (int i_ = 0; i_ < 12; ++i_) prof_acc[i_] = 0; \
    unsigned long long prof_t = __builtin_amdgcn_s_memtime();
#define PROF(i)                                                  \
    {                                                            \
        unsigned long long t_ = __builtin_amdgcn_s_memtime();    \
        prof_acc[i] += t_ - prof_t;                              \
        prof_t = t_;                                             \
    }
#define PROF_END \
    if (gl == 0 && bvalid) for (int i_ = 0; i_ < 12; ++i_) atomicAdd(&g_prof[i_], prof_acc[i_]);
#else
#define PROF_DECL
#define PROF(i)
#define PROF_END
#endif

// ------------------------------------------------------------------------------------------
// the solver kernel.  A 64-lane wavefront carries G = 64 / GL MPC instances, one per aligned group
// of GL lanes (GL = 16, 32 or 64, the smallest with N + 1 <= GL).  Within a group, lane k-1 owns
// stage k = 1..N: its 9 soft rows and the 4 box rows of control k-1, whose interior-point state
// lives in that lane's registers (row ids are compile-time, so the row coefficients fold away).
// The stage-wise recursions (Riccati factorisation and solves, rollouts) run group-uniformly
// from the group's LDS region: one instruction stream serves G instances, which is what pays for
// the inherently sequential part of the algorithm on a 64-wide SIMD.
// All branching is group-uniform, so a group that has converged simply drops out of the exec mask.
// ------------------------------------------------------------------------------------------
// soft-row id of lane slot j: without obstacles the slots hold rows 0-5 and 8
template <bool OBS>
__device__ __forceinline__ constexpr int rid(int j) { return OBS ? j : (j < 6 ? j : 8); }

// Launch modes.  MODE_FULL: crossover (polish = 2), interior point, polish, outputs -- one launch per
// batch.  The split pair MODE_XO + MODE_IPM is the same computation in two launches: MODE_XO runs the
// setup and the crossover for every instance, writes the outputs of the instances it certifies and
// appends the others to a device work list; MODE_IPM then runs the interior point (and polish) on the
// listed instances only.  Results are identical (a failed crossover leaves no state behind), but the
// expensive instances all start at once instead of queueing behind cheap ones on the same SIMD
// ("two-phase launch").  MODE_ONE is MODE_FULL for a single QP (sqp_iters = 1):
// the SQP loop is then a compile-time single pass, so no state is carried across it (the runtime loop
// costs the one-launch kernels ~400 B of scratch per lane at N = 40).
#define MODE_FULL 0
#define MODE_XO 1
#define MODE_IPM 2
#define MODE_ONE 3

// NT > 0: kernel specialised for horizon N = NT (the stage recursions are unrolled); NT = 0: any N.
template <int GL, bool OBS, int MODE, int NT>
__global__ void __launch_bounds__(WAVE, MODE == MODE_XO ? 2 : 1)   // crossover: two waves per SIMD (256 VGPRs)
mpc_solve_kernel(DevTable tab, KParams Pr, int B, const double* __restrict__ x0g, const double* __restrict__ obsg,
                 const int* __restrict__ nobsg, const double* __restrict__ ubarg, double* __restrict__ u0g,
                 double* __restrict__ Ug, double* __restrict__ Xg, int* __restrict__ statusg,
                 int* __restrict__ itersg, int* __restrict__ wlist, int* __restrict__ wcount,
                 double* __restrict__ stc, int* __restrict__ wnext) {
    constexpr int G = WAVE / GL;
    constexpr int NR = OBS ? NROW : NROW - 2;    // soft rows held per lane (6, 7: obstacle rows)
    // the Riccati solves of the horizon-specialised kernels are fully unrolled, obstacle kernels included.
    // (Round 1 kept them looped in the obstacle kernels, whose lanes hold 9 rows, for fewer spills; since
    // the split kernels carry no runtime SQP loop, unrolled is faster there too: C4 0.660 -> 0.609 ms,
    // C3 -0.8%, and C5 5.67 -> 4.16 ms together with the unrolled factorisation of NT = 40.)
    constexpr int NTR = NT;
    // row right-hand sides recomputed after the solve (WRC) instead of held live across it: obstacle
    // kernels only (measured neutral on the obstacle-free N = 20 kernel)
    constexpr bool WRC = OBS;
    // the factorisation's copy-free A'M block (fac_step): obstacle kernels only (see fac_step)
    constexpr bool FAC_CF = OBS;
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const int ln = threadIdx.x;
    const int grp = ln / GL, gl = ln % GL;
    int b;
    bool bvalid;
    int cslot = 0;      // MODE_IPM: work-list slot whose record this group uses (a spare group repeats the last)
    // MODE_XO of an eager call zeroes the other of the context's two list counters for the next call
    // (launch_solve), so no memset launch separates the batches
    if (MODE == MODE_XO && wnext && blockIdx.x == 0 && threadIdx.x == 0) *wnext = 0;
    if (MODE == MODE_IPM) {
        // instances deferred by the MODE_XO launch; waves past the end of the list exit at once
        const int cnt = *wcount;
        if ((int)blockIdx.x * G >= cnt) return;
        const int slot = blockIdx.x * G + grp;
        bvalid = slot < cnt;
        cslot = bvalid ? slot : cnt - 1;
        b = wlist[cslot];
    } else {
        b = blockIdx.x * G + grp;
        bvalid = b < B;
        if (!bvalid) b = B - 1;      // a spare group repeats the last instance; its outputs are dropped
    }
    PROF_DECL
    const Grp<GL> Q{grp * GL};
    const int N = NT > 0 ? NT : Pr.N;
    const int NP = N + 1;
    const double dt = Pr.dt;
    const double rho = Pr.rho;
    const double hL = Pr.L / 2.0;
    constexpr bool LITE = MODE == MODE_XO;          // lite LDS layout (see lds_doubles)
    constexpr bool ACL = acl_on(GL, NT) && !LITE;
    Lds S = carve(smem + (size_t)grp * lds_doubles(N, ACL, LITE), N, ACL, LITE);

    double x0[5];
#pragma unroll
    for (int j = 0; j < 5; ++j) x0[j] = x0g[5 * (size_t)b + j];
    // n_obs may be NULL with an obstacle slab: every instance then uses all max_obs rows (as the
    // host entry mpc_solve_batch does)
    int nobs = nobsg ? nobsg[b] : (obsg ? Pr.max_obs : 0);
    nobs = nobs < 0 ? 0 : (nobs > Pr.max_obs ? Pr.max_obs : nobs);
    const double* obs = obsg ? obsg + (size_t)b * Pr.max_obs * 2 : nullptr;
    const bool has_obs = nobs > 0;

    const int k = gl + 1;            // stage of this lane
    const bool live = k <= N;        // lane owns the rows of stage k and the boxes of control k-1
    // rowon: the row exists for this instance (group-uniform: the obstacle rows need obstacles);
    // ron = rowon on a live lane.  The per-iteration phases use rowon only: dead lanes (stages past N)
    // compute discarded values and are masked where lane values meet (the group reductions)
    bool ron[NR], rowon[NR];
    double cf[NR][4];
#pragma unroll
    for (int j = 0; j < NR; ++j) {
        rowon[j] = row_exists(rid<OBS>(j), has_obs);
        ron[j] = live && rowon[j];
        row_coef(rid<OBS>(j), hL, Pr.L, Pr.tgap, cf[j]);
    }

    // stage cache of the split launch (stc != nullptr): MODE_XO leaves each deferred instance's
    // linearisation point ub [N][2] and nominal rollout Xr [N+1][5] at its work-list slot, so MODE_IPM
    // loads them instead of repeating the warm start and the rollout (stage_cache_doubles)
    const bool cached = MODE == MODE_IPM && stc != nullptr;
    const double* stc_in = nullptr;
    if (cached) stc_in = stc + (size_t)cslot * stage_cache_doubles(N);
    // ---- K1: linearisation point ---------------------------------------------------------
    if (cached) {
        if (gl < N) {
            S.ub[2 * gl] = stc_in[2 * gl];
            S.ub[2 * gl + 1] = stc_in[2 * gl + 1];
        }
        for (int i = gl; i < 5 * NP; i += GL) S.Xr[i] = stc_in[2 * N + i];
    } else if (gl < N) {
        if (ubarg) {
            S.ub[2 * gl] = ubarg[(size_t)b * 2 * N + 2 * gl];
            S.ub[2 * gl + 1] = ubarg[(size_t)b * 2 * N + 2 * gl + 1];
        } else {
            // warm start, trajectory_tracking.py:224-246: s_curr advanced by repeated addition,
            // sticky brake flag over steps 0..gl.  The kernel's own text of loop_steps.h's warm_ref_begin /
            // warm_ref_advance / warm_ref_control (which the host backend and the carry kernel walk): through
            // them every instantiation's register allocation moved
            double s_curr = x0[0], v_curr = x0[4];
            bool brake = false;
            for (int j = 0; j <= gl; ++j) {
                if (j > 0) s_curr += v_curr * dt;
                for (int i = 0; i < nobs; ++i)
                    if ((obs[2 * i] - s_curr) < Pr.brake_distance) brake = true;
            }
            double ur[2];
            get_control(tab, s_curr, ur);
            S.ub[2 * gl] = ur[0];
            S.ub[2 * gl + 1] = brake ? Pr.brake_accel : ur[1];
        }
    }
    wave_sync();

    int nsoft = 0;
    for (int jj = 0; jj < NROW; ++jj) nsoft += row_exists(jj, has_obs) ? 1 : 0;
    const double Mtot = (double)(2 * nsoft * N + NBOX * N);
    const double R0 = 2.0 * Pr.w_u1, R1 = 2.0 * Pr.w_u2;

    // 0: return ubar and predict(x0, ubar).  The split launch (MODE_XO + MODE_IPM) runs single-QP solves
    // only (launch_solve), so there the SQP loop is a compile-time single pass: nothing is carried across it
    const int nsqp = MODE != MODE_FULL ? 1 : (Pr.sqp_iters < 0 ? 0 : Pr.sqp_iters);
    static_assert(MODE == MODE_FULL || MODE == MODE_XO || MODE == MODE_IPM || MODE == MODE_ONE, "launch mode");
    int status = MPC_OK, total_it = 0;
    // SQP state carried across re-linearisations (MODE_FULL): the row / box classification the last polish
    // left (2 bits per row, then one per box row), which starts the next QP's crossover (oracle polish_from,
    // given = 2); U two QPs back at this lane's control; the count of elastic QPs in a row
    int wcls = 0, ninf = 0;
    bool sqp_conv = false;
    double pb0 = 0.0, pb1 = 0.0;
    bool xo_ok = false;                    // MODE_XO: the crossover certified this instance
    double cstr[6] = {0, 0, 0, 0, 0, 0};   // LITE: cost data of stage k (this lane's only)
    // the lookup at this lane's stage (get_state at the nominal s_gl, with slopes): MODE_XO keeps it for the
    // stage cache.  Obstacle-free kernels only (LKC): in the obstacle kernels the longer-lived lookups moved
    // the register allocation against it (C3 +0.6%, C5 +0.3%; C4 -1.2%)
    constexpr bool LKC = !OBS;
    double refk[5] = {0, 0, 0, 0, 0}, slk[4] = {0, 0, 0, 0};
    for (int sqp = 0; sqp < nsqp; ++sqp) {
        // ---- K1: nominal rollout == predict(x0, ubar), into Xr (cached: loaded above), with the stage
        // lookups; cached: the lookups come from the stage cache ---------------------------------------
        if (!LKC) {
            if (!cached) predict_grp(tab, N, dt, x0, S.ub, S.Xr, S.kap, gl);
            if (gl <= N) get_state(tab, S.Xr[5 * gl], refk, slk);
        } else if (!cached) {
            predict_grp(tab, N, dt, x0, S.ub, S.Xr, S.kap, gl, refk, slk);
        } else if (gl <= N) {
            const double2* lk = reinterpret_cast<const double2*>(stc_in + stage_cache_lk(N) + 8 * gl);
            const double2 l0 = lk[0], l1 = lk[1], l2 = lk[2], l3 = lk[3];
            refk[1] = l0.x; refk[2] = l0.y; refk[3] = l1.x; refk[4] = l1.y;
            slk[0] = l2.x; slk[1] = l2.y; slk[2] = l3.x; slk[3] = l3.y;
        }
        // ---- K2: stage data of QP(ubar) ----------------------------------------------------
        // The A5 / AC coefficients, the row values v[] and the box values bb[] below are the kernel's own text of
        // tracker_model.h's stage_A, nearest_obstacle + row_values and box_values, which the host backend calls:
        // this kernel sits at 512 registers, and through the shared functions (each of the four parts alone)
        // no instantiation came out instruction-identical.  Change them together
        const bool gn = Pr.linearization != 0;
        if (gl < N) {
            const double* x = S.Xr + 5 * gl;
            double dk = gn ? slk[2] : 0.0;
            S.A5[A5S * gl + 0] = dt * x[4];
            S.A5[A5S * gl + 1] = dt * x[2];
            S.A5[A5S * gl + 2] = dt * (-x[4] * dk);
            S.A5[A5S * gl + 3] = dt * x[4];
            S.A5[A5S * gl + 4] = dt * (x[3] - refk[3]);
            S.A5[A5S * gl + 5] = dt;      // a04, read by the per-lane gathers (DLane)
            S.A5[A5S * gl + 6] = 0.0;     // the gathers' zero slot
            S.A5[A5S * gl + 7] = 0.0;
            if (ACL) {
                // rows 0..2 of the forward solve's closed-loop matrix are A_t's (B has rows 3, 4 only)
                double* ac = S.AC + 30 * gl;
                const double a12 = dt * x[4], a14 = dt * x[2], a20 = dt * (-x[4] * dk), a23 = dt * x[4];
                const double a24 = dt * (x[3] - refk[3]);
                ac[0] = 1.0; ac[1] = 0.0; ac[2] = 0.0; ac[3] = 0.0; ac[4] = dt; ac[5] = 0.0;
                ac[6] = 0.0; ac[7] = 1.0; ac[8] = a12; ac[9] = 0.0; ac[10] = a14; ac[11] = 0.0;
                ac[12] = a20; ac[13] = 0.0; ac[14] = 1.0; ac[15] = a23; ac[16] = a24; ac[17] = 0.0;
            }
        }
        if (gl <= N) {
            // the k row of QR is structurally zero (no cost or row touches k); the k entry of QH is
            // written as zero by every QH writer (QH shares its space with Xr, which is live here)
#pragma unroll
            for (int j = 0; j < 4; ++j) S.QR[QRS * gl + 12 + j] = 0.0;
        }
        // cost data of stage k (lookups done by lane k of the group)
        {
            const int src = k < GL ? k : GL - 1;
            const double rk1 = Q.get(refk[1], src), rk2 = Q.get(refk[2], src), rk4 = Q.get(refk[4], src);
            const double sk0 = Q.get(slk[0], src), sk1 = Q.get(slk[1], src), sk3 = Q.get(slk[3], src);
            if (live) {
                const double* x = S.Xr + 5 * k;
                double* c = LITE ? cstr : S.cst + 6 * k;
                c[0] = gn ? -sk0 : 0.0;
                c[1] = gn ? -sk1 : 0.0;
                c[2] = gn ? -sk3 : 0.0;
                c[3] = x[1] - rk1;
                c[4] = x[2] - rk2;
                c[5] = x[4] - rk4;
            }
        }
        // row bounds of stage k, box bounds of control k-1
        double bk[NR], bb[NBOX];
        double bscale_l = 0.0;
        {
            double shat = INFINITY;
            if (live && has_obs)
                for (int i = 0; i < nobs; ++i) {
                    double sp = obs[2 * i] + obs[2 * i + 1] * (k * dt);
                    shat = sp < shat ? sp : shat;
                }
            const double* x = S.Xr + 5 * (live ? k : 0);
            const double sl = Pr.sl;
            const double pv0 = x[1], pv1 = x[1] + hL * x[2], pv2 = x[1] + Pr.L * x[2];
            double v[NROW];  // by row id
            v[0] = -sl - pv0;
            v[1] = -(sl - pv0);
            v[2] = -sl - pv1;
            v[3] = -(sl - pv1);
            v[4] = -sl - pv2;
            v[5] = -(sl - pv2);
            v[6] = has_obs ? -(shat - Pr.osd - x[0]) : 0.0;
            v[7] = has_obs ? -(shat - x[0] - Pr.tgap * x[4]) : 0.0;
            v[8] = -x[4];
#pragma unroll
            for (int j = 0; j < NR; ++j) {
                bk[j] = ron[j] ? v[rid<OBS>(j)] : 0.0;
                bscale_l = fmax(bscale_l, fabs(bk[j]));
            }
            const double ub0 = live ? S.ub[2 * (k - 1)] : 0.0, ub1 = live ? S.ub[2 * (k - 1) + 1] : 0.0;
            bb[0] = live ? Pr.u_min0 - ub0 : 0.0;
            bb[1] = live ? -(Pr.u_max0 - ub0) : 0.0;
            bb[2] = live ? Pr.u_min1 - ub1 : 0.0;
            bb[3] = live ? -(Pr.u_max1 - ub1) : 0.0;
#pragma unroll
            for (int j = 0; j < NBOX; ++j) bscale_l = fmax(bscale_l, fabs(bb[j]));
        }
        const double bscale = Q.max(bscale_l);
        wave_sync();

        // ---- K4: crossover, then (if it does not certify) PDIP and the polish of its iterate ------
        // Phase 0 is the active-set solve started from the unconstrained optimum: all rows inactive,
        // multipliers 0, du = 0 (oracle pdip(): XO_ROUNDS rounds).  When it certifies (KKT-consistent),
        // it is the exact optimum and no interior-point iteration runs (70% of the C2 batch).
        double rs[NR], rl[NR], rxi[NR], rnu[NR], sb[NBOX], lb[NBOX];
#pragma unroll
        for (int j = 0; j < NR; ++j) { rs[j] = 0.0; rl[j] = 0.0; rxi[j] = 0.0; rnu[j] = 0.0; }
#pragma unroll
        for (int j = 0; j < NBOX; ++j) { sb[j] = 0.0; lb[j] = 0.0; }
        int it = 0, st_here = MPC_MAX_ITER, stall = 0;
        double mu = 0.0;
        // x4: state of stage k along the current iterate, G du (du = 0 at the start); updated with the
        // state direction of every step, so the linear rollout never re-runs (it is linear in du)
        double x4[4] = {0.0, 0.0, 0.0, 0.0};
        double du0 = 0.0, du1 = 0.0;        // control k-1 of the current iterate
        // MODE_XO runs phase 0 only and MODE_IPM phase 1 only (both compile-time)
        const int phase_lo = MODE == MODE_XO ? 0 : (MODE == MODE_IPM ? 1 : (Pr.polish >= 2 ? 0 : 1));
        constexpr int phase_hi = MODE == MODE_XO ? 1 : 2;
        for (int phase = phase_lo; phase < phase_hi; ++phase) {
        bool accepted = false;
        double bad = 0.0;
        // checkpoint: chk = the interior point stopped there (segment end), checked = it was tried this QP
        bool chk = false, checked = false;
        if (phase == 1) {
            // Start centred at the unconstrained optimum of QP(ubar) (oracle pdip): one
            // factorisation and solve without rows gives du and the state x4 of stage k there (or du = 0, see
            // below); each soft row of
            // value r gets slack max(r, 0) + START_SHIFT and elastic slack max(-r, 0) + START_SHIFT, and its
            // multiplier pair the pair's central point with lambda + nu = rho; box rows the mean row
            // complementarity.  (Round 2 started at du = 0 with s lam = 1000, lam <= rho / 2 and stopped at
            // mu <= 1e-9: C2 22 -> 20 iterations at most, C5 29 -> 27)
            // The crossover (phase 0 from the all-inactive classification) solved exactly this system: the same
            // factorisation inputs and right-hand side, in the same solve form, so its solution is the start's
            // bit for bit.  MODE_FULL / MODE_ONE still hold it in dX / dud; MODE_IPM reads it from the stage
            // cache; otherwise (no crossover ran, a warm SQP crossover, or no cache) it is recomputed here, in
            // the crossover's solve form (the K-row form wherever the split launch exists, G >= 2).
            const bool xo_start = (MODE == MODE_IPM) ? cached : (phase_lo == 0 && !(MODE == MODE_FULL && sqp > 0));
            if (live && !xo_start) {
                double Qs[10], qs[4];
                stage_cost(LITE ? cstr : S.cst + 6 * k, Pr.w_d, Pr.w_o, Pr.w_v, Qs, qs);
#pragma unroll
                for (int a = 0; a < 4; ++a) {
#pragma unroll
                    for (int c = 0; c < 4; ++c) S.QR[QRS * k + 4 * st4(a) + c] = Qs[p4(a, c)];
                    S.QH[QHS * k + st4(a)] = -qs[a];
                }
                S.QH[QHS * k + 3] = 0.0;
                S.QH[QHS * k + 5] = 0.0;
                S.Rt[2 * (k - 1)] = R0;
                S.Rt[2 * (k - 1) + 1] = R1;
                S.gh[2 * (k - 1)] = -(R0 * S.ub[2 * (k - 1)]);
                S.gh[2 * (k - 1) + 1] = -(R1 * S.ub[2 * (k - 1) + 1]);
            }
            if (!xo_start) {
                wave_sync();
                riccati_factor<NT, FAC_CF>(S, N, dt, gl);
                // GL = 64 crossovers solve on the AC rows (phase 0 below), so their start does too; the GL = 64
                // interior-point kernels of the split launch (MPC_IPM_GL64, N = 20) follow a GL = 32 MODE_XO
                // crossover, which solved in K-row form: so does the start they recompute without the stage cache
                if constexpr (ACL && GL == 64 && !(MODE == MODE_IPM && NT == 20)) riccati_solve<NTR, ACL>(S, N, dt, gl);
                else riccati_solve<NTR, false>(S, N, dt, gl);
            }
            if (MODE == MODE_IPM && cached) {
                const double* xo = stc_in + stage_cache_xo(N) + 6 * (live ? k - 1 : 0);
                du0 = live ? xo[0] : 0.0;
                du1 = live ? xo[1] : 0.0;
#pragma unroll
                for (int a = 0; a < 4; ++a) x4[a] = live ? xo[2 + a] : 0.0;
            } else {
#pragma unroll
                for (int a = 0; a < 4; ++a) x4[a] = live ? S.dX[5 * k + st4(a)] : 0.0;
                du0 = live ? S.dud[2 * (k - 1)] : 0.0;
                du1 = live ? S.dud[2 * (k - 1) + 1] : 0.0;
            }
            {
                // primal point: the unconstrained optimum, or du = 0 (the warm start ubar, which already brakes
                // for obstacles ahead) when the soft rows are less violated there (sum of max(-r, 0))
                double vu = 0.0, vb = 0.0;
    #pragma unroll
                for (int j = 0; j < NR; ++j)
                    if (ron[j]) {
                        const double r = rdot(rid<OBS>(j), cf[j], x4) - bk[j];
                        vu += r < 0.0 ? -r : 0.0;
                        vb += bk[j] > 0.0 ? bk[j] : 0.0;
                    }
                vu = Q.sum(vu);
                vb = Q.sum(vb);
                if (vb < vu) {
    #pragma unroll
                    for (int a = 0; a < 4; ++a) x4[a] = 0.0;
                    du0 = 0.0;
                    du1 = 0.0;
                }
            }
            double rowc = 0.0;
    #pragma unroll
            for (int j = 0; j < NR; ++j) {
                const double r = rdot(rid<OBS>(j), cf[j], x4) - bk[j];
                const double sv = (r > 0.0 ? r : 0.0) + START_SHIFT, xi = (r < 0.0 ? -r : 0.0) + START_SHIFT;
                const double iq = rho * frcp(sv + xi);
                rs[j] = sv; rxi[j] = xi; rl[j] = xi * iq; rnu[j] = sv * iq;
                if (ron[j]) rowc += sv * rl[j];
            }
            const double mrow = Q.sum(live ? rowc : 0.0) / (double)(nsoft * N);
    #pragma unroll
            for (int j = 0; j < NBOX; ++j) {
                const double v = bsign(j) * (j < 2 ? du0 : du1) - bb[j];
                sb[j] = v > 1.0 ? v : 1.0;
                lb[j] = mrow * frcp(sb[j]);
            }
            wave_sync();
        }
        for (;;) {      // segments: interior point (to convergence or the checkpoint), polish; resume if needed
        if (phase == 1) {
        PROF(0)
        for (int iter = it; iter < Pr.max_iter; ++iter) {
            PROF(1)
            // the row bounds are loop-invariant; keeping them opaque stops the compiler from hoisting
            // everything derived from them out of this loop (it would stay live in registers and spill)
#pragma unroll
            for (int j = 0; j < NR; ++j) asm volatile("" : "+v"(bk[j]));
#pragma unroll
            for (int j = 0; j < NBOX; ++j) asm volatile("" : "+v"(bb[j]));
            // -- stage-parallel residuals ------------------------------------------------------
            double rpmax = 0.0, rxmax = 0.0, comp = 0.0;
            double ya[4] = {0, 0, 0, 0};
#pragma unroll
            for (int j = 0; j < NR; ++j) {
                if (!rowon[j]) continue;
                const double rp = rdot(rid<OBS>(j), cf[j], x4) + rxi[j] - rs[j] - bk[j];
                const double rx = rho - rl[j] - rnu[j];
#pragma unroll
                for (int a = 0; a < 4; ++a) ya[a] = fma(-rl[j], cf[j][a], ya[a]);
                rpmax = vmaxabs(rpmax, rp);
                rxmax = vmaxabs(rxmax, rx);
                comp = fma(rs[j], rl[j], fma(rxi[j], rnu[j], comp));
            }
            // dual-residual stage terms of stage k / control k-1: yc (cost), zc (control cost), za (box
            // multipliers); ya (row multipliers) accumulated above
            auto dual_terms = [&](double yc[4], double zc[2], double za[2]) {
                double Qs[10], qs[4];
                stage_cost(LITE ? cstr : S.cst + 6 * k, Pr.w_d, Pr.w_o, Pr.w_v, Qs, qs);
#pragma unroll
                for (int a = 0; a < 4; ++a) {
                    double acc = qs[a];
#pragma unroll
                    for (int c = 0; c < 4; ++c) acc = fma(Qs[p4(a, c)], x4[c], acc);
                    yc[a] = acc;
                }
                zc[0] = fma(R0, du0, R0 * S.ub[2 * (k - 1)]);
                zc[1] = fma(R1, du1, R1 * S.ub[2 * (k - 1) + 1]);
                za[0] = lb[1] - lb[0];
                za[1] = lb[3] - lb[2];
            };
            if (live) {
#pragma unroll
                for (int j = 0; j < NBOX; ++j) {
                    const double rp = bsign(j) * (j < 2 ? du0 : du1) - sb[j] - bb[j];
                    rpmax = vmaxabs(rpmax, rp);
                    comp = fma(sb[j], lb[j], comp);
                }
                double yc[4], zc[2], za[2];
                dual_terms(yc, zc, za);
#pragma unroll
                for (int a = 0; a < 4; ++a) S.ys[4 * k + a] = yc[a] + ya[a];
                S.zs[2 * (k - 1)] = zc[0] + za[0];
                S.zs[2 * (k - 1) + 1] = zc[1] + za[1];
            }
            rpmax = Q.max(live ? rpmax : 0.0);
            rxmax = Q.max(live ? rxmax : 0.0);
            comp = Q.sum(live ? comp : 0.0);
            wave_sync();
            PROF(2)
            mu = comp / Mtot;
            if (!(mu == mu)) { st_here = MPC_NUMERICAL; it = iter; break; }
            if (mu <= Pr.tol_mu && rpmax <= 10.0 * Pr.tol * (1.0 + bscale) && rxmax <= Pr.tol * rho) {
                // converged: the polish then makes the active set exact;
                // the dual residual carries O(eps/mu) multiplier noise, required to 1e4*tol.  Its
                // adjoint recursion is only run here, once per solve.
                if (live) {
                    double yc[4], zc[2], za[2];
                    dual_terms(yc, zc, za);
#pragma unroll
                    for (int a = 0; a < 4; ++a) {
                        S.QR[QRS * k + DQ_YC + a] = yc[a];
                        S.QR[QRS * k + DQ_YA + a] = ya[a];
                    }
                    S.QR[QRS * (k - 1) + DQ_ZC] = zc[0];
                    S.QR[QRS * (k - 1) + DQ_ZC + 1] = zc[1];
                    S.QR[QRS * (k - 1) + DQ_ZA] = za[0];
                    S.QR[QRS * (k - 1) + DQ_ZA + 1] = za[1];
                }
                wave_sync();
                double rdmax, sd;
                dual_norms(S, N, dt, rdmax, sd);
                PROF(3)
                st_here = rdmax <= 1e4 * Pr.tol * (1.0 + sd) ? MPC_OK : MPC_NUMERICAL;
                it = iter;
                break;
            }
            if (Pr.polish && !checked && mu <= Pr.mu_check) {
                double tie = 0.0;
#pragma unroll
                for (int j = 0; j < NR; ++j)
                    if (rowon[j] && (!(rs[j] > CHECK_SEP * rl[j] || rl[j] > CHECK_SEP * rs[j]) ||
                                     !(rxi[j] > CHECK_SEP * rnu[j] || rnu[j] > CHECK_SEP * rxi[j])))
                        tie = 1.0;
#pragma unroll
                for (int j = 0; j < NBOX; ++j)
                    if (!(sb[j] > CHECK_SEP * lb[j] || lb[j] > CHECK_SEP * sb[j])) tie = 1.0;
                if (Q.max(live ? tie : 0.0) == 0.0) {
                    chk = true;
                    it = iter;
                    break;
                }
            }
            // -- barrier weights, augmented stage Hessians ---------------------------------------
            double il[NR], inu[NR], wv[NR], ilb[NBOX], wb[NBOX];
            {
                double Qp[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
                for (int j = 0; j < NR; ++j) {
                    il[j] = frcp(rl[j]);
                    inu[j] = frcp(rnu[j]);
                    wv[j] = rowon[j] ? frcp(fma(rs[j], il[j], rxi[j] * inu[j])) : 0.0;   // 1/d
#pragma unroll
                    for (int a = 0; a < 4; ++a)
#pragma unroll
                        for (int c = a; c < 4; ++c)
                            if (row_nz(rid<OBS>(j), a) && row_nz(rid<OBS>(j), c))
                                Qp[p4(a, c)] = fma(wv[j] * cf[j][a], cf[j][c], Qp[p4(a, c)]);
                }
#pragma unroll
                for (int j = 0; j < NBOX; ++j) {
                    ilb[j] = frcp(lb[j]);
                    wb[j] = live ? lb[j] * frcp(sb[j]) : 0.0;
                }
                if (live) {
                    double Qs[10], qs[4];
                    stage_cost(LITE ? cstr : S.cst + 6 * k, Pr.w_d, Pr.w_o, Pr.w_v, Qs, qs);
#pragma unroll
                    for (int a = 0; a < 4; ++a)
#pragma unroll
                        for (int c = 0; c < 4; ++c) S.QR[QRS * k + 4 * st4(a) + c] = Qp[p4(a, c)] + Qs[p4(a, c)];
                    S.Rt[2 * (k - 1)] = R0 + (wb[0] + wb[1]);
                    S.Rt[2 * (k - 1) + 1] = R1 + (wb[2] + wb[3]);
                }
            }
            wave_sync();
            PROF(4)
            riccati_factor<NT, FAC_CF>(S, N, dt, gl);
            PROF(5)
            // -- predictor, corrector (and, if needed, centred) solves ---------------------------------
            double p4v[NR], p5v[NR], pbv[NBOX];
#pragma unroll
            for (int j = 0; j < NR; ++j) { p4v[j] = 0.0; p5v[j] = 0.0; }
#pragma unroll
            for (int j = 0; j < NBOX; ++j) pbv[j] = 0.0;
            double sig = 0.0;
            bool breakdown = false;
            // The passes (predictor, corrector, centred direction) are unrolled in the N = 20 kernels: no
            // loop-carried copies of the predictor products at the back edge (C2 -3%).  The runtime-horizon
            // kernels keep the loop (unrolled, C4 +2%, C5 +4%): their pass count is opaque, so the full-unroll
            // request does not apply there (built with -Wno-pass-failed).
            int npass = 3;
            if constexpr (NT == 0) asm volatile("" : "+s"(npass));
#pragma unroll
            for (int pass = 0; pass < npass; ++pass) {
                // pass 0: affine predictor; 1: Mehrotra corrector; 2: plain centred direction, taken when
                // the corrector would not reduce complementarity (oracle: comp_after > comp)
                const double smu = (pass >= 1) ? sig * mu : 0.0;
                const double cw = (pass == 1) ? 1.0 : 0.0;     // weight of the second-order term
                // reduced right-hand side per row, scaled by 1/d: wr = rh / d  (newton() of the oracle).
                // Recomputed after the solve rather than held live across it (register pressure).
                auto row_wr = [&](int j) {
                    const double r4 = fma(cw, p4v[j], fma(rs[j], rl[j], -smu));
                    const double r5 = fma(cw, p5v[j], fma(rxi[j], rnu[j], -smu));
                    const double rp = rdot(rid<OBS>(j), cf[j], x4) + rxi[j] - rs[j] - bk[j];
                    const double rx = rho - rl[j] - rnu[j];
                    const double rh = -rp - r4 * il[j] + fma(rxi[j], rx, r5) * inu[j];
                    return rowon[j] ? rh * wv[j] : 0.0;
                };
                auto box_wr = [&](int j) {
                    const double r4 = fma(cw, pbv[j], fma(sb[j], lb[j], -smu));
                    const double rp = bsign(j) * (j < 2 ? du0 : du1) - sb[j] - bb[j];
                    return (-rp - r4 * ilb[j]) * wb[j];
                };
                double wr[NR], wrb[NBOX];     // kept live by the obstacle-free variant only
                {
                    double q4[4] = {0, 0, 0, 0}, g0 = 0.0, g1 = 0.0;
#pragma unroll
                    for (int j = 0; j < NR; ++j) {
                        double w;
                        if constexpr (WRC) {
                            w = row_wr(j);
                        } else {
                            const double r4 = fma(cw, p4v[j], fma(rs[j], rl[j], -smu));
                            const double r5 = fma(cw, p5v[j], fma(rxi[j], rnu[j], -smu));
                            const double rp = rdot(rid<OBS>(j), cf[j], x4) + rxi[j] - rs[j] - bk[j];
                            const double rx = rho - rl[j] - rnu[j];
                            const double rh = -rp - r4 * il[j] + fma(rxi[j], rx, r5) * inu[j];
                            wr[j] = rowon[j] ? rh * wv[j] : 0.0;
                            w = wr[j];
                        }
#pragma unroll
                        for (int a = 0; a < 4; ++a)
                            if (row_nz(rid<OBS>(j), a)) q4[a] = fma(cf[j][a], w, q4[a]);
                    }
#pragma unroll
                    for (int j = 0; j < NBOX; ++j) {
                        double w;
                        if constexpr (WRC) {
                            w = box_wr(j);
                        } else {
                            const double r4 = fma(cw, pbv[j], fma(sb[j], lb[j], -smu));
                            const double rp = bsign(j) * (j < 2 ? du0 : du1) - sb[j] - bb[j];
                            wrb[j] = (-rp - r4 * ilb[j]) * wb[j];
                            w = wrb[j];
                        }
                        if (j < 2) g0 += bsign(j) * w; else g1 += bsign(j) * w;
                    }
                    if (live) {
                        // the dual-residual terms are read before any write (see ac_rows)
                        double ysv[4], zs0, zs1;
                        ld2(S.ys + 4 * k, ysv[0], ysv[1]);
                        ld2(S.ys + 4 * k + 2, ysv[2], ysv[3]);
                        ld2(S.zs + 2 * (k - 1), zs0, zs1);
#pragma unroll
                        for (int a = 0; a < 4; ++a) S.QH[QHS * k + st4(a)] = q4[a] - ysv[a];
                        S.QH[QHS * k + 3] = 0.0;
                        S.QH[QHS * k + 5] = 0.0;
                        *reinterpret_cast<double2*>(S.gh + 2 * (k - 1)) = make_double2(g0 - zs0, g1 - zs1);
                    }
                }
                wave_sync();
                PROF(6)
                riccati_solve<NTR, ACL>(S, N, dt, gl);
                PROF(7)
                // row directions and the largest feasible step
                double dx4[4];
#pragma unroll
                for (int a = 0; a < 4; ++a) dx4[a] = live ? S.dX[5 * k + st4(a)] : 0.0;
                const double dd0 = live ? S.dud[2 * (k - 1)] : 0.0, dd1 = live ? S.dud[2 * (k - 1) + 1] : 0.0;
                double dsv[NR], dlv[NR], dxv[NR], dnv[NR], dsb[NBOX], dlb[NBOX];
                // ratio tests as rmax = max(1, max_j -d_j / x_j); the step to the boundary is 1 / rmax.
                // The reciprocals of lam, nu (rows) and lam (boxes) are the barrier weights' il, inu,
                // ilb; s, xi (rows) and s (boxes) take the approximate v_rcp_f64 (enough for a step
                // length).  A product and a max per term (no compare, select or NaN canonicalisation).
                double rmax = 1.0;
#pragma unroll
                for (int j = 0; j < NR; ++j) {
                    const double r4 = fma(cw, p4v[j], fma(rs[j], rl[j], -smu));
                    const double r5 = fma(cw, p5v[j], fma(rxi[j], rnu[j], -smu));
                    const double rx = rho - rl[j] - rnu[j];
                    double wj;
                    if constexpr (WRC) wj = row_wr(j); else wj = wr[j];
                    const double dl = fma(-wv[j], rdot(rid<OBS>(j), cf[j], dx4), wj);
                    const double ds = -fma(rs[j], dl, r4) * il[j];
                    const double dn = rx - dl;
                    const double dxi = -fma(rxi[j], dn, r5) * inu[j];
                    const bool on = rowon[j];
                    dsv[j] = on ? ds : 0.0;
                    dlv[j] = on ? dl : 0.0;
                    dxv[j] = on ? dxi : 0.0;
                    dnv[j] = on ? dn : 0.0;
                    rmax = vmax(rmax, -dsv[j] * __builtin_amdgcn_rcp(rs[j]));
                    rmax = vmax(rmax, -dlv[j] * il[j]);
                    rmax = vmax(rmax, -dxv[j] * __builtin_amdgcn_rcp(rxi[j]));
                    rmax = vmax(rmax, -dnv[j] * inu[j]);
                }
#pragma unroll
                for (int j = 0; j < NBOX; ++j) {
                    const double r4 = fma(cw, pbv[j], fma(sb[j], lb[j], -smu));
                    double wj;
                    if constexpr (WRC) wj = box_wr(j); else wj = wrb[j];
                    const double dl = fma(-wb[j] * bsign(j), (j < 2 ? dd0 : dd1), wj);
                    const double ds = -fma(sb[j], dl, r4) * ilb[j];
                    dsb[j] = ds;
                    dlb[j] = dl;
                    rmax = vmax(rmax, -dsb[j] * __builtin_amdgcn_rcp(sb[j]));
                    rmax = vmax(rmax, -dlb[j] * ilb[j]);
                }
                const double amax = __builtin_amdgcn_rcp(Q.max(live ? rmax : 1.0));
                // complementarity after the step (pass 0: at the full affine step length)
                const double a_try = (pass == 0) ? amax : fmin(1.0, TAU * amax);
                double ca = 0.0;
#pragma unroll
                for (int j = 0; j < NR; ++j)
                    if (rowon[j])
                        ca += fma(a_try, dsv[j], rs[j]) * fma(a_try, dlv[j], rl[j]) +
                              fma(a_try, dxv[j], rxi[j]) * fma(a_try, dnv[j], rnu[j]);
#pragma unroll
                for (int j = 0; j < NBOX; ++j) ca += fma(a_try, dsb[j], sb[j]) * fma(a_try, dlb[j], lb[j]);
                if (!(fabs(dd0) < INFINITY && fabs(dd1) < INFINITY)) ca = NAN;   // breakdown guard input
                ca = Q.sum(live ? ca : 0.0);
                PROF(11)
                if (pass == 0) {
                    const double r = ca / comp;
                    sig = r * r * r;
#pragma unroll
                    for (int j = 0; j < NR; ++j) { p4v[j] = dsv[j] * dlv[j]; p5v[j] = dxv[j] * dnv[j]; }
#pragma unroll
                    for (int j = 0; j < NBOX; ++j) pbv[j] = dsb[j] * dlb[j];
                    continue;
                }
                if (pass == 1 && ca > comp) continue;     // safeguard: take the centred direction
                if (!(ca < INFINITY)) {                    // breakdown guard (oracle pdip): the step is not
                    breakdown = true;                      // taken, the current iterate goes to the polish
                    break;
                }
                const double alpha = a_try;
                stall = (mu < 1e-6 && ca > 0.9 * comp) ? stall + 1 : 0;
#pragma unroll
                for (int j = 0; j < NR; ++j) {
                    rs[j] = fma(alpha, dsv[j], rs[j]);
                    rl[j] = fma(alpha, dlv[j], rl[j]);
                    rxi[j] = fma(alpha, dxv[j], rxi[j]);
                    rnu[j] = fma(alpha, dnv[j], rnu[j]);
                }
#pragma unroll
                for (int j = 0; j < NBOX; ++j) {
                    sb[j] = fma(alpha, dsb[j], sb[j]);
                    lb[j] = fma(alpha, dlb[j], lb[j]);
                }
                du0 = fma(alpha, dd0, du0);
                du1 = fma(alpha, dd1, du1);
#pragma unroll
                for (int a = 0; a < 4; ++a) x4[a] = fma(alpha, dx4[a], x4[a]);
                break;
            }
            wave_sync();
            PROF(8)
            it = iter + 1;
            if (stall >= 5 || breakdown) { st_here = MPC_NUMERICAL; break; }
        }
        if (!chk) {
        total_it += it;
        // NaN guard and the infeasibility flag
        if (live) bad = (du0 == du0 && du1 == du1) ? 0.0 : 1.0;
        bad = Q.max(bad);
        if (bad > 0.0) {
            st_here = MPC_NUMERICAL;
            du0 = 0.0;
            du1 = 0.0;
        } else if (st_here == MPC_OK) {
            double inf = 0.0;
#pragma unroll
            for (int j = 0; j < NR; ++j)
                if (ron[j] && rxi[j] > 1e-6 * (1.0 + fabs(bk[j]))) inf = 1.0;
            if (Q.max(inf) > 0.0) st_here = MPC_INFEASIBLE;
        }
        }
        wave_sync();
        }   // phase 1: interior point

        // ---- active-set polish (oracle polish()) ----------------------------
        PROF(8)
        if (Pr.polish && bad == 0.0) {
            // opaque copies of the row bounds (see the interior-point loop): nothing the polish derives
            // from them is hoisted into long-lived registers
            double bkp[NR], bbp[NBOX];
#pragma unroll
            for (int j = 0; j < NR; ++j) { bkp[j] = bk[j]; asm volatile("" : "+v"(bkp[j])); }
#pragma unroll
            for (int j = 0; j < NBOX; ++j) { bbp[j] = bb[j]; asm volatile("" : "+v"(bbp[j])); }
            // class per row: 0 inactive, 1 active (equality), 2 violated (multiplier fixed at rho)
            int cls[NR], clb[NBOX];
#pragma unroll
            for (int j = 0; j < NR; ++j) cls[j] = !ron[j] ? 0 : (rxi[j] > rnu[j] ? 2 : (rl[j] > rs[j] ? 1 : 0));
#pragma unroll
            for (int j = 0; j < NBOX; ++j) clb[j] = (live && lb[j] > sb[j]) ? 1 : 0;
            if (MODE == MODE_FULL && phase == 0 && sqp > 0) {
                // re-linearisation: the crossover starts from the previous QP's classification
#pragma unroll
                for (int j = 0; j < NR; ++j) cls[j] = ron[j] ? (wcls >> (2 * j)) & 3 : 0;
#pragma unroll
                for (int j = 0; j < NBOX; ++j) clb[j] = live ? (wcls >> (2 * NR + j)) & 1 : 0;
            }
            // the interior-point iterate (du, x4) is the start of every round and the fallback
            double pu0 = du0, pu1 = du1;
            double nviol_acc = 0.0;
            const int rounds = phase == 0 ? XO_ROUNDS : (chk ? CHECK_ROUNDS : POLISH_ROUNDS);
            for (int round = 0; round < rounds; ++round) {
                double tl[NR], tlb[NBOX];
#pragma unroll
                for (int j = 0; j < NR; ++j) tl[j] = rl[j];
#pragma unroll
                for (int j = 0; j < NBOX; ++j) tlb[j] = lb[j];
                if (live) {
                    double Qp[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
                    for (int j = 0; j < NR; ++j) {
                        const double w = cls[j] == 1 ? 1.0 / POLISH_DELTA : 0.0;
#pragma unroll
                        for (int a = 0; a < 4; ++a)
#pragma unroll
                            for (int c = a; c < 4; ++c)
                                if (row_nz(rid<OBS>(j), a) && row_nz(rid<OBS>(j), c))
                                    Qp[p4(a, c)] = fma(w * cf[j][a], cf[j][c], Qp[p4(a, c)]);
                    }
                    double Qs[10], qs[4];
                    stage_cost(LITE ? cstr : S.cst + 6 * k, Pr.w_d, Pr.w_o, Pr.w_v, Qs, qs);
#pragma unroll
                    for (int a = 0; a < 4; ++a)
#pragma unroll
                        for (int c = 0; c < 4; ++c) S.QR[QRS * k + 4 * st4(a) + c] = Qp[p4(a, c)] + Qs[p4(a, c)];
                    S.Rt[2 * (k - 1)] = R0 + (clb[0] + clb[1]) * (1.0 / POLISH_DELTA);
                    S.Rt[2 * (k - 1) + 1] = R1 + (clb[2] + clb[3]) * (1.0 / POLISH_DELTA);
                }
                wave_sync();
                riccati_factor<NT, FAC_CF>(S, N, dt, gl);
                double xp[4] = {x4[0], x4[1], x4[2], x4[3]};
                pu0 = du0;
                pu1 = du1;
                // the crossover from the all-inactive classification solves the unconstrained LQR: the first solve
                // is its exact optimum (no active-row penalties to refine), so it runs one solve, not
                // POLISH_REFINE (oracle polish_from, host backend active_set)
                const int nref = (phase == 0 && !(MODE == MODE_FULL && sqp > 0)) ? 1 : POLISH_REFINE;
#pragma unroll 1
                for (int r = 0; r < nref; ++r) {
                    // exact KKT residual of the equality QP -> LQR right-hand side
                    double r2[NR], r2b[NBOX];
#pragma unroll
                    for (int j = 0; j < NR; ++j) r2[j] = (cls[j] == 1) ? bkp[j] - rdot(rid<OBS>(j), cf[j], xp) : 0.0;
#pragma unroll
                    for (int j = 0; j < NBOX; ++j) r2b[j] = (clb[j] == 1) ? bbp[j] - bsign(j) * (j < 2 ? pu0 : pu1) : 0.0;
                    if (live) {
                        double q4[4] = {0, 0, 0, 0}, g0 = 0.0, g1 = 0.0;
#pragma unroll
                        for (int j = 0; j < NR; ++j) {
                            const double wgt = (cls[j] == 2) ? rho : (cls[j] == 1 ? tl[j] + r2[j] * (1.0 / POLISH_DELTA) : 0.0);
#pragma unroll
                            for (int a = 0; a < 4; ++a)
                                if (row_nz(rid<OBS>(j), a)) q4[a] = fma(cf[j][a], wgt, q4[a]);
                        }
#pragma unroll
                        for (int j = 0; j < NBOX; ++j) {
                            const double v = (clb[j] == 1) ? bsign(j) * (tlb[j] + r2b[j] * (1.0 / POLISH_DELTA)) : 0.0;
                            if (j < 2) g0 += v; else g1 += v;
                        }
                        double Qs[10], qs[4], ub0, ub1;
                        stage_cost(LITE ? cstr : S.cst + 6 * k, Pr.w_d, Pr.w_o, Pr.w_v, Qs, qs);
                        ld2(S.ub + 2 * (k - 1), ub0, ub1);        // reads before the writes (see ac_rows)
#pragma unroll
                        for (int a = 0; a < 4; ++a) {
                            double acc = qs[a];
#pragma unroll
                            for (int c = 0; c < 4; ++c) acc = fma(Qs[p4(a, c)], xp[c], acc);
                            S.QH[QHS * k + st4(a)] = q4[a] - acc;
                        }
                        S.QH[QHS * k + 3] = 0.0;
                        S.QH[QHS * k + 5] = 0.0;
                        *reinterpret_cast<double2*>(S.gh + 2 * (k - 1)) =
                            make_double2(g0 - fma(R0, pu0, R0 * ub0), g1 - fma(R1, pu1, R1 * ub1));
                    }
                    wave_sync();
                    // the crossover (phase 0) solves in K-row form wherever the two-phase launch exists
                    // (G >= 2): the MODE_XO launch has no AC rows (lite LDS layout), and MODE_FULL must give
                    // bit-identical results.  GL = 64 (G = 1) is never split and keeps the AC rows (the
                    // K-row crossover cost C5 4%).
                    if (ACL && (phase == 1 || GL == 64)) riccati_solve<NTR, ACL>(S, N, dt, gl);
                    else riccati_solve<NTR, false>(S, N, dt, gl);
                    {
                        double dx4[4];
#pragma unroll
                        for (int a = 0; a < 4; ++a) dx4[a] = live ? S.dX[5 * k + st4(a)] : 0.0;
#pragma unroll
                        for (int j = 0; j < NR; ++j)
                            if (cls[j] == 1) tl[j] += (r2[j] - rdot(rid<OBS>(j), cf[j], dx4)) * (1.0 / POLISH_DELTA);
                        const double dd0 = live ? S.dud[2 * (k - 1)] : 0.0, dd1 = live ? S.dud[2 * (k - 1) + 1] : 0.0;
#pragma unroll
                        for (int j = 0; j < NBOX; ++j)
                            if (clb[j] == 1) tlb[j] += (r2b[j] - bsign(j) * (j < 2 ? dd0 : dd1)) * (1.0 / POLISH_DELTA);
#pragma unroll
                        for (int a = 0; a < 4; ++a) xp[a] += dx4[a];
                        pu0 += dd0;
                        pu1 += dd1;
                    }
                    wave_sync();
                }
                // acceptance: KKT consistency; otherwise flip every offending row and retry
                double lmax = 1.0;
#pragma unroll
                for (int j = 0; j < NR; ++j)
                    if (cls[j] == 1) lmax = vmaxabs(lmax, tl[j]);
#pragma unroll
                for (int j = 0; j < NBOX; ++j)
                    if (clb[j] == 1) lmax = vmaxabs(lmax, tlb[j]);
                lmax = Q.max(lmax);
                // a row is offending when its KKT condition fails (oracle polish_from: bad > 0); only the
                // flags matter, so no division by the scales (each IEEE division is ~10 instructions)
                double worst = 0.0, nviol = 0.0, finite = 1.0;
                bool flip[NR], flipb[NBOX];
                if (live && (!(pu0 == pu0) || !(pu1 == pu1))) finite = 0.0;
#pragma unroll
                for (int j = 0; j < NR; ++j) {
                    flip[j] = false;
                    if (!ron[j]) continue;
                    const double bsc = 1.0 + fabs(bkp[j]);
                    const double r = rdot(rid<OBS>(j), cf[j], xp) - bkp[j];
                    bool badv;
                    if (cls[j] == 1) {
                        badv = tl[j] < -1e-9 * lmax || tl[j] > rho * (1.0 + 1e-9) || fabs(r) > 1e-7 * bsc;
                    } else if (cls[j] == 2) {
                        badv = r > 1e-9 * bsc;
                        if (r < -1e-6 * bsc) nviol += 1.0;
                    } else {
                        badv = r < -1e-9 * bsc;
                    }
                    if (badv) worst = 1.0;
                    flip[j] = badv;
                }
#pragma unroll
                for (int j = 0; j < NBOX; ++j) {
                    flipb[j] = false;
                    if (!live) continue;
                    const double bsc = 1.0 + fabs(bbp[j]);
                    const double r = bsign(j) * (j < 2 ? pu0 : pu1) - bbp[j];
                    const bool badv = clb[j] == 1 ? (tlb[j] < -1e-9 * lmax || fabs(r) > 1e-7 * bsc) : r < -1e-9 * bsc;
                    if (badv) worst = 1.0;
                    flipb[j] = badv;
                }
                worst = Q.max(worst);
                nviol = Q.sum(nviol);
                finite = Q.min(finite);
                if (finite == 0.0) break;
                if (worst == 0.0) {
                    accepted = true;
                    nviol_acc = nviol;
                    break;
                }
#pragma unroll
                for (int j = 0; j < NR; ++j)
                    if (flip[j]) cls[j] = (cls[j] == 1) ? (tl[j] > rho ? 2 : 0) : 1;
#pragma unroll
                for (int j = 0; j < NBOX; ++j)
                    if (flipb[j]) clb[j] = 1 - clb[j];
                wave_sync();
            }
            if (MODE == MODE_FULL && nsqp > 1) {
                wcls = 0;
#pragma unroll
                for (int j = 0; j < NR; ++j) wcls |= cls[j] << (2 * j);
#pragma unroll
                for (int j = 0; j < NBOX; ++j) wcls |= clb[j] << (2 * NR + j);
            }
            if (accepted) {
                du0 = pu0;
                du1 = pu1;
                st_here = nviol_acc > 0.0 ? MPC_INFEASIBLE : MPC_OK;
            }
            wave_sync();
        }
        if (chk) {
            if (!accepted) {          // not certified: the interior point continues from the unchanged iterate
                chk = false;
                checked = true;
                continue;
            }
            total_it += it;
        }
        break;
        }   // segments
        if (phase == 0) xo_ok = accepted;
        if (accepted || phase == 1) break;
        }   // phases
        status = st_here;
        double ua0 = 0.0, ua1 = 0.0;       // this QP's linearisation point: U one QP back
        if (live) {
            ua0 = S.ub[2 * (k - 1)];
            ua1 = S.ub[2 * (k - 1) + 1];
            S.ub[2 * (k - 1)] = ua0 + du0;
            S.ub[2 * (k - 1) + 1] = ua1 + du1;
        }
        wave_sync();
        // SQP: stop once the re-linearised QP no longer moves U, on a 2-cycle, or after SQP_INF_STREAK elastic
        // QPs in a row (oracle orc_solve; all group-uniform)
        if (nsqp > 1) {
            const double stp = Q.max(live ? vmaxabs(fabs(du0), du1) : 0.0);
            const double b2 = Q.max(live ? vmaxabs(fabs((ua0 + du0) - pb0), (ua1 + du1) - pb1) : 0.0);
            pb0 = ua0;
            pb1 = ua1;
            ninf = status == MPC_INFEASIBLE ? ninf + 1 : 0;
            if (stp <= Pr.sqp_tol) { sqp_conv = true; break; }
            if (Pr.sqp_tol > 0.0 && ((sqp >= 2 && b2 <= SQP_CYCLE_REL * stp) || ninf >= SQP_INF_STREAK)) break;
        }
    }

    if (MODE == MODE_FULL && nsqp > 1 && Pr.sqp_tol > 0.0 && !sqp_conv) status |= MPC_SQP_UNCONVERGED;

    // ---- K5: outputs: U*, u0, predict(x0, U*) ----------------------------------------------
    PROF(9)
    // The instance index and x0 are recomputed / re-read here (from the lane id, the work list and an
    // opaque index that defeats CSE with the first load) rather than held in registers across the
    // interior point, where they would be spilled to scratch.
    int ln2 = __lane_id();
    asm volatile("" : "+v"(ln2));
    const int grp2 = ln2 / GL;
    {
        if (MODE == MODE_IPM) {
            const int cnt = *wcount;
            const int slot = blockIdx.x * G + grp2;
            bvalid = slot < cnt;
            b = wlist[bvalid ? slot : cnt - 1];
        } else {
            b = blockIdx.x * G + grp2;
            bvalid = b < B;
            if (!bvalid) b = B - 1;
        }
#pragma unroll
        for (int j = 0; j < 5; ++j) x0[j] = x0g[5 * (size_t)b + j];
    }
    predict_grp(tab, N, dt, x0, S.ub, S.Xr, S.kap, gl);
    if (MODE == MODE_XO && !xo_ok) {
        // not certified: defer to the MODE_IPM launch (group-uniform); S.ub is still the warm start and
        // S.Xr its rollout (a failed crossover leaves no state behind), which the stage cache keeps
        int slot = 0;
        if (bvalid && gl == 0) {
            if (Pr.dbg & 1) {
                slot = b;
            } else {
                slot = atomicAdd(wcount, 1);
                wlist[slot] = b;
            }
        }
        slot = __shfl(slot, grp2 * GL, WAVE);
        if (bvalid && stc) {
            double* o = stc + (size_t)slot * stage_cache_doubles(N);
            if (gl < N) {
                o[2 * gl] = S.ub[2 * gl];
                o[2 * gl + 1] = S.ub[2 * gl + 1];
            }
            for (int i = gl; i < 5 * NP; i += GL) o[2 * N + i] = S.Xr[i];
            if (LKC && gl <= N) {
                double2* lk = reinterpret_cast<double2*>(o + stage_cache_lk(N) + 8 * gl);
                lk[0] = make_double2(refk[1], refk[2]);
                lk[1] = make_double2(refk[3], refk[4]);
                lk[2] = make_double2(slk[0], slk[1]);
                lk[3] = make_double2(slk[2], slk[3]);
            }
            // the crossover's solve (the interior point's start): still in dud / dX (the epilogue's rollout
            // writes Xr and kap only)
            if (gl < N) {
                double* xo = o + stage_cache_xo(N) + 6 * gl;
                xo[0] = S.dud[2 * gl];
                xo[1] = S.dud[2 * gl + 1];
#pragma unroll
                for (int a = 0; a < 4; ++a) xo[2 + a] = S.dX[5 * (gl + 1) + st4(a)];
            }
        }
    } else if (bvalid) {
        // one 16-B store per lane (full cache lines, not two half-filled strided stores) when the caller's
        // buffers allow it; 8-B aligned views (e.g. a tensor slice at an odd offset) take two 8-B stores
        const bool a16 = ((((uintptr_t)Ug) | ((uintptr_t)u0g)) & 15) == 0;
        if (gl < N && Ug) {
            double* o = Ug + (size_t)b * 2 * N + 2 * gl;
            if (a16) {
                *reinterpret_cast<double2*>(o) = make_double2(S.ub[2 * gl], S.ub[2 * gl + 1]);
            } else {
                o[0] = S.ub[2 * gl];
                o[1] = S.ub[2 * gl + 1];
            }
        }
        if (Xg)
            for (int i = gl; i < 5 * NP; i += GL) Xg[(size_t)b * 5 * NP + i] = S.Xr[i];
        if (gl == 0) {
            if (u0g) {
                double* o = u0g + 2 * (size_t)b;
                if (a16) {
                    *reinterpret_cast<double2*>(o) = make_double2(S.ub[0], S.ub[1]);
                } else {
                    o[0] = S.ub[0];
                    o[1] = S.ub[1];
                }
            }
            if (statusg) statusg[b] = status;
            if (itersg) itersg[b] = total_it;
        }
    }
    PROF(10)
    PROF_END
}

__global__ void mpc_lookup_kernel(DevTable tab, int n, const double* __restrict__ s, double* __restrict__ st,
                                  double* __restrict__ ct) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double o[5], c[2];
    get_state(tab, s[i], o, nullptr);
    get_control(tab, s[i], c);
    if (st)
        for (int j = 0; j < 5; ++j) st[5 * (size_t)i + j] = o[j];
    if (ct) { ct[2 * (size_t)i] = c[0]; ct[2 * (size_t)i + 1] = c[1]; }
}
