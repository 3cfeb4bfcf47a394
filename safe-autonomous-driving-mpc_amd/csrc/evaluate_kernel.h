// evaluate_kernel.h -- the batched evaluator (mpc_evaluate_batch, include/mpcqp.h): for any control sequence U the
// nonlinear rollout predict(x0, U) (trajectory_tracking.py:87-114), the reference's cost (:116-152), its constraint
// rows (:155-211) and a per-instance summary of them.  No QP, no solver state.
//
// The solver's layout: one lane group of GL lanes per instance (GL = 16, 32, 64 by N + 1, 64 / GL instances per
// wavefront).  predict_grp rolls the instance out (lane 0 rolls s, k, v; lane j looks the table up at s_j; lane 0
// rolls d, o) and leaves lane j the whole reference state at s_j, so no table is searched twice.  Lane j = 1..N then
// owns stage j (its three cost terms, its 7 + n_obs rows, written straight to its slice of `rows`) and lane
// j = 0..N-1 owns control j (its two cost terms, its box excess).  Minima and counts go through Grp<GL>; the two
// sums whose bits must not depend on GL, the running cost and the L1 violation, are added by lane 0 from LDS in the
// order the header states.  Host restatement, bit for bit: mpcqp_cpu::evaluate_one (cpu_backend.h).
//
// Per-instance LDS (doubles): the rollout Xr [N+1][5], kap [N+1] (k_ref of the rollout; once the rollout is done,
// the L1 partial of stage j at kap[j-1]) and ct [N][5]: the cost terms (d, o, v) of stage j+1 and (u1, u2) of
// control j.  Until the rollout's first phase is over ct also stages U for lane 0.  The array is static, sized for
// the longest horizon of the lane group (N = GL - 1): 5.4 - 5.5 KB per wavefront for every GL.
#pragma once
#include "device_common.h"

__host__ __device__ constexpr int ev_lds_doubles(int N) { return (11 * N + 6 + 1) & ~1; }

// NaN-propagating running minimum (numpy's min): once a NaN was seen it stays
__device__ __forceinline__ void ev_nmin(double& m, bool& nan, double r) {
    if (!nan) {
        if (r != r) nan = true;
        else if (r < m) m = r;
    }
}

#define EV_NAN_ROW 1
#define EV_NAN_LANE 2
#define EV_NAN_OBS 4
#define EV_NAN_V 8
#define EV_NAN_BOX 16

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
    const double dt = Pr.dt;
    double* Xr = smem + grp * LD;
    double* kap = Xr + 5 * NP;
    double* ct = kap + NP;
    const double inf = __builtin_inf(), qnan = __builtin_nan("");

    double x0[5];
#pragma unroll
    for (int j = 0; j < 5; ++j) x0[j] = x0g[5 * (size_t)b + j];
    // the obstacle count as the solver reads it: NULL = all max_obs rows, clamped to [0, max_obs]
    int nobs = 0;
    const double* obs = nullptr;
    if (OBS) {
        nobs = nobsg ? nobsg[b] : Pr.max_obs;
        nobs = nobs < 0 ? 0 : (nobs > Pr.max_obs ? Pr.max_obs : nobs);
        obs = obsg + (size_t)b * Pr.max_obs * 2;
    }

    const bool ctrl = gl < N;                  // this lane owns control gl
    const bool stage = gl >= 1 && gl <= N;     // this lane owns stage gl
    double u1 = 0.0, u2 = 0.0;
    if (ctrl) {
        u1 = Ug[(size_t)b * 2 * N + 2 * gl];
        u2 = Ug[(size_t)b * 2 * N + 2 * gl + 1];
        ct[2 * gl] = u1;
        ct[2 * gl + 1] = u2;
    }
    wave_sync();
    double st[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    predict_grp(tab, N, dt, x0, ct, Xr, kap, gl, st, nullptr);
    // lane 0 read U from ct before predict_grp's first barrier; ct and kap are free from here on

    // ---- control gl: cost terms and the excess over the bounds handed to SLSQP (:249-252) ----
    double bx = 0.0;
    bool bxnan = false;
    if (ctrl) {
        ct[5 * gl + 3] = Pr.w_u1 * (u1 * u1);
        ct[5 * gl + 4] = Pr.w_u2 * (u2 * u2);
        const double e[4] = {Pr.u_min0 - u1, u1 - Pr.u_max0, Pr.u_min1 - u2, u2 - Pr.u_max1};
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            if (e[a] != e[a]) bxnan = true;
            else if (e[a] > bx) bx = e[a];
        }
    }

    // ---- stage gl: cost terms and rows, visited in the reference's order ----------------------
    double smin = inf, p1 = 0.0, fl = inf, fo = inf, fv = inf;
    bool snan = false, flnan = false, fonan = false, fvnan = false;
    int skind = 0, nneg = 0;
    if (stage) {
        const double s = Xr[5 * gl], d = Xr[5 * gl + 1], o = Xr[5 * gl + 2], v = Xr[5 * gl + 4];
        const double ed = d - st[1], eo = o - st[2], ev = v - st[4];
        ct[5 * (gl - 1)] = Pr.w_d * (ed * ed);
        ct[5 * (gl - 1) + 1] = Pr.w_o * (eo * eo);
        ct[5 * (gl - 1) + 2] = Pr.w_v * (ev * ev);
        double* ro = bvalid && rowg ? rowg + ((size_t)b * N + (gl - 1)) * rw : nullptr;
        auto visit = [&](double r, int kind) {
            if (!snan && (r != r || r < smin)) {
                smin = r;
                skind = kind;
                snan = r != r;
            }
            p1 = p1 + (r != r ? r : (r < 0.0 ? -r : 0.0));
            nneg += r < 0.0 ? 1 : 0;
            if (ro) ro[kind] = r;
        };
        const double sl = Pr.sl;
        const double vf = d + (Pr.L / 2.0) * o, vl = d + Pr.L * o;
        const double g[6] = {sl - d, d + sl, sl - vf, vf + sl, sl - vl, vl + sl};
#pragma unroll
        for (int a = 0; a < 6; ++a) {
            visit(g[a], a);
            ev_nmin(fl, flnan, g[a]);
        }
        if (OBS) {
            const double tk = (double)gl * dt;
            const double vt = v * Pr.tgap;
            const double safe = vt > Pr.osd ? vt : Pr.osd;       // the reference's max(osd, v * tgap)
            for (int i = 0; i < nobs; ++i) {
                const double sop = obs[2 * i] + obs[2 * i + 1] * tk;
                const double r = (sop - s) - safe;
                visit(r, 7 + i);
                ev_nmin(fo, fonan, r);
            }
        }
        if (ro)
            for (int i = 7 + nobs; i < rw; ++i) ro[i] = qnan;
        visit(v, 6);
        ev_nmin(fv, fvnan, v);
        kap[gl - 1] = p1;
    }

    // ---- group summary -------------------------------------------------------------------------
    const int myflags = (snan ? EV_NAN_ROW : 0) | (flnan ? EV_NAN_LANE : 0) | (fonan ? EV_NAN_OBS : 0) |
                        (fvnan ? EV_NAN_V : 0) | (bxnan ? EV_NAN_BOX : 0);
    const int flags = (int)__double_as_longlong(Q.reduce(__longlong_as_double((long long)myflags), [](double a, double c) {
        return __longlong_as_double(__double_as_longlong(a) | __double_as_longlong(c));
    }));
    const bool anyn = (flags & EV_NAN_ROW) != 0;
    const double m = Q.min(stage && !snan ? smin : inf);
    // np.argmin: the first NaN row if there is one, else the first row equal to the minimum
    const bool mine = stage && (anyn ? snan : (!snan && smin == m));
    const int astage = (int)Q.min(mine ? (double)gl : 1e9);
    const double mfirst = Q.get(smin, astage);                  // the first minimum's own bits
    const double minrow = anyn ? qnan : mfirst;
    const int akind = __shfl(skind, Q.base + astage, WAVE);
    const double cnt = Q.sum((double)nneg);
    const double mlane = Q.min(fl), mobs = Q.min(fo), mv = Q.min(fv), mbox = Q.max(bx);
    wave_sync();

    if (bvalid && gl == 0) {
        // the reference's running cost: stages 1..N (d, o, v), then controls 0..N-1 (u1, u2), one sum
        double cost = 0.0, t[5] = {0.0, 0.0, 0.0, 0.0, 0.0}, l1 = 0.0;
        for (int j = 0; j < N; ++j) {
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                cost = cost + ct[5 * j + a];
                t[a] = t[a] + ct[5 * j + a];
            }
            l1 = l1 + kap[j];
        }
        for (int j = 0; j < N; ++j) {
#pragma unroll
            for (int a = 3; a < 5; ++a) {
                cost = cost + ct[5 * j + a];
                t[a] = t[a] + ct[5 * j + a];
            }
        }
        if (sumg) {
            double* o = sumg + (size_t)b * MPC_EV_NQ;
            o[MPC_EVQ_COST] = cost;
            o[MPC_EVQ_MIN_ROW] = minrow;
            o[MPC_EVQ_ARGMIN_STAGE] = (double)astage;
            o[MPC_EVQ_ARGMIN_KIND] = (double)akind;
            o[MPC_EVQ_L1] = l1;
            o[MPC_EVQ_N_NEG] = cnt;
            // + 0.0: a minimum of -0.0 and 0.0 comes out as 0.0 whichever the reduction met first
            o[MPC_EVQ_MIN_LANE] = (flags & EV_NAN_LANE) ? qnan : mlane + 0.0;
            o[MPC_EVQ_MIN_OBS] = ((flags & EV_NAN_OBS) || nobs == 0) ? qnan : mobs + 0.0;
            o[MPC_EVQ_MIN_V] = (flags & EV_NAN_V) ? qnan : mv + 0.0;
            o[MPC_EVQ_BOX] = (flags & EV_NAN_BOX) ? qnan : mbox + 0.0;
        }
        if (termg) {
#pragma unroll
            for (int a = 0; a < 5; ++a) termg[(size_t)b * 5 + a] = t[a];
        }
    }
    if (bvalid && Xg)
        for (int i = gl; i < 5 * NP; i += GL) Xg[(size_t)b * 5 * NP + i] = Xr[i];
}
