// riccati_lanes.h -- the lane-distributed Riccati recursions of the solver kernel (factorisation, backward and
// forward solves; inline-asm v_fmac_f64_dpp chains, checked by tools/dpp_hazard_check.py), and the stage-wise
// helpers next to them (dual_norms, stage_cost).
#pragma once
#include "device_common.h"

// ------------------------------------------------------------------------------------------
// distributed recursions.  The Riccati factorisation and solves run on lanes i = 0..4 of each
// lane group: lane i holds row i of P (factorisation), component i of the co-state p (backward
// solve) and of the state direction x (forward solve).  Every cross-lane term is a
// v_fmac_f64_dpp with row_newbcast:l, i.e. a broadcast of lane l's register within its 16-lane row
// fused into the FMA (same issue cost as a plain v_fmac_f64 on gfx950).  Compared with running the
// whole 5x5 recursion redundantly on every lane, a stage costs ~90 instead of ~210 VALU
// instructions.  The other lanes of the group compute discarded values (their per-lane records are
// clamped to lane 4's; their stores are masked off).  Groups are aligned to 16-lane rows, so the
// broadcasts never cross groups.
// ------------------------------------------------------------------------------------------
// dst += src@L * c  (src broadcast from lane L of each 16-lane row); asm operand lists are written
// with early-clobber accumulators, so no accumulator shares a register with a source.  The leading
// s_nop 1 covers the VALU-write -> DPP-read hazard (2 wait states) of the sources.
#define DPPF(d, s, c, L) "v_fmac_f64_dpp " d ", " s ", " c " row_newbcast:" #L " row_mask:0xf bank_mask:0xf\n\t"
// dst -= src@L * c (DPP source negation modifier)
#define DPPFN(d, s, c, L) "v_fmac_f64_dpp " d ", -" s ", " c " row_newbcast:" #L " row_mask:0xf bank_mask:0xf\n\t"


// Per-lane constants of the distributed recursions.  A_t = I + J'_t with J' nonzero in rows 0..2 only:
// J'(0,4) = dt, J'(1,2) = a12, J'(1,4) = a14, J'(2,0) = a20, J'(2,3) = a23, J'(2,4) = a24.  Lane i needs
// e_l(i) = J'(l,i) (column i; backward recursions) and f_m(i) = J'(i,m) (row i; forward solve).  Both
// are gathered per lane from the stage's A5 record (a12, a14, a20, a23, a24, dt, 0, 0): oXX is the
// record offset a lane reads (6 = a zero slot).
struct DLane {
    int i;                     // row / component of this lane (clamped to 4 for lanes >= 5)
    int oe1, oe2, of0, of2, of3, of4;
    double e0;                 // J'(0,i) = dt for i = 4 (constant)
    double bu;                 // B(i,:) u = bu * u_r: dt on lanes 3 (r = 0) and 4 (r = 1), else 0
    int kr, ur;                // K row r the lane reads in the forward solve (offset kr = 6 r in KR), r
    int ps;                    // slot of p_i in the backward solve's co-state record: (i + 2) % 5
    double k0, k1, k2, k3;     // symmetrisation: lane keeps its own P(i,j) when i <= j
    double r1, r2, r3, r4;     // lane is row 1, 2, 3, 4
};
__device__ __forceinline__ DLane dlane(int gl, double dt) {
    // opaque lane index: the constants are rebuilt at every recursion (a few VALU) instead of being
    // hoisted out of the interior-point loop and held in registers across the row phases
    asm volatile("" : "+v"(gl));
    DLane D;
    D.i = gl < 5 ? gl : 4;
    const int z = 6;
    D.oe1 = gl == 2 ? 0 : (gl == 4 ? 1 : z);
    D.oe2 = gl == 0 ? 2 : (gl == 3 ? 3 : (gl == 4 ? 4 : z));
    D.of0 = gl == 2 ? 2 : z;
    D.of2 = gl == 1 ? 0 : z;
    D.of3 = gl == 2 ? 3 : z;
    D.of4 = gl == 0 ? 5 : (gl == 1 ? 1 : (gl == 2 ? 4 : z));
    D.e0 = gl == 4 ? dt : 0.0;
    D.bu = gl >= 3 ? dt : 0.0;
    D.ur = gl >= 4 ? 1 : 0;
    D.kr = 6 * D.ur;
    D.ps = gl >= 3 ? gl - 3 : gl + 2;
    D.k0 = gl <= 0 ? 1.0 : 0.0;
    D.k1 = gl <= 1 ? 1.0 : 0.0;
    D.k2 = gl <= 2 ? 1.0 : 0.0;
    D.k3 = gl <= 3 ? 1.0 : 0.0;
    D.r1 = gl == 1 ? 1.0 : 0.0;
    D.r2 = gl == 2 ? 1.0 : 0.0;
    D.r3 = gl == 3 ? 1.0 : 0.0;
    D.r4 = gl == 4 ? 1.0 : 0.0;
    return D;
}

// Riccati factorisation of  min sum 0.5 x'Qt x + 0.5 u'Rt u,  x_{t+1} = A_t x_t + B u_t,  x_0 = 0.
// Per stage: S = Rt + B'P B = Ls Ls', M = P A, W = Ls^-1 B'M, K = -Ls^-T W, P <- A'M - W'W + Qt.  The
// Cholesky form keeps ~2 more digits than an explicit S^-1 once barrier weights reach 1e12 (DESIGN.md
// section 3); Qt is added last for the same reason (adding it before the cancellation A'M - W'W would
// round that difference at Qt's magnitude).  Lane i: row i of M locally; the W terms from M(3,i),
// M(4,i); row i of A'M and of W'W by broadcasts.  Restates riccati_factor() of oracle/mpc_oracle.c.
struct FacRec { double a[5], r0, r1, e1, e2, q[4]; };
__device__ __forceinline__ void load_fac(const Lds& S, const DLane& L, int t, FacRec& F) {
    const double* a5 = S.A5 + A5S * t;
    ld_a5(a5, F.a);
    ld2(S.Rt + 2 * t, F.r0, F.r1);
    F.e1 = a5[L.oe1];
    F.e2 = a5[L.oe2];
    ld2(S.QR + QRS * t + 4 * L.i, F.q[0], F.q[1]);
    ld2(S.QR + QRS * t + 4 * L.i + 2, F.q[2], F.q[3]);
}
// CF: the copy-free form (the A'M block reads p1, p3, p4 from its in-place accumulators, so pr[1], pr[3], pr[4]
// need no register copies, and a bare pivot floor): 4 instructions fewer per stage, bit-identical.  The obstacle
// kernels use it (C3 -0.7%); in the obstacle-free N = 20 interior-point kernel the same code measured +0.3%
// (300-launch A/B), so it keeps the plain form
template <bool CF>
__device__ __forceinline__ void fac_step(const Lds& S, const DLane& L, int t, bool upd, double dt, double dt2,
                                         const FacRec& F, double pr[5]) {
    const double a12 = F.a[0], a14 = F.a[1], a20 = F.a[2], a23 = F.a[3], a24 = F.a[4];
    // S = Rt + dt^2 P[{3,4},{3,4}]: P(3,3), P(3,4) from lane 3, P(4,4) from lane 4
    double s00 = F.r0, s01 = 0.0, s11 = F.r1;
    asm("s_nop 1\n\t" DPPF("%0", "%3", "%5", 3) DPPF("%1", "%4", "%5", 3) DPPF("%2", "%4", "%5", 4)
        : "+&v"(s00), "+&v"(s01), "+&v"(s11) : "v"(pr[3]), "v"(pr[4]), "v"(dt2));
    // pivot floors: never active in practice (s00 >= Rt >= 2 w_u1 > 0); a NaN pivot is floored too, the
    // NaN still reaches P and K through V and M
    if constexpr (CF) {
        // bare v_max_f64 (as vmax): fmax first quiets the asm result with a v_max_f64 x, x, x
        const double floor_ = 1e-300;
        asm("v_max_f64 %0, %0, %1" : "+v"(s00) : "s"(floor_));
    } else {
        s00 = fmax(s00, 1e-300);
    }
    const double il00 = frsqrt(s00), l10 = s01 * il00;
    const double r11 = fmax(s11 - l10 * l10, 1e-14 * s11);
    const double il11 = frsqrt(r11);
    const double c0 = dt * il00, c1 = dt * il11, c2 = -l10 * il11;
    // row i of M = P A (local)
    double m[5];
    // (update stages: m[0], m[2..4] are formed inside the A'M block below, so that block needs no s_nop)
    if (!upd) {
        m[0] = fma(pr[2], a20, pr[0]);
        m[1] = pr[1];
        m[2] = fma(pr[1], a12, pr[2]);
        m[3] = fma(pr[2], a23, pr[3]);
        m[4] = fma(pr[0], dt, fma(pr[1], a14, fma(pr[2], a24, pr[4])));
    }
    // row i of A'M = M(i,:) + sum_l J'(l,i) M(l,:), and V3 = M(3,i), V4 = M(4,i) = P(i,{3,4}) +
    // sum_l J'(l,i) P(l,{3,4}), all in place.  Source lane l only changes in the broadcast of a lane l'
    // with J'(l',l) != 0; with J' nonzero at (0,4), (1,2), (1,4), (2,0), (2,3), (2,4) the order l = 0, 2, 1
    // reads every source lane before its own update (a zero coefficient leaves a value unchanged).
    // The same register is written and then broadcast 7 instructions later (the DPP hazard needs 2).
    double v3 = pr[3], v4 = pr[4];
    if (upd) {
        // The VALU-write -> DPP-read hazard (2 wait states) without an s_nop: the block first forms the rows of
        // M = P A it broadcasts (the same fma()s as above, in the same order), so every register a DPP reads was
        // written at least 2 instructions earlier inside the block (m[0] 5 before the first broadcast, m[4]
        // 4 before its own), and whatever the compiler wrote before the block is 6 or more instructions back.
        m[1] = pr[1];
        if constexpr (!CF) {
        asm("v_fma_f64 %0, %10, %13, %11\n\t"          // m0 = fma(p2, a20, p0)
            "v_fma_f64 %2, %12, %14, %10\n\t"          // m2 = fma(p1, a12, p2)
            "v_fma_f64 %3, %10, %15, %16\n\t"          // m3 = fma(p2, a23, p3)
            "v_fma_f64 %4, %10, %17, %18\n\t"          // t = fma(p2, a24, p4)
            "v_fma_f64 %4, %12, %19, %4\n\t"           // t = fma(p1, a14, t)
            "v_fma_f64 %4, %11, %20, %4\n\t"           // m4 = fma(p0, dt, t)
            DPPF("%0", "%0", "%7", 0) DPPF("%1", "%1", "%7", 0) DPPF("%2", "%2", "%7", 0) DPPF("%3", "%3", "%7", 0)
            DPPF("%4", "%4", "%7", 0) DPPF("%5", "%5", "%7", 0) DPPF("%6", "%6", "%7", 0)
            DPPF("%0", "%0", "%8", 2) DPPF("%1", "%1", "%8", 2) DPPF("%2", "%2", "%8", 2) DPPF("%3", "%3", "%8", 2)
            DPPF("%4", "%4", "%8", 2) DPPF("%5", "%5", "%8", 2) DPPF("%6", "%6", "%8", 2)
            DPPF("%0", "%0", "%9", 1) DPPF("%1", "%1", "%9", 1) DPPF("%2", "%2", "%9", 1) DPPF("%3", "%3", "%9", 1)
            DPPF("%4", "%4", "%9", 1) DPPF("%5", "%5", "%9", 1) DPPF("%6", "%6", "%9", 1)
            : "=&v"(m[0]), "+&v"(m[1]), "=&v"(m[2]), "=&v"(m[3]), "=&v"(m[4]), "+&v"(v3), "+&v"(v4)
            : "v"(L.e0), "v"(F.e2), "v"(F.e1), "v"(pr[2]), "v"(pr[0]), "v"(pr[1]),
              "v"(a20), "v"(a12), "v"(a23), "v"(pr[3]), "v"(a24), "v"(pr[4]), "v"(a14), "v"(dt));
        } else {
        // p1, p3, p4 are read from the in-place accumulators m1, v3, v4 themselves (they still hold them: the
        // broadcasts come after the six fma()s), so pr[1], pr[3], pr[4] need no copies of their own
        asm("v_fma_f64 %0, %10, %12, %11\n\t"          // m0 = fma(p2, a20, p0)
            "v_fma_f64 %2, %1, %13, %10\n\t"           // m2 = fma(p1, a12, p2)
            "v_fma_f64 %3, %10, %14, %5\n\t"           // m3 = fma(p2, a23, p3)
            "v_fma_f64 %4, %10, %15, %6\n\t"           // t = fma(p2, a24, p4)
            "v_fma_f64 %4, %1, %16, %4\n\t"            // t = fma(p1, a14, t)
            "v_fma_f64 %4, %11, %17, %4\n\t"           // m4 = fma(p0, dt, t)
            DPPF("%0", "%0", "%7", 0) DPPF("%1", "%1", "%7", 0) DPPF("%2", "%2", "%7", 0) DPPF("%3", "%3", "%7", 0)
            DPPF("%4", "%4", "%7", 0) DPPF("%5", "%5", "%7", 0) DPPF("%6", "%6", "%7", 0)
            DPPF("%0", "%0", "%8", 2) DPPF("%1", "%1", "%8", 2) DPPF("%2", "%2", "%8", 2) DPPF("%3", "%3", "%8", 2)
            DPPF("%4", "%4", "%8", 2) DPPF("%5", "%5", "%8", 2) DPPF("%6", "%6", "%8", 2)
            DPPF("%0", "%0", "%9", 1) DPPF("%1", "%1", "%9", 1) DPPF("%2", "%2", "%9", 1) DPPF("%3", "%3", "%9", 1)
            DPPF("%4", "%4", "%9", 1) DPPF("%5", "%5", "%9", 1) DPPF("%6", "%6", "%9", 1)
            : "=&v"(m[0]), "+&v"(m[1]), "=&v"(m[2]), "=&v"(m[3]), "=&v"(m[4]), "+&v"(v3), "+&v"(v4)
            : "v"(L.e0), "v"(F.e2), "v"(F.e1), "v"(pr[2]), "v"(pr[0]),
              "v"(a20), "v"(a12), "v"(a23), "v"(a24), "v"(a14), "v"(dt));
        }
    } else {
        asm("s_nop 1\n\t" DPPF("%0", "%0", "%2", 0) DPPF("%1", "%1", "%2", 0) "s_nop 1\n\t"
            DPPF("%0", "%0", "%3", 2) DPPF("%1", "%1", "%3", 2) "s_nop 1\n\t"
            DPPF("%0", "%0", "%4", 1) DPPF("%1", "%1", "%4", 1)
            : "+v"(v3), "+v"(v4) : "v"(L.e0), "v"(F.e2), "v"(F.e1));
    }
    double* am = m;
    double w0, w1, K1, K0;
    if (upd) {
        // W, K and then P -= W'W: the block first forms w0, w1, K1, K0 (the same operations as below, in the
        // same order, no contraction), so w1 is 4 instructions old at its first broadcast: no s_nop
        double tt;
        asm("v_mul_f64 %5, %9, %10\n\t"                // w0 = c0 * v3
            "v_mul_f64 %7, %11, %5\n\t"                // t = c2 * w0
            "v_fma_f64 %6, %12, %13, %7\n\t"           // w1 = fma(c1, v4, t)
            "v_mul_f64 %8, -%6, %14\n\t"               // K1 = -w1 * il11
            "v_mul_f64 %7, %15, %8\n\t"                // t = l10 * K1
            "v_add_f64 %7, %5, %7\n\t"                 // t = w0 + t
            "v_mul_f64 %7, -%7, %16\n\t"               // K0 = -t * il00
            DPPFN("%0", "%6", "%6", 0) DPPFN("%1", "%6", "%6", 1) DPPFN("%2", "%6", "%6", 2)
            DPPFN("%3", "%6", "%6", 3) DPPFN("%4", "%6", "%6", 4) DPPFN("%0", "%5", "%5", 0) DPPFN("%1", "%5", "%5", 1)
            DPPFN("%2", "%5", "%5", 2) DPPFN("%3", "%5", "%5", 3) DPPFN("%4", "%5", "%5", 4)
            : "+&v"(am[0]), "+&v"(am[1]), "+&v"(am[2]), "+&v"(am[3]), "+&v"(am[4]), "=&v"(w0), "=&v"(w1),
              "=&v"(tt), "=&v"(K1)
            : "v"(c0), "v"(v3), "v"(c2), "v"(c1), "v"(v4), "v"(il11), "v"(l10), "v"(il00));
        K0 = tt;
    } else {
        w0 = c0 * v3;
        w1 = fma(c1, v4, c2 * w0);
        K1 = -w1 * il11;
        K0 = -(w0 + l10 * K1) * il00;
    }
    // K by rows (lane i writes column i); the Cholesky factor of S is group-uniform: all five lanes write
    // the same values
    S.KR[KRS * t + L.i] = K0;
    S.KR[KRS * t + 6 + L.i] = K1;
    S.Si[SIS * t] = il00;
    S.Si[SIS * t + 1] = l10;
    S.Si[SIS * t + 2] = il11;
    if (upd) {
        // P(i,j) = A'M(i,j) - W1_i W1_j - W0_i W0_j (done above) + Qt(i,j), then the symmetrisation: lane i
        // takes P(j,i) from row j for j < i, so P is exactly symmetric (the upper triangle is the reference,
        // as in the oracle's packed recursion).  Lane-computed lower entries differ by rounding, and with
        // barrier weights near 1e12 that asymmetry costs interior-point iterations on hard elastic instances.
        // The block forms P's rows and the kept upper entries first (plain additions and products, no
        // contraction), so each broadcast row is 5 or more instructions old: no s_nop
        double sy0, sy1, sy2, sy3, p0, p1, p2, p4;
        asm("v_add_f64 %5, %9, %13\n\t"                // p1 = am1 + q1
            "v_add_f64 %6, %10, %14\n\t"               // p2 = am2 + q2
            "v_add_f64 %7, %12, %15\n\t"               // p4 = am4 + q3
            "v_add_f64 %4, %8, %16\n\t"                // p0 = am0 + q0
            "v_mul_f64 %1, %5, %18\n\t"                // sy1 = p1 * k1
            "v_mul_f64 %2, %6, %19\n\t"                // sy2 = p2 * k2
            "v_mul_f64 %3, %11, %20\n\t"               // sy3 = am3 * k3
            "v_mul_f64 %0, %4, %17\n\t"                // sy0 = p0 * k0
            DPPF("%0", "%5", "%21", 0) DPPF("%1", "%6", "%22", 1) DPPF("%2", "%11", "%23", 2)
            DPPF("%3", "%7", "%24", 3) DPPF("%0", "%6", "%22", 0) DPPF("%1", "%11", "%23", 1) DPPF("%2", "%7", "%24", 2)
            DPPF("%0", "%11", "%23", 0) DPPF("%1", "%7", "%24", 1) DPPF("%0", "%7", "%24", 0)
            : "=&v"(sy0), "=&v"(sy1), "=&v"(sy2), "=&v"(sy3), "=&v"(p0), "=&v"(p1), "=&v"(p2), "=&v"(p4)
            : "v"(am[0]), "v"(am[1]), "v"(am[2]), "v"(am[3]), "v"(am[4]), "v"(F.q[1]), "v"(F.q[2]), "v"(F.q[3]),
              "v"(F.q[0]), "v"(L.k0), "v"(L.k1), "v"(L.k2), "v"(L.k3), "v"(L.r1), "v"(L.r2), "v"(L.r3), "v"(L.r4));
        (void)p0;
        pr[0] = sy0;
        pr[1] = sy1;
        pr[2] = sy2;
        pr[3] = sy3;
        pr[4] = p4;
    }
}
// NT > 0: horizon fixed at compile time, stages fully unrolled (immediate LDS offsets, no loop control)
template <int NT, bool CF>
__device__ __forceinline__ void riccati_factor_lanes(const Lds& S, int Nrt, double dt, int gl) {
    const int N = NT > 0 ? NT : Nrt;
    const DLane L = dlane(gl, dt);
    const double dt2 = dt * dt;
    double pr[5];
    ld2(S.QR + QRS * N + 4 * L.i, pr[0], pr[1]);
    ld2(S.QR + QRS * N + 4 * L.i + 2, pr[2], pr[4]);
    pr[3] = 0.0;
    if constexpr (NT > 0) {
        FacRec buf[2];
        load_fac(S, L, NT - 1, buf[0]);
#pragma unroll
        for (int t = NT - 1; t >= 0; --t) {
            lds_fence();
            load_fac(S, L, t >= 1 ? t - 1 : 0, buf[(NT - t) & 1]);
            sched_fence();
            fac_step<CF>(S, L, t, t >= 1, dt, dt2, buf[(NT - 1 - t) & 1], pr);
        }
    } else {
        FacRec A, B;
        load_fac(S, L, N - 1, A);
        int t = N - 1;
        while (true) {
            lds_fence();
            load_fac(S, L, t >= 1 ? t - 1 : 0, B);      // unconditional: keeps the LDS wait counts exact
            sched_fence();
            fac_step<CF>(S, L, t, t >= 1, dt, dt2, A, pr);
            if (--t < 0) break;
            lds_fence();
            load_fac(S, L, t >= 1 ? t - 1 : 0, A);
            sched_fence();
            fac_step<CF>(S, L, t, t >= 1, dt, dt2, B, pr);
            if (--t < 0) break;
        }
    }
}
// the recursion runs on lanes 0..4 of each group only (exec narrowed): the other lanes would compute
// discarded values, and with them out of exec every store is a plain store
template <int NT, bool CF>
__device__ void riccati_factor(const Lds& S, int Nrt, double dt, int gl) {
    if (gl < 5) riccati_factor_lanes<NT, CF>(S, Nrt, dt, gl);
    wave_sync();
}

// LQR solve with the factorisation: linear terms -QH (stages 1..N), -gh (controls).  Writes dud
// (controls) and dX (states, x_0 = 0).  Three phases (restates riccati_solve() of oracle/mpc_oracle.c):
//  1. backward, lanes 0..4 (lane i holds p_i): p_t = (A_t + B K_t)' p_{t+1} + QH_t + K_t' gh_t, the
//     closed-loop form (one accumulator chain of five broadcast FMAs per stage);
//  2. stage-parallel, lane t: kk_t = S_t^-1 (gh_t + B' p_{t+1}) into slot 5 of the K rows;
//  3. forward, lanes 0..4 (lane i holds x_i): u_r = kk_r + K_t(r,:) x, x <- A_t x + B u.
// The co-states p_{t+1} pass from phase 1 to phase 2 through QR (dead between factorisations), in
// record slots (p3, p4, p0, p1, p2) so that phase 2 reads (p3, p4) with one ds_read_b128.
struct BwdRec { double g0, g1, qi, K0, K1, e1, e2; };
struct FwdRec { double K[5], kk, f0, f2, f3, f4; };
__device__ __forceinline__ void load_bwd(const Lds& S, const DLane& L, int t, BwdRec& B) {
    const double* a5 = S.A5 + A5S * t;
    ld2(S.gh + 2 * t, B.g0, B.g1);
    B.qi = S.QH[QHS * t + L.i];
    B.K0 = S.KR[KRS * t + L.i];
    B.K1 = S.KR[KRS * t + 6 + L.i];
    B.e1 = a5[L.oe1];
    B.e2 = a5[L.oe2];
}
__device__ __forceinline__ void load_fwd(const Lds& S, const DLane& L, int t, FwdRec& F) {
    const double* a5 = S.A5 + A5S * t;
    const double* kr = S.KR + KRS * t + L.kr;
    ld2(kr, F.K[0], F.K[1]);
    ld2(kr + 2, F.K[2], F.K[3]);
    ld2(kr + 4, F.K[4], F.kk);
    F.f0 = a5[L.of0];
    F.f2 = a5[L.of2];
    F.f3 = a5[L.of3];
    F.f4 = a5[L.of4];
}
// step t: p = p_{t+1} on entry (stored for phase 2), p_t on exit (t >= 1)
// The hazard-free block (dt K products first, no s_nop): C3 -2.6% (profiles/r06_ab_hazard.log); in every kernel
// since the stage lookups (C2 -0.1..-0.3%, profiles/r06_ab_bwd_all.log).  The s_nop forms those logs compare
// against (of this step and of fac_step's update blocks) were removed after commit e8c7245, where they can be read.
__device__ __forceinline__ void bwd_step(const Lds& S, const DLane& L, int t, double dt, const BwdRec& B, double& p) {
    S.QR[QRS * (t + 1) + L.ps] = p;
    if (t >= 1) {
        double acc = fma(B.K0, B.g0, fma(B.K1, B.g1, B.qi));
        // the two products dt K(r, i) are the block's first two instructions: they are the two wait states the
        // VALU-write -> DPP-read hazard on p needs (p was written by the previous step), so no s_nop
        double kd0, kd1;
        asm("v_mul_f64 %1, %7, %9\n\t"
            "v_mul_f64 %2, %8, %9\n\t"
            DPPF("%0", "%3", "%1", 3) DPPF("%0", "%3", "%2", 4) DPPF("%0", "%3", "%4", 2)
            DPPF("%0", "%3", "%5", 1) DPPF("%0", "%3", "%6", 0)
            : "+&v"(acc), "=&v"(kd0), "=&v"(kd1)
            : "v"(p), "v"(B.e2), "v"(B.e1), "v"(L.e0), "v"(B.K0), "v"(B.K1), "v"(dt));
        p = acc + p;
    }
}
__device__ __forceinline__ void kk_stage(const Lds& S, int t, double dt) {
    double g0, g1, si0, si1, si2, pad, p3, p4;
    ld2(S.gh + 2 * t, g0, g1);
    ld2(S.Si + SIS * t, si0, si1);
    ld2(S.Si + SIS * t + 2, si2, pad);
    ld2(S.QR + QRS * (t + 1), p3, p4);
    const double h0 = fma(p3, dt, g0), h1 = fma(p4, dt, g1);
    const double w0 = h0 * si0;
    const double w1 = (h1 - si1 * w0) * si2;
    const double k1 = w1 * si2;
    const double k0 = (w0 - si1 * k1) * si0;
    S.KR[KRS * t + 5] = k0;
    S.KR[KRS * t + 11] = k1;
}
// closed-loop rows 3, 4 of stage t for the forward solve: e_{3+r}' + dt K_t(r,:) and dt kk_r
// Every LDS read of a stage-parallel phase is issued before its first LDS write: the compiler cannot tell the
// arrays of the layout apart, so a read after a write would wait for it (one LDS round trip per element)
__device__ __forceinline__ void ac_rows(const Lds& S, int t, double dt) {
    const double* kr = S.KR + KRS * t;
    double* ac = S.AC + 30 * t + 18;
    double k[2][6];
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int m = 0; m < 6; m += 2) ld2(kr + 6 * r + m, k[r][m], k[r][m + 1]);
#pragma unroll
    for (int r = 0; r < 2; ++r) {
#pragma unroll
        for (int m = 0; m < 5; ++m) ac[6 * r + m] = (m == 3 + r) ? fma(dt, k[r][m], 1.0) : dt * k[r][m];
        ac[6 * r + 5] = dt * k[r][5];
    }
}
// u_t = kk_t + K_t x_t after the closed-loop forward solve (stage-parallel; the accumulation order of
// the K-row forward step)
__device__ __forceinline__ void u_stage(const Lds& S, int t) {
    const double* kr = S.KR + KRS * t;
    const double* x = S.dX + 5 * t;
    double xv[5], k[2][6];
#pragma unroll
    for (int m = 0; m < 5; ++m) xv[m] = x[m];
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int m = 0; m < 6; m += 2) ld2(kr + 6 * r + m, k[r][m], k[r][m + 1]);
    double u[2];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        u[r] = k[r][5];
#pragma unroll
        for (int m = 0; m < 5; ++m) u[r] = fma(xv[m], k[r][m], u[r]);
    }
    *reinterpret_cast<double2*>(S.dud + 2 * t) = make_double2(u[0], u[1]);
}
struct AclRec { double c[5], d; };
__device__ __forceinline__ void load_acl(const Lds& S, const DLane& L, int t, AclRec& F) {
    const double* ac = S.AC + 30 * t + 6 * L.i;
    ld2(ac, F.c[0], F.c[1]);
    ld2(ac + 2, F.c[2], F.c[3]);
    ld2(ac + 4, F.c[4], F.d);
}
// x_{t+1}(i) = sum_m Acl_t(i,m) x_m + (B kk_t)_i: one chain of five broadcast FMAs.
// NOP: the s_nop 1 covering the VALU-write -> DPP-read hazard on x.  Only the first step needs it (x = 0 was
// just materialised); in the unrolled recursions every later x is the previous chain's last FMA, followed by
// its LDS store, the next record's loads and waits (tools/dpp_hazard_check.py checks the listing)
template <bool NOP = true>
__device__ __forceinline__ void acl_step(const Lds& S, const DLane& L, int t, AclRec& F, double& x) {
    if constexpr (NOP)
        asm("s_nop 1\n\t" DPPF("%0", "%1", "%2", 0) DPPF("%0", "%1", "%3", 1) DPPF("%0", "%1", "%4", 2)
            DPPF("%0", "%1", "%5", 3) DPPF("%0", "%1", "%6", 4)
            : "+&v"(F.d) : "v"(x), "v"(F.c[0]), "v"(F.c[1]), "v"(F.c[2]), "v"(F.c[3]), "v"(F.c[4]));
    else
        asm(DPPF("%0", "%1", "%2", 0) DPPF("%0", "%1", "%3", 1) DPPF("%0", "%1", "%4", 2)
            DPPF("%0", "%1", "%5", 3) DPPF("%0", "%1", "%6", 4)
            : "+&v"(F.d) : "v"(x), "v"(F.c[0]), "v"(F.c[1]), "v"(F.c[2]), "v"(F.c[3]), "v"(F.c[4]));
    x = F.d;
    S.dX[5 * (t + 1) + L.i] = x;
}
__device__ __forceinline__ void fwd_step(const Lds& S, const DLane& L, int t, const FwdRec& F, double& x) {
    // u: lanes 0..3 accumulate row 0 of K (u0), lane 4 row 1 (u1); xa = J'_t x (row i)
    double u = F.kk, xa = 0.0;
    asm("s_nop 1\n\t" DPPF("%0", "%2", "%3", 0) DPPF("%1", "%2", "%8", 0) DPPF("%0", "%2", "%4", 1)
        DPPF("%1", "%2", "%9", 2) DPPF("%0", "%2", "%5", 2) DPPF("%1", "%2", "%10", 3) DPPF("%0", "%2", "%6", 3)
        DPPF("%1", "%2", "%11", 4) DPPF("%0", "%2", "%7", 4)
        : "+&v"(u), "+&v"(xa)
        : "v"(x), "v"(F.K[0]), "v"(F.K[1]), "v"(F.K[2]), "v"(F.K[3]), "v"(F.K[4]), "v"(F.f0), "v"(F.f2),
          "v"(F.f3), "v"(F.f4));
    x = fma(L.bu, u, x + xa);
    S.dX[5 * (t + 1) + L.i] = x;
    S.dud[2 * t + L.ur] = u;
}

// NT > 0: the horizon is a compile-time constant and the recursions are fully unrolled.
template <int NT>
__device__ __forceinline__ void solve_bwd_lanes(const Lds& S, int N, double dt, int gl) {
    const DLane L = dlane(gl, dt);
    double p = S.QH[QHS * N + L.i];
    if constexpr (NT > 0) {
        BwdRec buf[2];
        load_bwd(S, L, NT - 1, buf[0]);
#pragma unroll
        for (int t = NT - 1; t >= 0; --t) {
            sched_fence();
            load_bwd(S, L, t >= 1 ? t - 1 : 0, buf[(NT - t) & 1]);
            sched_fence();
            bwd_step(S, L, t, dt, buf[(NT - 1 - t) & 1], p);
        }
    } else {
        BwdRec A, B;
        load_bwd(S, L, N - 1, A);
        int t = N - 1;
        while (true) {
            sched_fence();
            load_bwd(S, L, t >= 1 ? t - 1 : 0, B);
            sched_fence();
            bwd_step(S, L, t, dt, A, p);
            if (--t < 0) break;
            sched_fence();
            load_bwd(S, L, t >= 1 ? t - 1 : 0, A);
            sched_fence();
            bwd_step(S, L, t, dt, B, p);
            if (--t < 0) break;
        }
    }
}
template <int NT>
__device__ __forceinline__ void solve_acl_lanes(const Lds& S, int N, double dt, int gl) {
    const DLane L = dlane(gl, dt);
    double x = 0.0;
    S.dX[L.i] = 0.0;
    if constexpr (NT > 0) {
        AclRec buf[2];
        load_acl(S, L, 0, buf[0]);
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            sched_fence();
            load_acl(S, L, t + 1 < NT ? t + 1 : t, buf[(t + 1) & 1]);
            sched_fence();
            if (t == 0) acl_step<true>(S, L, t, buf[t & 1], x);
            else acl_step<false>(S, L, t, buf[t & 1], x);
        }
    } else {
        AclRec A, B;
        load_acl(S, L, 0, A);
        int t = 0;
        while (true) {
            sched_fence();
            load_acl(S, L, t + 1 < N ? t + 1 : t, B);
            sched_fence();
            acl_step(S, L, t, A, x);
            if (++t >= N) break;
            sched_fence();
            load_acl(S, L, t + 1 < N ? t + 1 : t, A);
            sched_fence();
            acl_step(S, L, t, B, x);
            if (++t >= N) break;
        }
    }
}
template <int NT>
__device__ __forceinline__ void solve_fwd_lanes(const Lds& S, int N, double dt, int gl) {
    const DLane L = dlane(gl, dt);
    double x = 0.0;
    S.dX[L.i] = 0.0;
    if constexpr (NT > 0) {
        FwdRec buf[2];
        load_fwd(S, L, 0, buf[0]);
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            sched_fence();
            load_fwd(S, L, t + 1 < NT ? t + 1 : t, buf[(t + 1) & 1]);
            sched_fence();
            fwd_step(S, L, t, buf[t & 1], x);
        }
    } else {
        FwdRec A, B;
        load_fwd(S, L, 0, A);
        int t = 0;
        while (true) {
            sched_fence();
            load_fwd(S, L, t + 1 < N ? t + 1 : t, B);
            sched_fence();
            fwd_step(S, L, t, A, x);
            if (++t >= N) break;
            sched_fence();
            load_fwd(S, L, t + 1 < N ? t + 1 : t, A);
            sched_fence();
            fwd_step(S, L, t, B, x);
            if (++t >= N) break;
        }
    }
}
// the recursions run on lanes 0..4 of each group (exec narrowed), the stage phases on lanes 0..N-1.
// ACL: the forward solve runs on closed-loop rows (built with kk) and u follows stage-parallel.
template <int NT, bool ACL>
__device__ void riccati_solve(const Lds& S, int Nrt, double dt, int gl) {
    const int N = NT > 0 ? NT : Nrt;
    if (gl < 5) solve_bwd_lanes<NT>(S, N, dt, gl);
    wave_sync();
    if (gl < N) {
        kk_stage(S, gl, dt);
        if (ACL) ac_rows(S, gl, dt);
    }
    wave_sync();
    if (ACL) {
        if (gl < 5) solve_acl_lanes<NT>(S, N, dt, gl);
        wave_sync();
        if (gl < N) u_stage(S, gl);
    } else {
        if (gl < 5) solve_fwd_lanes<NT>(S, N, dt, gl);
    }
    wave_sync();
}

// max |g| and the scale max(|g_cost|, |g_mult|) of the dual residual g = G'y + z (adjoint recursion)
__device__ void dual_norms(const Lds& S, int N, double dt, double& rdmax, double& sd) {
    double mc[5] = {0, 0, 0, 0, 0}, ma[5] = {0, 0, 0, 0, 0};
    rdmax = 0.0;
    sd = 0.0;
    for (int k = N; k >= 1; --k) {
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            mc[st4(a)] += S.QR[QRS * k + DQ_YC + a];
            ma[st4(a)] += S.QR[QRS * k + DQ_YA + a];
        }
        const int t = k - 1;
        double gc0 = fma(dt, mc[3], S.QR[QRS * t + DQ_ZC]), gc1 = fma(dt, mc[4], S.QR[QRS * t + DQ_ZC + 1]);
        double ga0 = fma(dt, ma[3], S.QR[QRS * t + DQ_ZA]), ga1 = fma(dt, ma[4], S.QR[QRS * t + DQ_ZA + 1]);
        rdmax = fmax(rdmax, fmax(fabs(gc0 + ga0), fabs(gc1 + ga1)));
        sd = fmax(sd, fmax(fmax(fabs(gc0), fabs(gc1)), fmax(fabs(ga0), fabs(ga1))));
        double y[5];
        applyAT(S.A5 + A5S * t, dt, mc, y);
#pragma unroll
        for (int a = 0; a < 5; ++a) mc[a] = y[a];
        applyAT(S.A5 + A5S * t, dt, ma, y);
#pragma unroll
        for (int a = 0; a < 5; ++a) ma[a] = y[a];
    }
}

// cost Hessian (packed 4x4 on s,d,o,v) and gradient of stage k from cst = (-d', -o', -v', r_d, r_o, r_v):
// Q = 2 sum_j w_j m_j m_j',  q = 2 sum_j w_j r_j m_j,  m_j = e_j + (-ref_j') e_s   
__device__ __forceinline__ void stage_cost(const double* cst, double wd, double wo, double wv, double Q[10],
                                           double q[4]) {
    const double w[3] = {2.0 * wd, 2.0 * wo, 2.0 * wv};
#pragma unroll
    for (int a = 0; a < 10; ++a) Q[a] = 0.0;
#pragma unroll
    for (int a = 0; a < 4; ++a) q[a] = 0.0;
#pragma unroll
    for (int jj = 0; jj < 3; ++jj) {
        const double m0 = cst[jj];        // s entry; the own entry (index jj+1) is 1
        const double r = cst[3 + jj];
        Q[p4(0, 0)] = fma(w[jj] * m0, m0, Q[p4(0, 0)]);
        Q[p4(0, jj + 1)] += w[jj] * m0;
        Q[p4(jj + 1, jj + 1)] += w[jj];
        q[0] = fma(w[jj] * r, m0, q[0]);
        q[jj + 1] += w[jj] * r;
    }
}
