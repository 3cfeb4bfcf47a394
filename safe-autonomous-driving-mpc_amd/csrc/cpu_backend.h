// cpu_backend.h -- the host (CPU) backend of libmpcqp: mpc_create(..., device = -1, ...).
//
// BASELINE config 1 ("trajectory1.json, N=10, single ego, CPU path") runs the reference's tracker without a
// GPU.  This backend serves that case behind the same C ABI: the same QP(ubar), the same
// solver (crossover first, Mehrotra PDIP on the stage-wise Riccati recursion, active-set polish, the
// Gauss-Newton SQP with warm crossovers and its stopping rules) and the same outputs
// and status codes as the HIP kernels, computed per instance in IEEE double on host threads (batch split
// over std::thread workers, each with its own scratch).  It is product code: it shares the trajectory table
// builder (host_table.h), the model (tracker_model.h) and the loop steps (loop_steps.h) with the device path and
// nothing with the test oracle.
//
// Reference functions restated here (medinammartin3/Safe-Autonomous-Driving-MPC):
//   warm start  trajectory_tracking.py:224-246      predict     :87-114 (dynamics :50-67)
//   cost        :116-152 (Gauss-Newton model)        constraints :155-211 (6 row types, min over obstacles)
//   solve       :213-263 (SLSQP replaced)            get_state / get_control  trajectory_loader.py:86-102
//   get_global_pose  trajectory_loader.py:104-116    ObstaclesFSM.update :330-374, run_simulation :377-443
#ifndef MPCQP_CPU_BACKEND_H
#define MPCQP_CPU_BACKEND_H

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <new>
#include <thread>
#include <vector>

#include "host_table.h"
#include "loop_steps.h"
#include "scripted_loop.h"

namespace mpcqp_cpu {

using mpcqp_host::HostTable;

constexpr int kMaxN = MPC_MAX_N;
// MPC_CHECKPOINT=0 in the environment switches the checkpoint off (A/B; the device kernels read the same flag)
inline bool checkpoint_on() {
    static const bool on = [] {
        const char* e = std::getenv("MPC_CHECKPOINT");
        return !(e && e[0] == '0');
    }();
    return on;
}
constexpr double kBoxSign[NBOX] = {1.0, -1.0, 1.0, -1.0};
constexpr int kBoxComp[NBOX] = {0, 0, 1, 1};

// ---------------------------------------------------------------------------------------------
// one instance: QP(ubar) stage data, interior-point state, Riccati factors, directions
// ---------------------------------------------------------------------------------------------
struct StageQp {
    int N = 0;
    bool obs = false;
    double dt = 0.0, rho = 0.0;
    double Xb[kMaxN + 1][5];                                   // nominal rollout predict(x0, ubar)
    double a12[kMaxN], a14[kMaxN], a20[kMaxN], a23[kMaxN], a24[kMaxN];   // A_k = I + J'_k (J'(0,4) = dt)
    double Q[kMaxN + 1][5][5], q[kMaxN + 1][5];                // Gauss-Newton state cost, stages 1..N
    double R[2], r[kMaxN][2];                                  // control cost
    double C[NROW][5];                                        // soft-row coefficients (C x + xi >= b + s)
    bool on[NROW];
    double b[kMaxN + 1][NROW];
    double bb[kMaxN][NBOX];                                    // box rows (hard)
};
struct IpState {
    double du[2 * kMaxN];
    double s[kMaxN + 1][NROW], l[kMaxN + 1][NROW], xi[kMaxN + 1][NROW], nu[kMaxN + 1][NROW];
    double sb[kMaxN][NBOX], lb[kMaxN][NBOX];
};
struct Factors {
    double K[kMaxN][2][5], Lc[kMaxN][3];                        // feedback, Cholesky factor (l00, l10, l11) of S
    double Qt[kMaxN + 1][5][5], Rt[kMaxN][2];                  // augmented stage Hessians
    double d[kMaxN + 1][NROW], db[kMaxN][NBOX];               // barrier diagonals
};
struct Direction {
    double du[2 * kMaxN], dX[kMaxN + 1][5];
    double dl[kMaxN + 1][NROW], ds[kMaxN + 1][NROW], dxi[kMaxN + 1][NROW], dnu[kMaxN + 1][NROW];
    double dlb[kMaxN][NBOX], dsb[kMaxN][NBOX];
};

static inline double dot5(const double a[5], const double b[5]) {
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2] + a[3] * b[3] + a[4] * b[4];
}

class Worker {
public:
    Worker(const DevTable& ref, const mpc_params& p) : R_(ref), p_(p), K_(model_params(p)) {}

    // TrajectoryTracker.solve (trajectory_tracking.py:213-263) for one instance; returns the status code
    int solve(const double x0[5], const double* obs, int nobs, const double* ubar, double* u0, double* U,
              double* Xpred, int* iters) {
        const int N = p_.N;
        double ub[2 * kMaxN], uo[2 * kMaxN], u2[2 * kMaxN];
        if (ubar) std::memcpy(ub, ubar, sizeof(double) * 2 * N);
        else warm_start(x0, obs, nobs, ub);
        std::memcpy(uo, ub, sizeof(double) * 2 * N);
        std::memcpy(u2, ub, sizeof(double) * 2 * N);
        const int nsqp = p_.sqp_iters < 0 ? 0 : p_.sqp_iters;
        int status = MPC_OK, total = 0, ninf = 0;
        bool conv = false;
        for (int it = 0; it < nsqp; ++it) {
            build(x0, obs, nobs, ub);
            int ni = 0;
            status = pdip(ni, it > 0);
            total += ni;
            double step = 0.0, back2 = 0.0;
            for (int i = 0; i < 2 * N; ++i) {
                uo[i] = ub[i] + S_.du[i];
                step = std::max(step, std::fabs(S_.du[i]));
                back2 = std::max(back2, std::fabs(uo[i] - u2[i]));
            }
            std::memcpy(u2, ub, sizeof(double) * 2 * N);
            std::memcpy(ub, uo, sizeof(double) * 2 * N);
            ninf = status == MPC_INFEASIBLE ? ninf + 1 : 0;
            if (nsqp > 1) {
                if (step <= p_.sqp_tol) { conv = true; break; }                  // re-linearisation converged
                if (p_.sqp_tol > 0.0 && ((it >= 2 && back2 <= SQP_CYCLE_REL * step) || ninf >= SQP_INF_STREAK)) break;
            }
        }
        if (U) std::memcpy(U, uo, sizeof(double) * 2 * N);
        if (u0) { u0[0] = uo[0]; u0[1] = uo[1]; }
        if (Xpred) predict(x0, uo, reinterpret_cast<double(*)[5]>(Xpred));    // :261
        if (iters) *iters = total;
        if (nsqp > 1 && p_.sqp_tol > 0.0 && !conv) status |= MPC_SQP_UNCONVERGED;
        return status;
    }

    // warm start ubar (trajectory_tracking.py:224-246): loop_steps.h's reference warm start, every stage of it
    void warm_start(const double x0[5], const double* obs, int nobs, double* ub) const {
        WarmRef w = warm_ref_begin(x0);
        for (int j = 0; j < p_.N; ++j) {
            warm_ref_advance(w, j, p_.dt, obs, nobs, p_.brake_distance);
            warm_ref_control(w, p_.brake_accel, [&](double s, double* ur) { get_control(R_, s, ur); }, ub[2 * j],
                             ub[2 * j + 1]);
        }
    }

    // explicit-Euler rollout (trajectory_tracking.py:87-114), k_ref looked up at the predicted s
    void predict(const double x0[5], const double* U, double (*X)[5]) const {
        const double dt = p_.dt;
        double x[5];
        std::memcpy(x, x0, sizeof(x));
        std::memcpy(X[0], x0, sizeof(x));
        for (int k = 0; k < p_.N; ++k) {
            double st[5];
            get_state(R_, x[0], st);
            plant_step(x, dt, U[2 * k], U[2 * k + 1], st[3]);
            std::memcpy(X[k + 1], x, sizeof(x));
        }
    }

private:
    const DevTable& R_;
    const mpc_params& p_;
    const KParams K_;        // the model derived from p_ (tracker_model.h)
    StageQp q_;
    IpState S_, Z_, T_, C_;
    Factors F_;
    Direction D_, Da_;
    unsigned char cls_[kMaxN + 1][NROW], clb_[kMaxN][NBOX];      // 0 inactive, 1 active, 2 violated
    unsigned char flip_[kMaxN + 1][NROW], flipb_[kMaxN][NBOX];
    unsigned char last_cls_[kMaxN + 1][NROW], last_clb_[kMaxN][NBOX];   // the SQP's warm crossover
    double xo_du_[2 * kMaxN];   // du of the last cold crossover solve: the unconstrained optimum (interior-point start)

    // ---- QP(ubar): Gauss-Newton model of cost/constraints around the nominal rollout
    void build(const double x0[5], const double* obs, int nobs, const double* ub) {
        StageQp& Q = q_;
        const int N = p_.N;
        const double dt = p_.dt;
        const bool gn = p_.linearization != 0;
        Q.N = N;
        Q.dt = dt;
        Q.rho = p_.elastic_rho;
        Q.obs = nobs > 0;
        predict(x0, ub, Q.Xb);
        for (int k = 0; k < N; ++k) {
            const double* x = Q.Xb[k];
            double st[5], sl[4];
            get_state(R_, x[0], st, sl);
            double a[5];
            stage_A(x, dt, st[3], gn ? sl[2] : 0.0, a);
            Q.a12[k] = a[0];
            Q.a14[k] = a[1];
            Q.a20[k] = a[2];
            Q.a23[k] = a[3];
            Q.a24[k] = a[4];
        }
        const double w[3] = {p_.w_d, p_.w_o, p_.w_v};
        const int comp[3] = {1, 2, 4};
        std::memset(Q.Q, 0, sizeof(Q.Q));
        std::memset(Q.q, 0, sizeof(Q.q));
        for (int k = 1; k <= N; ++k) {
            const double* x = Q.Xb[k];
            double st[5], sl[4];
            get_state(R_, x[0], st, sl);
            const double ref[3] = {st[1], st[2], st[4]};
            const double dref[3] = {gn ? sl[0] : 0.0, gn ? sl[1] : 0.0, gn ? sl[3] : 0.0};
            for (int j = 0; j < 3; ++j) {
                // residual x_c - ref_c(s): gradient e_c - ref_c'(s) e_s
                double m[5] = {0, 0, 0, 0, 0};
                m[comp[j]] = 1.0;
                m[0] = -dref[j];
                const double r0 = x[comp[j]] - ref[j];
                for (int a = 0; a < 5; ++a) {
                    Q.q[k][a] += 2.0 * w[j] * r0 * m[a];
                    for (int c = 0; c < 5; ++c) Q.Q[k][a][c] += 2.0 * w[j] * m[a] * m[c];
                }
            }
        }
        Q.R[0] = 2.0 * p_.w_u1;
        Q.R[1] = 2.0 * p_.w_u2;
        for (int k = 0; k < N; ++k) {
            Q.r[k][0] = Q.R[0] * ub[2 * k];
            Q.r[k][1] = Q.R[1] * ub[2 * k + 1];
        }
        // the rows and boxes: tracker_model.h's coefficients (with a zero k entry) and values
        for (int j = 0; j < NROW; ++j) {
            double c[4];
            row_coef(j, K_.L / 2.0, K_.L, K_.tgap, c);
            const double c5[5] = {c[0], c[1], c[2], 0.0, c[3]};
            std::memcpy(Q.C[j], c5, sizeof(c5));
            Q.on[j] = row_exists(j, Q.obs);
        }
        for (int k = 1; k <= N; ++k)
            row_values(K_, Q.Xb[k], nearest_obstacle(obs, nobs, k, dt), Q.obs, Q.b[k]);
        for (int k = 0; k < N; ++k) box_values(K_, ub[2 * k], ub[2 * k + 1], Q.bb[k]);
    }

    // ---- linear model pieces: x_{k+1} = A_k x_k + B u_k, B = dt e3 e1' + dt e4 e2'
    void apply_A(int k, const double x[5], double y[5]) const {
        const StageQp& Q = q_;
        y[0] = x[0] + Q.dt * x[4];
        y[1] = x[1] + Q.a12[k] * x[2] + Q.a14[k] * x[4];
        y[2] = x[2] + Q.a20[k] * x[0] + Q.a23[k] * x[3] + Q.a24[k] * x[4];
        y[3] = x[3];
        y[4] = x[4];
    }
    void apply_AT(int k, const double m[5], double y[5]) const {
        const StageQp& Q = q_;
        y[0] = m[0] + Q.a20[k] * m[2];
        y[1] = m[1];
        y[2] = m[2] + Q.a12[k] * m[1];
        y[3] = m[3] + Q.a23[k] * m[2];
        y[4] = m[4] + Q.dt * m[0] + Q.a14[k] * m[1] + Q.a24[k] * m[2];
    }
    void rollout(const double* du, double (*X)[5]) const {
        std::memset(X[0], 0, sizeof(double) * 5);
        for (int k = 0; k < q_.N; ++k) {
            apply_A(k, X[k], X[k + 1]);
            X[k + 1][3] += q_.dt * du[2 * k];
            X[k + 1][4] += q_.dt * du[2 * k + 1];
        }
    }
    // g_t = z_t + B' mu_{t+1} with mu_N = y_N, mu_k = A_k' mu_{k+1} + y_k: the dual residual in control space
    void adjoint(const double (*y)[5], const double (*z)[2], double* g) const {
        double mu[5] = {0, 0, 0, 0, 0};
        for (int k = q_.N; k >= 1; --k) {
            for (int a = 0; a < 5; ++a) mu[a] += y[k][a];
            g[2 * (k - 1)] = z[k - 1][0] + q_.dt * mu[3];
            g[2 * (k - 1) + 1] = z[k - 1][1] + q_.dt * mu[4];
            double m2[5];
            apply_AT(k - 1, mu, m2);
            std::memcpy(mu, m2, sizeof(mu));
        }
    }

    // ---- Riccati factorisation of  min sum 0.5 x'Qt x + 0.5 u'Rt u  (Cholesky form of S)
    void riccati_factor() {
        const StageQp& Q = q_;
        Factors& F = F_;
        const int N = Q.N;
        const double dt = Q.dt;
        double P[5][5];
        std::memcpy(P, F.Qt[N], sizeof(P));
        for (int k = N - 1; k >= 0; --k) {
            double M[5][5];                                    // P A_k
            for (int i = 0; i < 5; ++i) {
                M[i][0] = P[i][0] + P[i][2] * Q.a20[k];
                M[i][1] = P[i][1];
                M[i][2] = P[i][2] + P[i][1] * Q.a12[k];
                M[i][3] = P[i][3] + P[i][2] * Q.a23[k];
                M[i][4] = P[i][4] + P[i][0] * dt + P[i][1] * Q.a14[k] + P[i][2] * Q.a24[k];
            }
            double s00 = F.Rt[k][0] + dt * dt * P[3][3];
            const double s01 = dt * dt * P[3][4];
            const double s11 = F.Rt[k][1] + dt * dt * P[4][4];
            if (!(s00 > 0.0)) s00 = 1e-300 + std::fabs(s00);
            const double l00 = std::sqrt(s00), l10 = s01 / l00;
            double r11 = s11 - l10 * l10;
            if (!(r11 > 1e-14 * s11)) r11 = 1e-14 * std::fabs(s11) + 1e-300;
            const double l11 = std::sqrt(r11);
            F.Lc[k][0] = l00;
            F.Lc[k][1] = l10;
            F.Lc[k][2] = l11;
            double W0[5], W1[5];
            for (int j = 0; j < 5; ++j) {
                W0[j] = dt * M[3][j] / l00;
                W1[j] = (dt * M[4][j] - l10 * W0[j]) / l11;
                const double z1 = W1[j] / l11;
                F.K[k][1][j] = -z1;
                F.K[k][0][j] = -(W0[j] - l10 * z1) / l00;
            }
            if (k == 0) break;
            double Pn[5][5];
            for (int j = 0; j < 5; ++j) {
                double col[5] = {M[0][j], M[1][j], M[2][j], M[3][j], M[4][j]}, at[5];
                apply_AT(k, col, at);
                for (int i = 0; i < 5; ++i) Pn[i][j] = at[i];
            }
            for (int i = 0; i < 5; ++i)
                for (int j = 0; j < 5; ++j) Pn[i][j] += F.Qt[k][i][j] - (W0[i] * W0[j] + W1[i] * W1[j]);
            for (int i = 0; i < 5; ++i)
                for (int j = 0; j < 5; ++j) P[i][j] = 0.5 * (Pn[i][j] + Pn[j][i]);
        }
    }
    // LQR solve for the linear terms -qh (states 1..N) and -gh (controls); writes D.du, D.dX (x_0 = 0)
    void riccati_solve(const double (*qh)[5], const double (*gh)[2], Direction& D) const {
        const StageQp& Q = q_;
        const Factors& F = F_;
        const int N = Q.N;
        const double dt = Q.dt;
        double p[5], kk[kMaxN][2];
        std::memcpy(p, qh[N], sizeof(p));
        for (int k = N - 1; k >= 0; --k) {
            const double h0 = gh[k][0] + dt * p[3], h1 = gh[k][1] + dt * p[4];
            const double* Lc = F.Lc[k];
            const double w0 = h0 / Lc[0], w1 = (h1 - Lc[1] * w0) / Lc[2];
            kk[k][1] = w1 / Lc[2];
            kk[k][0] = (w0 - Lc[1] * kk[k][1]) / Lc[0];
            if (k >= 1) {
                double pa[5];
                apply_AT(k, p, pa);
                for (int a = 0; a < 5; ++a) p[a] = qh[k][a] + pa[a] + F.K[k][0][a] * h0 + F.K[k][1][a] * h1;
            }
        }
        std::memset(D.dX[0], 0, sizeof(double) * 5);
        for (int k = 0; k < N; ++k) {
            const double* x = D.dX[k];
            const double v0 = kk[k][0] + dot5(F.K[k][0], x), v1 = kk[k][1] + dot5(F.K[k][1], x);
            D.du[2 * k] = v0;
            D.du[2 * k + 1] = v1;
            apply_A(k, x, D.dX[k + 1]);
            D.dX[k + 1][3] += dt * v0;
            D.dX[k + 1][4] += dt * v1;
        }
    }

    // barrier diagonals, augmented Hessians and the factorisation at the current iterate
    void factor() {
        const StageQp& Q = q_;
        for (int k = 1; k <= Q.N; ++k) {
            std::memcpy(F_.Qt[k], Q.Q[k], sizeof(F_.Qt[k]));
            for (int j = 0; j < NROW; ++j) {
                if (!Q.on[j]) continue;
                const double d = S_.s[k][j] / S_.l[k][j] + S_.xi[k][j] / S_.nu[k][j];
                F_.d[k][j] = d;
                const double w = 1.0 / d;
                for (int a = 0; a < 5; ++a)
                    for (int c = 0; c < 5; ++c) F_.Qt[k][a][c] += w * Q.C[j][a] * Q.C[j][c];
            }
        }
        for (int t = 0; t < Q.N; ++t) {
            F_.Rt[t][0] = Q.R[0];
            F_.Rt[t][1] = Q.R[1];
            for (int j = 0; j < NBOX; ++j) {
                const double d = S_.sb[t][j] / S_.lb[t][j];
                F_.db[t][j] = d;
                F_.Rt[t][kBoxComp[j]] += 1.0 / d;
            }
        }
        riccati_factor();
    }

    // Newton direction for complementarity targets r4 (s lam), r5 (xi nu), r4b (box), residuals rp/rpb/rx and
    // the dual residual pieces y (stages) / z (controls), eliminated row-wise onto the Riccati system
    void newton(const double (*rp)[NROW], const double (*rpb)[NBOX], const double (*rx)[NROW],
                const double (*y)[5], const double (*z)[2], const double (*r4)[NROW], const double (*r5)[NROW],
                const double (*r4b)[NBOX], Direction& D) {
        const StageQp& Q = q_;
        const int N = Q.N;
        double qh[kMaxN + 1][5], gh[kMaxN][2], rh[kMaxN + 1][NROW], rhb[kMaxN][NBOX];
        for (int k = 1; k <= N; ++k) {
            for (int a = 0; a < 5; ++a) qh[k][a] = -y[k][a];
            for (int j = 0; j < NROW; ++j) {
                if (!Q.on[j]) continue;
                const double v = -rp[k][j] - r4[k][j] / S_.l[k][j] + (r5[k][j] + S_.xi[k][j] * rx[k][j]) / S_.nu[k][j];
                rh[k][j] = v;
                const double w = v / F_.d[k][j];
                for (int a = 0; a < 5; ++a) qh[k][a] += Q.C[j][a] * w;
            }
        }
        for (int t = 0; t < N; ++t) {
            gh[t][0] = -z[t][0];
            gh[t][1] = -z[t][1];
            for (int j = 0; j < NBOX; ++j) {
                const double v = -rpb[t][j] - r4b[t][j] / S_.lb[t][j];
                rhb[t][j] = v;
                gh[t][kBoxComp[j]] += kBoxSign[j] * v / F_.db[t][j];
            }
        }
        riccati_solve(qh, gh, D);
        for (int k = 1; k <= N; ++k)
            for (int j = 0; j < NROW; ++j) {
                if (!Q.on[j]) continue;
                const double dl = (rh[k][j] - dot5(Q.C[j], D.dX[k])) / F_.d[k][j];
                D.dl[k][j] = dl;
                D.ds[k][j] = -(r4[k][j] + S_.s[k][j] * dl) / S_.l[k][j];
                const double dn = rx[k][j] - dl;
                D.dnu[k][j] = dn;
                D.dxi[k][j] = -(r5[k][j] + S_.xi[k][j] * dn) / S_.nu[k][j];
            }
        for (int t = 0; t < N; ++t)
            for (int j = 0; j < NBOX; ++j) {
                const double dl = (rhb[t][j] - kBoxSign[j] * D.du[2 * t + kBoxComp[j]]) / F_.db[t][j];
                D.dlb[t][j] = dl;
                D.dsb[t][j] = -(r4b[t][j] + S_.sb[t][j] * dl) / S_.lb[t][j];
            }
    }

    // largest step in (0, 1] keeping every slack and multiplier positive
    double max_step(const Direction& D) const {
        double a = 1.0;
        auto ratio = [&a](double v, double dv) { if (dv < 0.0 && -v / dv < a) a = -v / dv; };
        for (int k = 1; k <= q_.N; ++k)
            for (int j = 0; j < NROW; ++j) {
                if (!q_.on[j]) continue;
                ratio(S_.s[k][j], D.ds[k][j]);
                ratio(S_.l[k][j], D.dl[k][j]);
                ratio(S_.xi[k][j], D.dxi[k][j]);
                ratio(S_.nu[k][j], D.dnu[k][j]);
            }
        for (int t = 0; t < q_.N; ++t)
            for (int j = 0; j < NBOX; ++j) {
                ratio(S_.sb[t][j], D.dsb[t][j]);
                ratio(S_.lb[t][j], D.dlb[t][j]);
            }
        return a;
    }
    // total complementarity after a step of length a along D
    double comp_after(const Direction& D, double a) const {
        double c = 0.0;
        for (int k = 1; k <= q_.N; ++k)
            for (int j = 0; j < NROW; ++j) {
                if (!q_.on[j]) continue;
                c += (S_.s[k][j] + a * D.ds[k][j]) * (S_.l[k][j] + a * D.dl[k][j]) +
                     (S_.xi[k][j] + a * D.dxi[k][j]) * (S_.nu[k][j] + a * D.dnu[k][j]);
            }
        for (int t = 0; t < q_.N; ++t)
            for (int j = 0; j < NBOX; ++j) c += (S_.sb[t][j] + a * D.dsb[t][j]) * (S_.lb[t][j] + a * D.dlb[t][j]);
        return c;
    }

    // ---- active-set solve (crossover / polish).  Rows classified active (equality, penalty 1/delta plus
    // iterative refinement on the exact KKT residual), violated (multiplier fixed at rho) or inactive; the
    // result is accepted when KKT-consistent, otherwise every offending row changes class and the round
    // repeats.  from: 0 = classify the iterate X, 1 = all inactive (crossover), 2 = the previous QP's final
    // classification (the SQP's warm crossover).  Returns true when accepted (X.du replaced).
    bool active_set(IpState& X, int from, int rounds, bool& infeasible) {
        const StageQp& Q = q_;
        const int N = Q.N;
        const double rho = Q.rho;
        for (int k = 1; k <= N; ++k)
            for (int j = 0; j < NROW; ++j) {
                unsigned char c = 0;
                if (Q.on[j] && from != 1) {
                    if (from == 2) c = last_cls_[k][j];
                    else if (X.xi[k][j] > X.nu[k][j]) c = 2;
                    else if (X.l[k][j] > X.s[k][j]) c = 1;
                }
                cls_[k][j] = c;
            }
        for (int t = 0; t < N; ++t)
            for (int j = 0; j < NBOX; ++j)
                clb_[t][j] = from == 1 ? 0 : (from == 2 ? last_clb_[t][j] : (X.lb[t][j] > X.sb[t][j]));
        bool accepted = false;
        double Xs[kMaxN + 1][5];
        for (int round = 0; round < rounds && !accepted; ++round) {
            IpState& W = T_;
            std::memcpy(&W, &X, sizeof(W));
            for (int k = 1; k <= N; ++k) {
                std::memcpy(F_.Qt[k], Q.Q[k], sizeof(F_.Qt[k]));
                for (int j = 0; j < NROW; ++j)
                    if (Q.on[j] && cls_[k][j] == 1) {
                        for (int a = 0; a < 5; ++a)
                            for (int c = 0; c < 5; ++c) F_.Qt[k][a][c] += Q.C[j][a] * Q.C[j][c] / POLISH_DELTA;
                        if (!(X.l[k][j] > 0.0)) W.l[k][j] = 0.0;
                    }
            }
            for (int t = 0; t < N; ++t) {
                F_.Rt[t][0] = Q.R[0];
                F_.Rt[t][1] = Q.R[1];
                for (int j = 0; j < NBOX; ++j)
                    if (clb_[t][j]) F_.Rt[t][kBoxComp[j]] += 1.0 / POLISH_DELTA;
            }
            riccati_factor();
            // from the all-inactive classification (the crossover) the first solve is the unconstrained LQR's exact
            // optimum: one solve, nothing to refine (oracle polish_from, kernel MODE_XO)
            const int nref = from == 1 ? 1 : POLISH_REFINE;
            for (int r = 0; r <= nref; ++r) {
                rollout(W.du, Xs);
                double qh[kMaxN + 1][5], gh[kMaxN][2], r2[kMaxN + 1][NROW], r2b[kMaxN][NBOX];
                for (int k = 1; k <= N; ++k) {
                    for (int a = 0; a < 5; ++a) {
                        double acc = Q.q[k][a];
                        for (int c = 0; c < 5; ++c) acc += Q.Q[k][a][c] * Xs[k][c];
                        qh[k][a] = -acc;
                    }
                    for (int j = 0; j < NROW; ++j) {
                        if (!Q.on[j] || cls_[k][j] == 0) continue;
                        const double lam = cls_[k][j] == 2 ? rho : W.l[k][j];
                        for (int a = 0; a < 5; ++a) qh[k][a] += lam * Q.C[j][a];
                        if (cls_[k][j] == 1) {
                            r2[k][j] = Q.b[k][j] - dot5(Q.C[j], Xs[k]);
                            for (int a = 0; a < 5; ++a) qh[k][a] += Q.C[j][a] * r2[k][j] / POLISH_DELTA;
                        }
                    }
                }
                for (int t = 0; t < N; ++t) {
                    gh[t][0] = -(Q.R[0] * W.du[2 * t] + Q.r[t][0]);
                    gh[t][1] = -(Q.R[1] * W.du[2 * t + 1] + Q.r[t][1]);
                    for (int j = 0; j < NBOX; ++j) {
                        if (!clb_[t][j]) continue;
                        const double sg = kBoxSign[j];
                        gh[t][kBoxComp[j]] += sg * W.lb[t][j];
                        r2b[t][j] = Q.bb[t][j] - sg * W.du[2 * t + kBoxComp[j]];
                        gh[t][kBoxComp[j]] += sg * r2b[t][j] / POLISH_DELTA;
                    }
                }
                if (r == nref) break;
                riccati_solve(qh, gh, D_);
                for (int i = 0; i < 2 * N; ++i) W.du[i] += D_.du[i];
                for (int k = 1; k <= N; ++k)
                    for (int j = 0; j < NROW; ++j)
                        if (Q.on[j] && cls_[k][j] == 1) W.l[k][j] += (r2[k][j] - dot5(Q.C[j], D_.dX[k])) / POLISH_DELTA;
                for (int t = 0; t < N; ++t)
                    for (int j = 0; j < NBOX; ++j)
                        if (clb_[t][j]) W.lb[t][j] += (r2b[t][j] - kBoxSign[j] * D_.du[2 * t + kBoxComp[j]]) / POLISH_DELTA;
            }
            // the crossover's solve is the unconstrained optimum of QP(ubar): kept for the interior-point start
            if (from == 1 && round == 0) std::memcpy(xo_du_, W.du, sizeof(double) * 2 * N);
            // KKT consistency of the solved point
            double lmax = 1.0;
            for (int k = 1; k <= N; ++k)
                for (int j = 0; j < NROW; ++j)
                    if (Q.on[j] && cls_[k][j] == 1) lmax = std::max(lmax, std::fabs(W.l[k][j]));
            for (int t = 0; t < N; ++t)
                for (int j = 0; j < NBOX; ++j)
                    if (clb_[t][j]) lmax = std::max(lmax, std::fabs(W.lb[t][j]));
            int nviol = 0;
            bool offending = false;
            for (int k = 1; k <= N; ++k)
                for (int j = 0; j < NROW; ++j) {
                    flip_[k][j] = 0;
                    if (!Q.on[j]) continue;
                    const double bsc = 1.0 + std::fabs(Q.b[k][j]);
                    const double r = dot5(Q.C[j], Xs[k]) - Q.b[k][j];
                    bool bad = false;
                    if (cls_[k][j] == 1) {
                        const double l = W.l[k][j];
                        bad = l < -1e-9 * lmax || l > rho * (1.0 + 1e-9) || std::fabs(r) > 1e-7 * bsc;
                    } else if (cls_[k][j] == 2) {
                        bad = r > 1e-9 * bsc;
                        if (r < -1e-6 * bsc) ++nviol;
                    } else {
                        bad = r < -1e-9 * bsc;
                    }
                    flip_[k][j] = bad;
                    offending = offending || bad;
                }
            for (int t = 0; t < N; ++t)
                for (int j = 0; j < NBOX; ++j) {
                    const double bsc = 1.0 + std::fabs(Q.bb[t][j]);
                    const double r = kBoxSign[j] * W.du[2 * t + kBoxComp[j]] - Q.bb[t][j];
                    const bool bad = clb_[t][j] ? (W.lb[t][j] < -1e-9 * lmax || std::fabs(r) > 1e-7 * bsc)
                                                : r < -1e-9 * bsc;
                    flipb_[t][j] = bad;
                    offending = offending || bad;
                }
            bool finite = true;
            for (int i = 0; i < 2 * N; ++i) finite = finite && W.du[i] == W.du[i];
            if (!finite) break;
            if (!offending) {
                std::memcpy(X.du, W.du, sizeof(double) * 2 * N);
                infeasible = nviol > 0;
                accepted = true;
                break;
            }
            for (int k = 1; k <= N; ++k)
                for (int j = 0; j < NROW; ++j)
                    if (flip_[k][j]) cls_[k][j] = cls_[k][j] == 1 ? (W.l[k][j] > rho ? 2 : 0) : 1;
            for (int t = 0; t < N; ++t)
                for (int j = 0; j < NBOX; ++j)
                    if (flipb_[t][j]) clb_[t][j] = !clb_[t][j];
        }
        std::memcpy(last_cls_, cls_, sizeof(last_cls_));
        std::memcpy(last_clb_, clb_, sizeof(last_clb_));
        return accepted;
    }

    // ---- crossover, then (if it does not certify) Mehrotra predictor-corrector PDIP and the polish
    int pdip(int& iters, bool warm) {
        const StageQp& Q = q_;
        const int N = Q.N;
        const double rho = Q.rho;
        std::memset(&S_, 0, sizeof(S_));
        iters = 0;
        if (p_.polish >= 2) {
            std::memset(&Z_, 0, sizeof(Z_));
            bool inf = false;
            if (active_set(Z_, warm ? 2 : 1, XO_ROUNDS, inf)) {
                std::memcpy(S_.du, Z_.du, sizeof(double) * 2 * N);
                return inf ? MPC_INFEASIBLE : MPC_OK;
            }
        }
        int nsoft = 0;
        for (int j = 0; j < NROW; ++j) nsoft += Q.on[j];
        const double Mtot = (double)(2 * nsoft * N + NBOX * N);
        // start centred at the unconstrained optimum of QP(ubar) (one factorisation and solve without rows), or
        // at du = 0 when the soft rows are less violated there:
        // slack max(r, 0) + shift, elastic slack max(-r, 0) + shift for the row value r there, the multiplier
        // pair on the pair's central path with lambda + nu = rho; box rows at the mean row complementarity
        double X[kMaxN + 1][5];
        if (p_.polish >= 2 && !warm) {
            // the crossover solved exactly this system (all rows inactive): its solution is the start's
            std::memcpy(S_.du, xo_du_, sizeof(double) * 2 * N);
        } else {
            double qh[kMaxN + 1][5], gh[kMaxN][2];
            for (int k = 1; k <= N; ++k) {
                std::memcpy(F_.Qt[k], Q.Q[k], sizeof(F_.Qt[k]));
                for (int a = 0; a < 5; ++a) qh[k][a] = -Q.q[k][a];
            }
            for (int t = 0; t < N; ++t) {
                F_.Rt[t][0] = Q.R[0];
                F_.Rt[t][1] = Q.R[1];
                gh[t][0] = -Q.r[t][0];
                gh[t][1] = -Q.r[t][1];
            }
            riccati_factor();
            riccati_solve(qh, gh, D_);
            std::memcpy(S_.du, D_.du, sizeof(double) * 2 * N);
        }
        rollout(S_.du, X);
        {
            // primal point: the unconstrained optimum, or du = 0 (ubar) when the soft rows are less violated there
            double v_unc = 0.0, v_bar = 0.0;
            for (int k = 1; k <= N; ++k)
                for (int j = 0; j < NROW; ++j) {
                    if (!Q.on[j]) continue;
                    const double r = dot5(Q.C[j], X[k]) - Q.b[k][j];
                    v_unc += r < 0.0 ? -r : 0.0;
                    v_bar += Q.b[k][j] > 0.0 ? Q.b[k][j] : 0.0;
                }
            if (v_bar < v_unc) {
                std::memset(S_.du, 0, sizeof(double) * 2 * N);
                rollout(S_.du, X);
            }
        }
        double bscale = 0.0, rowc = 0.0;
        for (int k = 1; k <= N; ++k)
            for (int j = 0; j < NROW; ++j) {
                if (!Q.on[j]) continue;
                const double r = dot5(Q.C[j], X[k]) - Q.b[k][j];
                const double sv = (r > 0.0 ? r : 0.0) + START_SHIFT, xi = (r < 0.0 ? -r : 0.0) + START_SHIFT;
                S_.s[k][j] = sv;
                S_.xi[k][j] = xi;
                S_.l[k][j] = rho * xi / (sv + xi);
                S_.nu[k][j] = rho * sv / (sv + xi);
                rowc += sv * S_.l[k][j];
                bscale = std::max(bscale, std::fabs(Q.b[k][j]));
            }
        const double mrow = rowc / (double)(nsoft * N);
        for (int t = 0; t < N; ++t)
            for (int j = 0; j < NBOX; ++j) {
                const double v = kBoxSign[j] * S_.du[2 * t + kBoxComp[j]] - Q.bb[t][j];
                S_.sb[t][j] = v > 1.0 ? v : 1.0;
                S_.lb[t][j] = mrow / S_.sb[t][j];
                bscale = std::max(bscale, std::fabs(Q.bb[t][j]));
            }
        double y[kMaxN + 1][5], yc[kMaxN + 1][5], ya[kMaxN + 1][5];
        double z[kMaxN][2], zc[kMaxN][2], za[kMaxN][2];
        double rp[kMaxN + 1][NROW], rx[kMaxN + 1][NROW], rpb[kMaxN][NBOX];
        double r4[kMaxN + 1][NROW], r5[kMaxN + 1][NROW], r4b[kMaxN][NBOX];
        int status = MPC_MAX_ITER, it = 0, stall = 0;
        bool checked = false;
        for (it = 0; it < p_.max_iter; ++it) {
            rollout(S_.du, X);
            double rpmax = 0.0, rxmax = 0.0, comp = 0.0;
            for (int k = 1; k <= N; ++k) {
                for (int a = 0; a < 5; ++a) {
                    double acc = Q.q[k][a];
                    for (int c = 0; c < 5; ++c) acc += Q.Q[k][a][c] * X[k][c];
                    yc[k][a] = acc;
                    ya[k][a] = 0.0;
                }
                for (int j = 0; j < NROW; ++j) {
                    if (!Q.on[j]) continue;
                    for (int a = 0; a < 5; ++a) ya[k][a] -= S_.l[k][j] * Q.C[j][a];
                    rp[k][j] = dot5(Q.C[j], X[k]) + S_.xi[k][j] - S_.s[k][j] - Q.b[k][j];
                    rx[k][j] = rho - S_.l[k][j] - S_.nu[k][j];
                    rpmax = std::max(rpmax, std::fabs(rp[k][j]));
                    rxmax = std::max(rxmax, std::fabs(rx[k][j]));
                    comp += S_.s[k][j] * S_.l[k][j] + S_.xi[k][j] * S_.nu[k][j];
                }
                for (int a = 0; a < 5; ++a) y[k][a] = yc[k][a] + ya[k][a];
            }
            for (int t = 0; t < N; ++t) {
                zc[t][0] = Q.R[0] * S_.du[2 * t] + Q.r[t][0];
                zc[t][1] = Q.R[1] * S_.du[2 * t + 1] + Q.r[t][1];
                za[t][0] = -S_.lb[t][0] + S_.lb[t][1];
                za[t][1] = -S_.lb[t][2] + S_.lb[t][3];
                z[t][0] = zc[t][0] + za[t][0];
                z[t][1] = zc[t][1] + za[t][1];
                for (int j = 0; j < NBOX; ++j) {
                    rpb[t][j] = kBoxSign[j] * S_.du[2 * t + kBoxComp[j]] - S_.sb[t][j] - Q.bb[t][j];
                    rpmax = std::max(rpmax, std::fabs(rpb[t][j]));
                    comp += S_.sb[t][j] * S_.lb[t][j];
                }
            }
            const double mu = comp / Mtot;
            if (!(mu == mu)) { status = MPC_NUMERICAL; break; }
            if (mu <= p_.tol_mu && rpmax <= 10.0 * p_.tol * (1.0 + bscale) && rxmax <= p_.tol * rho) {
                // converged: the dual residual (an adjoint recursion, once per solve) carries O(eps/mu)
                // multiplier noise and is required to 1e4 tol; the polish then makes the active set exact
                double gd[2 * kMaxN], gc[2 * kMaxN], ga[2 * kMaxN];
                adjoint(y, z, gd);
                adjoint(yc, zc, gc);
                adjoint(ya, za, ga);
                double rdmax = 0.0, sd = 0.0;
                for (int i = 0; i < 2 * N; ++i) {
                    rdmax = std::max(rdmax, std::fabs(gd[i]));
                    sd = std::max(sd, std::max(std::fabs(gc[i]), std::fabs(ga[i])));
                }
                status = rdmax <= 1e4 * p_.tol * (1.0 + sd) ? MPC_OK : MPC_NUMERICAL;
                break;
            }
            // checkpoint (once per QP): no near-tie between any row's slack and multiplier at mu <= MU_CHECK ->
            // CHECK_ROUNDS polish rounds from the iterate's classification; certified = the exact optimum, else
            // the interior point continues from the unchanged iterate
            if (p_.polish && !checked && mu <= MU_CHECK && checkpoint_on()) {
                bool tie = false;
                for (int k = 1; k <= N && !tie; ++k)
                    for (int j = 0; j < NROW; ++j) {
                        if (!Q.on[j]) continue;
                        const double s = S_.s[k][j], l = S_.l[k][j], x = S_.xi[k][j], n = S_.nu[k][j];
                        if (!(s > CHECK_SEP * l || l > CHECK_SEP * s) || !(x > CHECK_SEP * n || n > CHECK_SEP * x)) tie = true;
                    }
                for (int t = 0; t < N && !tie; ++t)
                    for (int j = 0; j < NBOX; ++j)
                        if (!(S_.sb[t][j] > CHECK_SEP * S_.lb[t][j] || S_.lb[t][j] > CHECK_SEP * S_.sb[t][j])) tie = true;
                if (!tie) {
                    checked = true;
                    std::memcpy(&C_, &S_, sizeof(C_));
                    bool inf = false;
                    if (active_set(C_, 0, CHECK_ROUNDS, inf)) {
                        std::memcpy(S_.du, C_.du, sizeof(double) * 2 * N);
                        iters = it;
                        return inf ? MPC_INFEASIBLE : MPC_OK;
                    }
                }
            }
            factor();
            // predictor (affine scaling)
            for (int k = 1; k <= N; ++k)
                for (int j = 0; j < NROW; ++j) {
                    r4[k][j] = S_.s[k][j] * S_.l[k][j];
                    r5[k][j] = S_.xi[k][j] * S_.nu[k][j];
                }
            for (int t = 0; t < N; ++t)
                for (int j = 0; j < NBOX; ++j) r4b[t][j] = S_.sb[t][j] * S_.lb[t][j];
            newton(rp, rpb, rx, y, z, r4, r5, r4b, Da_);
            const double aa = max_step(Da_);
            double sig = comp_after(Da_, aa) / Mtot / mu;
            sig = sig * sig * sig;
            // Mehrotra corrector
            for (int k = 1; k <= N; ++k)
                for (int j = 0; j < NROW; ++j) {
                    r4[k][j] = S_.s[k][j] * S_.l[k][j] + Da_.ds[k][j] * Da_.dl[k][j] - sig * mu;
                    r5[k][j] = S_.xi[k][j] * S_.nu[k][j] + Da_.dxi[k][j] * Da_.dnu[k][j] - sig * mu;
                }
            for (int t = 0; t < N; ++t)
                for (int j = 0; j < NBOX; ++j)
                    r4b[t][j] = S_.sb[t][j] * S_.lb[t][j] + Da_.dsb[t][j] * Da_.dlb[t][j] - sig * mu;
            newton(rp, rpb, rx, y, z, r4, r5, r4b, D_);
            double a = std::min(1.0, TAU * max_step(D_));
            double cnew = comp_after(D_, a);
            if (cnew > comp) {
                // safeguard: the second-order term made it worse; take the plain centred direction
                for (int k = 1; k <= N; ++k)
                    for (int j = 0; j < NROW; ++j) {
                        r4[k][j] = S_.s[k][j] * S_.l[k][j] - sig * mu;
                        r5[k][j] = S_.xi[k][j] * S_.nu[k][j] - sig * mu;
                    }
                for (int t = 0; t < N; ++t)
                    for (int j = 0; j < NBOX; ++j) r4b[t][j] = S_.sb[t][j] * S_.lb[t][j] - sig * mu;
                newton(rp, rpb, rx, y, z, r4, r5, r4b, D_);
                a = std::min(1.0, TAU * max_step(D_));
                cnew = comp_after(D_, a);
            }
            // breakdown guard: a step whose complementarity or control direction is not finite is not taken
            bool fin = cnew == cnew && cnew < INFINITY;
            for (int i = 0; i < 2 * N && fin; ++i) fin = D_.du[i] == D_.du[i] && std::fabs(D_.du[i]) < INFINITY;
            if (!fin) { status = MPC_NUMERICAL; ++it; break; }
            stall = (mu < 1e-6 && cnew > 0.9 * comp) ? stall + 1 : 0;     // late-phase no-progress counter
            for (int i = 0; i < 2 * N; ++i) S_.du[i] += a * D_.du[i];
            for (int k = 1; k <= N; ++k)
                for (int j = 0; j < NROW; ++j) {
                    if (!Q.on[j]) continue;
                    S_.s[k][j] += a * D_.ds[k][j];
                    S_.l[k][j] += a * D_.dl[k][j];
                    S_.xi[k][j] += a * D_.dxi[k][j];
                    S_.nu[k][j] += a * D_.dnu[k][j];
                }
            for (int t = 0; t < N; ++t)
                for (int j = 0; j < NBOX; ++j) {
                    S_.sb[t][j] += a * D_.dsb[t][j];
                    S_.lb[t][j] += a * D_.dlb[t][j];
                }
            if (stall >= 5) { status = MPC_NUMERICAL; ++it; break; }
        }
        iters = it;
        for (int i = 0; i < 2 * N; ++i)
            if (!(S_.du[i] == S_.du[i])) {
                std::memset(S_.du, 0, sizeof(double) * 2 * N);
                return MPC_NUMERICAL;
            }
        if (status == MPC_OK)
            for (int k = 1; k <= N; ++k)
                for (int j = 0; j < NROW; ++j)
                    if (Q.on[j] && S_.xi[k][j] > 1e-6 * (1.0 + std::fabs(Q.b[k][j]))) status = MPC_INFEASIBLE;
        if (p_.polish) {
            bool inf = false;
            if (active_set(S_, 0, POLISH_ROUNDS, inf)) status = inf ? MPC_INFEASIBLE : MPC_OK;
        }
        return status;
    }
};

// ---------------------------------------------------------------------------------------------
// the backend object behind a device = -1 context
// ---------------------------------------------------------------------------------------------
inline void sweep_max_step_ms(int B, const int* n_steps, const std::vector<double>& ms, double* quant);

// mpc_noise_draw on the host (the noise source is loop_steps.h's); words and z may be null
inline void noise_draw(unsigned long long seed, int n, const long long* ego, const int* step, const int* channel,
                       unsigned* words, double* z) {
    for (int i = 0; i < n; ++i) {
        const unsigned long long g = (unsigned long long)ego[i];
        unsigned w[4];
        noise_words((unsigned)g, (unsigned)(g >> 32), (unsigned)step[i], (unsigned)channel[i], (unsigned)seed,
                    (unsigned)(seed >> 32), w);
        if (words) std::memcpy(words + 4 * (size_t)i, w, sizeof(w));
        if (z) z[i] = noise_variate(w);
    }
}

// mpc_evaluate_batch for one instance (include/mpcqp.h): tracker_model.h's steps of a control and of a stage, which
// mpc_evaluate_kernel (evaluate_kernel.h) runs a lane each, folded here one after the other, so every output
// equals the device's bit for bit.  X is the rollout predict(x0, U) [N+1][5]; rw the row width 7 + params.max_obs;
// summary [MPC_EV_NQ], terms [5] and rows [N][rw] may be null.
inline void evaluate_one(const DevTable& R, const mpc_params& p, const double (*X)[5], const double* obs, int nobs,
                         int rw, const double* U, double* summary, double* terms, double* rows) {
    const int N = p.N;
    const KParams P = model_params(p);
    double ct[kMaxN][5], part[kMaxN];
    EvRun run = ev_run_begin();
    // np.argmin takes the first NaN row if there is one, else the first minimum
    double gmin = INFINITY, cnt = 0.0;
    bool gnan = false;
    int astage = 0, akind = 0;
    for (int k = 0; k < N; ++k) ev_control(P, U[2 * k], U[2 * k + 1], ct[k], run);
    for (int j = 1; j <= N; ++j) {
        double st[5];
        get_state(R, X[j][0], st);
        EvStage S = ev_stage_begin();
        ev_stage(P, j, X[j], st, obs, nobs, rw, ct[j - 1], rows ? rows + (size_t)(j - 1) * rw : nullptr, S, run);
        part[j - 1] = S.p1;
        cnt += (double)S.nneg;
        if (!gnan && (astage == 0 || S.snan || S.smin < gmin)) {
            gmin = S.smin;
            gnan = S.snan;
            astage = j;
            akind = S.skind;
        }
    }
    const EvSums Z = ev_sums(N, &ct[0][0], part);
    if (summary)
        ev_summary(summary, Z, gnan ? (double)NAN : gmin, astage, akind, cnt, run.fl, run.fo, run.fv, run.bx,
                   ev_flags(run, gnan), nobs);
    if (terms) std::memcpy(terms, Z.t, sizeof(Z.t));
}

// The linearisation the gradient, the multiplier estimate and the Hessian-vector products start from, for one instance:
// the host twin of evaluator_common.h's evc_linearise and evc_sweeps, folded over the stages one after the other.  From
// the rollout X [N+1][5] it fills the cost terms ct and the zero L1 partials (ev_sums' operands), A_0..A_N-1, the
// slopes of the reference at s_0..s_N, the stage gradients q and c (c weighted by lam [N][rw], zero without it), and
// then sweeps q (and c, with lam) in place into the costates; g0 = A_0' p_1 of the cost.  With `rows` [rw] each stage's
// rows are stored there and after_stage(j) is called while they hold stage j's.
struct Linearised {
    double ct[kMaxN][5], part[kMaxN], A[kMaxN][5], q[kMaxN][5], c[kMaxN][5], sl[kMaxN + 1][4], g0[5];
};
template <typename AfterStage>
inline void linearise_one(const DevTable& R, const KParams& P, int N, const double (*X)[5], const double* obs, int nobs,
                          int rw, const double* U, const double* lam, double* rows, Linearised& L, GrRun& G,
                          AfterStage after_stage) {
    EvRun run = ev_run_begin();
    for (int k = 0; k < N; ++k) ev_control(P, U[2 * k], U[2 * k + 1], L.ct[k], run);
    for (int j = 0; j <= N; ++j) {
        double st[5];
        get_state(R, X[j][0], st, L.sl[j]);
        if (j < N) stage_A(X[j], P.dt, st[3], L.sl[j][2], L.A[j]);
        if (j >= 1) {
            EvStage S = ev_stage_begin();
            ev_stage(P, j, X[j], st, obs, nobs, rw, L.ct[j - 1], rows, S, run);
            gr_stage(P, j, X[j], st, L.sl[j], obs, nobs, lam ? lam + (size_t)(j - 1) * rw : nullptr, L.q[j - 1],
                     L.c[j - 1], G);
            L.part[j - 1] = 0.0;
            after_stage(j);
        }
    }
    double g0r[5];
    for (int rows_too = 0; rows_too <= (lam ? 1 : 0); ++rows_too)
        gr_sweep(N, P.dt, &L.A[0][0], rows_too ? &L.c[0][0] : &L.q[0][0], rows_too ? g0r : L.g0);
}
inline void linearise_one(const DevTable& R, const KParams& P, int N, const double (*X)[5], const double* obs, int nobs,
                          int rw, const double* U, const double* lam, Linearised& L, GrRun& G) {
    linearise_one(R, P, N, X, obs, nobs, rw, U, lam, nullptr, L, G, [](int) {});
}

// mpc_gradient_batch for one instance (include/mpcqp.h): the linearisation above, then tracker_model.h's step of a
// control, which mpc_gradient_kernel (gradient_kernel.h) runs a lane each, folded here one after the other, so every
// output equals the device's bit for bit.  X is the rollout predict(x0, U) [N+1][5]; lam [N][rw]
// (rw = 7 + params.max_obs), grad [N][2], jtl [N][2], gx0 [5], costate [N][5] and summary [MPC_GR_NQ] may be null.
inline void gradient_one(const DevTable& R, const mpc_params& p, const double (*X)[5], const double* obs, int nobs,
                         int rw, const double* U, const double* lam, double* grad, double* jtl, double* gx0,
                         double* costate, double* summary) {
    const int N = p.N;
    const KParams P = model_params(p);
    Linearised L;
    GrRun G = gr_run_begin();
    linearise_one(R, P, N, X, obs, nobs, rw, U, lam, L, G);
    for (int k = 0; k < N; ++k) {
        double g[2], jt[2];
        gr_control(P, U[2 * k], U[2 * k + 1], L.q[k], lam ? L.c[k] : nullptr, g, jt, G);
        if (grad) std::memcpy(grad + 2 * k, g, sizeof(g));
        if (jtl) std::memcpy(jtl + 2 * k, jt, sizeof(jt));
    }
    if (gx0) std::memcpy(gx0, L.g0, sizeof(L.g0));
    if (costate) std::memcpy(costate, L.q, sizeof(double) * 5 * N);
    if (summary) gr_summary(summary, ev_sums(N, &L.ct[0][0], L.part).cost, G, lam != nullptr);
}

// mpc_multipliers_batch for one instance (include/mpcqp.h): the linearisation above without row weights, its rows
// listed stage by stage, then tracker_model.h's mu_* steps, which mpc_multipliers_kernel (multiplier_kernel.h) runs with a lane per
// active row, folded here one after the other in the order the header states, so every output equals the device's
// bit for bit.  lam [N][rw], active [MPC_MAX_ACTIVE] and summary [MPC_MU_NQ] may be null.
inline void multipliers_one(const DevTable& R, const mpc_params& p, const double (*X)[5], const double* obs, int nobs,
                            int rw, const double* U, double active_tol, double bound_tol, double rank_tol, double* lam,
                            int* active, double* summary) {
    constexpr int MA = MPC_MAX_ACTIVE;
    const int N = p.N, n2 = 2 * N;
    const KParams P = model_params(p);
    double rows[7 + MPC_MAX_OBS];
    int list[MA], na = 0;
    bool nonfinite = false;
    Linearised L;
    GrRun Gd = gr_run_begin();
    linearise_one(R, P, N, X, obs, nobs, rw, U, nullptr, rows, L, Gd, [&](int j) {
        for (int i = 0; i < 7 + nobs; ++i) {
            const int col = mu_list_col(i, nobs);
            if (rows[col] != rows[col]) nonfinite = true;
            if (!mu_active(rows[col], active_tol)) continue;
            if (na < MA) list[na] = (j - 1) * rw + col;
            ++na;
        }
    });
    const double(*A)[5] = L.A, (*q)[5] = L.q;
    double grad[2 * kMaxN];
    bool fr[2 * kMaxN];
    int nf = 0;
    for (int k = 0; k < N; ++k) {
        double jt[2];
        gr_control(P, U[2 * k], U[2 * k + 1], q[k], nullptr, grad + 2 * k, jt, Gd);
        fr[2 * k] = mu_free(U[2 * k], P.u_min0, P.u_max0, bound_tol);
        fr[2 * k + 1] = mu_free(U[2 * k + 1], P.u_min1, P.u_max1, bound_tol);
        for (int c = 0; c < 2; ++c)
            if (fr[2 * k + c]) {
                ++nf;
                if (!mu_finite(grad[2 * k + c])) nonfinite = true;
            }
    }
    const bool listed = na <= MA && na > 0 && nf > 0;
    static thread_local double J[MA][2 * kMaxN], W[MA][MA];
    if (listed)
        for (int a = 0; a < na; ++a) {
            const int t = list[a] / rw + 1;
            double c[5];
            mu_row_grad(P, list[a] % rw, X[t], c);
            for (int i = 0; i < n2; ++i) J[a][i] = 0.0;
            mu_row_chain(t, P.dt, &A[0][0], c, [&](int i, double v) {
                J[a][i] = v;
                if (fr[i] && !mu_finite(v)) nonfinite = true;
            });
        }
    const int status = mu_status(na, nf, nonfinite);
    double lamv[MA], resid = 0.0, minpiv = INFINITY;
    bool keep[MA];
    int nu = 0;
    for (int a = 0; a < MA; ++a) { lamv[a] = 0.0; keep[a] = false; }
    if (status == MPC_MU_OK) {
        const int m = listed ? na : 0;
        double r[MA], g0[MA];
        for (int a = 0; a < m; ++a) {
            for (int b = 0; b <= a; ++b) {
                double s = 0.0;
                for (int i = 0; i < n2; ++i)
                    if (fr[i]) s = s + J[a][i] * J[b][i];
                W[a][b] = s;
            }
            double s = 0.0;
            for (int i = 0; i < n2; ++i)
                if (fr[i]) s = s + J[a][i] * grad[i];
            r[a] = s;
            g0[a] = W[a][a];
        }
        // right-looking: after column c every later row has L[a][c] L[b][c] taken off its entries, so the terms of
        // an entry are subtracted in increasing c; r turns into y the same way
        for (int c = 0; c < m; ++c) {
            const double d = W[c][c];
            keep[c] = mu_keep(d, g0[c], rank_tol);
            if (!keep[c]) continue;
            ++nu;
            const double piv = d / g0[c];
            if (piv < minpiv) minpiv = piv;
            const double lcc = std::sqrt(d);
            W[c][c] = lcc;
            r[c] = r[c] / lcc;
            for (int a = c + 1; a < m; ++a) {
                W[a][c] = W[a][c] / lcc;
                r[a] = r[a] - W[a][c] * r[c];
                for (int b = c + 1; b <= a; ++b) W[a][b] = W[a][b] - W[a][c] * W[b][c];
            }
        }
        for (int c = m - 1; c >= 0; --c) {
            if (!keep[c]) continue;
            lamv[c] = r[c] / W[c][c];
            for (int a = 0; a < c; ++a) r[a] = r[a] - W[c][a] * lamv[c];
        }
        for (int i = 0; i < n2; ++i) {
            if (!fr[i]) continue;
            double s = 0.0;
            for (int a = 0; a < m; ++a)
                if (keep[a]) s = s + lamv[a] * J[a][i];
            gr_nmax(resid, fabs(grad[i] - s));
        }
    }
    if (lam) {
        for (int i = 0; i < N * rw; ++i) lam[i] = 0.0;
        for (int a = 0; a < MA; ++a)
            if (keep[a]) lam[list[a]] = lamv[a];
    }
    if (active)
        for (int a = 0; a < MA; ++a) active[a] = (na <= MA && a < na) ? list[a] : -1;
    if (summary) mu_summary(summary, status, na, nf, nu, resid, minpiv);
}

// mpc_hessvec_batch for one instance (include/mpcqp.h): the linearisation above (the rollout's stage data, both
// reverse sweeps), pi = p - p', then tracker_model.h's hv_* steps, which mpc_hessvec_kernel
// (hessvec_kernel.h) runs with a lane per direction, folded here one direction after the other, so every output
// equals the device's bit for bit.  V [M][N][2] or null (unit directions), HV [M][N][2], JV [M][N][rw], curv [M][2]
// and summary [MPC_HV_NQ] may be null.
inline void hessvec_one(const DevTable& R, const mpc_params& p, const double (*X)[5], const double* obs, int nobs,
                        int rw, const double* U, const double* lam, int M, const double* V, int mode, double* HV,
                        double* JV, double* curv, double* summary) {
    const int N = p.N;
    const KParams P = model_params(p);
    const bool exact = mode == MPC_HV_EXACT;
    Linearised L;
    GrRun G = gr_run_begin();
    linearise_one(R, P, N, X, obs, nobs, rw, U, lam, L, G);
    double(*q)[5] = L.q;
    const double(*A)[5] = L.A, (*sl)[4] = L.sl;
    if (lam)
        for (int k = 0; k < N; ++k)
            for (int a = 0; a < 5; ++a) q[k][a] = q[k][a] - L.c[k][a];    // pi = p - p'
    double cvs[MPC_HV_MAX_DIRS][2];
    for (int m = 0; m < M; ++m) {
        const double* Vd = V ? V + (size_t)m * 2 * N : nullptr;
        double dX[kMaxN][5];                   // dX[k] = dx_k+1
        double dx[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
        for (int k = 0; k < N; ++k) {
            hv_tangent_step(A[k], P.dt, dx, hv_dir(Vd, m, k, 0), hv_dir(Vd, m, k, 1), dX[k]);
            std::memcpy(dx, dX[k], sizeof(dx));
        }
        if (JV)
            for (int k = 0; k < N; ++k)
                for (int col = 0; col < rw; ++col)
                    JV[((size_t)m * N + k) * rw + col] = hv_row_tangent(P, col, nobs, X[k + 1], dX[k]);
        if (!HV && !curv && !summary) continue;
        double dp[5] = {0.0, 0.0, 0.0, 0.0, 0.0}, qd[5], e[5] = {0.0, 0.0, 0.0, 0.0, 0.0}, y[5], dpc[kMaxN][2];
        for (int k = N; k >= 1; --k) {
            hv_stage(P, sl[k], dX[k - 1], qd);
            if (k == N) {
                std::memcpy(y, qd, sizeof(y));
            } else {
                if (exact) hv_second_order(P.dt, sl[k][2], dX[k - 1], q[k], e);
                hv_reverse_step(A[k], P.dt, qd, dp, exact, e, y);
            }
            std::memcpy(dp, y, sizeof(dp));
            dpc[k - 1][0] = y[3];
            dpc[k - 1][1] = y[4];
        }
        double cv[2] = {0.0, 0.0}, hv[2];
        for (int k = 0; k < N; ++k) {
            const double v1 = hv_dir(Vd, m, k, 0), v2 = hv_dir(Vd, m, k, 1);
            dp[3] = dpc[k][0];
            dp[4] = dpc[k][1];
            hv_control(P, v1, v2, dp, hv);
            hv_curv(cv, v1, hv[0]);
            hv_curv(cv, v2, hv[1]);
            if (HV) std::memcpy(HV + ((size_t)m * N + k) * 2, hv, sizeof(hv));
        }
        cvs[m][0] = cv[0];
        cvs[m][1] = cv[1];
    }
    if (curv) std::memcpy(curv, cvs, sizeof(double) * 2 * M);
    if (summary) hv_summary(summary, ev_sums(N, &L.ct[0][0], L.part).cost, M, &cvs[0][0]);
}

// ---------------------------------------------------------------------------------------------
// shared pieces of the closed-loop members of Backend
// ---------------------------------------------------------------------------------------------
// a history array before the loop: steps that never run stay NaN / -1
template <typename T>
inline void hist_prefill(T* h, size_t n, T v) {
    if (h) std::fill(h, h + n, v);
}

// What every closed-loop member keeps per ego, the outputs they share and the plant step.  quant is
// [B][MPC_CL_NQ]; history rows exist for the egos with slot[b] >= 0 (row slot[b] of the [n_hist][...] arrays);
// the histories and step_ms are optional.  The steps and the quantity rules are loop_steps.h's
struct LoopEgos {
    const int B;
    const size_t ns;
    const double s_stop;
    const int* const slot;
    double* const quant;
    double *const hist_x, *const hist_u;
    int* const hist_status;
    double* const step_ms;
    std::vector<double> x, ms;
    std::vector<int> qflags, active, nrun;

    LoopEgos(int B_, const double* x_init, int max_steps, double s_stop_, double* quant_, int n_hist, const int* slot_,
             double* hist_x_, double* hist_u_, int* hist_status_, double* step_ms_)
        : B(B_), ns((size_t)max_steps), s_stop(s_stop_), slot(slot_), quant(quant_), hist_x(hist_x_), hist_u(hist_u_),
          hist_status(hist_status_), step_ms(step_ms_), x(x_init, x_init + (size_t)B_ * 5), qflags((size_t)B_, 0),
          active((size_t)B_), nrun((size_t)B_, 0) {
        const size_t nh = (size_t)n_hist;
        hist_prefill(hist_x, nh * (ns + 1) * 5, (double)NAN);
        hist_prefill(hist_u, nh * ns * 2, (double)NAN);
        hist_prefill(hist_status, nh * ns, -1);
        hist_prefill(step_ms, ns, (double)NAN);
        for (int b = 0; b < B; ++b) {
            active[b] = x[5 * (size_t)b] <= s_stop;
            if (hist_x && slot[b] >= 0)
                std::memcpy(hist_x + (size_t)slot[b] * (ns + 1) * 5, x.data() + 5 * (size_t)b, 5 * sizeof(double));
            quant_init(quant + (size_t)b * MPC_CL_NQ, b, x[5 * (size_t)b], x[5 * (size_t)b + 1]);
        }
    }

    // The plant step x + dt f(x, ua, k_ref(s)) (:403-406) of ego b with the applied control ua, then perturb(x)
    // on the new state; the kept history rows and the plant-side quantities (u: the commanded control)
    template <typename Perturb>
    void plant(const DevTable& ref, double dt, int b, int step, const double* u, const double* ua, int status,
               Perturb perturb) {
        double* xb = x.data() + 5 * (size_t)b;
        double st[5];
        get_state(ref, xb[0], st);
        plant_step(xb, dt, ua[0], ua[1], st[3]);
        perturb(xb);
        if (slot[b] >= 0) {
            const size_t h = (size_t)slot[b];
            if (hist_x) std::memcpy(hist_x + (h * (ns + 1) + step + 1) * 5, xb, 5 * sizeof(double));
            if (hist_u) std::memcpy(hist_u + (h * ns + step) * 2, u, 2 * sizeof(double));
            if (hist_status) hist_status[h * ns + step] = status;
        }
        nrun[b] = step + 1;
        plant_quant(quant + (size_t)b * MPC_CL_NQ, step, xb, u[0], u[1], status);
        if (!(xb[0] <= s_stop)) active[b] = 0;
    }

    // after the loop: MPC_CLQ_MAX_STEP_MS and the optional n_steps
    void finish(int* n_steps) {
        sweep_max_step_ms(B, nrun.data(), ms, quant);
        if (n_steps) std::memcpy(n_steps, nrun.data(), (size_t)B * sizeof(int));
    }
};

// One ego's script of A actors for one step: actor_step per actor on its own state (fl, val), visited in index
// order; o takes what they emit and their number is returned.  Updates the gap and red-pass quantities (q, e: the
// ego's quant and extra rows), green (bit a: actor a is a GREEN light) and car_s (the first car on the road, else
// NaN)
inline int script_step(const mpc_actor* sc, int A, double dt, double s, double v, int* fls, double* vals, double* o,
                       double* q, double* e, int& qflags, int& green, double& car_s) {
    int n = 0, have_car = 0;
    green = 0;
    car_s = NAN;
    for (int a = 0; a < A; ++a) {
        if (sc[a].kind == MPC_ACTOR_NONE) continue;
        double os, ov;
        const int r = actor_step(sc[a], dt, s, v, fls[a], vals[a], os, ov);
        if (r & ACTOR_GREEN) green |= 1 << a;
        if (r & ACTOR_RAN_RED) {
            q[MPC_CLQ_RED_PASS] = 1.0;
            e[MPC_TRX_N_RED_PASS] += 1.0;
        }
        if (!(r & ACTOR_EMITS)) continue;
        o[2 * n] = os;
        o[2 * n + 1] = ov;
        ++n;
        if (sc[a].kind != MPC_ACTOR_CAR) continue;
        if (!have_car) { have_car = 1; car_s = os; }
        if (os == os && min_gap(q[MPC_CLQ_MIN_OBS_DIST], qflags, os - s)) e[MPC_TRX_MIN_GAP_ACTOR] = (double)a;
    }
    return n;
}

struct Backend {
    HostTable table;
    const DevTable ref;      // the table seen by tracker_model.h's lookups
    int threads = 0;

    explicit Backend(HostTable&& t) : table(std::move(t)), ref(table.view()) {
        const char* e = std::getenv("MPC_CPU_THREADS");
        threads = e ? std::atoi(e) : 0;
        if (threads <= 0) threads = (int)std::max(1u, std::thread::hardware_concurrency());
    }

    // run body(worker, i) for i in [0, n) over the worker threads (dynamic chunks of 8 instances)
    template <typename Body>
    void parallel(const mpc_params& p, int n, Body body) const {
        const int nt = std::max(1, std::min(threads, (n + 7) / 8));
        std::atomic<int> next(0);
        // a worker that cannot get its scratch leaves its share to the others; no exception leaves a thread
        auto run = [&]() {
            std::unique_ptr<Worker> w;
            try {
                w.reset(new Worker(ref, p));
            } catch (...) {
                return;
            }
            for (;;) {
                const int i0 = next.fetch_add(8);
                if (i0 >= n) break;
                for (int i = i0; i < std::min(n, i0 + 8); ++i) body(*w, i);
            }
        };
        std::vector<std::thread> pool;
        if (nt > 1) {
            try {
                pool.reserve(nt - 1);
                for (int t = 1; t < nt; ++t) pool.emplace_back(run);
            } catch (...) {
                // fewer threads than asked: the ones that started and this one finish the work
            }
        }
        run();
        for (auto& th : pool) th.join();
        // every worker failed to start: nothing was solved
        if (next.load() < n) throw std::bad_alloc();
    }

    // mpc_solve_batch on host buffers (the device entry's argument contract)
    void solve_batch(const mpc_params& p, int B, const double* x0, const double* obs, const int* n_obs,
                     const double* ubar, double* u0, double* U, double* Xpred, int* status, int* iters) const {
        const int N = p.N, mo = obs ? p.max_obs : 0;
        parallel(p, B, [&](Worker& w, int b) {
            const int no = obstacle_count(obs, n_obs, mo, b);
            int it = 0;
            const int st = w.solve(x0 + 5 * (size_t)b, obs ? obs + (size_t)b * mo * 2 : nullptr, no,
                                   ubar ? ubar + (size_t)b * 2 * N : nullptr, u0 ? u0 + 2 * (size_t)b : nullptr,
                                   U ? U + (size_t)b * 2 * N : nullptr,
                                   Xpred ? Xpred + (size_t)b * 5 * (N + 1) : nullptr, &it);
            if (status) status[b] = st;
            if (iters) iters[b] = it;
        });
    }

    // the obstacle count of instance b as the solver reads it: none without obs, NULL = all max_obs rows, clamped
    static int obstacle_count(const double* obs, const int* n_obs, int mo, int b) {
        const int no = obs ? (n_obs ? n_obs[b] : mo) : 0;
        return no < 0 ? 0 : (no > mo ? mo : no);
    }
    // instance b's part of an optional array of `stride` elements per instance
    template <typename T>
    static T* at(T* a, int b, size_t stride) { return a ? a + (size_t)b * stride : nullptr; }

    // What the evaluators do per instance (the host twin of evaluator_common.h's evc_instance and evc_rollout): the
    // obstacle slab and count, the control sequence and the rollout X = predict(x0, U); one(b, X, Ub, obs_b, no)
    // then computes the entry's outputs of instance b
    template <typename One>
    void evaluator_instances(const mpc_params& p, int B, const double* x0, const double* obs, const int* n_obs,
                             const double* U, One one) const {
        const int N = p.N, mo = obs ? p.max_obs : 0;
        parallel(p, B, [&](Worker& w, int b) {
            double X[kMaxN + 1][5];
            const double* Ub = U + (size_t)b * 2 * N;
            w.predict(x0 + 5 * (size_t)b, Ub, X);
            one(b, X, Ub, at(obs, b, (size_t)mo * 2), obstacle_count(obs, n_obs, mo, b));
        });
    }

    // mpc_evaluate_batch on host buffers (the device entry's argument contract); rows are [B][N][7 + p.max_obs]
    void evaluate_batch(const mpc_params& p, int B, const double* x0, const double* obs, const int* n_obs,
                        const double* U, double* Xpred, double* summary, double* terms, double* rows) const {
        const size_t N = p.N, rw = 7 + p.max_obs;
        evaluator_instances(p, B, x0, obs, n_obs, U, [&](int b, const double (*X)[5], const double* Ub, const double* ob, int no) {
            if (Xpred) std::memcpy(Xpred + (size_t)b * 5 * (N + 1), X, sizeof(double) * 5 * (N + 1));
            if (summary || terms || rows)
                evaluate_one(ref, p, X, ob, no, (int)rw, Ub, at(summary, b, MPC_EV_NQ), at(terms, b, 5), at(rows, b, N * rw));
        });
    }

    // mpc_gradient_batch on host buffers (the device entry's argument contract); lam is [B][N][7 + p.max_obs]
    void gradient_batch(const mpc_params& p, int B, const double* x0, const double* obs, const int* n_obs,
                        const double* U, const double* lam, double* grad, double* jtl, double* gx0, double* costate,
                        double* summary) const {
        const size_t N = p.N, rw = 7 + p.max_obs;
        evaluator_instances(p, B, x0, obs, n_obs, U, [&](int b, const double (*X)[5], const double* Ub, const double* ob, int no) {
            gradient_one(ref, p, X, ob, no, (int)rw, Ub, at(lam, b, N * rw), at(grad, b, 2 * N), at(jtl, b, 2 * N),
                         at(gx0, b, 5), at(costate, b, 5 * N), at(summary, b, MPC_GR_NQ));
        });
    }

    // mpc_multipliers_batch on host buffers (the device entry's argument contract); lam is [B][N][7 + p.max_obs]
    void multipliers_batch(const mpc_params& p, int B, const double* x0, const double* obs, const int* n_obs,
                           const double* U, double active_tol, double bound_tol, double rank_tol, double* lam,
                           int* active, double* summary) const {
        const size_t N = p.N, rw = 7 + p.max_obs;
        evaluator_instances(p, B, x0, obs, n_obs, U, [&](int b, const double (*X)[5], const double* Ub, const double* ob, int no) {
            multipliers_one(ref, p, X, ob, no, (int)rw, Ub, active_tol, bound_tol, rank_tol, at(lam, b, N * rw),
                            at(active, b, MPC_MAX_ACTIVE), at(summary, b, MPC_MU_NQ));
        });
    }

    // mpc_hessvec_batch on host buffers (the device entry's argument contract)
    void hessvec_batch(const mpc_params& p, int B, const double* x0, const double* obs, const int* n_obs,
                       const double* U, const double* lam, int M, const double* V, int mode, double* HV, double* JV,
                       double* curv, double* summary) const {
        const size_t N = p.N, rw = 7 + p.max_obs, m = (size_t)M;
        evaluator_instances(p, B, x0, obs, n_obs, U, [&](int b, const double (*X)[5], const double* Ub, const double* ob, int no) {
            hessvec_one(ref, p, X, ob, no, (int)rw, Ub, at(lam, b, N * rw), M, at(V, b, m * 2 * N), mode, at(HV, b, m * 2 * N),
                        at(JV, b, m * N * rw), at(curv, b, m * 2), at(summary, b, MPC_HV_NQ));
        });
    }

    void lookup(int n, const double* s, double* st, double* ct) const {
        for (int i = 0; i < n; ++i) {
            double o[5], c[2];
            get_state(ref, s[i], o);
            get_control(ref, s[i], c);
            if (st) std::memcpy(st + 5 * (size_t)i, o, sizeof(o));
            if (ct) std::memcpy(ct + 2 * (size_t)i, c, sizeof(c));
        }
    }

    void pose(int n, const double* s, const double* d, double* out) const {
        for (int i = 0; i < n; ++i) global_pose(ref, s[i], d[i], out + 3 * (size_t)i);
    }

    // The loop of every closed-loop member, step-synchronous like the device loop.  Per step: the list of the
    // egos still in the loop; rank(alist) (the convoys' ordering; a no-op elsewhere); for the i-th listed ego b,
    // sense(step, b, xs, obs) fills the state xs [5] and the slab obs [ow][2] the solver receives and returns
    // n_obs; one batched solve over the list (with the slab when with_obs, p.max_obs == ow); then
    // plant(step, b, u0, status) per listed ego.  The step times go to E.ms and the optional E.step_ms.
    // planned: the solver is also asked for its U and Xpred, and after the plant steps trace(step, b, U, Xpred)
    // runs per listed ego.  carried: before the solve carry(step, b, xs, obs, n_obs, ubar) fills the listed ego's
    // row of the ubar [N][2] the solver is handed, the solver is asked for its U, and after the plant steps (and
    // trace) keep(step, b, U, ubar, status, n_obs) runs per listed ego
    template <typename Rank, typename Sense, typename Plant>
    void run_loop(const mpc_params& p, LoopEgos& E, int max_steps, bool with_obs, size_t ow, Rank rank, Sense sense,
                  Plant plant) const {
        run_loop(p, E, max_steps, with_obs, ow, rank, sense, plant, false, [](int, int, const double*, const double*) {});
    }
    template <typename Rank, typename Sense, typename Plant, typename Trace>
    void run_loop(const mpc_params& p, LoopEgos& E, int max_steps, bool with_obs, size_t ow, Rank rank, Sense sense,
                  Plant plant, bool planned, Trace trace) const {
        run_loop(p, E, max_steps, with_obs, ow, rank, sense, plant, planned, trace, false,
                 [](int, int, const double*, const double*, int, double*) {},
                 [](int, int, const double*, const double*, int, int) {});
    }
    template <typename Rank, typename Sense, typename Plant, typename Trace, typename Carry, typename Keep>
    void run_loop(const mpc_params& p, LoopEgos& E, int max_steps, bool with_obs, size_t ow, Rank rank, Sense sense,
                  Plant plant, bool planned, Trace trace, bool carried, Carry carry, Keep keep) const {
        std::vector<int> alist, nobsa, sta;
        std::vector<double> xa, obsa, u0a, Ua, Xpa, ubara;
        const size_t nu = 2 * (size_t)p.N, nxp = 5 * ((size_t)p.N + 1);
        for (int step = 0; step < max_steps; ++step) {
            const auto t0 = std::chrono::steady_clock::now();
            alist.clear();
            for (int b = 0; b < E.B; ++b)
                if (E.active[b]) alist.push_back(b);
            if (alist.empty()) break;
            const int nl = (int)alist.size();
            rank(alist);
            xa.assign((size_t)nl * 5, 0.0);
            obsa.assign((size_t)nl * ow * 2, 0.0);
            nobsa.assign(nl, 0);
            u0a.assign((size_t)nl * 2, 0.0);
            sta.assign(nl, 0);
            for (int i = 0; i < nl; ++i)
                nobsa[i] = sense(step, alist[i], xa.data() + 5 * (size_t)i, obsa.data() + (size_t)i * ow * 2);
            if (planned || carried) Ua.assign((size_t)nl * nu, 0.0);
            if (planned) Xpa.assign((size_t)nl * nxp, 0.0);
            if (carried) {
                ubara.assign((size_t)nl * nu, 0.0);
                for (int i = 0; i < nl; ++i)
                    carry(step, alist[i], xa.data() + 5 * (size_t)i, obsa.data() + (size_t)i * ow * 2,
                          with_obs ? nobsa[i] : 0, ubara.data() + (size_t)i * nu);
            }
            solve_batch(p, nl, xa.data(), with_obs ? obsa.data() : nullptr, with_obs ? nobsa.data() : nullptr,
                        carried ? ubara.data() : nullptr, u0a.data(), planned || carried ? Ua.data() : nullptr,
                        planned ? Xpa.data() : nullptr, sta.data(), nullptr);
            for (int i = 0; i < nl; ++i) plant(step, alist[i], u0a.data() + 2 * (size_t)i, sta[i]);
            if (planned)
                for (int i = 0; i < nl; ++i) trace(step, alist[i], Ua.data() + (size_t)i * nu, Xpa.data() + (size_t)i * nxp);
            if (carried)
                for (int i = 0; i < nl; ++i)
                    keep(step, alist[i], Ua.data() + (size_t)i * nu, ubara.data() + (size_t)i * nu, sta[i],
                         with_obs ? nobsa[i] : 0);
            E.ms.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
            if (E.step_ms) E.step_ms[step] = E.ms.back();
        }
    }

    // run_simulation (trajectory_tracking.py:377-443) for B egos: mpc_closed_loop on the host is the sweep below
    // with one scenario, every ego's history kept ([B] rows) and the quantities dropped
    int closed_loop(const mpc_params& p0, int B, const double* x_init, const mpc_fsm& F, bool with_fsm,
                    int max_steps, double s_stop, double* hist_x, double* hist_u, double* hist_obs_s,
                    int* hist_tl, int* hist_status, int* n_steps, double* step_ms) const {
        std::vector<int> slot((size_t)B);
        for (int b = 0; b < B; ++b) slot[b] = b;
        std::vector<double> quant((size_t)B * MPC_CL_NQ);
        return closed_loop_sweep(p0, B, x_init, &F, 1, with_fsm, max_steps, s_stop, quant.data(), B, slot.data(),
                                 hist_x, hist_u, hist_obs_s, hist_tl, hist_status, n_steps, step_ms);
    }

    // mpc_closed_loop_sweep on the host: per step the ObstaclesFSM of every ego in the loop with ego b's scenario
    // fsm[n_fsm == 1 ? 0 : b], one batched solve over them, the Euler plant step; the check quantities
    // (include/mpcqp.h, MPC_CLQ_*) accumulate while the loop runs.  n_steps is optional
    int closed_loop_sweep(const mpc_params& p0, int B, const double* x_init, const mpc_fsm* fsm, int n_fsm,
                          bool with_fsm, int max_steps, double s_stop, double* quant, int n_hist, const int* slot,
                          double* hist_x, double* hist_u, double* hist_obs_s, int* hist_tl, int* hist_status,
                          int* n_steps, double* step_ms) const {
        mpc_params p = p0;
        p.max_obs = with_fsm ? 2 : 0;
        const size_t nb = (size_t)B, ns = (size_t)max_steps, nh = (size_t)n_hist;
        hist_prefill(hist_obs_s, nh * ns, (double)NAN);
        hist_prefill(hist_tl, nh * ns, -1);
        LoopEgos E(B, x_init, max_steps, s_stop, quant, n_hist, slot, hist_x, hist_u, hist_status, step_ms);
        std::vector<double> car(nb), timer(nb, 0.0);
        std::vector<int> flags(nb * 4, 0);
        for (int b = 0; b < B; ++b) car[b] = fsm[n_fsm == 1 ? 0 : b].obs_start_s;
        run_loop(p, E, max_steps, with_fsm, 2, [](const std::vector<int>&) {},
                 [&](int step, int b, double* xs, double* o) {
                     const mpc_fsm& F = fsm[n_fsm == 1 ? 0 : b];
                     const double s = E.x[5 * (size_t)b], v = E.x[5 * (size_t)b + 4];
                     int* fl = flags.data() + 4 * (size_t)b;
                     double* q = quant + (size_t)b * MPC_CL_NQ;
                     double car_s;
                     const int n = fsm_step(F, p.dt, s, v, fl, car[b], timer[b], o, car_s);
                     std::memcpy(xs, E.x.data() + 5 * (size_t)b, 5 * sizeof(double));
                     if (car_s == car_s) min_gap(q[MPC_CLQ_MIN_OBS_DIST], E.qflags[b], car_s - s);
                     red_pass_step(F, s, fl[2], q, E.qflags[b]);
                     if (slot[b] >= 0) {
                         if (hist_obs_s) hist_obs_s[(size_t)slot[b] * ns + step] = car_s;
                         if (hist_tl) hist_tl[(size_t)slot[b] * ns + step] = fl[2];
                     }
                     return n;
                 },
                 [&](int step, int b, const double* u, int status) {
                     E.plant(ref, p.dt, b, step, u, u, status, [](double*) {});
                 });
        E.finish(n_steps);
        return MPC_SUCCESS;
    }

    // The five scripted entries on the host: the request `a` (scripted_loop.h) as the entry filled it, slot[b] the
    // history row of ego b or -1.  Ego b runs the script a.script(b) (script_step); the slab takes what its actors
    // emit, then (s, v) of its leaders, n_obs entries of A + K.  with_slab: the solver runs with max_obs = A + K.
    //   worlds (K > 0): per step every world's egos [w*W, (w+1)*W) still in the loop are sorted by the ahead-of
    //     order (the larger s first, on equal s the lower index) on the states before the step; an ego's leaders
    //     are its predecessors in that order, nearest first, at most K, cut at the first gap >= lead_range.
    //   noise (the sigmas a.noise_of(b); ego b draws as global ego ego_offset + b): the FSMs, the
    //     leader ranking, the gap quantities, hist_slab and the exit test use the true states; the solver receives
    //     x + meas_sigma * z and a perturbed copy of the slab; the plant integrates the clamped u + act_sigma * z
    //     and adds (dt * proc_sigma) * z.
    //   traces (n_look > 0, hist_pred or hist_plan): the solver's U and Xpred of every step are kept; after the
    //     plant step every ego stores stage j of its prediction in its ring for lookahead j and compares its new true
    //     state with the prediction made j - 1 steps before (loop_steps.h, trace_gap); gapq is
    //     [B][n_look][MPC_TG_NQ], hist_pred [n_hist][max_steps][N+1][5], hist_plan [n_hist][max_steps][N][2].
    //   warm starts (warm != NULL): the solver is handed an explicit ubar, the reference warm start restated or the
    //     ego's kept plan shifted by one stage (loop_steps.h, warm_reset and warm_source); after the plant step the
    //     solver's U, its status and the step's n_obs are kept and the move from ubar enters warmq
    //     [B][MPC_WQ_NQ]; hist_ubar is [n_hist][max_steps][N][2].
    // extra is [B][nx] (MPC_TR_NX; MPC_CV_NX with worlds; MPC_NZ_NX with noise); extra, n_steps, step_ms and every
    // history are optional; hist_slab is [n_hist][max_steps][A+K][2], hist_lead [n_hist][max_steps][K]
    int closed_loop_scripted(const mpc_params& p0, const ScriptedLoop& a, const int* slot) const {
        const int B = a.B, W = a.W, K = a.K, A = a.A, nx = a.nx();
        mpc_params p = p0;
        const int AK = A + K;
        p.max_obs = a.with_slab ? AK : 0;
        const size_t nb = (size_t)B, ns = (size_t)a.max_steps, nh = (size_t)a.n_hist, na = (size_t)A, nk = (size_t)K;
        const size_t nak = (size_t)AK, nxs = (size_t)nx;
        hist_prefill(a.hist_ua, nh * ns * 2, (double)NAN);
        hist_prefill(a.hist_xm, nh * ns * 5, (double)NAN);
        hist_prefill(a.hist_car_s, nh * ns, (double)NAN);
        hist_prefill(a.hist_tl, nh * ns, -1);
        hist_prefill(a.hist_nobs, nh * ns, -1);
        hist_prefill(a.hist_slab, nh * ns * nak * 2, (double)NAN);
        hist_prefill(a.hist_lead, nh * ns * nk, -1);
        const size_t nu = 2 * (size_t)p.N, nxp = 5 * ((size_t)p.N + 1);
        hist_prefill(a.hist_pred, nh * ns * nxp, (double)NAN);
        hist_prefill(a.hist_plan, nh * ns * nu, (double)NAN);
        hist_prefill(a.hist_ubar, nh * ns * nu, (double)NAN);
        // the kept plan [N][2], status (-1: none yet) and n_obs of every ego, and its warm row
        std::vector<double> kplan(a.warm ? nb * nu : 0, 0.0), wq(a.warm ? nb * MPC_WQ_NQ : 0);
        std::vector<int> kstatus(a.warm ? nb : 0, -1), knobs(a.warm ? nb : 0, 0);
        for (size_t b = 0; a.warm && b < nb; ++b) warm_init(wq.data() + b * MPC_WQ_NQ);
        size_t slots = 0;                                 // ring slots of one ego, lookahead i's from ring0[i] on
        size_t ring0[MPC_MAX_LOOK] = {};
        for (int i = 0; i < a.n_look; ++i) {
            ring0[i] = slots;
            slots += (size_t)a.lookahead[i];
        }
        std::vector<double> ring(nb * slots * 3, 0.0);
        for (size_t k = 0; k < nb * (size_t)a.n_look; ++k) trace_init(a.gapq + k * MPC_TG_NQ);
        LoopEgos E(B, a.x_init, a.max_steps, a.s_stop, a.quant, a.n_hist, slot, a.hist_x, a.hist_u, a.hist_status,
                   a.step_ms);
        std::vector<double> aval(nb * na, 0.0), ex(nb * nxs, 0.0);
        std::vector<int> aflags(nb * na, 0);
        std::vector<int> order(nb), rank(nb, -1), wbeg((size_t)(B / W) + 1, 0);
        for (int b = 0; b < B; ++b) {
            const mpc_actor* sc = a.script(b);
            for (int a = 0; a < A; ++a)
                if (sc[a].kind == MPC_ACTOR_CAR) aval[(size_t)b * na + a] = sc[a].pos_s;
            double* e = ex.data() + (size_t)b * nxs;
            e[MPC_TRX_MIN_GAP_ACTOR] = -1.0;
            if (nx >= MPC_CV_NX) {
                e[MPC_CVX_MIN_LEAD_GAP] = NAN;
                e[MPC_CVX_MIN_LEAD_EGO] = -1.0;
            }
        }
        run_loop(p, E, a.max_steps, a.with_slab, nak,
                 [&](const std::vector<int>& alist) {
                     if (K == 0) return;
                     // alist is increasing, so each world's egos in the loop are one run of it: sort the run, and
                     // order[rank[b] - 1], order[rank[b] - 2], .. down to the run's start are ego b's leaders
                     const int nl = (int)alist.size();
                     order = alist;
                     for (int i = 0, w = 0; w <= B / W; ++w) {
                         while (i < nl && alist[i] < w * W) ++i;
                         wbeg[w] = i;
                     }
                     for (int w = 0; w < B / W; ++w)
                         std::sort(order.begin() + wbeg[w], order.begin() + wbeg[w + 1], [&](int a, int b) {
                             const double sa = E.x[5 * (size_t)a], sb = E.x[5 * (size_t)b];
                             return sa > sb || (sa == sb && a < b);
                         });
                     for (int i = 0; i < nl; ++i) rank[order[i]] = i;
                 },
                 [&](int step, int b, double* xm, double* oa) {
                     const mpc_noise& Z = a.noise_of(b);
                     const NoiseAt at = {(unsigned)a.seed, (unsigned)(a.seed >> 32),
                                         (unsigned long long)a.ego_offset + (unsigned long long)b, step};
                     const double s = E.x[5 * (size_t)b], v = E.x[5 * (size_t)b + 4];
                     double o[2 * MPC_MAX_ACTORS];            // the true slab of this step
                     double* q = a.quant + (size_t)b * MPC_CL_NQ;
                     double* e = ex.data() + (size_t)b * nxs;
                     int green;
                     double car_s;
                     int n = script_step(a.script(b), A, p.dt, s, v, aflags.data() + (size_t)b * na,
                                         aval.data() + (size_t)b * na, o, q, e, E.qflags[b], green, car_s);
                     if (K > 0) {                             // the leaders, nearest first
                         int* hlead =
                             a.hist_lead && slot[b] >= 0 ? a.hist_lead + ((size_t)slot[b] * ns + step) * nk : nullptr;
                         const int r = rank[b], r0 = wbeg[b / W];
                         int nlead = 0;
                         for (; nlead < K && r - 1 - nlead >= r0; ++nlead) {
                             const int j = order[r - 1 - nlead];
                             const double sj = E.x[5 * (size_t)j], gap = sj - s;
                             if (gap >= a.lead_range) break;
                             o[2 * n] = sj;
                             o[2 * n + 1] = E.x[5 * (size_t)j + 4];
                             ++n;
                             if (hlead) hlead[nlead] = j;
                             if (min_gap(q[MPC_CLQ_MIN_OBS_DIST], E.qflags[b], gap))   // a leader is a car
                                 e[MPC_TRX_MIN_GAP_ACTOR] = -1.0;
                             int lf = e[MPC_CVX_MIN_LEAD_EGO] >= 0.0;     // bit 0: a leader gap was recorded
                             if (min_gap(e[MPC_CVX_MIN_LEAD_GAP], lf, gap)) e[MPC_CVX_MIN_LEAD_EGO] = (double)j;
                         }
                         if ((double)nlead > e[MPC_CVX_MAX_LEADERS]) e[MPC_CVX_MAX_LEADERS] = (double)nlead;
                     }
                     if ((double)n > e[MPC_TRX_MAX_NOBS]) e[MPC_TRX_MAX_NOBS] = (double)n;
                     // what the solver receives: the measured state and the perceived slab
                     for (int j = 0; j < 5; ++j)
                         xm[j] = noise_add(E.x[5 * (size_t)b + j], Z.meas_sigma[j], at, MPC_NZ_CH_MEAS + j);
                     for (int j = 0; j < 2 * n; ++j)          // entry j / 2: s on the even channel, v on the odd
                         oa[j] = noise_add(o[j], Z.perc_sigma[j & 1], at, MPC_NZ_CH_PERC + j);
                     if (slot[b] >= 0) {
                         const size_t h = (size_t)slot[b] * ns + step;
                         if (a.hist_car_s) a.hist_car_s[h] = car_s;
                         if (a.hist_tl) a.hist_tl[h] = green;
                         if (a.hist_nobs) a.hist_nobs[h] = n;
                         if (a.hist_slab && n)
                             std::memcpy(a.hist_slab + h * nak * 2, o, (size_t)n * 2 * sizeof(double));
                         if (a.hist_xm) std::memcpy(a.hist_xm + h * 5, xm, 5 * sizeof(double));
                     }
                     return n;
                 },
                 [&](int step, int b, const double* u, int status) {
                     const mpc_noise& Z = a.noise_of(b);
                     const NoiseAt at = {(unsigned)a.seed, (unsigned)(a.seed >> 32),
                                         (unsigned long long)a.ego_offset + (unsigned long long)b, step};
                     double ua[2];                            // the applied control
                     bool clamped = false;
                     for (int k = 0; k < 2; ++k)
                         ua[k] = apply_actuation(u[k], Z.act_sigma[k], at, MPC_NZ_CH_ACT + k, p.u_min[k], p.u_max[k],
                                                 clamped);
                     E.plant(ref, p.dt, b, step, u, ua, status, [&](double* xb) {
                         for (int j = 0; j < 5; ++j)
                             xb[j] = noise_add(xb[j], Z.proc_sigma[j], at, MPC_NZ_CH_PROC + j, p.dt);
                     });
                     if (nx < MPC_NZ_NX) return;
                     double* e = ex.data() + (size_t)b * nxs;
                     if (slot[b] >= 0 && a.hist_ua)
                         std::memcpy(a.hist_ua + ((size_t)slot[b] * ns + step) * 2, ua, sizeof(ua));
                     extremes4(e, MPC_NZX_U1A_MIN, step, ua[0], ua[1]);
                     if (clamped) e[MPC_NZX_N_CLAMPED] += 1.0;
                 },
                 a.traced(),
                 [&](int step, int b, const double* U, const double* Xp) {
                     const double* x = E.x.data() + 5 * (size_t)b;       // the true state after the step
                     for (int i = 0; i < a.n_look; ++i) {
                         const int j = a.lookahead[i];
                         double* rg = ring.data() + ((size_t)b * slots + ring0[i]) * 3;
                         double* w = rg + 3 * (size_t)trace_slot(step, j);
                         w[0] = Xp[5 * j];
                         w[1] = Xp[5 * j + 1];
                         w[2] = Xp[5 * j + 4];
                         if (!trace_pair(step, j)) continue;
                         const int t0 = step + 1 - j;                    // j == 1: the slot just written
                         const double* r = rg + 3 * (size_t)trace_slot(t0, j);
                         trace_gap(a.gapq + ((size_t)b * a.n_look + i) * MPC_TG_NQ, t0, r[0], r[1], r[2], x[0], x[1],
                                   x[4]);
                     }
                     if (slot[b] < 0) return;
                     const size_t h = (size_t)slot[b] * ns + step;
                     if (a.hist_pred) std::memcpy(a.hist_pred + h * nxp, Xp, nxp * sizeof(double));
                     if (a.hist_plan) std::memcpy(a.hist_plan + h * nu, U, nu * sizeof(double));
                 },
                 a.warm != nullptr,
                 [&](int step, int b, const double* xm, const double* oa, int nobs, double* ub) {
                     const int N = p.N;
                     const double* kp = kplan.data() + (size_t)b * nu;
                     bool finite = true;
                     if (kstatus[b] >= 0 && a.warm->mode == MPC_WARM_CARRY)
                         for (size_t e = 0; e < nu; ++e) finite = finite && warm_finite(kp[e]);
                     const bool reset = warm_reset(*a.warm, kstatus[b], finite, knobs[b], nobs);
                     const bool walk = reset || a.warm->tail == MPC_WTAIL_REFERENCE;
                     WarmRef w = warm_ref_begin(xm);
                     for (int k = 0; k < N; ++k) {
                         const int src = reset ? -1 : warm_source(k, N, a.warm->tail);
                         if (walk) warm_ref_advance(w, k, p.dt, oa, nobs, p.brake_distance);
                         if (src < 0) {
                             warm_ref_control(w, p.brake_accel, [&](double s, double* ur) { get_control(ref, s, ur); },
                                              ub[2 * k], ub[2 * k + 1]);
                         } else {
                             ub[2 * k] = clamp_control(kp[2 * src], p.u_min[0], p.u_max[0]);
                             ub[2 * k + 1] = clamp_control(kp[2 * src + 1], p.u_min[1], p.u_max[1]);
                         }
                     }
                     if (reset) wq[(size_t)b * MPC_WQ_NQ + MPC_WQ_N_RESET] += 1.0;
                     if (a.hist_ubar && slot[b] >= 0)
                         std::memcpy(a.hist_ubar + ((size_t)slot[b] * ns + step) * nu, ub, nu * sizeof(double));
                 },
                 [&](int step, int b, const double* U, const double* ub, int status, int nobs) {
                     double move = 0.0;
                     for (size_t e = 0; e < nu; ++e) warm_move_element(move, U[e], ub[e]);
                     std::memcpy(kplan.data() + (size_t)b * nu, U, nu * sizeof(double));
                     kstatus[b] = status;
                     knobs[b] = nobs;
                     warm_move(wq.data() + (size_t)b * MPC_WQ_NQ, step, move);
                 });
        E.finish(a.n_steps);
        if (a.warmq) std::memcpy(a.warmq, wq.data(), nb * MPC_WQ_NQ * sizeof(double));
        if (a.extra) std::memcpy(a.extra, ex.data(), nb * nxs * sizeof(double));
        return MPC_SUCCESS;
    }

};

// MPC_CLQ_MAX_STEP_MS of every ego: the prefix max of the step times over the steps it ran, max(ms[:n]) with
// numpy's NaN rule, 0 for an ego that never ran (shared by the device path of mpc_closed_loop_sweep)
inline void sweep_max_step_ms(int B, const int* n_steps, const std::vector<double>& ms, double* quant) {
    std::vector<double> pm(ms.size() + 1, 0.0);
    for (size_t i = 0; i < ms.size(); ++i)
        pm[i + 1] = (i == 0 || ms[i] > pm[i] || ms[i] != ms[i]) ? ms[i] : pm[i];
    for (int b = 0; b < B; ++b) {
        const size_t n = std::min((size_t)std::max(n_steps[b], 0), ms.size());
        quant[(size_t)b * MPC_CL_NQ + MPC_CLQ_MAX_STEP_MS] = pm[n];
    }
}

// mpc_cl_verdicts: sanity_checks.check_verdicts row by row on quant [B][MPC_CL_NQ] (each test negated like
// there, so a NaN passes the same way); the control bounds are p's.  verdicts and counts may be null
inline void cl_verdicts(const mpc_params& p, int B, const double* quant, double s_total, int* verdicts,
                        int* counts) {
    if (counts)
        for (int k = 0; k < 8; ++k) counts[k] = 0;
    const double* lo = p.u_min;
    const double* hi = p.u_max;
    for (int b = 0; b < B; ++b) {
        const double* q = quant + (size_t)b * MPC_CL_NQ;
        int v = 0;
        if (!(q[MPC_CLQ_S_FINAL] < s_total - MPC_CL_DEST_TOL)) v |= MPC_CLV_DESTINATION;
        if (!(q[MPC_CLQ_MAX_DEV] > MPC_CL_LATERAL_LIMIT)) v |= MPC_CLV_ON_ROAD;
        if (!(q[MPC_CLQ_U1_MIN] < lo[0] - MPC_CL_CONTROLS_TOL || q[MPC_CLQ_U1_MAX] > hi[0] + MPC_CL_CONTROLS_TOL))
            v |= MPC_CLV_STEER_OK;
        if (!(q[MPC_CLQ_U2_MIN] < lo[1] - MPC_CL_CONTROLS_TOL || q[MPC_CLQ_U2_MAX] > hi[1] + MPC_CL_CONTROLS_TOL))
            v |= MPC_CLV_ACCEL_OK;
        if (!(q[MPC_CLQ_MAX_STEP_MS] > MPC_CL_STEP_MS_LIMIT)) v |= MPC_CLV_REALTIME;
        const double gap = q[MPC_CLQ_MIN_OBS_DIST];
        if (gap != gap || !(gap < MPC_CL_SAFETY_DIST)) v |= MPC_CLV_OBSTACLE_OK;
        if (q[MPC_CLQ_RED_PASS] == 0.0) v |= MPC_CLV_LIGHT_OK;
        if (v == MPC_CLV_PASSED - 1) v |= MPC_CLV_PASSED;
        if (verdicts) verdicts[b] = v;
        if (counts)
            for (int k = 0; k < 8; ++k) counts[k] += (v >> k) & 1;
    }
}

}  // namespace mpcqp_cpu

#endif  // MPCQP_CPU_BACKEND_H
