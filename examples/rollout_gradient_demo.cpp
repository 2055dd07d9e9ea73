// The gradient of a closed-loop cost with respect to the initial state, from host C++ (no torch): the linear MPC of warm_shift_demo.cpp
// (two double integrators, nx = 4 states, nu = 2 inputs, horizon N, 1-norm stage costs, a box on u; theta = x_0 enters b, u = u_0, the
// plant theta+ = A theta + B u + w), run as a closed loop of T steps per instance, every step solved cold.  The cost is
//     L = 1/2 sum_{t=0..T} |theta_t|^2 + rho/2 sum_{t<T} |u_t|^2,    so    dL/du_t = rho u_t,   dL/dtheta_t = theta_t,
// and dL/dtheta_0 comes from rolloutJacobian (the rollout that also records J_t = du_t / dtheta_t, one launch) followed by
// rolloutGradient (the backward sweep through theta_{t+1} = A theta_t + B u_t, one small kernel).  Printed, each the median of 5 (the
// kernels between HIP events on the handle's stream, and the wall clock of the calls):
//   (a) rollout                                  the simulation alone
//   (b) rolloutJacobian + rolloutGradient        the simulation with its gradient
//   (c) T x (stepParam + paramJacobian)          the host loop that gives the same Jacobians, then the same backward sweep on the host
//   (d) central differences: 2 k rollouts at eps = 1e-4, with max and median |grad - grad_fd| over the instances whose steps all ended
//       optimal on every run, and how many instances lie within 1e-3 of their own largest finite-difference entry.  The stage costs
//       are 1-norms, so u(theta) is piecewise affine: where a step of an instance has a change of the active set within eps of its
//       theta, a central difference across the kink is not the derivative, and at a degenerate optimum the adjoint value is a smoothed
//       one (eicos_amd.h) -- the median is the figure that describes the agreement, the maximum the worst such instance.
//   g++ -std=c++17 -Iinclude examples/rollout_gradient_demo.cpp -Leicos_amd -leicos_amd -Wl,-rpath,$PWD/eicos_amd -o rollout_gradient_demo
//   ./rollout_gradient_demo [batch = 1024] [N = 20] [T = 20]
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <tuple>
#include <vector>

#include "eicos.hpp"

namespace {
constexpr int NX = 4, NU = 2;
constexpr double DT = 0.5, RHO = 0.1, UMAX = 1.0;
const double Ad[NX][NX] = {{1, DT, 0, 0}, {0, 1, 0, 0}, {0, 0, 1, DT}, {0, 0, 0, 1}};
const double Bd[NX][NU] = {{DT * DT / 2, 0}, {DT, 0}, {0, DT * DT / 2}, {0, DT}};

struct Csc { // a sparse matrix from (row, column, value) triplets, columns sorted, rows sorted inside a column
    std::vector<int> jc, ir;
    std::vector<double> pr;
    Csc(int ncols, std::vector<std::tuple<int, int, double>> t) {
        std::sort(t.begin(), t.end(), [](const auto &a, const auto &b) { return std::get<1>(a) != std::get<1>(b) ? std::get<1>(a) < std::get<1>(b) : std::get<0>(a) < std::get<0>(b); });
        jc.assign(ncols + 1, 0);
        for (const auto &e : t) { jc[std::get<1>(e) + 1]++; ir.push_back(std::get<0>(e)); pr.push_back(std::get<2>(e)); }
        for (int j = 0; j < ncols; j++) jc[j + 1] += jc[j];
    }
};

struct Affine { // base vector + CSR matrix, as eicos_affine_map reads them
    std::vector<double> base, val;
    std::vector<int> rowptr, col;
    eicos_affine_map view() const { return {base.data(), rowptr.data(), col.data(), val.data()}; }
    void row_done() { rowptr.push_back((int)col.size()); }
    explicit Affine(int rows) : base(rows, 0.), rowptr(1, 0) {}
};

} // namespace

int main(int argc, char **argv) {
    const int B = argc > 1 ? std::atoi(argv[1]) : 1024, N = argc > 2 ? std::atoi(argv[2]) : 20, T = argc > 3 ? std::atoi(argv[3]) : 20;
    if (B < 1 || N < 2 || T < 1) { std::fprintf(stderr, "usage: rollout_gradient_demo [batch] [N >= 2] [T >= 1]\n"); return 2; }
    // ---- the problem, stage by stage
    const int S = 2 * NX + 2 * NU, MS = 2 * NX + 4 * NU, n = N * S, m = N * MS, p = N * NX;
    std::vector<std::tuple<int, int, double>> tg, ta;
    std::vector<double> c(n, 0.), h(m, 0.), b(p, 0.);
    for (int t = 0; t < N; t++) {
        const int u0 = t * S, x1 = u0 + NU, e0 = x1 + NX, f0 = e0 + NX, g0 = t * MS, a0 = t * NX;
        for (int i = 0; i < NX; i++) {
            c[e0 + i] = 1.;
            tg.push_back({g0 + 2 * i, x1 + i, 1.}); tg.push_back({g0 + 2 * i, e0 + i, -1.});
            tg.push_back({g0 + 2 * i + 1, x1 + i, -1.}); tg.push_back({g0 + 2 * i + 1, e0 + i, -1.});
            ta.push_back({a0 + i, x1 + i, 1.});
            for (int j = 0; j < NX; j++) if (t > 0 && Ad[i][j] != 0.) ta.push_back({a0 + i, x1 - S + j, -Ad[i][j]});
            for (int j = 0; j < NU; j++) if (Bd[i][j] != 0.) ta.push_back({a0 + i, u0 + j, -Bd[i][j]});
        }
        for (int i = 0; i < NU; i++) {
            c[f0 + i] = RHO;
            const int r = g0 + 2 * NX + 4 * i;
            tg.push_back({r, u0 + i, 1.}); tg.push_back({r, f0 + i, -1.});
            tg.push_back({r + 1, u0 + i, -1.}); tg.push_back({r + 1, f0 + i, -1.});
            tg.push_back({r + 2, u0 + i, 1.}); h[r + 2] = UMAX;
            tg.push_back({r + 3, u0 + i, -1.}); h[r + 3] = UMAX;
        }
    }
    const Csc G(n, tg), A(n, ta);
    // ---- the maps: theta = x_0 enters b of stage 0 as A theta; u = u_0; theta+ = A theta + B u (+ w)
    Affine bmap(p), omap(NU), plant(NX);
    for (int i = 0; i < p; i++) {
        if (i < NX) for (int j = 0; j < NX; j++) if (Ad[i][j] != 0.) { bmap.col.push_back(j); bmap.val.push_back(Ad[i][j]); }
        bmap.row_done();
    }
    for (int i = 0; i < NU; i++) { omap.col.push_back(i); omap.val.push_back(1.); omap.row_done(); }
    for (int i = 0; i < NX; i++) {
        for (int j = 0; j < NX; j++) if (Ad[i][j] != 0.) { plant.col.push_back(j); plant.val.push_back(Ad[i][j]); }
        for (int j = 0; j < NU; j++) if (Bd[i][j] != 0.) { plant.col.push_back(NX + j); plant.val.push_back(Bd[i][j]); }
        plant.row_done();
    }
    const eicos_affine_map vb = bmap.view(), vo = omap.view(), vf = plant.view();
    // ---- the batch: the same model, different measured states and disturbances
    unsigned long long st = 88172645463325252ull;
    auto rnd = [&] { st = st * 6364136223846793005ull + 1442695040888963407ull; return (double)((st >> 11) & 0xFFFFFFFFFFFFull) / (double)(1ull << 48); };
    std::vector<double> theta0((size_t)B * NX), w((size_t)B * T * NX);
    for (int i = 0; i < B; i++)
        for (int j = 0; j < NX; j++) theta0[(size_t)i * NX + j] = (j % 2 == 0 ? 2.0 : 0.5) * (2 * rnd() - 1);
    for (double &v : w) v = 0.01 * (2 * rnd() - 1);
    auto rep = [&](const std::vector<double> &row) { std::vector<double> out; out.reserve(row.size() * B); for (int i = 0; i < B; i++) out.insert(out.end(), row.begin(), row.end()); return out; };
    const std::vector<double> Gb = rep(G.pr), Ab = rep(A.pr), cb = rep(c), hb = rep(h), bb = rep(b);

    auto median = [](std::vector<double> v) { std::sort(v.begin(), v.end()); return v[v.size() / 2]; };
    auto now = [] { return std::chrono::steady_clock::now(); };
    auto since = [](std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); };
    const size_t nU = (size_t)B * T * NU, nTh = (size_t)B * (T + 1) * NX, nJ = (size_t)B * T * NU * NX;
    try {
        EiCOS::BatchSolver solver(n, m, p, 0, nullptr, G.jc.data(), G.ir.data(), A.jc.data(), A.ir.data(), B, std::vector<int>{0});
        solver.updateData(Gb.data(), Ab.data(), cb.data(), hb.data(), bb.data());
        solver.setParamMap(NX, nullptr, nullptr, &vb);
        solver.setOutputMap(NU, &vo);
        solver.setPlantMap(&vf);
        eicos_batch *h = solver.handle();
        auto kernel_ms = [&](bool adjoint) { float ms = 0.f; if (adjoint) eicos_batch_last_adjoint_ms(h, &ms); else eicos_batch_last_solve_ms(h, &ms); return (double)ms; };
        auto cost = [&](const std::vector<double> &u, const std::vector<double> &th, int i) {
            double L = 0.;
            for (int t = 0; t <= T; t++) for (int j = 0; j < NX; j++) { const double v = th[((size_t)i * (T + 1) + t) * NX + j]; L += 0.5 * v * v; }
            for (int t = 0; t < T; t++) for (int j = 0; j < NU; j++) { const double v = u[((size_t)i * T + t) * NU + j]; L += 0.5 * RHO * v * v; }
            return L;
        };
        std::vector<double> u(nU), th(nTh), J(nJ), gu(nU), grad((size_t)B * NX), ka, wa, kb, wb, kc, wc;
        std::vector<EiCOS::exitcode> codes;
        // (a) the rollout alone
        for (int q = 0; q < 5; q++) {
            const auto t0 = now();
            solver.rollout(T, theta0.data(), u.data(), w.data(), th.data());
            wa.push_back(since(t0)); ka.push_back(kernel_ms(false));
        }
        // (b) the rollout with its Jacobians, and the backward sweep
        for (int q = 0; q < 5; q++) {
            const auto t0 = now();
            codes = solver.rolloutJacobian(T, theta0.data(), u.data(), J.data(), w.data(), th.data());
            double k_ms = kernel_ms(false);
            for (size_t e = 0; e < nU; e++) gu[e] = RHO * u[e];
            solver.rolloutGradient(gu.data(), th.data(), grad.data());
            wb.push_back(since(t0)); kb.push_back(k_ms + kernel_ms(true));
        }
        const int launches = eicos_batch_last_rollout_launches(h);
        std::vector<int> optimal(B, 1);
        for (int i = 0; i < B; i++) for (int t = 0; t < T; t++) if ((int)codes[(size_t)i * T + t] != EICOS_OPTIMAL) optimal[i] = 0;
        // (c) the host loop: T x (stepParam + paramJacobian), the plant and the backward sweep on the host
        std::vector<double> grad_host((size_t)B * NX), u1((size_t)B * NU), J1((size_t)B * NU * NX), thc, Jh(nJ), uh(nU), thh(nTh);
        for (int q = 0; q < 5; q++) {
            const auto t0 = now();
            double k_ms = 0.;
            thc = theta0;
            for (int i = 0; i < B; i++) for (int j = 0; j < NX; j++) thh[(size_t)i * (T + 1) * NX + j] = theta0[(size_t)i * NX + j];
            for (int t = 0; t < T; t++) {
                solver.stepParam(thc.data(), u1.data()); k_ms += kernel_ms(false);
                solver.paramJacobian(J1.data()); k_ms += kernel_ms(true);
                for (int i = 0; i < B; i++) {
                    double nx[NX];
                    for (int a = 0; a < NX; a++) {
                        double acc = 0.;
                        for (int j = 0; j < NX; j++) if (Ad[a][j] != 0.) acc = acc + Ad[a][j] * thc[(size_t)i * NX + j];
                        for (int j = 0; j < NU; j++) if (Bd[a][j] != 0.) acc = acc + Bd[a][j] * u1[(size_t)i * NU + j];
                        nx[a] = acc + w[((size_t)i * T + t) * NX + a];
                    }
                    for (int a = 0; a < NX; a++) { thc[(size_t)i * NX + a] = nx[a]; thh[((size_t)i * (T + 1) + t + 1) * NX + a] = nx[a]; }
                    for (int j = 0; j < NU; j++) uh[((size_t)i * T + t) * NU + j] = u1[(size_t)i * NU + j];
                    for (int e = 0; e < NU * NX; e++) Jh[((size_t)i * T + t) * NU * NX + e] = J1[(size_t)i * NU * NX + e];
                }
            }
            for (int i = 0; i < B; i++) { // lambda_t = theta_t + J_t' mu + A' lambda_{t+1},  mu = rho u_t + B' lambda_{t+1}
                double lam[NX];
                for (int j = 0; j < NX; j++) lam[j] = thh[((size_t)i * (T + 1) + T) * NX + j];
                for (int t = T - 1; t >= 0; t--) {
                    double mu[NU], nl[NX];
                    for (int j = 0; j < NU; j++) { mu[j] = RHO * uh[((size_t)i * T + t) * NU + j]; for (int a = 0; a < NX; a++) mu[j] += Bd[a][j] * lam[a]; }
                    for (int c2 = 0; c2 < NX; c2++) {
                        nl[c2] = thh[((size_t)i * (T + 1) + t) * NX + c2];
                        for (int a = 0; a < NX; a++) nl[c2] += Ad[a][c2] * lam[a];
                        for (int j = 0; j < NU; j++) nl[c2] += Jh[(((size_t)i * T + t) * NU + j) * NX + c2] * mu[j];
                    }
                    for (int j = 0; j < NX; j++) lam[j] = nl[j];
                }
                for (int j = 0; j < NX; j++) grad_host[(size_t)i * NX + j] = lam[j];
            }
            wc.push_back(since(t0)); kc.push_back(k_ms);
        }
        double host_dist = 0.;
        for (int i = 0; i < B; i++) if (optimal[i]) for (int j = 0; j < NX; j++) host_dist = std::max(host_dist, std::fabs(grad_host[(size_t)i * NX + j] - grad[(size_t)i * NX + j]));
        // (d) central differences: 2 k rollouts
        const double eps = 1e-4;
        std::vector<double> tp(theta0), up(nU), thp(nTh), fd((size_t)B * NX, 0.);
        std::vector<int> fd_ok(optimal);
        double kd = 0.;
        const auto t0 = now();
        for (int j = 0; j < NX; j++) {
            std::vector<double> Ls[2];
            for (int sg = 0; sg < 2; sg++) {
                for (int i = 0; i < B; i++) tp[(size_t)i * NX + j] = theta0[(size_t)i * NX + j] + (sg == 0 ? eps : -eps);
                const auto cd = solver.rollout(T, tp.data(), up.data(), w.data(), thp.data());
                kd += kernel_ms(false);
                for (int i = 0; i < B; i++) {
                    for (int t = 0; t < T; t++) if ((int)cd[(size_t)i * T + t] != EICOS_OPTIMAL) fd_ok[i] = 0;
                    Ls[sg].push_back(cost(up, thp, i));
                }
            }
            for (int i = 0; i < B; i++) { tp[(size_t)i * NX + j] = theta0[(size_t)i * NX + j]; fd[(size_t)i * NX + j] = (Ls[0][i] - Ls[1][i]) / (2 * eps); }
        }
        const double wd = since(t0);
        double worst = 0., scale = 0.;
        int compared = 0, within = 0;
        std::vector<double> dists;
        for (int i = 0; i < B; i++) {
            if (!fd_ok[i]) continue;
            compared++;
            double d = 0., sc = 0.;
            for (int j = 0; j < NX; j++) { d = std::max(d, std::fabs(grad[(size_t)i * NX + j] - fd[(size_t)i * NX + j])); sc = std::max(sc, std::fabs(fd[(size_t)i * NX + j])); }
            dists.push_back(d);
            within += d <= 1e-3 * sc ? 1 : 0;
            worst = std::max(worst, d); scale = std::max(scale, sc);
        }
        std::printf("linear MPC, nx = %d, nu = %d, horizon %d: n = %d, m = %d, p = %d; batch %d, %d closed-loop steps, %d launch(es) per rollout\n", NX, NU, N, n, m, p, B, T, launches);
        std::printf("(a) rollout                            : kernels %9.3f ms, wall clock %9.3f ms\n", median(ka), median(wa));
        std::printf("(b) rolloutJacobian + rolloutGradient  : kernels %9.3f ms, wall clock %9.3f ms\n", median(kb), median(wb));
        std::printf("(c) %2d x (stepParam + paramJacobian)   : kernels %9.3f ms, wall clock %9.3f ms   (max |grad_host - grad| %.3e)\n", T, median(kc), median(wc), host_dist);
        std::printf("(d) central differences, %d rollouts    : kernels %9.3f ms, wall clock %9.3f ms\n", 2 * NX, kd, wd);
        std::printf("max |grad - grad_fd| over %d of %d instances (all steps optimal on every run): %.3e, median %.3e; %d within 1e-3 of their own max |grad_fd|   (eps = %.0e, max |grad_fd| %.3e)\n",
                    compared, B, worst, dists.empty() ? 0. : median(dists), within, eps, scale);
    } catch (const std::exception &e) {
        std::fprintf(stderr, "rollout_gradient_demo: %s\n", e.what());
        return 1;
    }
    return 0;
}
