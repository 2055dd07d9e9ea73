// The gradient of a closed-loop cost with respect to the CONTROLLER's own data, from host C++ (no torch): the linear MPC of
// warm_shift_demo.cpp (two double integrators, nx = 4 states, nu = 2 inputs, horizon N, 1-norm stage costs, a box on u; theta = x_0
// enters b, u = u_0, the plant theta+ = A theta + B u + w), run as a closed loop of T steps per instance, every step solved cold, with
// the cost of rollout_gradient_demo.cpp,
//     L = 1/2 sum_{t=0..T} |theta_t|^2 + rho/2 sum_{t<T} |u_t|^2.
// The tunables are the stage-cost weights held in c0 -- one weight per state (the entries of c on the 1-norm bounds of x, every stage)
// and one per input (those on the bounds of u), nx + nu numbers -- and, beside them, the input bound u_max held in h0.  A recording
// rolloutJacobian followed by rolloutDataGradient gives grad_c and grad_h per instance; a tunable's gradient is the sum of the entries
// it sits in.  Printed, each the median of 5 (the kernels between HIP events on the handle's stream):
//   (a) rolloutJacobian, recording off
//   (b) rolloutJacobian, recording on              (batch * T * (r + 1) * (n + m + p) * 8 bytes of records)
//   (c) rolloutDataGradient                        the second backward sweep
//   (d) central differences over the same tunables: 2 rollouts per tunable at eps = 1e-4, through updateData
// and max |grad - grad_fd| over the instances whose steps all ended optimal on every run, per kind of tunable.  The MPC is a linear
// program, so u is piecewise CONSTANT in the cost weights: their derivative is 0 wherever it exists, the adjoint returns its smoothed
// value and the central difference is 0 or, across a change of the active set, meaningless -- u_max is the tunable that moves u.
//   g++ -std=c++17 -Iinclude examples/controller_tuning_demo.cpp -Leicos_amd -leicos_amd -Wl,-rpath,$PWD/eicos_amd -o controller_tuning_demo
//   ./controller_tuning_demo [batch = 1024] [N = 20] [T = 20]
// -DCONTROLLER_TUNING_BASELINE: (a) alone, through calls a library without the recording entry points has -- the same figure from the
// commit before them, for a comparison on one machine.
#include <algorithm>
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
    if (B < 1 || N < 2 || T < 1) { std::fprintf(stderr, "usage: controller_tuning_demo [batch] [N >= 2] [T >= 1]\n"); return 2; }
    // ---- the problem, stage by stage; where[q] = the entries of c (q < NX + NU) or of h (q = NX + NU) tunable q sits in
    const int S = 2 * NX + 2 * NU, MS = 2 * NX + 4 * NU, n = N * S, m = N * MS, p = N * NX, NT = NX + NU + 1;
    std::vector<std::tuple<int, int, double>> tg, ta;
    std::vector<double> c(n, 0.), h(m, 0.), b(p, 0.);
    std::vector<std::vector<int>> where(NT);
    for (int t = 0; t < N; t++) {
        const int u0 = t * S, x1 = u0 + NU, e0 = x1 + NX, f0 = e0 + NX, g0 = t * MS, a0 = t * NX;
        for (int i = 0; i < NX; i++) {
            c[e0 + i] = 1.; where[i].push_back(e0 + i);
            tg.push_back({g0 + 2 * i, x1 + i, 1.}); tg.push_back({g0 + 2 * i, e0 + i, -1.});
            tg.push_back({g0 + 2 * i + 1, x1 + i, -1.}); tg.push_back({g0 + 2 * i + 1, e0 + i, -1.});
            ta.push_back({a0 + i, x1 + i, 1.});
            for (int j = 0; j < NX; j++) if (t > 0 && Ad[i][j] != 0.) ta.push_back({a0 + i, x1 - S + j, -Ad[i][j]});
            for (int j = 0; j < NU; j++) if (Bd[i][j] != 0.) ta.push_back({a0 + i, u0 + j, -Bd[i][j]});
        }
        for (int i = 0; i < NU; i++) {
            c[f0 + i] = RHO; where[NX + i].push_back(f0 + i);
            const int r = g0 + 2 * NX + 4 * i;
            tg.push_back({r, u0 + i, 1.}); tg.push_back({r, f0 + i, -1.});
            tg.push_back({r + 1, u0 + i, -1.}); tg.push_back({r + 1, f0 + i, -1.});
            tg.push_back({r + 2, u0 + i, 1.}); h[r + 2] = UMAX; where[NX + NU].push_back(r + 2);
            tg.push_back({r + 3, u0 + i, -1.}); h[r + 3] = UMAX; where[NX + NU].push_back(r + 3);
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
    // ---- the batch: the same controller, different measured states and disturbances
    unsigned long long st = 88172645463325252ull;
    auto rnd = [&] { st = st * 6364136223846793005ull + 1442695040888963407ull; return (double)((st >> 11) & 0xFFFFFFFFFFFFull) / (double)(1ull << 48); };
    std::vector<double> theta0((size_t)B * NX), w((size_t)B * T * NX);
    for (int i = 0; i < B; i++)
        for (int j = 0; j < NX; j++) theta0[(size_t)i * NX + j] = (j % 2 == 0 ? 2.0 : 0.5) * (2 * rnd() - 1);
    for (double &v : w) v = 0.01 * (2 * rnd() - 1);
    auto rep = [&](const std::vector<double> &row) { std::vector<double> out; out.reserve(row.size() * B); for (int i = 0; i < B; i++) out.insert(out.end(), row.begin(), row.end()); return out; };
    const std::vector<double> Gb = rep(G.pr), Ab = rep(A.pr), cb = rep(c), hb = rep(h), bb = rep(b);

    auto median = [](std::vector<double> v) { std::sort(v.begin(), v.end()); return v[v.size() / 2]; };
    const size_t nU = (size_t)B * T * NU, nTh = (size_t)B * (T + 1) * NX, nJ = (size_t)B * T * NU * NX;
    try {
        EiCOS::BatchSolver solver(n, m, p, 0, nullptr, G.jc.data(), G.ir.data(), A.jc.data(), A.ir.data(), B, std::vector<int>{0});
        solver.updateData(Gb.data(), Ab.data(), cb.data(), hb.data(), bb.data());
        solver.setParamMap(NX, nullptr, nullptr, &vb);
        solver.setOutputMap(NU, &vo);
        solver.setPlantMap(&vf);
        eicos_batch *hd = solver.handle();
        auto kernel_ms = [&](bool adjoint) { float ms = 0.f; if (adjoint) eicos_batch_last_adjoint_ms(hd, &ms); else eicos_batch_last_solve_ms(hd, &ms); return (double)ms; };
        std::vector<double> u(nU), th(nTh), J(nJ), ka, kb, kc;
        std::vector<EiCOS::exitcode> codes;
        std::printf("linear MPC, nx = %d, nu = %d, horizon %d: n = %d, m = %d, p = %d; batch %d, %d closed-loop steps\n", NX, NU, N, n, m, p, B, T);
        // (a) the rollout with its Jacobians, recording off
        for (int q = 0; q < 5; q++) {
            codes = solver.rolloutJacobian(T, theta0.data(), u.data(), J.data(), w.data(), th.data());
            ka.push_back(kernel_ms(false));
        }
        std::printf("(a) rolloutJacobian, recording off     : kernels %9.3f ms\n", median(ka));
#ifndef CONTROLLER_TUNING_BASELINE
        // (b) the same with recording on
        solver.setRolloutRecording(true);
        for (int q = 0; q < 5; q++) {
            codes = solver.rolloutJacobian(T, theta0.data(), u.data(), J.data(), w.data(), th.data());
            kb.push_back(kernel_ms(false));
        }
        std::vector<int> optimal(B, 1);
        for (int i = 0; i < B; i++) for (int t = 0; t < T; t++) if ((int)codes[(size_t)i * T + t] != EICOS_OPTIMAL) optimal[i] = 0;
        // (c) the second backward sweep: dL/du_t = rho u_t, dL/dtheta_t = theta_t
        std::vector<double> gu(nU), gc((size_t)B * n), gh((size_t)B * m);
        for (size_t e = 0; e < nU; e++) gu[e] = RHO * u[e];
        eicos_data_gradient out{};
        out.grad_c = gc.data(); out.grad_h = gh.data();
        for (int q = 0; q < 5; q++) {
            solver.rolloutDataGradient(gu.data(), th.data(), th.data(), out);
            kc.push_back(kernel_ms(true));
        }
        std::vector<double> grad((size_t)B * NT, 0.);
        for (int i = 0; i < B; i++)
            for (int q = 0; q < NT; q++)
                for (int e : where[q]) grad[(size_t)i * NT + q] += q < NX + NU ? gc[(size_t)i * n + e] : gh[(size_t)i * m + e];
        // (d) central differences over the same tunables: 2 rollouts per tunable, the data through updateData
        solver.setRolloutRecording(false);
        auto cost = [&](const std::vector<double> &uu, const std::vector<double> &tt, int i) {
            double L = 0.;
            for (int t = 0; t <= T; t++) for (int j = 0; j < NX; j++) { const double v = tt[((size_t)i * (T + 1) + t) * NX + j]; L += 0.5 * v * v; }
            for (int t = 0; t < T; t++) for (int j = 0; j < NU; j++) { const double v = uu[((size_t)i * T + t) * NU + j]; L += 0.5 * RHO * v * v; }
            return L;
        };
        const double eps = 1e-4;
        std::vector<double> up(nU), thp(nTh), fd((size_t)B * NT, 0.);
        std::vector<int> fd_ok(optimal);
        double kd = 0.;
        for (int q = 0; q < NT; q++) {
            std::vector<double> Ls[2];
            for (int sg = 0; sg < 2; sg++) {
                std::vector<double> cp(c), hp(h);
                for (int e : where[q]) (q < NX + NU ? cp[e] : hp[e]) += sg == 0 ? eps : -eps;
                const std::vector<double> cpb = rep(cp), hpb = rep(hp);
                solver.updateData(Gb.data(), Ab.data(), cpb.data(), hpb.data(), bb.data());
                const auto cd = solver.rollout(T, theta0.data(), up.data(), w.data(), thp.data());
                kd += kernel_ms(false);
                for (int i = 0; i < B; i++) {
                    for (int t = 0; t < T; t++) if ((int)cd[(size_t)i * T + t] != EICOS_OPTIMAL) fd_ok[i] = 0;
                    Ls[sg].push_back(cost(up, thp, i));
                }
            }
            for (int i = 0; i < B; i++) fd[(size_t)i * NT + q] = (Ls[0][i] - Ls[1][i]) / (2 * eps);
        }
        solver.updateData(Gb.data(), Ab.data(), cb.data(), hb.data(), bb.data());
        const double rec_gb = (double)B * T * (NU + 1) * ((double)n + m + p) * 8. / 1e9;
        std::printf("(b) rolloutJacobian, recording on      : kernels %9.3f ms   (%.2f GB of records)\n", median(kb), rec_gb);
        std::printf("(c) rolloutDataGradient                : kernels %9.3f ms\n", median(kc));
        std::printf("(d) central differences, %2d rollouts   : kernels %9.3f ms\n", 2 * NT, kd);
        int compared = 0;
        for (int i = 0; i < B; i++) compared += fd_ok[i];
        for (int kind = 0; kind < 2; kind++) { // the cost weights, then u_max
            double worst = 0., scale = 0., gmax = 0.;
            std::vector<double> dists;
            for (int i = 0; i < B; i++) {
                if (!fd_ok[i]) continue;
                double d = 0.;
                for (int q = kind == 0 ? 0 : NX + NU; q < (kind == 0 ? NX + NU : NT); q++) {
                    d = std::max(d, std::fabs(grad[(size_t)i * NT + q] - fd[(size_t)i * NT + q]));
                    scale = std::max(scale, std::fabs(fd[(size_t)i * NT + q])); gmax = std::max(gmax, std::fabs(grad[(size_t)i * NT + q]));
                }
                dists.push_back(d); worst = std::max(worst, d);
            }
            std::printf("%s: max |grad - grad_fd| over %d of %d instances (all steps optimal on every run) %.3e, median %.3e   (eps = %.0e, max |grad_fd| %.3e, max |grad| %.3e)\n",
                        kind == 0 ? "stage-cost weights in c0" : "u_max in h0             ", compared, B, worst, dists.empty() ? 0. : median(dists), eps, scale, gmax);
        }
#endif
    } catch (const std::exception &e) {
        std::fprintf(stderr, "controller_tuning_demo: %s\n", e.what());
        return 1;
    }
    return 0;
}
