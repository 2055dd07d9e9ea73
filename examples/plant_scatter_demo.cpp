// One controller against a scatter of plants, from host C++ (no torch): the linear MPC of warm_shift_demo.cpp (two double integrators,
// nx = 4 states, nu = 2 inputs, horizon N, 1-norm stage costs, a box on u; theta = x_0 enters b, u = u_0) designed for the nominal plant
// theta+ = A theta + B u, while instance i of the batch is SIMULATED against a plant of its own: every entry of A and B scaled by a
// factor drawn within +-10 % (setPlantValues; the pattern stays the shared one).  All instances start from the same state, so the spread
// of the closed-loop cost  L = 1/2 sum_{t=0..T} |theta_t|^2 + rho/2 sum_{t<T} |u_t|^2  is the plants' doing alone.  Printed:
//   (a) the rollout with per-instance values and the rollout of the same handle after clearPlantValues, interleaved, each the median of
//       5 (the kernel between HIP events on the handle's stream, and the wall clock of the call);
//   (b) the spread of L over the plants, beside L of the nominal plant;
//   (c) rolloutJacobian + rolloutPlantGradient (the gradient of L with respect to every plant entry of every instance) beside
//       rolloutJacobian + rolloutGradient, median of 5;
//   (d) one entry of grad_val against a central difference of two rollouts (eps = 1e-4), over the instances whose steps all ended
//       optimal on the three runs: the 1-norm costs make u(theta) piecewise affine, so an instance with a change of the active set
//       inside the difference stencil disagrees -- the median is the figure that describes the agreement.
//   g++ -std=c++17 -Iinclude examples/plant_scatter_demo.cpp -Leicos_amd -leicos_amd -Wl,-rpath,$PWD/eicos_amd -o plant_scatter_demo
//   ./plant_scatter_demo [batch = 1024] [N = 20] [T = 20]
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
    if (B < 1 || N < 2 || T < 1) { std::fprintf(stderr, "usage: plant_scatter_demo [batch] [N >= 2] [T >= 1]\n"); return 2; }
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
    // ---- the maps: theta = x_0 enters b of stage 0 as A theta; u = u_0; the nominal plant theta+ = A theta + B u
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
    const int nnzF = (int)plant.val.size();
    // ---- the batch: one initial state, a plant per instance (instance 0 keeps the nominal one)
    unsigned long long st = 88172645463325252ull;
    auto rnd = [&] { st = st * 6364136223846793005ull + 1442695040888963407ull; return (double)((st >> 11) & 0xFFFFFFFFFFFFull) / (double)(1ull << 48); };
    std::vector<double> theta0((size_t)B * NX), vals((size_t)B * nnzF);
    for (int i = 0; i < B; i++) {
        const double x0[NX] = {1.5, -0.3, -1.0, 0.4};
        for (int j = 0; j < NX; j++) theta0[(size_t)i * NX + j] = x0[j];
        for (int s = 0; s < nnzF; s++) vals[(size_t)i * nnzF + s] = plant.val[s] * (i == 0 ? 1. : 0.9 + 0.2 * rnd());
    }
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
        eicos_batch *hd = solver.handle();
        auto kernel_ms = [&](bool adjoint) { float ms = 0.f; if (adjoint) eicos_batch_last_adjoint_ms(hd, &ms); else eicos_batch_last_solve_ms(hd, &ms); return (double)ms; };
        auto cost = [&](const std::vector<double> &u, const std::vector<double> &th, int i) {
            double L = 0.;
            for (int t = 0; t <= T; t++) for (int j = 0; j < NX; j++) { const double v = th[((size_t)i * (T + 1) + t) * NX + j]; L += 0.5 * v * v; }
            for (int t = 0; t < T; t++) for (int j = 0; j < NU; j++) { const double v = u[((size_t)i * T + t) * NU + j]; L += 0.5 * RHO * v * v; }
            return L;
        };
        std::vector<double> u(nU), th(nTh), us(nU), ths(nTh), J(nJ), gu(nU), grad((size_t)B * NX), gval((size_t)B * nnzF), gf0((size_t)B * NX);
        std::vector<double> kv, wv, ks, ws, kp, wp, kg, wg;
        std::vector<EiCOS::exitcode> codes;
        // (a) the rollout with per-instance values and with the shared plant, taking turns
        for (int q = 0; q < 5; q++) {
            solver.setPlantValues(0, B, nullptr, vals.data());
            auto t0 = now();
            solver.rollout(T, theta0.data(), u.data(), nullptr, th.data());
            wv.push_back(since(t0)); kv.push_back(kernel_ms(false));
            solver.clearPlantValues();
            t0 = now();
            solver.rollout(T, theta0.data(), us.data(), nullptr, ths.data());
            ws.push_back(since(t0)); ks.push_back(kernel_ms(false));
        }
        const int launches = eicos_batch_last_rollout_launches(hd);
        // (b) the spread of the closed-loop cost over the plants
        std::vector<double> Ls(B);
        for (int i = 0; i < B; i++) Ls[i] = cost(u, th, i);
        std::vector<double> sorted(Ls);
        std::sort(sorted.begin(), sorted.end());
        const double nominal = cost(us, ths, 0);
        // (c) the gradient with respect to every plant entry, beside the gradient with respect to theta_0 alone
        solver.setPlantValues(0, B, nullptr, vals.data());
        for (int q = 0; q < 5; q++) {
            auto t0 = now();
            codes = solver.rolloutJacobian(T, theta0.data(), u.data(), J.data(), nullptr, th.data());
            double k_ms = kernel_ms(false);
            for (size_t e = 0; e < nU; e++) gu[e] = RHO * u[e];
            solver.rolloutPlantGradient(gu.data(), th.data(), u.data(), th.data(), grad.data(), nullptr, gf0.data(), gval.data());
            wp.push_back(since(t0)); kp.push_back(k_ms + kernel_ms(true));
            t0 = now();
            codes = solver.rolloutJacobian(T, theta0.data(), u.data(), J.data(), nullptr, th.data());
            k_ms = kernel_ms(false);
            for (size_t e = 0; e < nU; e++) gu[e] = RHO * u[e];
            solver.rolloutGradient(gu.data(), th.data(), grad.data());
            wg.push_back(since(t0)); kg.push_back(k_ms + kernel_ms(true));
        }
        std::vector<int> ok(B, 1);
        for (int i = 0; i < B; i++) for (int t = 0; t < T; t++) if ((int)codes[(size_t)i * T + t] != EICOS_OPTIMAL) ok[i] = 0;
        // (d) one entry of grad_val -- A[0][1], the coupling of the first position to its velocity -- against a central difference
        const int s_fd = 1;
        const double eps = 1e-4;
        std::vector<double> vp(vals), up(nU), thp(nTh), Lpm[2];
        for (int sg = 0; sg < 2; sg++) {
            for (int i = 0; i < B; i++) vp[(size_t)i * nnzF + s_fd] = vals[(size_t)i * nnzF + s_fd] + (sg == 0 ? eps : -eps);
            solver.setPlantValues(0, B, nullptr, vp.data());
            const auto cd = solver.rollout(T, theta0.data(), up.data(), nullptr, thp.data());
            for (int i = 0; i < B; i++) {
                for (int t = 0; t < T; t++) if ((int)cd[(size_t)i * T + t] != EICOS_OPTIMAL) ok[i] = 0;
                Lpm[sg].push_back(cost(up, thp, i));
            }
        }
        std::vector<double> dists;
        double scale = 0.;
        int within = 0;
        for (int i = 0; i < B; i++) {
            if (!ok[i]) continue;
            const double fd = (Lpm[0][i] - Lpm[1][i]) / (2 * eps), d = std::fabs(gval[(size_t)i * nnzF + s_fd] - fd);
            dists.push_back(d); scale = std::max(scale, std::fabs(fd));
            within += d <= 1e-3 * std::fabs(fd) ? 1 : 0;
        }
        std::printf("linear MPC, nx = %d, nu = %d, horizon %d: n = %d, m = %d, p = %d; batch %d, %d closed-loop steps, %d launch(es) per rollout; %d plant entries per instance\n",
                    NX, NU, N, n, m, p, B, T, launches, nnzF);
        std::printf("(a) rollout, per-instance plant values      : kernel %9.3f ms, wall clock %9.3f ms\n", median(kv), median(wv));
        std::printf("    rollout, after clearPlantValues         : kernel %9.3f ms, wall clock %9.3f ms\n", median(ks), median(ws));
        std::printf("(b) closed-loop cost over %d plants within +-10 %%: min %.4f, median %.4f, max %.4f; the nominal plant %.4f\n", B, sorted.front(),
                    sorted[sorted.size() / 2], sorted.back(), nominal);
        std::printf("(c) rolloutJacobian + rolloutPlantGradient  : kernels %9.3f ms, wall clock %9.3f ms\n", median(kp), median(wp));
        std::printf("    rolloutJacobian + rolloutGradient       : kernels %9.3f ms, wall clock %9.3f ms\n", median(kg), median(wg));
        std::printf("(d) dL/dA[0][1] of instance 0: %.6e (adjoint), %.6e (central difference, eps = %.0e)\n", gval[s_fd], (Lpm[0][0] - Lpm[1][0]) / (2 * eps), eps);
        std::printf("    |grad_val - fd| over %zu of %d instances (all steps optimal on the three runs): median %.3e, max %.3e; %d within 1e-3 of their own |fd|   (max |fd| %.3e)\n",
                    dists.size(), B, dists.empty() ? 0. : median(dists), dists.empty() ? 0. : *std::max_element(dists.begin(), dists.end()), within, scale);
    } catch (const std::exception &e) {
        std::fprintf(stderr, "plant_scatter_demo: %s\n", e.what());
        return 1;
    }
    return 0;
}
