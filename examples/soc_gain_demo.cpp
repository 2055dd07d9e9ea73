// The local feedback gain of a linear MPC law with a EUCLIDEAN input bound, from host C++ (no torch): J = du_0 / dx_0 of every instance
// of a batch by adjoint sensitivities (EiCOS::BatchSolver::paramJacobian) under both cone scalings of the adjoint -- EICOS_ADJOINT_NT,
// the default, and EICOS_ADJOINT_CENTRED (setAdjointScaling) -- against central differences of the closed-loop step (stepParam).
//
// The problem is the stage-ordered linear MPC of warm_shift_demo.cpp and jacobian_demo.cpp -- dynamics x+ = A x + B u (two double
// integrators: nx = 4 states, nu = 2 inputs), horizon N, stage cost |x|_1 + rho |u|_1 through epigraph variables -- with its input box
// replaced by |u_t|_2 <= umax: one second-order cone of dimension 3 per stage, (umax, u_t) in Q^3.  The measured states are drawn large
// enough that the first inputs saturate the bound: the optimum then lies on the cones' surfaces and slides along them with x_0, which
// is where the NT scaling of the returned (s, z) gives a gain that is wrong by a factor of order one and the centred one gives the
// derivative (include/eicos_amd.h).
// Printed: how many instances have u_0 on the bound; per mode the median over the instances of max |J - J_fd| / max |J_fd| and how
// many instances lie within 1e-2 (an instance with a change of the active set within eps has no derivative to compare with), for
// the saturated instances and for the others; and the time of the adjoint launch in both modes (HIP events around the kernel, the two modes
// interleaved on the same handle, median of 5).
//   g++ -std=c++17 -Iinclude examples/soc_gain_demo.cpp -Leicos_amd -leicos_amd -Wl,-rpath,$PWD/eicos_amd -o soc_gain_demo
//   ./soc_gain_demo [batch = 1024] [N = 20]
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
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
    const int B = argc > 1 ? std::atoi(argv[1]) : 1024, N = argc > 2 ? std::atoi(argv[2]) : 20;
    if (B < 1 || N < 2) { std::fprintf(stderr, "usage: soc_gain_demo [batch >= 1] [N >= 2]\n"); return 2; }
    // ---- the problem: the LP rows stage by stage (the epigraphs of |x|_1 and |u|_1), then one cone of dimension 3 per stage
    const int S = 2 * NX + 2 * NU, LS = 2 * NX + 2 * NU, l = N * LS, n = N * S, m = l + 3 * N, p = N * NX;
    std::vector<std::tuple<int, int, double>> tg, ta;
    std::vector<double> c(n, 0.), h(m, 0.), b(p, 0.);
    const std::vector<int> q(N, 3);
    for (int t = 0; t < N; t++) {
        const int u0 = t * S, x1 = u0 + NU, e0 = x1 + NX, f0 = e0 + NX, g0 = t * LS, a0 = t * NX, k0 = l + 3 * t;
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
            const int r = g0 + 2 * NX + 2 * i;
            tg.push_back({r, u0 + i, 1.}); tg.push_back({r, f0 + i, -1.});
            tg.push_back({r + 1, u0 + i, -1.}); tg.push_back({r + 1, f0 + i, -1.});
            tg.push_back({k0 + 1 + i, u0 + i, -1.}); // s = h - G x = (umax, u_t): |u_t|_2 <= umax
        }
        h[k0] = UMAX;
    }
    const Csc G(n, tg), A(n, ta);
    // ---- the maps: theta = x_0 enters b of stage 0 as A theta; u = u_0
    Affine bmap(p), omap(NU);
    for (int i = 0; i < p; i++) {
        if (i < NX) for (int j = 0; j < NX; j++) if (Ad[i][j] != 0.) { bmap.col.push_back(j); bmap.val.push_back(Ad[i][j]); }
        bmap.row_done();
    }
    for (int i = 0; i < NU; i++) { omap.col.push_back(i); omap.val.push_back(1.); omap.row_done(); }
    const eicos_affine_map vb = bmap.view(), vo = omap.view();
    // ---- the batch: the same model, measured states far enough from the origin that the first inputs sit on the bound
    unsigned long long st = 88172645463325252ull;
    auto rnd = [&] { st = st * 6364136223846793005ull + 1442695040888963407ull; return (double)((st >> 11) & 0xFFFFFFFFFFFFull) / (double)(1ull << 48); };
    std::vector<double> theta0((size_t)B * NX);
    for (int i = 0; i < B; i++)
        for (int j = 0; j < NX; j++) theta0[(size_t)i * NX + j] = (j % 2 == 0 ? 4.0 : 1.0) * (2 * rnd() - 1);
    auto rep = [&](const std::vector<double> &row) { std::vector<double> out; out.reserve(row.size() * B); for (int i = 0; i < B; i++) out.insert(out.end(), row.begin(), row.end()); return out; };
    const std::vector<double> Gb = rep(G.pr), Ab = rep(A.pr), cb = rep(c), hb = rep(h), bb = rep(b);
    auto median = [](std::vector<float> v) { std::sort(v.begin(), v.end()); return v[v.size() / 2]; };
    try {
        EiCOS::BatchSolver solver(n, m, p, N, q.data(), G.jc.data(), G.ir.data(), A.jc.data(), A.ir.data(), B, std::vector<int>{0});
        solver.updateData(Gb.data(), Ab.data(), cb.data(), hb.data(), bb.data());
        solver.setParamMap(NX, nullptr, nullptr, &vb);
        solver.setOutputMap(NU, &vo);
        const size_t nj = (size_t)B * NU * NX;
        std::vector<double> u((size_t)B * NU), Jnt(nj), Jce(nj), res((size_t)B * NU), Jfd(nj, 0.);
        const auto codes = solver.stepParam(theta0.data(), u.data());
        int optimal = 0;
        for (const auto code : codes) optimal += (int)code == EICOS_OPTIMAL ? 1 : 0;
        std::vector<float> t_nt, t_ce;
        for (int rep5 = 0; rep5 < 5; rep5++) { // the two modes interleaved, at the iterate of the one solve above
            float ms = 0.f;
            solver.setAdjointScaling(EICOS_ADJOINT_NT);
            solver.paramJacobian(Jnt.data(), res.data());
            eicos_batch_last_adjoint_ms(solver.handle(), &ms); t_nt.push_back(ms);
            solver.setAdjointScaling(EICOS_ADJOINT_CENTRED);
            solver.paramJacobian(Jce.data(), res.data());
            eicos_batch_last_adjoint_ms(solver.handle(), &ms); t_ce.push_back(ms);
        }
        // central differences: 2 k closed-loop steps
        const double eps = 1e-4;
        std::vector<double> th(theta0), up((size_t)B * NU), um((size_t)B * NU);
        for (int j = 0; j < NX; j++) {
            for (int i = 0; i < B; i++) th[(size_t)i * NX + j] = theta0[(size_t)i * NX + j] + eps;
            solver.stepParam(th.data(), up.data());
            for (int i = 0; i < B; i++) th[(size_t)i * NX + j] = theta0[(size_t)i * NX + j] - eps;
            solver.stepParam(th.data(), um.data());
            for (int i = 0; i < B; i++) {
                th[(size_t)i * NX + j] = theta0[(size_t)i * NX + j];
                for (int r = 0; r < NU; r++) Jfd[((size_t)i * NU + r) * NX + j] = (up[(size_t)i * NU + r] - um[(size_t)i * NU + r]) / (2 * eps);
            }
        }
        // per instance: max |J - J_fd| / max |J_fd| under each mode; the worst and the median over the saturated and over the other instances
        std::vector<double> dn[2], dc[2];
        int saturated = 0;
        for (int i = 0; i < B; i++) {
            bool finite = true;
            double an = 0., ac = 0., scale = 0.;
            for (int e = 0; e < NU * NX; e++) {
                const double a = Jnt[(size_t)i * NU * NX + e], ce = Jce[(size_t)i * NU * NX + e], f = Jfd[(size_t)i * NU * NX + e];
                finite = finite && std::isfinite(a) && std::isfinite(ce) && std::isfinite(f);
                an = std::max(an, std::fabs(a - f)); ac = std::max(ac, std::fabs(ce - f)); scale = std::max(scale, std::fabs(f));
            }
            const bool sat = std::hypot(u[(size_t)i * NU], u[(size_t)i * NU + 1]) >= UMAX * (1. - 1e-6);
            saturated += sat ? 1 : 0;
            if (!finite || scale == 0.) continue;
            dn[sat ? 0 : 1].push_back(an / scale); dc[sat ? 0 : 1].push_back(ac / scale);
        }
        auto stats = [](std::vector<double> v, double &med, int &close) { // the median, and how many lie within 1e-2
            close = 0; med = 0.;
            if (v.empty()) return;
            std::sort(v.begin(), v.end());
            med = v[v.size() / 2];
            for (const double x : v) close += x <= 1e-2 ? 1 : 0;
        };
        std::printf("linear MPC with |u_t|_2 <= %.1f, nx = %d, nu = %d, horizon %d: n = %d, m = %d (%d cones of dimension 3), p = %d; batch %d, %d solves optimal, %d with u_0 on the bound\n",
                    UMAX, NX, NU, N, n, m, N, p, B, optimal, saturated);
        const char *group[2] = {"u_0 on the bound", "u_0 inside"};
        for (int gI = 0; gI < 2; gI++) {
            double dnm, dcm;
            int cn, cc;
            stats(dn[gI], dnm, cn); stats(dc[gI], dcm, cc);
            std::printf("%-17s (%4zu instances, J_fd != 0): max |J - J_fd| / max |J_fd|   NT: median %.3e, %d within 1e-2   centred: median %.3e, %d within 1e-2   (eps = %.0e)\n",
                        group[gI], dn[gI].size(), dnm, cn, dcm, cc, eps);
        }
        std::printf("paramJacobian (k = %d, r = %d), adjoint launch: NT %.3f ms, centred %.3f ms (%+.1f %%)  (HIP events, interleaved, median of 5)\n",
                    NX, NU, median(t_nt), median(t_ce), 100. * (median(t_ce) / median(t_nt) - 1.));
    } catch (const std::exception &e) {
        std::fprintf(stderr, "soc_gain_demo: %s\n", e.what());
        return 1;
    }
    return 0;
}
