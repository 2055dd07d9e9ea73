// The local feedback gain of a successively linearised MPC law from host C++ (no torch): J = du_0 / dx_0 when the MODEL MATRICES depend on
// the measured state.  EiCOS::BatchSolver::paramJacobian contracts r = nu adjoint solves per instance with the parameter map AND the
// matrix map on the GPU (the matrix terms are a sampled outer product on the pattern: no further factorisation or KKT solve);
// the alternative is 2 k = 2 nx further closed-loop steps of central differences, each a full updateData from theta and a solve.
//
// The problem is the stage-ordered linear MPC of warm_shift_demo.cpp: dynamics x+ = A x + B u (two double integrators: nx = 4 states,
// nu = 2 inputs), horizon N, stage cost |x|_1 + rho |u|_1 through epigraph variables, a box |u| <= umax; the parameter map
// b = b0 + Bm theta (theta = x_0, k = nx), the output map u = u_0 (r = nu) -- and a matrix map on the dynamics rows of every stage: the
// model is re-linearised around the measured state, the position-velocity coupling dt becomes dt (1 + SENS v_0) and the input gains
// B become B (1 + SENS p_0) with (p_0, v_0) the measured position and velocity of the axis.
// Printed: the time of paramJacobian, the time of outputJacobian on the same handle with the matrix map removed (the right-hand-side
// terms alone: what the matrix terms cost on top), the time of the finite-difference alternative (its 2 k solve launches by HIP
// events, and the wall clock of its 2 k steps, which also holds the 2 k updateData launches), max |J - J_fd| over the instances for
// which both are finite, and the count of OPTIMAL exits.  Kernels by HIP events, median of 5.
//   g++ -std=c++17 -Iinclude examples/matrix_jacobian_demo.cpp -Leicos_amd -leicos_amd -Wl,-rpath,$PWD/eicos_amd -o matrix_jacobian_demo
//   ./matrix_jacobian_demo [batch = 1024] [N = 20]
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
constexpr double DT = 0.5, RHO = 0.1, UMAX = 1.0, SENS = 0.05;
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
    if (B < 1 || N < 2) { std::fprintf(stderr, "usage: matrix_jacobian_demo [batch >= 1] [N >= 2]\n"); return 2; }
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
    // ---- the maps: theta = x_0 enters b of stage 0 as A theta; u = u_0
    Affine bmap(p), omap(NU);
    for (int i = 0; i < p; i++) {
        if (i < NX) for (int j = 0; j < NX; j++) if (Ad[i][j] != 0.) { bmap.col.push_back(j); bmap.val.push_back(Ad[i][j]); }
        bmap.row_done();
    }
    for (int i = 0; i < NU; i++) { omap.col.push_back(i); omap.val.push_back(1.); omap.row_done(); }
    // ---- the matrix map: one CSR row per stored value of A, in its CSC order.  Axis a has position 2a and velocity 2a + 1: the stored
    // value -dt at (row 2a, column of v_a) moves with theta[2a + 1], the stored values -B at (rows 2a, 2a + 1, column of u_a) with theta[2a]
    Affine amap((int)A.pr.size());
    amap.base = A.pr;
    for (int j = 0, e = 0; j < n; j++) {
        const int in_stage = j % S; // (0 .. NU-1: u; NU .. NU+NX-1: x+)
        for (; e < A.jc[j + 1]; e++) {
            const int i = A.ir[e] % NX; // the state row of the dynamics
            if (in_stage < NU && A.pr[e] != 0.) { amap.col.push_back(2 * in_stage); amap.val.push_back(SENS * A.pr[e]); }
            else if (in_stage >= NU && in_stage < NU + NX && i != in_stage - NU && A.pr[e] != 0.) { amap.col.push_back(i + 1); amap.val.push_back(SENS * A.pr[e]); }
            amap.row_done();
        }
    }
    const eicos_affine_map vb = bmap.view(), vo = omap.view(), va = amap.view();
    // ---- the batch: the same model, different measured states
    unsigned long long st = 88172645463325252ull;
    auto rnd = [&] { st = st * 6364136223846793005ull + 1442695040888963407ull; return (double)((st >> 11) & 0xFFFFFFFFFFFFull) / (double)(1ull << 48); };
    std::vector<double> theta0((size_t)B * NX);
    for (int i = 0; i < B; i++)
        for (int j = 0; j < NX; j++) theta0[(size_t)i * NX + j] = (j % 2 == 0 ? 2.0 : 0.5) * (2 * rnd() - 1);
    auto rep = [&](const std::vector<double> &row) { std::vector<double> out; out.reserve(row.size() * B); for (int i = 0; i < B; i++) out.insert(out.end(), row.begin(), row.end()); return out; };
    const std::vector<double> Gb = rep(G.pr), Ab = rep(A.pr), cb = rep(c), hb = rep(h), bb = rep(b);
    auto median = [](std::vector<float> v) { std::sort(v.begin(), v.end()); return v[v.size() / 2]; };
    try {
        EiCOS::BatchSolver solver(n, m, p, 0, nullptr, G.jc.data(), G.ir.data(), A.jc.data(), A.ir.data(), B, std::vector<int>{0});
        solver.updateData(Gb.data(), Ab.data(), cb.data(), hb.data(), bb.data());
        solver.setParamMap(NX, nullptr, nullptr, &vb);
        solver.setOutputMap(NU, &vo);
        EiCOS::MatrixMap mm;
        mm.A = &va;
        solver.setMatrixMap(mm);
        std::vector<double> u((size_t)B * NU), J((size_t)B * NU * NX), res((size_t)B * NU), Jfd((size_t)B * NU * NX, 0.);
        std::vector<float> t_solve, t_jac, t_out;
        int optimal = 0;
        for (int rep5 = 0; rep5 < 5; rep5++) {
            const auto codes = solver.stepParam(theta0.data(), u.data());
            float ms = 0.f;
            eicos_batch_last_solve_ms(solver.handle(), &ms); t_solve.push_back(ms);
            solver.paramJacobian(J.data(), res.data());
            eicos_batch_last_adjoint_ms(solver.handle(), &ms); t_jac.push_back(ms);
            optimal = 0;
            for (const auto code : codes) optimal += (int)code == EICOS_OPTIMAL ? 1 : 0;
        }
        // central differences: 2 k closed-loop steps
        const double eps = 1e-4;
        std::vector<double> th(theta0), up((size_t)B * NU), um((size_t)B * NU);
        float fd_kernel_ms = 0.f;
        const auto t0 = std::chrono::steady_clock::now();
        for (int j = 0; j < NX; j++) {
            float ms = 0.f;
            for (int i = 0; i < B; i++) th[(size_t)i * NX + j] = theta0[(size_t)i * NX + j] + eps;
            solver.stepParam(th.data(), up.data()); eicos_batch_last_solve_ms(solver.handle(), &ms); fd_kernel_ms += ms;
            for (int i = 0; i < B; i++) th[(size_t)i * NX + j] = theta0[(size_t)i * NX + j] - eps;
            solver.stepParam(th.data(), um.data()); eicos_batch_last_solve_ms(solver.handle(), &ms); fd_kernel_ms += ms;
            for (int i = 0; i < B; i++) {
                th[(size_t)i * NX + j] = theta0[(size_t)i * NX + j];
                for (int r = 0; r < NU; r++) Jfd[((size_t)i * NU + r) * NX + j] = (up[(size_t)i * NU + r] - um[(size_t)i * NU + r]) / (2 * eps);
            }
        }
        const double fd_wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        double worst = 0., worst_res = 0.;
        int compared = 0;
        for (int i = 0; i < B; i++) {
            bool finite = true;
            double dist = 0.;
            for (int e = 0; e < NU * NX; e++) {
                const double a = J[(size_t)i * NU * NX + e], f = Jfd[(size_t)i * NU * NX + e];
                finite = finite && std::isfinite(a) && std::isfinite(f);
                dist = std::max(dist, std::fabs(a - f));
            }
            if (!finite) continue;
            compared++;
            worst = std::max(worst, dist);
            for (int r = 0; r < NU; r++) worst_res = std::max(worst_res, res[(size_t)i * NU + r]);
        }
        // the right-hand-side terms alone: the same handle at the same iterates, the matrix map removed
        solver.stepParam(theta0.data(), u.data());
        solver.setMatrixMap(EiCOS::MatrixMap{});
        std::vector<double> Jv(J.size());
        for (int rep5 = 0; rep5 < 5; rep5++) {
            float ms = 0.f;
            solver.outputJacobian(Jv.data());
            eicos_batch_last_adjoint_ms(solver.handle(), &ms); t_out.push_back(ms);
        }
        std::printf("successively linearised MPC, nx = %d, nu = %d, horizon %d: n = %d, m = %d, p = %d; batch %d, %d of %d solves optimal\n", NX, NU, N, n, m, p, B, optimal, B);
        std::printf("paramJacobian under the matrix map (k = %d, r = %d, %d of %d stored values of A mapped): %.3f ms;  outputJacobian, matrix map removed: %.3f ms;  solve: %.3f ms  (kernels, HIP events, median of 5)\n",
                    NX, NU, (int)amap.col.size(), (int)A.pr.size(), median(t_jac), median(t_out), median(t_solve));
        std::printf("finite differences (%d steps): %.3f ms in the solve kernels, %.3f ms wall clock\n", 2 * NX, fd_kernel_ms, fd_wall_ms);
        std::printf("max |J - J_fd| over %d instances: %.3e   (eps = %.0e; largest res %.2e)\n", compared, worst, eps, worst_res);
    } catch (const std::exception &e) {
        std::fprintf(stderr, "matrix_jacobian_demo: %s\n", e.what());
        return 1;
    }
    return 0;
}
