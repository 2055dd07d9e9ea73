// What a looser tolerance buys a receding-horizon controller, from host C++ (no torch): the linear MPC and the closed loop of
// warm_shift_demo.cpp -- dynamics x+ = A x + B u (two double integrators: nx = 4 states, nu = 2 inputs), horizon N, stage cost
// |x|_1 + rho |u|_1 through epigraph variables, a box |u| <= umax, variables and rows stage by stage -- run at three settings of the exit
// tolerances (EiCOS::BatchSolver::setSettings: feastol = abstol = reltol = 1e-8, the default, then 1e-6 and 1e-4), each of them cold,
// warm-started from the previous step's solution as it lies, and warm-started from that solution moved one stage forward by a shift map.
// The closed loop: the parameter map b = b0 + Bm theta (theta = x_0, k = nx), the output map u = u_0 (r = nu), the plant map
// theta+ = A theta + B u + w -- rollout() runs T steps of every instance in one call.  Each of the nine runs takes a fresh solver through
// the same data, the same theta0 and the same disturbance, and prints the mean iteration count per step, the rollout time, the solves
// that did not end OPTIMAL, and the largest |u - u(1e-8)| over the whole trajectory against the run of the same kind at 1e-8: what the
// looser tolerance costs in the moves the controller applies.
//   g++ -std=c++17 -Iinclude examples/mpc_tolerance_demo.cpp -Leicos_amd -leicos_amd -Wl,-rpath,$PWD/eicos_amd -o mpc_tolerance_demo
//   ./mpc_tolerance_demo [batch = 1024] [N = 20] [T = 20] [devices = 0]        (a device may be listed twice: 0,0)
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <sstream>
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

// row j copies entry j + stride of the same vector; the last `stride` rows keep their own
Affine shift_by(int rows, int stride) {
    Affine a(rows);
    for (int j = 0; j < rows; j++) { a.col.push_back(j + stride < rows ? j + stride : j); a.val.push_back(1.); a.row_done(); }
    return a;
}

struct Result { double mean_iter, ms; int not_optimal, solves, launches, shards; std::vector<double> u; };
} // namespace

int main(int argc, char **argv) {
    const int B = argc > 1 ? std::atoi(argv[1]) : 1024, N = argc > 2 ? std::atoi(argv[2]) : 20, T = argc > 3 ? std::atoi(argv[3]) : 20;
    std::vector<int> devices;
    {
        std::stringstream ss(argc > 4 ? argv[4] : "0");
        for (std::string tok; std::getline(ss, tok, ',');) devices.push_back(std::atoi(tok.c_str()));
    }
    if (B < (int)devices.size() || N < 2 || T < 1) { std::fprintf(stderr, "usage: mpc_tolerance_demo [batch] [N >= 2] [T >= 1] [devices]\n"); return 2; }
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
    // ---- the maps: theta = x_0 enters b of stage 0 as A theta; u = u_0; theta+ = A theta + B u (+ w); the shift by one stage
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
    const Affine sx = shift_by(n, S), sy = shift_by(p, NX), sz = shift_by(m, MS);
    const eicos_affine_map vb = bmap.view(), vo = omap.view(), vf = plant.view(), vx = sx.view(), vy = sy.view(), vz = sz.view();
    // ---- the batch: the same model, different measured states and disturbances
    unsigned long long st = 88172645463325252ull;
    auto rnd = [&] { st = st * 6364136223846793005ull + 1442695040888963407ull; return (double)((st >> 11) & 0xFFFFFFFFFFFFull) / (double)(1ull << 48); };
    std::vector<double> theta0((size_t)B * NX), w((size_t)B * T * NX);
    for (int i = 0; i < B; i++)
        for (int j = 0; j < NX; j++) theta0[(size_t)i * NX + j] = (j % 2 == 0 ? 2.0 : 0.5) * (2 * rnd() - 1);
    for (double &v : w) v = 0.01 * (2 * rnd() - 1);
    auto rep = [&](const std::vector<double> &row) { std::vector<double> out; out.reserve(row.size() * B); for (int i = 0; i < B; i++) out.insert(out.end(), row.begin(), row.end()); return out; };
    const std::vector<double> Gb = rep(G.pr), Ab = rep(A.pr), cb = rep(c), hb = rep(h), bb = rep(b);

    auto run = [&](double tol, double warm, bool shift) -> Result {
        EiCOS::BatchSolver solver(n, m, p, 0, nullptr, G.jc.data(), G.ir.data(), A.jc.data(), A.ir.data(), B, devices);
        solver.updateData(Gb.data(), Ab.data(), cb.data(), hb.data(), bb.data());
        solver.setParamMap(NX, nullptr, nullptr, &vb);
        solver.setOutputMap(NU, &vo);
        solver.setPlantMap(&vf);
        solver.updateParam(theta0.data());
        solver.solve(); // (the solution a first warm step starts from, at the default tolerances; not timed, not counted)
        EiCOS::Settings st_ = solver.settings();
        st_.feastol = st_.abstol = st_.reltol = tol;
        solver.setSettings(st_);
        solver.setWarmStart(warm);
        if (shift) {
            EiCOS::ShiftMap sm;
            sm.x = &vx; sm.y = &vy; sm.z = &vz; sm.s = &vz;
            solver.setShiftMap(sm);
        }
        std::vector<double> u((size_t)B * T * NU);
        std::vector<int> iters((size_t)B * T);
        const auto t0 = std::chrono::steady_clock::now();
        const auto codes = solver.rollout(T, theta0.data(), u.data(), w.data(), nullptr, iters.data());
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        Result r{0., ms, 0, B * T, eicos_batch_last_rollout_launches(solver.handle()), solver.num_shards(), {}};
        for (int v : iters) r.mean_iter += (double)v / (double)iters.size();
        for (const auto code : codes) r.not_optimal += (int)code == EICOS_OPTIMAL ? 0 : 1;
        r.u = std::move(u);
        return r;
    };
    try {
        const double tols[3] = {1e-8, 1e-6, 1e-4};
        const char *name[3] = {"cold", "warm", "warm + shift"};
        std::vector<Result> tight; // the three runs at 1e-8: what the looser ones are compared with
        for (int ti = 0; ti < 3; ti++) {
            std::vector<Result> res;
            res.push_back(run(tols[ti], 0., false)); res.push_back(run(tols[ti], 0.1, false)); res.push_back(run(tols[ti], 0.1, true));
            if (ti == 0) {
                std::printf("linear MPC, nx = %d, nu = %d, horizon %d: n = %d, m = %d, p = %d; batch %d over %d shard(s), %d closed-loop steps, %d launch(es) per rollout and shard\n",
                            NX, NU, N, n, m, p, B, res[0].shards, T, res[0].launches);
                tight = res;
            }
            for (int q = 0; q < 3; q++) {
                double du = 0.;
                for (size_t j = 0; j < res[q].u.size(); j++) du = std::max(du, std::fabs(res[q].u[j] - tight[q].u[j]));
                std::printf("tol %.0e %-12s: mean iterations per step %.2f, rollout %.3f ms, %d of %d solves not optimal, max |u - u(1e-8)| %.3e\n",
                            tols[ti], name[q], res[q].mean_iter, res[q].ms, res[q].not_optimal, res[q].solves, du);
            }
        }
    } catch (const std::exception &e) {
        std::fprintf(stderr, "mpc_tolerance_demo: %s\n", e.what());
        return 1;
    }
    return 0;
}
