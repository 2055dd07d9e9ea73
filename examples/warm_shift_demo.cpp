// The receding-horizon warm start from host C++ (no torch): a small stage-ordered linear MPC written here, run as a closed loop on the
// GPU three ways -- every step solved cold, every step warm-started from the previous step's solution as it lies, and warm-started from
// that solution moved one stage forward by a shift map (EiCOS::BatchSolver::setShiftMap), which the solve kernel applies itself.
//
// The problem: dynamics x+ = A x + B u (two double integrators: nx = 4 states, nu = 2 inputs), horizon N, stage cost |x|_1 + rho |u|_1
// through epigraph variables, a box |u| <= umax.  Variables stage by stage, stage t = [u_t (nu) | x_{t+1} (nx) | e_t (nx) | f_t (nu)]:
//     minimise    sum_t 1'e_t + rho 1'f_t
//     subject to  x_{t+1} - A x_t - B u_t = 0   (x_0 = theta, the measured state: it enters b of stage 0 as A theta)
//                 +-x_{t+1} <= e_t,  +-u_t <= f_t,  +-u_t <= umax
// so that equality rows, inequality rows and variables of stage t + 1 sit one stage length behind those of stage t, and the standard
// MPC shift is a pure copy: entry j of x, y, z, s takes entry j + (stage length), the last stage keeps its own.
// The closed loop: the parameter map b = b0 + Bm theta (theta = x_0, k = nx), the output map u = u_0 (r = nu), the plant map
// theta+ = A theta + B u + w -- rollout() then runs T steps of every instance in one call.  Each of the three runs takes a fresh solver
// through the same data, the same theta0 and the same disturbance, and prints the mean iteration count per step and the rollout time.
//   g++ -std=c++17 -Iinclude examples/warm_shift_demo.cpp -Leicos_amd -leicos_amd -Wl,-rpath,$PWD/eicos_amd -o warm_shift_demo
//   ./warm_shift_demo [batch = 1024] [N = 20] [T = 20] [devices = 0]        (a device may be listed twice: 0,0)
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

struct Result { double mean_iter, ms; int optimal, solves, launches, shards; };
} // namespace

int main(int argc, char **argv) {
    const int B = argc > 1 ? std::atoi(argv[1]) : 1024, N = argc > 2 ? std::atoi(argv[2]) : 20, T = argc > 3 ? std::atoi(argv[3]) : 20;
    std::vector<int> devices;
    {
        std::stringstream ss(argc > 4 ? argv[4] : "0");
        for (std::string tok; std::getline(ss, tok, ',');) devices.push_back(std::atoi(tok.c_str()));
    }
    if (B < (int)devices.size() || N < 2 || T < 1) { std::fprintf(stderr, "usage: warm_shift_demo [batch] [N >= 2] [T >= 1] [devices]\n"); return 2; }
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

    auto run = [&](double warm, bool shift) -> Result {
        EiCOS::BatchSolver solver(n, m, p, 0, nullptr, G.jc.data(), G.ir.data(), A.jc.data(), A.ir.data(), B, devices);
        solver.updateData(Gb.data(), Ab.data(), cb.data(), hb.data(), bb.data());
        solver.setParamMap(NX, nullptr, nullptr, &vb);
        solver.setOutputMap(NU, &vo);
        solver.setPlantMap(&vf);
        solver.updateParam(theta0.data());
        solver.solve(); // (the solution a first warm step starts from; not timed, not counted)
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
        Result r{0., ms, 0, B * T, eicos_batch_last_rollout_launches(solver.handle()), solver.num_shards()};
        for (int v : iters) r.mean_iter += (double)v / (double)iters.size();
        for (const auto code : codes) r.optimal += (int)code == EICOS_OPTIMAL ? 1 : 0;
        return r;
    };
    try {
        const Result cold = run(0., false), warm = run(0.1, false), shifted = run(0.1, true);
        std::printf("linear MPC, nx = %d, nu = %d, horizon %d: n = %d, m = %d, p = %d; batch %d over %d shard(s), %d closed-loop steps, %d launch(es) per rollout and shard\n",
                    NX, NU, N, n, m, p, B, cold.shards, T, cold.launches);
        const char *name[3] = {"cold", "warm", "warm + shift"};
        const Result *res[3] = {&cold, &warm, &shifted};
        for (int q = 0; q < 3; q++)
            std::printf("%-12s: mean iterations per step %.2f, rollout %.3f ms, %d of %d solves optimal\n", name[q], res[q]->mean_iter, res[q]->ms,
                        res[q]->optimal, res[q]->solves);
    } catch (const std::exception &e) {
        std::fprintf(stderr, "warm_shift_demo: %s\n", e.what());
        return 1;
    }
    return 0;
}
