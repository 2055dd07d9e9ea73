// The fallback map from host C++ (no torch): the capped, warm-started closed loop of inlaunch_retry_demo.cpp -- the stage-ordered linear
// MPC with a shift map under an iteration cap low enough that some steps stop at it -- and what the plant gets from those steps, four ways,
// each ONE rollout launch:
//   (a) no policy: a step that stops at the cap hands the output map of its unfinished x to the plant;
//   (b) the fallback map alone (EiCOS::BatchSolver::setFallbackMap, mask sel_not_optimal): such a step applies u = K theta instead, a fixed
//       PD gain on the measured state, u_i = -(KP pos_i + KD vel_i) -- no second solve;
//   (c) the retry policy alone: the step is solved once more, cold, under a cap of its own (a real-time budget: cap + RETRY_EXTRA passes);
//   (d) both: the retry first, and the fallback law for the steps that fail twice.
// Prints the rollout time, the steps that did not end optimal, the retried and the fired steps, and the closed-loop cost
// sum_t |theta_t|^2 + |u_t|^2 over the batch.
//
// The problem: dynamics x+ = A x + B u (two double integrators: nx = 4 states, nu = 2 inputs), horizon N, stage cost |x|_1 + rho |u|_1
// through epigraph variables, a box |u| <= umax; variables stage by stage, stage t = [u_t (nu) | x_{t+1} (nx) | e_t (nx) | f_t (nu)];
// the parameter map b = b0 + Bm theta (theta = x_0), the output map u = u_0, the plant map theta+ = A theta + B u + w.
//   g++ -std=c++17 -Iinclude examples/fallback_demo.cpp -Leicos_amd -leicos_amd -Wl,-rpath,$PWD/eicos_amd -o fallback_demo
//   ./fallback_demo [batch = 1024] [N = 20] [T = 20] [cap = 0: chosen from an uncapped run]
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
constexpr int NX = 4, NU = 2, RETRY_EXTRA = 2;
constexpr double DT = 0.5, RHO = 0.1, UMAX = 1.0, KP = 0.4, KD = 0.9;
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

struct Result { double ms, cost; int not_optimal, retried, fired, steps; std::vector<int> iters; };
} // namespace

int main(int argc, char **argv) {
    const int B = argc > 1 ? std::atoi(argv[1]) : 1024, N = argc > 2 ? std::atoi(argv[2]) : 20, T = argc > 3 ? std::atoi(argv[3]) : 20;
    int cap = argc > 4 ? std::atoi(argv[4]) : 0;
    if (B < 1 || N < 2 || T < 1 || cap < 0 || cap > 100 - RETRY_EXTRA) { std::fprintf(stderr, "usage: fallback_demo [batch] [N >= 2] [T >= 1] [cap in 1 .. %d]\n", 100 - RETRY_EXTRA); return 2; }
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
    // ---- the maps: theta = x_0 enters b of stage 0 as A theta; u = u_0; theta+ = A theta + B u (+ w); the shift by one stage; the
    // fallback law u_i = -(KP theta[2 i] + KD theta[2 i + 1])
    Affine bmap(p), omap(NU), plant(NX), law(NU);
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
    for (int i = 0; i < NU; i++) {
        law.col.push_back(2 * i); law.val.push_back(-KP);
        law.col.push_back(2 * i + 1); law.val.push_back(-KD);
        law.row_done();
    }
    const Affine sx = shift_by(n, S), sy = shift_by(p, NX), sz = shift_by(m, MS);
    const eicos_affine_map vb = bmap.view(), vo = omap.view(), vf = plant.view(), vx = sx.view(), vy = sy.view(), vz = sz.view(), vk = law.view();
    // ---- the batch: the same model, different measured states and disturbances
    unsigned long long st = 88172645463325252ull;
    auto rnd = [&] { st = st * 6364136223846793005ull + 1442695040888963407ull; return (double)((st >> 11) & 0xFFFFFFFFFFFFull) / (double)(1ull << 48); };
    std::vector<double> theta0((size_t)B * NX), w((size_t)B * T * NX);
    for (int i = 0; i < B; i++)
        for (int j = 0; j < NX; j++) theta0[(size_t)i * NX + j] = (j % 2 == 0 ? 2.0 : 0.5) * (2 * rnd() - 1);
    for (double &v : w) v = 0.01 * (2 * rnd() - 1);
    auto rep = [&](const std::vector<double> &row) { std::vector<double> out; out.reserve(row.size() * B); for (int i = 0; i < B; i++) out.insert(out.end(), row.begin(), row.end()); return out; };
    const std::vector<double> Gb = rep(G.pr), Ab = rep(A.pr), cb = rep(c), hb = rep(h), bb = rep(b);

    auto capped = [&](int iter_max) { EiCOS::Settings s; s.iter_max = (size_t)iter_max; return s; };
    // one rollout launch of a fresh solver -- the same data, one cold solve at theta0 (what the first warm step starts from), warm start and
    // shift map on -- under `iter_max` (0: the defaults), with or without the retry policy and the fallback map
    auto rollout = [&](int iter_max, bool with_retry, bool with_fallback) -> Result {
        EiCOS::BatchSolver solver(n, m, p, 0, nullptr, G.jc.data(), G.ir.data(), A.jc.data(), A.ir.data(), B, std::vector<int>{0});
        solver.updateData(Gb.data(), Ab.data(), cb.data(), hb.data(), bb.data());
        solver.setParamMap(NX, nullptr, nullptr, &vb);
        solver.setOutputMap(NU, &vo);
        solver.setPlantMap(&vf);
        solver.updateParam(theta0.data());
        solver.solve();
        solver.setWarmStart(0.1);
        EiCOS::ShiftMap sm;
        sm.x = &vx; sm.y = &vy; sm.z = &vz; sm.s = &vz;
        solver.setShiftMap(sm);
        if (iter_max) solver.setSettings(capped(iter_max));
        if (with_retry) {
            EiCOS::Retry policy; // cold, no regularisation, the defaults under a cap of its own
            policy.mask = EiCOS::sel_not_optimal;
            policy.settings.iter_max = (size_t)(iter_max + RETRY_EXTRA);
            solver.setRetry(policy);
        }
        if (with_fallback) solver.setFallbackMap(EICOS_SEL_NOT_OPTIMAL, &vk);
        std::vector<double> u((size_t)B * T * NU), theta((size_t)B * (T + 1) * NX);
        Result r{0., 0., 0, 0, 0, B * T, std::vector<int>((size_t)B * T)};
        const auto t0 = std::chrono::steady_clock::now();
        const auto codes = solver.rollout(T, theta0.data(), u.data(), w.data(), theta.data(), r.iters.data());
        r.ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        for (const auto code : codes) r.not_optimal += (int)code == EICOS_OPTIMAL ? 0 : 1;
        for (int v : solver.retryCounts()) r.retried += v;
        for (int v : solver.fallbackCounts()) r.fired += v;
        for (int i = 0; i < B; i++)
            for (int t = 0; t < T; t++) {
                for (int j = 0; j < NX; j++) { const double v = theta[((size_t)i * (T + 1) + t) * NX + j]; r.cost += v * v; }
                for (int j = 0; j < NU; j++) { const double v = u[((size_t)i * T + t) * NU + j]; r.cost += v * v; }
            }
        if (eicos_batch_last_rollout_launches(solver.handle()) != 1) std::printf("(the rollout took %d launches)\n", eicos_batch_last_rollout_launches(solver.handle()));
        return r;
    };
    try {
        if (cap == 0) { // a cap that about a tenth of the uncapped steps exceed
            Result free_run = rollout(0, false, false);
            std::vector<int> sorted = free_run.iters;
            std::sort(sorted.begin(), sorted.end());
            cap = sorted[(size_t)(0.9 * (double)(sorted.size() - 1))];
            if (cap >= sorted.back()) cap = sorted.back() - 1;
            if (cap < 1) cap = 1;
            std::printf("uncapped: iterations per step %d .. %d, rollout %.3f ms, %d of %d steps not optimal, closed-loop cost %.6g -> cap %d\n", sorted.front(),
                        sorted.back(), free_run.ms, free_run.not_optimal, free_run.steps, free_run.cost, cap);
        }
        std::printf("linear MPC, nx = %d, nu = %d, horizon %d: n = %d, m = %d, p = %d; batch %d, %d closed-loop steps, warm start + shift map, iteration cap %d\n",
                    NX, NU, N, n, m, p, B, T, cap);
        std::printf("fallback law u_i = -(%.2f pos_i + %.2f vel_i) for steps that do not end optimal; the retry runs cold under a cap of %d\n", KP, KD, cap + RETRY_EXTRA);
        const char *name[4] = {"(a) no policy           ", "(b) fallback alone      ", "(c) retry alone         ", "(d) retry, then fallback"};
        for (int q = 0; q < 4; q++) {
            const Result r = rollout(cap, q >= 2, q == 1 || q == 3);
            std::printf("%s: %6d of %d steps not optimal, %6d retried, %6d fired, %9.3f ms, closed-loop cost %.6g\n", name[q], r.not_optimal, r.steps,
                        r.retried, r.fired, r.ms, r.cost);
        }
    } catch (const std::exception &e) {
        std::fprintf(stderr, "fallback_demo: %s\n", e.what());
        return 1;
    }
    return 0;
}
