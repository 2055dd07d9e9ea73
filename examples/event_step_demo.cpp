// An event-triggered fleet from host C++ (no torch): a batch of controllers of which, in every step, only those whose sample time fired
// get a new parameter row theta and are solved again; the others keep their state.  The maps are those of param_update_demo.cpp
// (c, h, b affine in k = 16 numbers; u = the first r = 4 variables through a small output map).  In each step a different eighth of the
// batch fires, and the step runs three ways side by side, each on its own solver from the same data in the same order:
//   (a) stepParamSubset: ONE call, pinned theta rows in, pinned u rows out;
//   (b) the three indexed calls: updateParam(indices, theta) + solveSubset(indices) + outputs(indices, u);
//   (c) what a caller had before the indexed calls: one updateParam(theta row, first = id, count = 1) per fired controller,
//       solveSubset(indices), gather(indices, x) and the output map evaluated on the host.
// u must be equal bit for bit on all three; the program prints the median step time of 20 steps (call -> u on the host) and the bytes per
// fired instance each way (the theta row and the 4-byte id for every call that takes the list in; the u row, or the x row, out).
//   g++ -std=c++17 -Iinclude examples/event_step_demo.cpp -Leicos_amd -leicos_amd -Wl,-rpath,$PWD/eicos_amd -o event_step_demo
//   ./event_step_demo tests/golden/MPC02.epb [batch = 1024] [dev[,dev...] = 0] [steps = 20]
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <sstream>
#include <vector>

#include "eicos.hpp"

// the host restatement of the output map must not fuse the product into the sum
#if defined(__clang__)
#pragma clang fp contract(off)
#elif defined(__GNUC__)
#pragma GCC optimize("fp-contract=off")
#endif

struct Group { // one group of a map: base vector + CSR matrix
    std::vector<double> base, val;
    std::vector<int> rowptr, col;
    eicos_affine_map view() const { return {base.data(), rowptr.data(), col.data(), val.data()}; }
    // out[i][r] = base[r] + sum over the row's entries, in stored order, of val * v[i][col]
    void evaluate(const std::vector<double> &v, int width, int count, std::vector<double> &out) const {
        const size_t rows = base.size();
        out.resize((size_t)count * rows);
        for (int i = 0; i < count; i++)
            for (size_t r = 0; r < rows; r++) {
                double acc = base[r];
                for (int t = rowptr[r]; t < rowptr[r + 1]; t++) { const double prod = val[t] * v[(size_t)i * width + col[t]]; acc = acc + prod; }
                out[(size_t)i * rows + r] = acc;
            }
    }
};

// 0 - 4 entries per row (some rows empty), values about 1e-3 of the base
static Group make_group(const double *base, int rows, int k, unsigned seed) {
    Group g;
    unsigned long long st = seed * 2654435761ull + 99991;
    auto rnd = [&] { st = st * 6364136223846793005ull + 1442695040888963407ull; return (double)((st >> 11) & 0xFFFFFFFFFFFFull) / (double)(1ull << 48); };
    g.base.assign(base, base + rows);
    g.rowptr.assign(1, 0);
    for (int r = 0; r < rows; r++) {
        const int len = std::min(k, (int)(rnd() * 5));
        const int c0 = (int)(rnd() * k);
        for (int j = 0; j < len; j++) { g.col.push_back((c0 + j) % k); g.val.push_back(1e-3 * (1 + std::fabs(base[r])) * (2 * rnd() - 1)); }
        g.rowptr.push_back((int)g.col.size());
    }
    return g;
}

int main(int argc, char **argv) {
    if (argc < 2) { std::fprintf(stderr, "usage: %s problem.epb [batch] [dev[,dev...]] [steps]\n", argv[0]); return 2; }
    std::ifstream f(argv[1], std::ios::binary);
    std::vector<char> raw((std::istreambuf_iterator<char>(f)), {});
    if (raw.size() < 36 || std::memcmp(raw.data(), "EPB1", 4)) { std::fprintf(stderr, "not an EPB1 file\n"); return 2; }
    const int B = argc > 2 ? std::atoi(argv[2]) : 1024;
    std::vector<int> devs;
    { std::stringstream ss(argc > 3 ? argv[3] : "0"); std::string tok; while (std::getline(ss, tok, ',')) devs.push_back(std::atoi(tok.c_str())); }
    const int steps = argc > 4 ? std::atoi(argv[4]) : 20, k = 16, PARTS = 8;
    if (B < PARTS || steps < 1 || devs.empty()) { std::fprintf(stderr, "need batch >= %d, steps >= 1 and a device\n", PARTS); return 2; }
    const int *hd = reinterpret_cast<const int *>(raw.data() + 4);
    const int n = hd[0], m = hd[1], p = hd[2], nc = hd[4], nnzG = hd[5], nnzA = hd[6];
    const int *ip = hd + 8;
    std::vector<int> q(ip, ip + nc); ip += nc;
    std::vector<int> Gjc(ip, ip + n + 1); ip += n + 1;
    std::vector<int> Gir(ip, ip + nnzG); ip += nnzG;
    std::vector<int> Ajc(ip, ip + n + 1); ip += n + 1;
    std::vector<int> Air(ip, ip + nnzA); ip += nnzA;
    const double *dp = reinterpret_cast<const double *>(ip);
    const double *Gpr = dp, *Apr = Gpr + nnzG, *c = Apr + nnzA, *h = c + n, *b = h + m;
    std::vector<double> G((size_t)B * nnzG), A((size_t)B * nnzA), C0((size_t)B * n), H0((size_t)B * m), B0((size_t)B * p);
    for (int i = 0; i < B; i++) {
        std::copy(Gpr, Gpr + nnzG, G.begin() + (size_t)i * nnzG);
        std::copy(Apr, Apr + nnzA, A.begin() + (size_t)i * nnzA);
        std::copy(c, c + n, C0.begin() + (size_t)i * n);
        std::copy(h, h + m, H0.begin() + (size_t)i * m);
        std::copy(b, b + p, B0.begin() + (size_t)i * p);
    }
    const Group gc = make_group(c, n, k, 1), gh = make_group(h, m, k, 2), gb = make_group(b, p, k, 3);
    const eicos_affine_map mc = gc.view(), mh = gh.view(), mb = gb.view();
    const int R = std::min(4, n);
    Group go; // the first R variables, un-scaled (row j = u0[j] + a * x[j] + b * x[j + 1]; the last row has one entry)
    go.rowptr.assign(1, 0);
    for (int j = 0; j < R; j++) {
        go.base.push_back(0.25 * j - 0.5);
        go.col.push_back(j); go.val.push_back(1.5 + 0.125 * j);
        if (j + 1 < R) { go.col.push_back(j + 1); go.val.push_back(-1. / 3.); }
        go.rowptr.push_back((int)go.col.size());
    }
    const eicos_affine_map mo = go.view();
    auto make = [&] {
        auto *s = new EiCOS::BatchSolver(n, m, p, nc, q.data(), m ? Gjc.data() : nullptr, m ? Gir.data() : nullptr, p ? Ajc.data() : nullptr,
                                         p ? Air.data() : nullptr, B, devs);
        s->updateData(m ? G.data() : nullptr, p ? A.data() : nullptr, C0.data(), m ? H0.data() : nullptr, p ? B0.data() : nullptr);
        s->setParamMap(k, &mc, m ? &mh : nullptr, p ? &mb : nullptr);
        s->setOutputMap(R, &mo);
        s->setWarmStart(0.1);
        s->solve();
        return s;
    };
    // the controllers that fire in step s: every PARTS-th one, starting at s mod PARTS, in descending order (a list need not be sorted)
    auto fired = [&](int s) {
        std::vector<int> ids;
        for (int i = B - 1; i >= 0; i--) if (i % PARTS == s % PARTS) ids.push_back(i);
        return ids;
    };
    auto theta_of = [&](int s, const std::vector<int> &ids) {
        std::vector<double> th(ids.size() * (size_t)k);
        for (size_t r = 0; r < ids.size(); r++)
            for (int j = 0; j < k; j++) th[r * k + j] = 0.5 + 0.4 * std::sin(0.05 * s + 0.01 * ids[r] + j);
        return th;
    };
    auto same = [&](const std::vector<double> &x, const std::vector<double> &y) { return x.size() == y.size() && std::memcmp(x.data(), y.data(), x.size() * sizeof(double)) == 0; };
    auto now = [] { return std::chrono::steady_clock::now(); };
    auto ms = [](std::chrono::steady_clock::time_point t0, std::chrono::steady_clock::time_point t1) { return std::chrono::duration<double, std::milli>(t1 - t0).count(); };

    EiCOS::BatchSolver *sa = make(), *sb = make(), *sc = make();
    const size_t most = (size_t)(B + PARTS - 1) / PARTS;
    double *pth = EiCOS::BatchSolver::hostAlloc(most * k), *pu = EiCOS::BatchSolver::hostAlloc(most * R);
    std::vector<double> ta, tb, tc, ua, ub, uc, xc;
    bool same_u = true, same_codes = true;
    size_t count = 0;
    for (int st = 0; st < steps + 2; st++) { // (the first two steps warm the paths up and are not timed)
        const std::vector<int> ids = fired(st);
        const std::vector<double> th = theta_of(st, ids);
        count = ids.size();
        std::copy(th.begin(), th.end(), pth);
        auto t0 = now();
        const std::vector<EiCOS::exitcode> ca = sa->stepParamSubset(ids, pth, pu);
        auto t1 = now();
        ua.assign(pu, pu + count * R);
        ub.assign(count * R, 0.);
        auto t2 = now();
        sb->updateParam(ids, th.data());
        const std::vector<EiCOS::exitcode> cb = sb->solveSubset(ids);
        sb->outputs(ids, ub.data());
        auto t3 = now();
        xc.assign(count * n, 0.);
        auto t4 = now();
        for (size_t r = 0; r < count; r++) sc->updateParam(th.data() + r * k, ids[r], 1);
        const std::vector<EiCOS::exitcode> cc = sc->solveSubset(ids);
        sc->gather(ids, xc.data());
        go.evaluate(xc, n, (int)count, uc);
        auto t5 = now();
        same_u = same_u && same(ua, ub) && same(ua, uc);
        same_codes = same_codes && ca == cb && ca == cc;
        if (st >= 2) { ta.push_back(ms(t0, t1)); tb.push_back(ms(t2, t3)); tc.push_back(ms(t4, t5)); }
    }
    const bool same_x = same(sa->solution(), sb->solution()) && same(sa->solution(), sc->solution());
    delete sa; delete sb; delete sc;
    EiCOS::BatchSolver::hostFree(pth); EiCOS::BatchSolver::hostFree(pu);
    auto median = [](std::vector<double> v) { std::sort(v.begin(), v.end()); return v.empty() ? 0. : 0.5 * (v[(v.size() - 1) / 2] + v[v.size() / 2]); };
    std::printf("u of the three forms, every step: %s; exit codes: %s; the whole batch's x after the loop: %s\n", same_u ? "bit-identical" : "DIFFERENT",
                same_codes ? "equal" : "DIFFERENT", same_x ? "bit-identical" : "DIFFERENT");
    std::printf("event-triggered step, batch %d of which %zu fire per step, k = %d, r = %d, %zu shard(s), median of %d steps; bytes per fired instance in / out:\n",
                B, count, k, R, devs.size(), steps);
    std::printf("  (a) stepParamSubset (pinned theta, pinned u)              %8.3f ms  %6d B in  %6d B out\n", median(ta), 8 * k + 4, 8 * R);
    std::printf("  (b) updateParam + solveSubset + outputs over the list     %8.3f ms  %6d B in  %6d B out\n", median(tb), 8 * k + 3 * 4, 8 * R);
    std::printf("  (c) %4zu x updateParam(count = 1) + solveSubset + gather   %8.3f ms  %6d B in  %6d B out  (+ the output map on the host)\n", count,
                median(tc), 8 * k + 2 * 4, 8 * n);
    return (same_u && same_codes && same_x) ? 0 : 1; // (bit-identity is the contract: it holds for every exit code)
}
