// Parametric right-hand-side updates from host C++ (no torch): in an MPC loop c, h and b are affine in a few numbers (the measured state,
// a reference, some bounds).  EiCOS::BatchSolver::setParamMap installs c = c0 + C theta, h = h0 + H theta, b = b0 + B theta once;
// updateParam then sends k doubles per instance and the GPU expands them -- the result must equal, bit for bit, updateRHS of the vectors
// evaluated on the host in the same order (every product and every sum rounded on its own).  Runs over a device list (a device may be
// listed twice: 0,0), checks updateParam + solve and a sub-range against updateRHS, then runs a short closed loop with warm starts --
// theta moves a little every step -- in four forms side by side, each on its own solver, and prints the median step time (update call ->
// result on the host) and the bytes per instance each way of each: updateRHS from pageable host vectors + solve + solution, updateParam
// from a pageable theta + solve + outputs, updateRHSDevice from vectors already in device memory + solve + solution (that leg needs the
// HIP runtime's allocation calls, looked up at run time; "n/a" without them), and stepParam -- the whole step in one call, pinned theta in,
// the r selected outputs u = u0 + U x into a pinned array out.  stepParam's u must equal the output map applied to solution() bit for bit.
// Last, a rollout: setPlantMap installs theta+ = f0 + F [theta | u] and rollout() runs 20 closed-loop steps of every instance in one call;
// its u and theta trajectories must equal, bit for bit, those of 20 stepParam calls on pinned theta with the plant evaluated on the host,
// and the wall time of both is printed (median of 5).
// Then the matrix map: setMatrixMap installs Gpr = G0 + Gm theta, Apr = A0 + Am theta (about a fifth of the stored values move), and the
// same closed-loop step runs two ways -- solve(Gpr, Apr, c, h, b, x) on pinned arrays evaluated on the host (the evaluation timed on its
// own) and stepParam under the matrix map, where only theta travels and the solve kernel forms the arrays itself; x must be equal bit for
// bit, and the median step time of 20 steps and the bytes per instance each way are printed.
//   g++ -std=c++17 -Iinclude examples/param_update_demo.cpp -Leicos_amd -leicos_amd -Wl,-rpath,$PWD/eicos_amd -o param_update_demo
//   ./param_update_demo tests/golden/MPC02.epb 64 0,0 [k = 16] [steps = 20]
#include <dlfcn.h>

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

// the host restatement must not fuse the product into the sum
#if defined(__clang__)
#pragma clang fp contract(off)
#elif defined(__GNUC__)
#pragma GCC optimize("fp-contract=off")
#endif

struct Group { // one group of the map: base vector + CSR matrix with k columns
    std::vector<double> base, val;
    std::vector<int> rowptr, col;
    eicos_affine_map view() const { return {base.data(), rowptr.data(), col.data(), val.data()}; }
    // out[i][r] = base[r] + sum over the row's entries, in stored order, of val * theta[i][col]
    void evaluate(const std::vector<double> &theta, int k, int B, std::vector<double> &out) const {
        const size_t rows = base.size();
        out.resize((size_t)B * rows);
        for (int i = 0; i < B; i++)
            for (size_t r = 0; r < rows; r++) {
                double acc = base[r];
                for (int t = rowptr[r]; t < rowptr[r + 1]; t++) { const double prod = val[t] * theta[(size_t)i * k + col[t]]; acc = acc + prod; }
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

// a matrix of the matrix map: about 80 % of the stored values fixed (empty rows), the others with 1 - 3 entries of about 1e-3 of the base
static Group make_matrix_group(const double *base, int rows, int k, unsigned seed) {
    Group g;
    unsigned long long st = seed * 2654435761ull + 99991;
    auto rnd = [&] { st = st * 6364136223846793005ull + 1442695040888963407ull; return (double)((st >> 11) & 0xFFFFFFFFFFFFull) / (double)(1ull << 48); };
    g.base.assign(base, base + rows);
    g.rowptr.assign(1, 0);
    for (int r = 0; r < rows; r++) {
        const int len = rnd() < 0.8 ? 0 : std::min(k, 1 + (int)(rnd() * 3));
        const int c0 = (int)(rnd() * k);
        for (int j = 0; j < len; j++) { g.col.push_back((c0 + j) % k); g.val.push_back(1e-3 * (1 + std::fabs(base[r])) * (2 * rnd() - 1)); }
        g.rowptr.push_back((int)g.col.size());
    }
    return g;
}

int main(int argc, char **argv) {
    if (argc < 4) { std::fprintf(stderr, "usage: %s problem.epb batch dev[,dev...] [k] [steps]\n", argv[0]); return 2; }
    std::ifstream f(argv[1], std::ios::binary);
    std::vector<char> raw((std::istreambuf_iterator<char>(f)), {});
    if (raw.size() < 36 || std::memcmp(raw.data(), "EPB1", 4)) { std::fprintf(stderr, "not an EPB1 file\n"); return 2; }
    const int B = std::atoi(argv[2]);
    std::vector<int> devs;
    { std::stringstream ss(argv[3]); std::string tok; while (std::getline(ss, tok, ',')) devs.push_back(std::atoi(tok.c_str())); }
    const int k = argc > 4 ? std::atoi(argv[4]) : 16, steps = argc > 5 ? std::atoi(argv[5]) : 20;
    if (B < 4 || k < 1 || steps < 1) { std::fprintf(stderr, "need batch >= 4, k >= 1, steps >= 1\n"); return 2; }
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
    // the map (a group the pattern does not have is left out) and theta of step s: every instance its own slowly moving point in [0, 1]^k
    const Group gc = make_group(c, n, k, 1), gh = make_group(h, m, k, 2), gb = make_group(b, p, k, 3);
    const eicos_affine_map mc = gc.view(), mh = gh.view(), mb = gb.view();
    auto theta_of = [&](int s) {
        std::vector<double> th((size_t)B * k);
        for (int i = 0; i < B; i++)
            for (int j = 0; j < k; j++) th[(size_t)i * k + j] = 0.5 + 0.4 * std::sin(0.05 * s + 0.01 * i + j);
        return th;
    };
    auto vectors_of = [&](const std::vector<double> &th, std::vector<double> &C, std::vector<double> &H, std::vector<double> &Bv) {
        gc.evaluate(th, k, B, C); gh.evaluate(th, k, B, H); gb.evaluate(th, k, B, Bv);
    };
    auto make = [&] {
        auto *s = new EiCOS::BatchSolver(n, m, p, nc, q.data(), m ? Gjc.data() : nullptr, m ? Gir.data() : nullptr, p ? Ajc.data() : nullptr,
                                         p ? Air.data() : nullptr, B, devs);
        s->updateData(m ? G.data() : nullptr, p ? A.data() : nullptr, C0.data(), m ? H0.data() : nullptr, p ? B0.data() : nullptr);
        s->solve();
        return s;
    };
    auto same = [&](const std::vector<double> &x, const std::vector<double> &y) { return x.size() == y.size() && std::memcmp(x.data(), y.data(), x.size() * sizeof(double)) == 0; };

    // (1) updateParam + solve against updateRHS of the host-evaluated vectors
    std::vector<double> C, H, Bv;
    const std::vector<double> th0 = theta_of(0), th1 = theta_of(1);
    EiCOS::BatchSolver *ref = make(), *s = make();
    s->setParamMap(k, &mc, m ? &mh : nullptr, p ? &mb : nullptr);
    vectors_of(th0, C, H, Bv);
    ref->updateRHS(C.data(), m ? H.data() : nullptr, p ? Bv.data() : nullptr);
    const std::vector<EiCOS::exitcode> codes_ref = ref->solve();
    s->updateParam(th0.data());
    const bool same_all = s->solve() == codes_ref && same(ref->solution(), s->solution());
    int ok = 0;
    for (auto cd : codes_ref) ok += cd == EiCOS::exitcode::optimal;
    std::printf("%d / %d optimal over %zu shard(s)\n", ok, B, devs.size());
    std::printf("updateParam + solve vs updateRHS of the host-evaluated vectors: %s\n", same_all ? "bit-identical" : "DIFFERENT");
    // (2) a sub-range: instances [B/4, B/2) move on to step 1's theta
    const int first = B / 4, count = B / 2 - B / 4;
    vectors_of(th1, C, H, Bv);
    ref->updateRHS(C.data() + (size_t)first * n, m ? H.data() + (size_t)first * m : nullptr, p ? Bv.data() + (size_t)first * p : nullptr, first, count);
    s->updateParam(th1.data() + (size_t)first * k, first, count);
    const bool same_sub = ref->solve() == s->solve() && same(ref->solution(), s->solution());
    std::printf("sub-range updateParam: %s\n", same_sub ? "bit-identical" : "DIFFERENT");
    delete ref; delete s;

    // the output map: the first R variables, un-scaled (row j = u0[j] + a * x[j] + b * x[j + 1]; the last row has one entry)
    const int R = std::min(4, n);
    Group go;
    go.rowptr.assign(1, 0);
    for (int j = 0; j < R; j++) {
        go.base.push_back(0.25 * j - 0.5);
        go.col.push_back(j); go.val.push_back(1.5 + 0.125 * j);
        if (j + 1 < R) { go.col.push_back(j + 1); go.val.push_back(-1. / 3.); }
        go.rowptr.push_back((int)go.col.size());
    }
    const eicos_affine_map mo = go.view();

    // (3) closed loop with warm starts, four forms side by side (each on its own solver, the same data in the same order)
    typedef int (*malloc_fn)(void **, size_t);
    typedef int (*memcpy_fn)(void *, const void *, size_t, int);
    typedef int (*free_fn)(void *);
    typedef int (*setdev_fn)(int);
    const malloc_fn dmalloc = (malloc_fn)dlsym(RTLD_DEFAULT, "hipMalloc");
    const memcpy_fn dmemcpy = (memcpy_fn)dlsym(RTLD_DEFAULT, "hipMemcpy");
    const free_fn dfree = (free_fn)dlsym(RTLD_DEFAULT, "hipFree");
    const setdev_fn dsetdev = (setdev_fn)dlsym(RTLD_DEFAULT, "hipSetDevice");
    EiCOS::BatchSolver *sa = make(), *sb = make(), *sc = nullptr, *sd = make();
    double *dC = nullptr, *dH = nullptr, *dB = nullptr;
    if (dmalloc && dmemcpy && dfree && dsetdev && dsetdev(devs[0]) == 0 && dmalloc((void **)&dC, C0.size() * 8 + 8) == 0 &&
        dmalloc((void **)&dH, H0.size() * 8 + 8) == 0 && dmalloc((void **)&dB, B0.size() * 8 + 8) == 0)
        sc = make();
    for (EiCOS::BatchSolver *v : {sb, sd}) { v->setParamMap(k, &mc, m ? &mh : nullptr, p ? &mb : nullptr); v->setOutputMap(R, &mo); }
    for (EiCOS::BatchSolver *v : {sa, sb, sc, sd}) if (v) v->setWarmStart(0.1);
    double *pth = EiCOS::BatchSolver::hostAlloc((size_t)B * k), *pu = EiCOS::BatchSolver::hostAlloc((size_t)B * R); // stepParam: pinned both ways
    std::vector<double> ta, tb, tc, td, xa((size_t)B * n), xc((size_t)B * n), ub((size_t)B * R), ud, uwant;
    bool same_loop = true, same_u = true;
    auto now = [] { return std::chrono::steady_clock::now(); };
    auto ms = [](std::chrono::steady_clock::time_point t0, std::chrono::steady_clock::time_point t1) { return std::chrono::duration<double, std::milli>(t1 - t0).count(); };
    for (int st = 0; st < steps + 2; st++) { // (the first two steps warm the paths up and are not timed)
        const std::vector<double> th = theta_of(st + 2);
        vectors_of(th, C, H, Bv);
        auto t0 = now();
        sa->updateRHS(C.data(), m ? H.data() : nullptr, p ? Bv.data() : nullptr);
        const std::vector<EiCOS::exitcode> ca = sa->solve();
        sa->solution(xa.data());
        auto t1 = now();
        sb->updateParam(th.data());
        const std::vector<EiCOS::exitcode> cb = sb->solve();
        sb->outputs(ub.data());
        auto t2 = now();
        same_loop = same_loop && ca == cb && same(xa, sb->solution());
        std::copy(th.begin(), th.end(), pth);
        auto t5 = now();
        const std::vector<EiCOS::exitcode> cd = sd->stepParam(pth, pu);
        auto t6 = now();
        ud.assign(pu, pu + (size_t)B * R);
        go.evaluate(xa, n, B, uwant); // (the map applied to solution(), on the host in the stated order)
        same_loop = same_loop && ca == cd && same(xa, sd->solution());
        same_u = same_u && same(ud, uwant) && same(ub, uwant);
        if (st >= 2) td.push_back(ms(t5, t6));
        if (st >= 2) { ta.push_back(ms(t0, t1)); tb.push_back(ms(t1, t2)); }
        if (sc) {
            dmemcpy(dC, C.data(), C.size() * 8, 1); dmemcpy(dH, H.data(), H.size() * 8, 1); dmemcpy(dB, Bv.data(), Bv.size() * 8, 1); // (host to device)
            auto t3 = now();
            sc->updateRHSDevice(devs[0], dC, m ? dH : nullptr, p ? dB : nullptr);
            const std::vector<EiCOS::exitcode> cc = sc->solve();
            sc->solution(xc.data());
            auto t4 = now();
            same_loop = same_loop && ca == cc && same(xa, xc);
            if (st >= 2) tc.push_back(ms(t3, t4));
        }
    }
    // (4) the rollout: T = 20 steps in one call against 20 stepParam calls with the plant on the host, the same solver state on both sides
    const int T = 20, REPS = 5;
    Group gf; // row j: theta+[j] = 0.05 + 0.9 theta[j] + 1e-3 u[j mod R] (the first row also a second theta entry, stored after the u entry)
    gf.rowptr.assign(1, 0);
    for (int j = 0; j < k; j++) {
        gf.base.push_back(0.05);
        gf.col.push_back(j); gf.val.push_back(0.9);
        gf.col.push_back(k + j % R); gf.val.push_back(1e-3);
        if (j == 0 && k > 1) { gf.col.push_back(k - 1); gf.val.push_back(-0.01); }
        gf.rowptr.push_back((int)gf.col.size());
    }
    const eicos_affine_map mf = gf.view();
    EiCOS::BatchSolver *se = make(), *sf = make();
    for (EiCOS::BatchSolver *v : {se, sf}) { v->setParamMap(k, &mc, m ? &mh : nullptr, p ? &mb : nullptr); v->setOutputMap(R, &mo); v->setWarmStart(0.1); }
    se->setPlantMap(&mf);
    std::vector<double> ut((size_t)B * T * R), tt((size_t)B * (T + 1) * k), ut_ref(ut.size()), tt_ref(tt.size()), z((size_t)B * (k + R)), nxt;
    std::vector<double> tr, tl;
    bool same_roll = true;
    for (int rep = 0; rep < REPS + 1; rep++) { // (the first repetition warms the paths up and is not timed)
        const std::vector<double> th = theta_of(rep);
        auto t0 = now();
        const std::vector<EiCOS::exitcode> ce = se->rollout(T, th.data(), ut.data(), nullptr, tt.data());
        auto t1 = now();
        std::copy(th.begin(), th.end(), pth);
        std::vector<EiCOS::exitcode> cf((size_t)B * T);
        for (int t = 0; t < T; t++) {
            for (int i = 0; i < B; i++) std::copy(pth + (size_t)i * k, pth + (size_t)(i + 1) * k, tt_ref.begin() + ((size_t)i * (T + 1) + t) * k);
            const std::vector<EiCOS::exitcode> cd = sf->stepParam(pth, pu);
            for (int i = 0; i < B; i++) {
                cf[(size_t)i * T + t] = cd[i];
                std::copy(pu + (size_t)i * R, pu + (size_t)(i + 1) * R, ut_ref.begin() + ((size_t)i * T + t) * R);
                std::copy(pth + (size_t)i * k, pth + (size_t)(i + 1) * k, z.begin() + (size_t)i * (k + R));
                std::copy(pu + (size_t)i * R, pu + (size_t)(i + 1) * R, z.begin() + (size_t)i * (k + R) + k);
            }
            gf.evaluate(z, k + R, B, nxt); // (the plant on the host, in the stated order)
            std::copy(nxt.begin(), nxt.end(), pth);
        }
        for (int i = 0; i < B; i++) std::copy(pth + (size_t)i * k, pth + (size_t)(i + 1) * k, tt_ref.begin() + ((size_t)i * (T + 1) + T) * k);
        auto t2 = now();
        same_roll = same_roll && ce == cf && same(ut, ut_ref) && same(tt, tt_ref) && same(se->solution(), sf->solution());
        if (rep >= 1) { tr.push_back(ms(t0, t1)); tl.push_back(ms(t1, t2)); }
    }
    delete se; delete sf;
    // (5) the matrix map: the same step from pinned host-evaluated full arrays and from theta alone
    const Group gG = make_matrix_group(Gpr, nnzG, k, 4), gA = make_matrix_group(Apr, nnzA, k, 5);
    const eicos_affine_map mG = gG.view(), mA = gA.view();
    EiCOS::BatchSolver *sg = make(), *sm = make();
    for (EiCOS::BatchSolver *v : {sg, sm}) v->setWarmStart(0.1);
    sm->setParamMap(k, &mc, m ? &mh : nullptr, p ? &mb : nullptr); sm->setOutputMap(R, &mo);
    EiCOS::MatrixMap mm;
    mm.G = nnzG ? &mG : nullptr; mm.A = nnzA ? &mA : nullptr;
    sm->setMatrixMap(mm);
    double *pG = EiCOS::BatchSolver::hostAlloc((size_t)B * nnzG), *pA = EiCOS::BatchSolver::hostAlloc((size_t)B * nnzA), *pC = EiCOS::BatchSolver::hostAlloc((size_t)B * n),
           *pH = EiCOS::BatchSolver::hostAlloc((size_t)B * m), *pB = EiCOS::BatchSolver::hostAlloc((size_t)B * p), *px = EiCOS::BatchSolver::hostAlloc((size_t)B * n);
    std::vector<double> Gt, At, te, tg, tm, xg((size_t)B * n);
    bool same_mat = true;
    for (int st = 0; st < steps + 2; st++) { // (the first two steps warm the paths up and are not timed)
        const std::vector<double> th = theta_of(st + 2);
        auto t0 = now();
        gG.evaluate(th, k, B, Gt); gA.evaluate(th, k, B, At); vectors_of(th, C, H, Bv);
        std::copy(Gt.begin(), Gt.end(), pG); std::copy(At.begin(), At.end(), pA); std::copy(C.begin(), C.end(), pC);
        std::copy(H.begin(), H.end(), pH); std::copy(Bv.begin(), Bv.end(), pB);
        auto t1 = now();
        const std::vector<EiCOS::exitcode> cg = sg->solve(nnzG ? pG : nullptr, nnzA ? pA : nullptr, pC, nnzG ? pH : nullptr, nnzA ? pB : nullptr, px);
        auto t2 = now();
        xg.assign(px, px + (size_t)B * n);
        std::copy(th.begin(), th.end(), pth);
        auto t3 = now();
        const std::vector<EiCOS::exitcode> cm = sm->stepParam(pth, pu);
        auto t4 = now();
        go.evaluate(xg, n, B, uwant);
        ud.assign(pu, pu + (size_t)B * R);
        same_mat = same_mat && cg == cm && same(xg, sm->solution()) && same(ud, uwant);
        if (st >= 2) { te.push_back(ms(t0, t1)); tg.push_back(ms(t1, t2)); tm.push_back(ms(t3, t4)); }
    }
    delete sg; delete sm;
    for (double *d : {pG, pA, pC, pH, pB, px}) EiCOS::BatchSolver::hostFree(d);
    const bool device_leg = sc != nullptr;
    delete sa; delete sb; delete sc; delete sd;
    EiCOS::BatchSolver::hostFree(pth); EiCOS::BatchSolver::hostFree(pu);
    if (dfree) for (double *d : {dC, dH, dB}) if (d) dfree(d);
    std::printf("closed loop, every step: %s\n", same_loop ? "bit-identical" : "DIFFERENT");
    auto median = [](std::vector<double> v) { std::sort(v.begin(), v.end()); return v.empty() ? 0. : 0.5 * (v[(v.size() - 1) / 2] + v[v.size() / 2]); };
    std::printf("stepParam u vs the output map applied to solution(): %s\n", same_u ? "bit-identical" : "DIFFERENT");
    std::printf("closed loop step (update call -> result on the host), batch %d, k = %d, r = %d, median of %d steps; bytes per instance in / out:\n", B, k, R, steps);
    std::printf("  updateRHS + solve + solution         %8.3f ms  %7d B in  %6d B out\n", median(ta), 8 * (n + m + p), 8 * n);
    std::printf("  updateParam + solve + outputs        %8.3f ms  %7d B in  %6d B out\n", median(tb), 8 * k, 8 * R);
    if (device_leg) std::printf("  updateRHSDevice + solve + solution   %8.3f ms  %7d B in  %6d B out  (inputs already in device memory)\n", median(tc), 0, 8 * n);
    else std::printf("  updateRHSDevice + solve + solution        n/a\n");
    std::printf("  stepParam (pinned theta, pinned u)   %8.3f ms  %7d B in  %6d B out\n", median(td), 8 * k, 8 * R);
    std::printf("rollout vs %d stepParam calls with the plant on the host: %s\n", T, same_roll ? "bit-identical" : "DIFFERENT");
    std::printf("closed loop of %d steps, batch %d, k = %d, r = %d, median of %d:\n", T, B, k, R, REPS);
    std::printf("  rollout (one call)                   %8.3f ms\n", median(tr));
    std::printf("  %d x stepParam, plant on the host    %8.3f ms\n", T, median(tl));
    std::printf("matrix map stepParam vs solve(Gpr, Apr, c, h, b) of the host-evaluated arrays: %s\n", same_mat ? "bit-identical" : "DIFFERENT");
    std::printf("closed loop step with moving matrices, batch %d, k = %d, r = %d, median of %d steps; bytes per instance in / out:\n", B, k, R, steps);
    std::printf("  solve(full pinned arrays, x)         %8.3f ms  %7d B in  %6d B out  (+ %8.3f ms to evaluate the arrays on the host)\n", median(tg),
                8 * (nnzG + nnzA + n + m + p), 8 * n, median(te));
    std::printf("  stepParam under the matrix map       %8.3f ms  %7d B in  %6d B out\n", median(tm), 8 * k, 8 * R);
    return (same_all && same_sub && same_loop && same_u && same_roll && same_mat) ? 0 : 1; // (bit-identity is the contract: it holds for every exit code)
}
