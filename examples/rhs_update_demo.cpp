// Right-hand-side-only updates from host C++ (no torch): an MPC-style loop changes c, h and b every step while G and A stay.
// EiCOS::BatchSolver::updateRHS sends only the vectors (G, A and their equilibration stay on the GPU); the result must equal, bit
// for bit, an updateData that re-sends the unchanged matrices.  Runs over a device list (a device may be listed twice: 0,0) and
// checks three forms against that reference: updateRHS + solve, the one-call solve(c, h, b, x_out) on pinned arrays, and a
// sub-range update.
//   g++ -std=c++17 -Iinclude examples/rhs_update_demo.cpp -Leicos_amd -leicos_amd -Wl,-rpath,$PWD/eicos_amd -o rhs_update_demo
//   ./rhs_update_demo tests/golden/MPC02.epb 64 0,0
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <sstream>
#include <vector>

#include "eicos.hpp"

int main(int argc, char **argv) {
    if (argc < 4) { std::fprintf(stderr, "usage: %s problem.epb batch dev[,dev...]\n", argv[0]); return 2; }
    std::ifstream f(argv[1], std::ios::binary);
    std::vector<char> raw((std::istreambuf_iterator<char>(f)), {});
    if (raw.size() < 36 || std::memcmp(raw.data(), "EPB1", 4)) { std::fprintf(stderr, "not an EPB1 file\n"); return 2; }
    const int B = std::atoi(argv[2]);
    std::vector<int> devs;
    { std::stringstream ss(argv[3]); std::string tok; while (std::getline(ss, tok, ',')) devs.push_back(std::atoi(tok.c_str())); }
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
    // [batch][...] arrays; step s of instance i relaxes every inequality by 1e-3 (i + s) (1 + |h|) and scales c by 1 + 1e-3 s
    std::vector<double> G((size_t)B * nnzG), A((size_t)B * nnzA);
    for (int i = 0; i < B; i++) {
        std::copy(Gpr, Gpr + nnzG, G.begin() + (size_t)i * nnzG);
        std::copy(Apr, Apr + nnzA, A.begin() + (size_t)i * nnzA);
    }
    auto rhs = [&](int s, std::vector<double> &C, std::vector<double> &H, std::vector<double> &Bv) {
        C.resize((size_t)B * n); H.resize((size_t)B * m); Bv.resize((size_t)B * p);
        for (int i = 0; i < B; i++) {
            for (int k = 0; k < n; k++) C[(size_t)i * n + k] = c[k] * (1 + 1e-3 * s);
            for (int k = 0; k < m; k++) H[(size_t)i * m + k] = h[k] + 1e-3 * (i + s) * (1 + (h[k] < 0 ? -h[k] : h[k]));
            std::copy(b, b + p, Bv.begin() + (size_t)i * p);
        }
    };
    std::vector<double> C0, H0, B0, C1, H1, B1;
    rhs(0, C0, H0, B0); rhs(1, C1, H1, B1);
    auto make = [&](const std::vector<int> &ids) {
        return new EiCOS::BatchSolver(n, m, p, nc, q.data(), m ? Gjc.data() : nullptr, m ? Gir.data() : nullptr, p ? Ajc.data() : nullptr,
                                      p ? Air.data() : nullptr, B, ids);
    };
    auto same = [&](const std::vector<double> &x, const double *y) { return std::memcmp(x.data(), y, x.size() * sizeof(double)) == 0; };
    // reference: every step re-sends the unchanged matrices with the new vectors
    EiCOS::BatchSolver *ref = make(devs);
    ref->updateData(m ? G.data() : nullptr, p ? A.data() : nullptr, C1.data(), m ? H1.data() : nullptr, p ? B1.data() : nullptr);
    const std::vector<EiCOS::exitcode> codes_ref = ref->solve();
    const std::vector<double> x_ref = ref->solution();
    delete ref;
    int ok = 0;
    for (auto cd : codes_ref) ok += cd == EiCOS::exitcode::optimal;
    std::printf("%d / %d optimal over %zu shard(s)\n", ok, B, devs.size());

    EiCOS::BatchSolver *s = make(devs);
    s->updateData(m ? G.data() : nullptr, p ? A.data() : nullptr, C0.data(), m ? H0.data() : nullptr, p ? B0.data() : nullptr);
    s->solve();
    // (1) updateRHS + solve: only c, h, b travel
    s->updateRHS(C1.data(), m ? H1.data() : nullptr, p ? B1.data() : nullptr);
    const bool same_rhs = s->solve() == codes_ref && same(x_ref, s->solution().data());
    std::printf("updateRHS + solve vs updateData with unchanged matrices: %s\n", same_rhs ? "bit-identical" : "DIFFERENT");
    // (2) the one-call form on pinned arrays: each shard's solve kernel scales its instances' vectors itself
    s->updateRHS(C0.data(), nullptr, nullptr);
    auto pin = [&](const std::vector<double> &v) { double *d = EiCOS::BatchSolver::hostAlloc(std::max<size_t>(v.size(), 1)); std::copy(v.begin(), v.end(), d); return d; };
    double *pC = pin(C1), *pH = pin(H1), *pB = pin(B1), *px = EiCOS::BatchSolver::hostAlloc((size_t)B * n);
    const bool same_fused = s->solve(pC, m ? pH : nullptr, p ? pB : nullptr, px) == codes_ref && same(x_ref, px);
    std::printf("one-call solve(c, h, b) on pinned arrays: %s\n", same_fused ? "bit-identical" : "DIFFERENT");
    for (double *d : {pC, pH, pB, px}) EiCOS::BatchSolver::hostFree(d);
    // (3) a sub-range: instances [B/4, B/2) get step 0's c back; the reference re-sends everything
    const int first = B / 4, count = B / 2 - B / 4;
    s->updateRHS(C0.data() + (size_t)first * n, nullptr, nullptr, first, count);
    std::vector<double> C2 = C1;
    std::copy(C0.begin() + (size_t)first * n, C0.begin() + (size_t)(first + count) * n, C2.begin() + (size_t)first * n);
    const std::vector<EiCOS::exitcode> codes_sub = s->solve();
    const std::vector<double> x_sub = s->solution();
    delete s;
    ref = make(devs);
    ref->updateData(m ? G.data() : nullptr, p ? A.data() : nullptr, C2.data(), m ? H1.data() : nullptr, p ? B1.data() : nullptr);
    const bool same_sub = ref->solve() == codes_sub && same(x_sub, ref->solution().data());
    delete ref;
    std::printf("sub-range updateRHS: %s\n", same_sub ? "bit-identical" : "DIFFERENT");
    return (same_rhs && same_fused && same_sub && ok > 0) ? 0 : 1;
}
