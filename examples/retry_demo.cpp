// Retry only what failed, from host C++ (no torch): a batch is solved under an iteration cap low enough that some instances stop at it;
// then EiCOS::BatchSolver::solveWhere(sel_not_optimal) solves exactly those again under the default settings -- one launch over the
// chosen instances, selected on the GPU by exit class -- and every other instance keeps its result.  Prints how many were retried, the
// subset launch against the whole-batch solve of the same handle (HIP events, median of 5) and whether the untouched rows of x changed.
//   g++ -std=c++17 -Iinclude examples/retry_demo.cpp -Leicos_amd -leicos_amd -Wl,-rpath,$PWD/eicos_amd -o retry_demo
//   ./retry_demo tests/golden/MPC02.epb [batch = 1024] [iteration cap = 0: one below the largest pass count of the batch] [device = 0]
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <vector>

#include "eicos.hpp"

int main(int argc, char **argv) {
    if (argc < 2) { std::fprintf(stderr, "usage: %s problem.epb [batch] [iteration cap] [device]\n", argv[0]); return 2; }
    std::ifstream f(argv[1], std::ios::binary);
    std::vector<char> raw((std::istreambuf_iterator<char>(f)), {});
    if (raw.size() < 36 || std::memcmp(raw.data(), "EPB1", 4)) { std::fprintf(stderr, "not an EPB1 file\n"); return 2; }
    const int B = argc > 2 ? std::atoi(argv[2]) : 1024, dev = argc > 4 ? std::atoi(argv[4]) : 0;
    int cap = argc > 3 ? std::atoi(argv[3]) : 0;
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
    // [batch][...] arrays: instance i relaxes every inequality by 1e-3 (i mod 97) (1 + |h|) and scales c by 1 + 1e-3 (i mod 13), so that
    // the instances differ in the number of passes they need
    std::vector<double> G((size_t)B * nnzG), A((size_t)B * nnzA), C((size_t)B * n), H((size_t)B * m), Bv((size_t)B * p);
    for (int i = 0; i < B; i++) {
        std::copy(Gpr, Gpr + nnzG, G.begin() + (size_t)i * nnzG);
        std::copy(Apr, Apr + nnzA, A.begin() + (size_t)i * nnzA);
        for (int k = 0; k < n; k++) C[(size_t)i * n + k] = c[k] * (1 + 1e-3 * (i % 13));
        for (int k = 0; k < m; k++) H[(size_t)i * m + k] = h[k] + 1e-3 * (i % 97) * (1 + (h[k] < 0 ? -h[k] : h[k]));
        std::copy(b, b + p, Bv.begin() + (size_t)i * p);
    }
    EiCOS::BatchSolver s(n, m, p, nc, q.data(), m ? Gjc.data() : nullptr, m ? Gir.data() : nullptr, p ? Ajc.data() : nullptr,
                         p ? Air.data() : nullptr, B, dev);
    s.updateData(m ? G.data() : nullptr, p ? A.data() : nullptr, C.data(), m ? H.data() : nullptr, p ? Bv.data() : nullptr);
    const EiCOS::Settings dflt = s.settings();
    if (cap <= 0) { // one pass fewer than the slowest instances need: exactly those stop at the cap
        s.solve();
        size_t most = 0;
        for (const EiCOS::Information &i : s.getInfo()) most = std::max(most, i.iter);
        cap = (int)most - 1;
        if (cap < 1) { std::fprintf(stderr, "the batch needs a single pass: nothing to cap\n"); return 1; }
    }
    EiCOS::Settings capped = dflt;
    capped.iter_max = (size_t)cap;
    auto last_ms = [&] { float ms = 0.f; eicos_batch_last_solve_ms(s.handle(), &ms); return ms; };
    auto median = [](std::vector<float> v) { std::sort(v.begin(), v.end()); return v[v.size() / 2]; };

    std::vector<float> t_whole, t_subset;
    std::vector<int> retried;
    bool untouched_same = true, retried_optimal = true;
    for (int rep = 0; rep < 5; rep++) {
        s.setSettings(dflt);
        s.solve(); // the whole batch under the defaults: the time a retry of everything would take
        t_whole.push_back(last_ms());
        s.setSettings(capped);
        s.solve(); // the whole batch under the cap: some instances stop there
        const std::vector<double> x_before = s.solution();
        s.setSettings(dflt);
        const auto again = s.solveWhere(EiCOS::sel_not_optimal); // only those, under the defaults
        if (again.first.empty()) break;
        t_subset.push_back(last_ms());
        retried = again.first;
        for (EiCOS::exitcode cd : again.second) retried_optimal = retried_optimal && cd == EiCOS::exitcode::optimal;
        const std::vector<double> x_after = s.solution();
        std::vector<char> in(B, 0);
        for (int i : retried) in[i] = 1;
        for (int i = 0; i < B; i++)
            if (!in[i] && std::memcmp(&x_before[(size_t)i * n], &x_after[(size_t)i * n], (size_t)n * sizeof(double))) untouched_same = false;
    }
    std::printf("batch %d, iteration cap %d: %zu instance(s) did not end optimal and were retried\n", B, cap, retried.size());
    if (retried.empty()) { std::printf("nothing to retry: lower the iteration cap\n"); return 1; }
    std::printf("subset launch %.3f ms, whole-batch solve of the same handle %.3f ms (HIP events, median of 5)\n", median(t_subset), median(t_whole));
    std::printf("retried instances after the retry: %s\n", retried_optimal ? "all optimal" : "NOT all optimal");
    std::printf("x of the %zu untouched instances: %s\n", (size_t)B - retried.size(), untouched_same ? "unchanged, bit for bit" : "CHANGED");
    return (untouched_same && retried_optimal) ? 0 : 1;
}
