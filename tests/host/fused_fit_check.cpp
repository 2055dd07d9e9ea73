// Host check of eicos_amd/csrc/fused_fit.hpp (tests/test_fused_fit.py builds this with -fsanitize=address,undefined and runs it): the
// rule "may this step run inside the solve launch" at every boundary, against the three expressions api.cpp held before the rule had a
// home of its own, written out literally below (quoted from commit 8e6bb2f; the knob EICOS_FUSED_UPDATE, which the call sites keep, left
// out).  Exit status 0 = all checks passed.
#include "fused_fit.hpp"

#include <cstdio>
#include <initializer_list>

using namespace eicos;

static int g_failed = 0, g_cases = 0;
#define CHECK(cond)                                                                   \
    do {                                                                              \
        g_cases++;                                                                    \
        if (!(cond)) { std::printf("line %d: %s\n", __LINE__, #cond); g_failed++; }   \
    } while (0)

// What the old expressions read: D = the pattern descriptor (h->dp), h = the handle.
struct OldDesc { int n, p, m, Npad; };
struct OldMap { int k; };
struct OldHandle { int threads, nlds; OldMap param, mat; };

// api.cpp:905 (launch_shape, the entry-parallel updateData kernels; S = the symbolic analysis, same n, p, m):
//     const bool small_vecs = S.n <= 8 * 512 && S.p <= 8 * 512 && S.m <= 16 * 512;
static bool old_small_vecs(const OldDesc &S) {
    const bool small_vecs = S.n <= 8 * 512 && S.p <= 8 * 512 && S.m <= 16 * 512;
    return small_vecs;
}
// api.cpp:1940-1942 (update_solve):
//     const bool own = D.n <= 8 * h->threads && D.p <= 8 * h->threads && D.m <= 16 * h->threads;
//     const bool fits = param ? (h->param.k <= D.Npad && (h->mat.k == 0 || own)) : (rhs || own);
//     const bool fused = h->nlds >= 1 && fits && env_knob("EICOS_FUSED_UPDATE", 1, 0, 1);
static bool old_step_fused(const OldDesc &D, const OldHandle *h, bool rhs, bool param) {
    const bool own = D.n <= 8 * h->threads && D.p <= 8 * h->threads && D.m <= 16 * h->threads;
    const bool fits = param ? (h->param.k <= D.Npad && (h->mat.k == 0 || own)) : (rhs || own);
    const bool fused = h->nlds >= 1 && fits;
    return fused;
}
// api.cpp:2152-2153 (eicos_batch_rollout):
//     const bool own = h->mat.k == 0 || (D.n <= 8 * h->threads && D.p <= 8 * h->threads && D.m <= 16 * h->threads); // (update_solve: the accumulator limit)
//     const bool fused = h->nlds >= 1 && k + r <= D.Npad && own && env_knob("EICOS_FUSED_UPDATE", 1, 0, 1);
static bool old_rollout_fused(const OldDesc &D, const OldHandle *h, int k, int r) {
    const bool own = h->mat.k == 0 || (D.n <= 8 * h->threads && D.p <= 8 * h->threads && D.m <= 16 * h->threads); // (update_solve: the accumulator limit)
    const bool fused = h->nlds >= 1 && k + r <= D.Npad && own;
    return fused;
}

// (the rule is usable in constant expressions)
static_assert(fused_full_fits(FitShape{2048, 2048, 4096, 64, 1, 256}) && !fused_full_fits(FitShape{2049, 0, 0, 64, 1, 256}), "");
static_assert(update_vectors_fit(4096, 4096, 8192) && !update_vectors_fit(0, 0, 8193), "");

int main() {
    const int Npad = 48; // (a multiple of 16, as api.cpp pads it)
    for (int T : {128, 256, 512})
        for (int n : {0, 8 * T, 8 * T + 1})
            for (int p : {0, 8 * T, 8 * T + 1})
                for (int m : {0, 16 * T, 16 * T + 1}) {
                    const OldDesc D = {n, p, m, Npad};
                    // the updateData case: the limit of the 512-thread kernels, whatever the handle's workgroup size
                    CHECK(update_vectors_fit(n, p, m) == old_small_vecs(D));
                    CHECK(accumulators_fit(n, p, m, T) == (n <= 8 * T && p <= 8 * T && m <= 16 * T));
                    for (int nlds : {0, 1, 2}) {
                        const FitShape s = {n, p, m, Npad, nlds, T};
                        for (int mat_k : {0, 1}) { // matrix map off / on (its k is the parameter map's; only "installed" matters)
                            const bool mmap = mat_k != 0;
                            OldHandle h = {T, nlds, {1}, {mat_k}};
                            CHECK(fused_full_fits(s) == old_step_fused(D, &h, false, false));
                            CHECK(fused_rhs_fits(s) == old_step_fused(D, &h, true, false));
                            for (int k : {1, Npad, Npad + 1}) {
                                h.param.k = k;
                                CHECK(fused_param_fits(s, k, mmap) == old_step_fused(D, &h, false, true));
                            }
                            for (int total : {Npad, Npad + 1}) // k + r, split at both ends (k, r >= 1)
                                for (int k : {1, total - 1}) {
                                    const int r = total - k;
                                    h.param.k = k;
                                    CHECK(fused_rollout_fits(s, k, r, mmap) == old_rollout_fused(D, &h, k, r));
                                }
                        }
                    }
                }
    // a few outcomes spelled out, so that two equal mistakes on both sides cannot pass
    const FitShape edge = {8 * 256, 8 * 256, 16 * 256, Npad, 1, 256}, over = {8 * 256 + 1, 0, 0, Npad, 1, 256}, no_lds = {0, 0, 0, Npad, 0, 256};
    CHECK(fused_full_fits(edge) && !fused_full_fits(over) && !fused_full_fits(no_lds));
    CHECK(fused_rhs_fits(over) && !fused_rhs_fits(no_lds));
    CHECK(fused_param_fits(over, Npad, false) && !fused_param_fits(over, Npad, true) && fused_param_fits(edge, Npad, true));
    CHECK(!fused_param_fits(edge, Npad + 1, false) && !fused_param_fits(no_lds, 1, false));
    CHECK(fused_rollout_fits(over, Npad - 1, 1, false) && !fused_rollout_fits(over, Npad - 1, 1, true) && !fused_rollout_fits(edge, Npad, 1, false));
    CHECK(!fused_rollout_fits(no_lds, 1, 1, false));
    CHECK(update_vectors_fit(8 * 512, 8 * 512, 16 * 512) && !update_vectors_fit(8 * 512 + 1, 0, 0) && !update_vectors_fit(0, 8 * 512 + 1, 0) &&
          !update_vectors_fit(0, 0, 16 * 512 + 1));
    const int walked = 3 * 27 * (2 + 3 * 2 * (2 + 3 + 4));
    if (g_cases != walked + 7) { std::printf("walked %d cases, expected %d\n", g_cases, walked + 7); g_failed++; }
    if (g_failed) { std::printf("%d check(s) failed\n", g_failed); return 1; }
    std::printf("fused_fit_check: %d cases, all passed\n", g_cases);
    return 0;
}
