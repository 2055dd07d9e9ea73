// Stand-alone check (tests/test_plan_step.py builds it with the address and undefined-behaviour sanitizers) of the host-only steps of handle
// creation and of the host self checks: eicos_amd/csrc/plan_step.cpp and host_check.cpp with symbolic.cpp, plans.cpp and tiles.cpp, no HIP.
//   plan_step_check plans <problem.epb>        every configuration of the pattern (below): analyse -> build_plan -> lds_budget, then an audit
//                                              of what the kernels will address -- pool slots, LDS regions, the 16-bit gather indices
//   plan_step_check checks <problem.epb>       the three host self checks on the pattern (scalar, tiles, hybrid)
//   plan_step_check fingerprint <problem.epb>  one line per configuration: a 64-bit FNV-1a over everything the plan step produced (to compare
//                                              two builds of the plan step; the lines are not a fixture: plans change when the planner does)
// Configurations: batch 1, 256, 1024 x arithmetic profile 0, 1 x dense apex off, and on where the analysis allows it; 256 CUs throughout.
// Exit status 0: everything held.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include "eicos_amd.h"
#include "last_error.hpp"
#include "plan_step.hpp"

using namespace eicos;

namespace {

constexpr int N_CU = 256;

struct Problem { int n = 0, m = 0, p = 0, l = 0, nc = 0; std::vector<int> q, Gjc, Gir, Ajc, Air; };

// The pattern part of an EPB1 file (as examples/ecos_runner.cpp reads it; the value sets behind the pattern are not needed here).
bool read_epb(const std::string &path, Problem &P) {
    std::ifstream f(path, std::ios::binary);
    std::vector<char> raw((std::istreambuf_iterator<char>(f)), {});
    if (raw.size() < 36 || std::memcmp(raw.data(), "EPB1", 4)) return false;
    int hd[8];
    std::memcpy(hd, raw.data() + 4, sizeof hd);
    P.n = hd[0]; P.m = hd[1]; P.p = hd[2]; P.l = hd[3]; P.nc = hd[4];
    const int nnzG = hd[5], nnzA = hd[6];
    if (P.n < 0 || P.nc < 0 || nnzG < 0 || nnzA < 0) return false;
    size_t at = 36;
    auto take_i = [&](std::vector<int> &v, size_t cnt) {
        if (at + cnt * sizeof(int) > raw.size()) return false;
        v.resize(cnt);
        if (cnt) std::memcpy(v.data(), raw.data() + at, cnt * sizeof(int));
        at += cnt * sizeof(int);
        return true;
    };
    return take_i(P.q, P.nc) && take_i(P.Gjc, (size_t)P.n + 1) && take_i(P.Gir, nnzG) && take_i(P.Ajc, (size_t)P.n + 1) && take_i(P.Air, nnzA);
}

// (an empty index array is still a given one: NULL would say "no such group")
const int *ptr(const std::vector<int> &v) { static const int none = 0; return v.empty() ? &none : v.data(); }

int failures = 0;
std::string where; // the configuration under audit, for the messages
#define EXPECT(cond, ...)                                                               \
    do {                                                                                \
        if (!(cond)) { failures++; std::printf("FAIL [%s] %s: ", where.c_str(), #cond); std::printf(__VA_ARGS__); std::printf("\n"); } \
    } while (0)

// ---- (a) + (c): the pattern image ----
struct Arr { const int *p = nullptr; size_t len = 0; }; // an array of the pool and its extent: up to the next array (or the pool's end)
Arr pool_array(const Plan &pl, const int *const &field) {
    std::vector<size_t> offs;
    size_t mine = (size_t)-1;
    for (const Plan::Slot &s : pl.slots) { offs.push_back(s.off); if (s.dst == &field) mine = s.off; }
    if (mine == (size_t)-1) { failures++; std::printf("FAIL [%s] a DevPat array has no slot in the pool\n", where.c_str()); return Arr{}; }
    std::sort(offs.begin(), offs.end());
    const auto next = std::upper_bound(offs.begin(), offs.end(), mine);
    return Arr{pl.pool.data.data() + mine, (next == offs.end() ? pl.pool.data.size() : *next) - mine};
}

void audit_slots(const Plan &pl) {
    for (const Plan::Slot &s : pl.slots) {
        EXPECT(s.off < pl.pool.data.size(), "slot offset %zu, pool of %zu ints", s.off, pl.pool.data.size());
        EXPECT(s.off * sizeof(int) % 16 == 0, "slot offset %zu is not 16-byte aligned", s.off);
    }
    EXPECT(pl.pool.data.size() * sizeof(int) % 16 == 0, "pool of %zu ints", pl.pool.data.size());
}

// One 16-bit packed index array against its 32-bit form, decoded by the kernel's rule (kernels.hip: load_indices<true>): the entry of lane t
// of a slice is off16 + t, `stride` words per entry of which two, from `word0`, hold the four indices of the lane; index kk of the lane is
// the 32-bit array's entry off + kk * lanes + t for kk < K and the pad value beyond; the entry d16 (inactive lanes) is all padding.
void audit_idx16(const char *name, Arr sl, int ns, Arr a16, size_t stride, size_t word0, Arr a32, int pad, int d16) {
    auto index_at = [&](size_t entry, int kk, int &v) {
        const size_t w = entry * stride + word0 + (size_t)(kk >> 1);
        if (w >= a16.len) return false;
        v = (int)(((unsigned)a16.p[w] >> (16 * (kk & 1))) & 0xffffu);
        return true;
    };
    if (!(4 * (size_t)ns <= sl.len)) { EXPECT(false, "%s: %d slices, table of %zu ints", name, ns, sl.len); return; }
    for (int i = 0; i < ns; i++) {
        PackedSlice ps;
        std::memcpy(&ps, sl.p + 4 * (size_t)i, sizeof ps);
        const int cnt = ps.bits & ((1 << PS_LG) - 1), lg = (ps.bits >> PS_LG) & 7, K = (ps.bits >> PS_K) & 7, lanes = cnt << lg;
        for (int t = 0; t < lanes; t++)
            for (int kk = 0; kk < ELL_KMAX; kk++) {
                int got = -1, want = pad;
                if (kk < K) {
                    const size_t slot = (size_t)ps.off + (size_t)kk * lanes + t;
                    if (slot >= a32.len) { EXPECT(false, "%s: slice %d lane %d kk %d reads slot %zu of %zu", name, i, t, kk, slot, a32.len); return; }
                    want = a32.p[slot];
                }
                if (!index_at((size_t)ps.off16 + t, kk, got)) { EXPECT(false, "%s: slice %d lane %d: entry %d outside the packed array", name, i, t, ps.off16 + t); return; }
                if (got != want) { EXPECT(false, "%s: slice %d lane %d kk %d: packed %d, 32-bit form %d", name, i, t, kk, got, want); return; }
            }
    }
    for (int kk = 0; kk < ELL_KMAX; kk++) {
        int got = -1;
        if (!index_at((size_t)d16, kk, got) || got != pad) { EXPECT(false, "%s: padding entry %d kk %d holds %d, pad value %d", name, d16, kk, got, pad); return; }
    }
}

void audit_idx16_forms(const Plan &pl) {
    const DevPat &D = pl.dp;
    if (!D.idx16) return;
    const Arr fsl = pool_array(pl, pl.fsl), bsl = pool_array(pl, pl.bsl), cag = pool_array(pl, pl.cag_sl), rA = pool_array(pl, pl.rA_sl),
              rG = pool_array(pl, pl.rG_sl), fac = pool_array(pl, pl.fac_sl);
    const int nf = D.nfs + D.nfs_solo + D.nfs_ext, nb = D.nbs + D.nbs_solo;
    audit_idx16("f_idx16", fsl, nf, pool_array(pl, D.f_idx16), 2, 0, pool_array(pl, D.f_idx), D.N, D.f_d16);
    audit_idx16("b_idx16", bsl, nb, pool_array(pl, D.b_idx16), 2, 0, pool_array(pl, D.b_idx), D.N, D.b_d16);
    audit_idx16("cag_k16", cag, D.cag_ns, pool_array(pl, D.cag_k16), 2, 0, pool_array(pl, D.cag_idx_k), D.N, D.cag_d16);
    audit_idx16("cag_yz16", cag, D.cag_ns, pool_array(pl, D.cag_yz16), 2, 0, pool_array(pl, D.cag_idx_yz), 0, D.cag_d16);
    audit_idx16("rA_16", rA, D.rA_ns, pool_array(pl, D.rA_16), 2, 0, pool_array(pl, D.rA_idx), 0, D.rA_d16);
    audit_idx16("rA_k16", rA, D.rA_ns, pool_array(pl, D.rA_k16), 2, 0, pool_array(pl, D.rA_idx_k), D.N, D.rA_d16);
    audit_idx16("rG_16", rG, D.rG_ns, pool_array(pl, D.rG_16), 2, 0, pool_array(pl, D.rG_idx), 0, D.rG_d16);
    audit_idx16("rG_k16", rG, D.rG_ns, pool_array(pl, D.rG_k16), 2, 0, pool_array(pl, D.rG_idx_k), D.N, D.rG_d16);
    // the factor program: 16 bytes per lane, the pa words then the pb words, in the stored-L and the deferred-L form; the pivot columns
    const Arr pa = pool_array(pl, D.fac_pa);
    audit_idx16("fac_p16 (stored L): pa", fac, D.fac_ns, pool_array(pl, pl.fac_p16_f), 4, 0, pa, D.nUB, D.fac_d16);
    audit_idx16("fac_p16 (stored L): pb", fac, D.fac_ns, pool_array(pl, pl.fac_p16_f), 4, 2, pool_array(pl, pl.fac_pb_f), D.nUF, D.fac_d16);
    audit_idx16("fac_p16 (deferred L): pa", fac, D.fac_ns, pool_array(pl, pl.fac_p16_u), 4, 0, pa, D.nUB, D.fac_d16);
    audit_idx16("fac_p16 (deferred L): pb", fac, D.fac_ns, pool_array(pl, pl.fac_p16_u), 4, 2, pool_array(pl, pl.fac_pb_u), D.nUB, D.fac_d16);
    audit_idx16("fac_k16", fac, D.fac_ns, pool_array(pl, D.fac_k16), 2, 0, pool_array(pl, D.fac_pk), pl.an->sym.N, D.fac_d16);
}

// ---- (b): the regions of the dynamic LDS that the DevPat names, in doubles from its start ----
void audit_lds(const Plan &pl, const Shape &sh) {
    const DevPat &D = pl.dp;
    struct Region { const char *name; size_t b, e; };
    std::vector<Region> rs;
    const int nvec = D.dual ? 2 : sh.nlds;
    const bool tile = D.tile != 0;
    if (nvec > 0) rs.push_back({"vectors", 0, (size_t)nvec * D.Npad});
    if (D.meta_lds) rs.push_back({"slice tables", (size_t)D.lds_tab, (size_t)D.lds_tab + (size_t)D.lm_total * sizeof(PackedSlice) / sizeof(double)});
    if (tile) {
        rs.push_back({"tile scratch", (size_t)D.tl_scratch, (size_t)D.tl_scratch + (size_t)(pl.threads / 64) * TILE_SCR});
        rs.push_back({"tile partial sums", (size_t)D.tl_part, (size_t)D.tl_part + (size_t)TILE_PARTS * 16 * 2});
    }
    if (D.apex_lds >= 0) rs.push_back({"apex image", (size_t)D.apex_lds, (size_t)D.apex_lds + APEX_IMG});
    if (sh.ldsres) {
        rs.push_back({"instance slab", (size_t)D.lr_inst, (size_t)D.lr_inst + ((D.inst_stride + 1) & ~(size_t)1)});
        rs.push_back({"workspace slab", (size_t)D.lr_work, (size_t)D.lr_work + ((D.work_stride + 1) & ~(size_t)1)});
    }
    for (const Region &r : rs)
        EXPECT(r.e * sizeof(double) <= sh.dyn_lds, "%s [%zu, %zu) doubles, dyn_lds %zu bytes", r.name, r.b, r.e, sh.dyn_lds);
    for (size_t i = 0; i < rs.size(); i++)
        for (size_t j = i + 1; j < rs.size(); j++) {
            // (the one placement of a region in another that lds_budget makes on purpose: the apex of an LDS-resident handle reads the
            // forward image where it is, in the LDS copy of the workspace slab -- DevPat::apex_inplace)
            if (D.apex_inplace && !std::strcmp(rs[i].name, "apex image") && !std::strcmp(rs[j].name, "workspace slab")) {
                EXPECT(rs[j].b <= rs[i].b && rs[i].e <= rs[j].e, "in-place apex image [%zu, %zu) outside the workspace slab [%zu, %zu)", rs[i].b, rs[i].e, rs[j].b, rs[j].e);
                continue;
            }
            EXPECT(rs[i].e <= rs[j].b || rs[j].e <= rs[i].b, "%s [%zu, %zu) overlaps %s [%zu, %zu)", rs[i].name, rs[i].b, rs[i].e, rs[j].name, rs[j].b, rs[j].e);
        }
    EXPECT(D.apex_inplace == 0 || sh.ldsres, "in-place apex without the LDS-resident build");
    EXPECT(sh.dyn_lds + LDS_STATIC <= LDS_PER_CU, "dyn_lds %zu bytes + the static block exceed the CU's LDS", sh.dyn_lds);
}

struct Fnv {
    uint64_t h = 1469598103934665603ull;
    void bytes(const void *p, size_t n) { const unsigned char *c = (const unsigned char *)p; for (size_t i = 0; i < n; i++) { h ^= c[i]; h *= 1099511628211ull; } }
    template <class T> void val(T v) { bytes(&v, sizeof v); }
};

uint64_t fingerprint(const Plan &pl, const Shape &sh) {
    Fnv f;
    f.bytes(pl.pool.data.data(), pl.pool.data.size() * sizeof(int));
    f.bytes(&pl.dp, sizeof pl.dp);
    f.bytes(pl.posB.data(), pl.posB.size() * sizeof(int));
    f.val(pl.ub_len); f.val(pl.threads);
    f.val(sh.nlds); f.val(sh.ldsres); f.val(sh.w2); f.val(sh.ubl); f.val(sh.dyn_lds); f.val(sh.bpc); f.val(sh.grid); f.val(sh.order_min);
    f.val(sh.upd_grid); f.val(sh.upd_vals_lds); f.val(sh.upd_lds); f.val((int)sh.apex_unplaced);
    return f.h;
}

int run_plans(const Problem &Q, const std::string &name, bool print_fingerprints) {
    int configs = 0;
    for (int batch : {1, 256, 1024})
        for (int profile : {0, 1}) {
            where = name + " batch " + std::to_string(batch) + " profile " + std::to_string(profile);
            int n = Q.n, m = Q.m, p = Q.p, nc = Q.nc;
            ProblemPattern P;
            int rc = check_pattern_args(n, m, p, Q.l, nc, ptr(Q.q), ptr(Q.Gjc), ptr(Q.Gir), ptr(Q.Ajc), ptr(Q.Air), batch);
            if (rc == EICOS_OK) rc = take_csc(n, m, p, nc, ptr(Q.q), ptr(Q.Gjc), ptr(Q.Gir), ptr(Q.Ajc), ptr(Q.Air), P);
            EXPECT(rc == EICOS_OK, "pattern intake: %d (%s)", rc, g_err.c_str());
            if (rc != EICOS_OK) continue;
            Analyses A;
            rc = analyse(P, batch, N_CU, profile, A);
            EXPECT(rc == EICOS_OK, "analyse: %d (%s)", rc, g_err.c_str());
            if (rc != EICOS_OK) continue;
            for (int apex = 0; apex <= (A.apex ? 1 : 0); apex++) {
                where = name + " batch " + std::to_string(batch) + " profile " + std::to_string(profile) + " apex " + std::to_string(apex);
                configs++;
                Plan pl;
                std::memset(&pl.dp, 0, sizeof pl.dp); // (the padding bytes of the struct too: the fingerprint reads its bytes)
                Shape sh;
                rc = build_plan(P, A, apex != 0, batch, N_CU, profile, pl);
                EXPECT(rc == EICOS_OK, "build_plan: %d (%s)", rc, g_err.c_str());
                if (rc != EICOS_OK) continue;
                lds_budget(pl, batch, N_CU, sh);
                if (print_fingerprints) { std::printf("%s batch=%d profile=%d apex=%d %016llx\n", name.c_str(), batch, profile, apex, (unsigned long long)fingerprint(pl, sh)); continue; }
                audit_slots(pl);
                // (a 128-thread plan with the apex that did not get the LDS-resident build: creation discards this shape and plans
                // again without the apex, so its LDS fields are not what a kernel will see)
                if (!sh.apex_unplaced) audit_lds(pl, sh);
                audit_idx16_forms(pl);
            }
        }
    if (!print_fingerprints) std::printf("plans: %s: %d configurations, %d failures\n", name.c_str(), configs, failures);
    return failures ? 1 : 0;
}

// The bounds of tests/test_abi_and_symbolic.py: residual in [0, 1e-12); hybrid: -10 (the pattern does not qualify) or in [0, 1e-12).
int run_checks(const Problem &Q, const std::string &name) {
    where = name;
    const int *q = ptr(Q.q), *Gjc = ptr(Q.Gjc), *Gir = ptr(Q.Gir), *Ajc = ptr(Q.Ajc), *Air = ptr(Q.Air);
    const double rs = eicos_debug_host_check(Q.n, Q.m, Q.p, Q.nc, q, Gjc, Gir, Ajc, Air, 1, -1, nullptr);
    std::printf("checks: %s: scalar %.3g", name.c_str(), rs);
    EXPECT(rs >= 0.0 && rs < 1e-12, "scalar residual %g (%s)", rs, g_err.c_str());
    if (Q.n > 0) { // (tiles and hybrid: not on the empty problem)
        const double rt = eicos_debug_host_check_tiles(Q.n, Q.m, Q.p, Q.nc, q, Gjc, Gir, Ajc, Air, 1, -1, nullptr);
        const double rh = eicos_debug_host_check_hybrid(Q.n, Q.m, Q.p, Q.nc, q, Gjc, Gir, Ajc, Air, 1, -1, nullptr);
        std::printf(" tiles %.3g hybrid %.3g", rt, rh);
        EXPECT(rt >= 0.0 && rt < 1e-12, "tiles residual %g (%s)", rt, g_err.c_str());
        EXPECT(rh == -10.0 || (rh >= 0.0 && rh < 1e-12), "hybrid residual %g (%s)", rh, g_err.c_str());
    }
    std::printf("\n");
    return failures ? 1 : 0;
}

} // namespace

int main(int argc, char **argv) {
    const std::string mode = argc == 3 ? argv[1] : "";
    if (mode != "plans" && mode != "checks" && mode != "fingerprint") { std::fprintf(stderr, "usage: %s plans|checks|fingerprint problem.epb\n", argv[0]); return 2; }
    Problem Q;
    if (!read_epb(argv[2], Q)) { std::fprintf(stderr, "cannot read %s\n", argv[2]); return 2; }
    std::string name = argv[2];
    name = name.substr(name.find_last_of('/') + 1);
    name = name.substr(0, name.rfind(".epb"));
    return mode == "checks" ? run_checks(Q, name) : run_plans(Q, name, mode == "fingerprint");
}
