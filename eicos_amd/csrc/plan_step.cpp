// The host-only steps of handle creation (plan_step.hpp): pattern intake, analysis, plan, LDS budget.  Pure index arithmetic -- no HIP
// call, no eicos_batch; compiled without a HIP include path.
#include "plan_step.hpp"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <stdexcept>
#include <string>

#include "../../include/eicos_amd.h"
#include "envknob.hpp"
#include "last_error.hpp"

namespace eicos {

// Workgroups per CU for a batch, at most `max_r`: the cheapest estimate of the launch's duration wins.
//   time of one "round" (every resident workgroup solves one instance) at r per CU, relative to r = 1:  1 + 0.5 (r - 1) up to r = 2; the
//   256-thread kernel beyond two per CU grows in proportion to r (+ 1.5 %): re-measured with the final round-5 library, same box, interleaved
//   (profiles/r06_log_ab_r04_r05_libs.log, r06_log_launch_shapes.log; MPC02): 11.15 ms per round of 512 at two per CU (the 256-VGPR build, dense
//   apex, residual head in LDS) against 17.0 ms per round of 768 at three (168 VGPRs, neither) -- 45.9 against 45.2 instances per ms: the
//   third workgroup buys nothing in the steady state any more, it only rounds a batch differently;
//   a partly filled LAST round costs more than its share (0.55 + 0.45 f) only when it follows a single full round (batch 768: 20.6 ms as
//   1.5 rounds at two per CU, 18.7 ms as one round at three); behind two or more full rounds the longest-first queue evens the tail out
//   and the share is what it costs (measured f = 2/3 behind two rounds: 0.63; f = 1/3 behind five: 0.22).
// MPC02 on 256 CUs: 3 per CU for 513 ... 768 instances only; 1024, 1536, 2048, 3072 and 4096 run at two (measured: +4 % at 1536, +2.5 % at
// 3072, +-1 % at 2048, -2 % at 4096 against three per CU -- inside the +-3 % spread between two processes on one box -- on 1.18 x instead of
// 1.33 x the algorithmic HBM traffic), so eicos_batch_create keeps the dense apex for the large batches.
int launch_blocks_per_cu(int batch, int n_cu, int max_r, int threads) {
    double best = 1e300; int best_r = 1;
    for (int r = 1; r <= max_r; r++) {
        const double rounds = (double)batch / ((double)n_cu * r);
        const double full = std::floor(rounds), f = rounds - full;
        const double round_time = (threads == 256 && r > 2) ? 1.5 * 1.015 * (r / 2.0) : 1.0 + 0.5 * (r - 1);
        const double cost = round_time * (full + (f > 0 ? (full >= 2 ? f : 0.55 + 0.45 * f) : 0.0));
        if (cost < best - 1e-12) { best = cost; best_r = r; }
    }
    return best_r;
}

// ---- pattern intake: the C arguments as a validated ProblemPattern ----
int check_pattern_args(int n, int &m, int &p, int l, int &ncones, const int *q, const int *Gjc, const int *Gir, const int *Ajc, const int *Air,
                       int batch) {
    if (n < 0 || m < 0 || p < 0 || ncones < 0 || batch < 1) return fail(EICOS_E_INVALID, "negative dimension or batch < 1");
    if (ncones > 0 && !q) return fail(EICOS_E_INVALID, "ncones > 0 but q is NULL");
    const bool haveG = Gjc && Gir, haveA = Ajc && Air;
    if (!haveG) { m = 0; ncones = 0; } // reference: groups given as NULL are empty (src/eicos.cpp:103-117)
    if (!haveA) p = 0;
    // The reference ignores `l` and derives it as m - sum(q) (src/eicos.cpp:91,155).  l < 0 means "derive"; a caller that
    // does pass l (ECOS convention: l + sum(q) = m) and gets it wrong would silently solve a different cone split.
    if (haveG && l >= 0) {
        long long qs = 0;
        for (int c = 0; c < ncones; c++) qs += q[c];
        if ((long long)l + qs != (long long)m) return fail(EICOS_E_INVALID, "l + sum(q) != m (pass l < 0 to derive l as the reference does)");
    }
    return EICOS_OK;
}

int take_csc(int n, int m, int p, int ncones, const int *q, const int *Gjc, const int *Gir, const int *Ajc, const int *Air, ProblemPattern &P) {
    const bool haveG = Gjc && Gir, haveA = Ajc && Air;
    // compressed CSC as the reference assumes (src/eicos.cpp:2038-2039): pointers start at 0 and do not decrease,
    // row indices in range and strictly increasing inside a column
    auto take = [&](const int *jc, const int *ir, int rows, std::vector<int> &ojc, std::vector<int> &oir, const char *nm) {
        if (jc[0] != 0) throw std::invalid_argument(std::string(nm) + ": column pointers must start at 0");
        for (int j = 0; j < n; j++) if (jc[j + 1] < jc[j]) throw std::invalid_argument(std::string(nm) + ": column pointers decrease");
        ojc.assign(jc, jc + n + 1); oir.assign(ir, ir + jc[n]);
        for (int j = 0; j < n; j++)
            for (int k = jc[j]; k < jc[j + 1]; k++) {
                if (ir[k] < 0 || ir[k] >= rows) throw std::invalid_argument(std::string(nm) + " row index out of range");
                if (k > jc[j] && ir[k] <= ir[k - 1]) throw std::invalid_argument(std::string(nm) + ": row indices of a column must be strictly increasing");
            }
    };
    try {
        P.n = n; P.m = m; P.p = p; P.nc = ncones;
        P.q.assign(q, q + ncones);
        if (haveG) take(Gjc, Gir, m, P.Gjc, P.Gir, "G"); else P.Gjc.assign(n + 1, 0);
        if (haveA) take(Ajc, Air, p, P.Ajc, P.Air, "A"); else P.Ajc.assign(n + 1, 0);
    } catch (const std::exception &e) { return fail(EICOS_E_INVALID, e.what()); }
    return EICOS_OK;
}

namespace {

constexpr int KI_MAX_HOST = 2; // right-hand sides of a dual solve (kernels.hip: KI_MAX)

struct SlabLayout {
    size_t size = 0;
    int add(size_t count) {
        int off = (int)size;
        size += (count + 7) & ~(size_t)7; // 64-byte granules
        return off;
    }
};

// G in dense 16 x 16 tiles (dense-front patterns on the tile path: the products are bandwidth-bound).
// Row block = 16 consecutive rows of G; its tiles = the sorted union of the columns of those rows, cut into groups of 16
// (so a tile's columns need not be consecutive).  One pass over the tiles yields G x (per row block, in registers) and the
// partial column sums of G' z (per tile, reduced per column in a second, fixed-order pass): G is streamed ONCE per
// evaluation instead of once in column form and once in row form, with no index bytes.  Taken when the tiles are at
// least half full; the sliced-ELL plans of the products then hold A only.
struct GTiles { int on = 0, nrb = 0, nt = 0, W = 0; std::vector<int> rbptr, col, src, cidx; };
GTiles plan_g_tiles(const Symbolic &S, int gv_rel) {
    GTiles GT;
    if (!(S.tile == 1 && S.nnzG > 0 && env_knob("EICOS_GTILES", 1, 0, 2))) return GT;
    const int nrb = (S.m + 15) / 16;
    GT.nrb = nrb; GT.rbptr.assign(nrb + 1, 0);
    std::vector<std::vector<int>> rbcols(nrb);
    for (int rb = 0; rb < nrb; rb++) {
        std::vector<int> &cs = rbcols[rb];
        for (int i = rb * 16; i < std::min(S.m, rb * 16 + 16); i++) for (int e = S.Gt_ptr[i]; e < S.Gt_ptr[i + 1]; e++) cs.push_back(S.Gt_col[e]);
        std::sort(cs.begin(), cs.end()); cs.erase(std::unique(cs.begin(), cs.end()), cs.end());
        GT.rbptr[rb + 1] = GT.rbptr[rb] + ((int)cs.size() + 15) / 16;
    }
    GT.nt = GT.rbptr[nrb];
    if (GT.nt > 0 && ((double)S.nnzG >= 0.5 * 256.0 * GT.nt || env_knob("EICOS_GTILES", 1, 0, 2) == 2)) { // (2: tests force it on sparse G)
        GT.on = 1;
        GT.col.assign((size_t)GT.nt * 16, -1); GT.src.assign((size_t)GT.nt * 256 + 1, -1);
        std::vector<int> ccount(S.n, 0);
        for (int rb = 0; rb < nrb; rb++) {
            const std::vector<int> &cs = rbcols[rb];
            for (size_t q = 0; q < cs.size(); q++) { GT.col[(size_t)GT.rbptr[rb] * 16 + q] = cs[q]; ccount[cs[q]]++; }
            for (int i = rb * 16; i < std::min(S.m, rb * 16 + 16); i++)
                for (int e = S.Gt_ptr[i]; e < S.Gt_ptr[i + 1]; e++) {
                    const int q = (int)(std::lower_bound(cs.begin(), cs.end(), S.Gt_col[e]) - cs.begin());
                    GT.src[(size_t)(GT.rbptr[rb] + q / 16) * 256 + tile_op(i - rb * 16, q % 16)] = gv_rel + S.Gt_pos[e];
                }
        }
        GT.W = 8; // contributions per column the kernel adds (fixed width, padded)
        if (*std::max_element(ccount.begin(), ccount.end()) > GT.W) GT.on = 0; // (a column met by more than 8 tiles: keep the ELL products)
        GT.cidx.assign((size_t)S.n * GT.W, -1); // padding
        std::fill(ccount.begin(), ccount.end(), 0);
        if (GT.on) for (int t = 0; t < GT.nt; t++) for (int k = 0; k < 16; k++) { const int j = GT.col[(size_t)t * 16 + k]; if (j >= 0) GT.cidx[(size_t)j * GT.W + ccount[j]++] = t * 16 + k; }
    }
    return GT;
}

// ---- device form of the slice tables (PackedSlice) and 16-bit gather indices ----
// One 8-byte entry per lane and slice = its ELL_KMAX gather indices; entry position = off16 of the slice + lane;
// the entry after the last slice is all padding (read by inactive lanes).  Used when every index fits 16 bits (else *ok = false).
std::vector<int> lane_offsets(const std::vector<SliceMeta> &sl, int &dummy) {
    std::vector<int> off16(sl.size());
    int pos = 0;
    for (size_t i = 0; i < sl.size(); i++) { off16[i] = pos; pos += sl[i].cnt << sl[i].lg; }
    dummy = pos;
    return off16;
}
std::vector<int> pack16(const std::vector<SliceMeta> &sl, const std::vector<int> &off16, int dummy, const std::vector<int> &idx, int pad, bool *ok) {
    std::vector<int> words(((size_t)dummy + 1) * 2, 0); // two 32-bit words = four 16-bit indices per lane entry
    auto set = [&](size_t entry, int kk, int v) {
        if (v < 0 || v > 65535) { *ok = false; v = 0; }
        words[entry * 2 + (kk >> 1)] |= v << (16 * (kk & 1));
    };
    for (size_t i = 0; i < sl.size(); i++) {
        const int lanes = sl[i].cnt << sl[i].lg;
        for (int t = 0; t < lanes; t++)
            for (int kk = 0; kk < ELL_KMAX; kk++)
                set((size_t)off16[i] + t, kk, kk < sl[i].K ? idx[(size_t)sl[i].off + (size_t)kk * lanes + t] : pad);
    }
    for (int kk = 0; kk < ELL_KMAX; kk++) set((size_t)dummy, kk, pad);
    return words;
}
std::vector<int> meta_ints(const std::vector<SliceMeta> &v, const std::vector<int> &off16) {
    std::vector<int> o(v.size() * 4);
    for (size_t i = 0; i < v.size(); i++) {
        const PackedSlice ps = pack_slice(v[i], off16.empty() ? 0 : off16[i]);
        std::memcpy(o.data() + 4 * i, &ps, sizeof ps);
    }
    return o;
}

// The plan step, in three parts that share the intermediate arrays: slab layouts and the sliced-ELL plans of the products
// (layout_and_products), the sweep and factor programs (programs), the pattern image (pool_image).  Pure host code.
struct Planner {
    const ProblemPattern &P; const Symbolic &S; const TilePlan &TP; Plan &pl; DevPat &D;
    const int batch, n_cu, profile;
    const bool tile;  // some part of L lives in 16 x 16 tiles: all of it (S.tile == 1) or the top block (hybrid, == 2)
    const bool tile1; // pure tile mode: no scalar programs at all
    const int NV;     // length of the KKT-space vectors on the device: dim_K in elimination order, or (tile mode) the blocks padded to 16
    SlabLayout Wl;    // the workspace slab
    std::vector<int> zexp0;
    GTiles GT;
    EllPlan pcag, prA, prG;
    std::vector<int> cag_idx_k, cag_idx_yz, cag_src, rA_idx, rA_src, rG_idx, rG_src, rA_idx_k, rG_idx_k, ipx, ipy, ipz, ipv, ipu;
    TriPlan planF, planB;
    FactorPlan planX;
    std::vector<int> col_of;
    std::vector<int> f_w16, b_w16, cag_k_w16, cag_yz_w16, rA_w16, rA_k_w16, rG_w16, rG_k_w16, fac_w16, fac_w16d, fac_k16;
    std::vector<int> fsl_i, bsl_i, fac_sl_i, cag_sl_i, rA_sl_i, rG_sl_i;

    Planner(const ProblemPattern &P_, const Analysis &an, Plan &pl_, int batch_, int n_cu_, int profile_)
        : P(P_), S(an.sym), TP(an.tiles), pl(pl_), D(pl_.dp), batch(batch_), n_cu(n_cu_), profile(profile_),
          tile(an.sym.tile != 0), tile1(an.sym.tile == 1), NV(an.sym.tile != 0 ? an.tiles.N16 : an.sym.N) {}
    int posK(int old) const { return tile ? TP.slot[S.iperm[old]] : S.iperm[old]; } // KKT index -> device slot
    int srcoff(int kind, int src) const {
        switch (kind) {
        case SRC_A: return D.i_Av + src;
        case SRC_G: return D.i_Gv + src;
        case SRC_V: return D.i_Vv + src;
        case SRC_POSDELTA: return D.i_cst + 0;
        case SRC_NEGDELTA: return D.i_cst + 1;
        default: return D.i_cst + 2;
        }
    }
    int layout_and_products();
    int programs();
    void pool_image();
};

int Planner::layout_and_products() {
    D.n = S.n; D.p = S.p; D.m = S.m; D.l = S.l; D.nc = S.nc; D.N = NV; D.mt = S.mt; D.nV = S.nV;
    D.nnzA = S.nnzA; D.nnzG = S.nnzG; D.nnzL = S.nnzL; D.nlev = S.nlev;

    // ---- slab layouts ----
    SlabLayout L;
    D.i_Av = L.add(S.nnzA); D.i_Gv = L.add(S.nnzG);
    // sliced-ELL plans of the matrix-vector products
    std::vector<int> cag_ptr(S.n + 1, 0), cag_val, cag_k, cag_yz; // stacked columns of [A; G]
    zexp0.assign(S.m, 0);
    { for (int i = 0; i < S.l; i++) zexp0[i] = i; for (int c = 0; c < S.nc; c++) for (int k = 0; k < S.q[c]; k++) zexp0[S.cone_off[c] + k] = S.cone_off[c] + k + 2 * c; }
    const int gv_rel = D.i_Gv - D.i_Av;
    GT = plan_g_tiles(S, gv_rel);
    const std::vector<int> Gt_ptr_used = GT.on ? std::vector<int>(S.m + 1, 0) : S.Gt_ptr; // (rows without entries: the epilogue still runs)
    for (int j = 0; j < S.n; j++) {
        for (int k = P.Ajc[j]; k < P.Ajc[j + 1]; k++) { cag_val.push_back(k); cag_k.push_back(S.n + P.Air[k]); cag_yz.push_back(P.Air[k]); }
        if (!GT.on) for (int k = P.Gjc[j]; k < P.Gjc[j + 1]; k++) { cag_val.push_back(gv_rel + k); cag_k.push_back(S.n + S.p + zexp0[P.Gir[k]]); cag_yz.push_back(-1 - P.Gir[k]); }
        cag_ptr[j + 1] = (int)cag_val.size();
    }
    pcag = build_ell_plan(cag_ptr, S.n, pl.threads); prA = build_ell_plan(S.At_ptr, S.p, pl.threads);
    prG = build_ell_plan(Gt_ptr_used, S.m, pl.threads);
    D.cag_ns = (int)pcag.sl.size(); D.rA_ns = (int)prA.sl.size(); D.rG_ns = (int)prG.sl.size();
    {   auto real = [](const std::vector<SliceMeta> &sl) { int c = (int)sl.size(); while (c > 0 && sl[(size_t)c - 1].cnt == 0) c--; return c; };
        D.cag_ns_r = real(pcag.sl); D.rA_ns_r = real(prA.sl); D.rG_ns_r = real(prG.sl); }
    D.cag_slots = pcag.slots; D.rA_slots = prA.slots; D.rG_slots = prG.slots;
    D.i_cag = L.add((size_t)pcag.slots + 8); D.i_rA = L.add((size_t)prA.slots + 8); D.i_rG = L.add((size_t)prG.slots + 8);
    D.gt_on = GT.on; D.gt_nrb = GT.nrb; D.gt_nt = GT.nt; D.gt_W = GT.W;
    D.i_Gt = GT.on ? (int)L.add((size_t)GT.nt * 256 + 8) : 0;
    D.i_c = L.add((size_t)S.n + S.p + S.m); D.i_b = D.i_c + S.n; D.i_h = D.i_b + S.p; // [c | b | h]: one array in [x | y | z] order (kkt_solve's epilogue)
    D.i_xe = L.add(S.n); D.i_ae = L.add(S.p); D.i_ge = L.add(S.m);
    D.i_Vv = L.add(S.nV); D.i_cst = L.add(4);
    D.i_x = L.add(S.n); D.i_y = L.add(S.p); D.i_z = L.add(S.m); D.i_s = L.add(S.m);
    D.i_info = L.add(DEVINFO_DOUBLES);
    cag_idx_k.resize(pcag.src.size()); cag_idx_yz.resize(pcag.src.size()); cag_src.resize(pcag.src.size());
    for (size_t sl = 0; sl < pcag.src.size(); sl++) {
        const int e = pcag.src[sl];
        cag_src[sl] = e < 0 ? -1 : cag_val[e];
        cag_idx_k[sl] = e < 0 ? NV : posK(cag_k[e]);                         // elimination order; padding -> zero slot N
        cag_idx_yz[sl] = e < 0 ? 0 : (cag_yz[e] >= 0 ? cag_yz[e] : (D.i_z - D.i_y) + (-1 - cag_yz[e])); // offset from y
    }
    rA_idx.resize(prA.src.size()); rA_src.resize(prA.src.size()); rG_idx.resize(prG.src.size()); rG_src.resize(prG.src.size());
    rA_idx_k.resize(prA.src.size()); rG_idx_k.resize(prG.src.size());
    for (size_t sl = 0; sl < prA.src.size(); sl++) { const int e = prA.src[sl]; rA_src[sl] = e < 0 ? -1 : S.At_pos[e]; rA_idx[sl] = e < 0 ? 0 : S.At_col[e]; rA_idx_k[sl] = e < 0 ? NV : posK(S.At_col[e]); }
    for (size_t sl = 0; sl < prG.src.size(); sl++) { const int e = prG.src[sl]; rG_src[sl] = e < 0 ? -1 : gv_rel + S.Gt_pos[e]; rG_idx[sl] = e < 0 ? 0 : S.Gt_col[e]; rG_idx_k[sl] = e < 0 ? NV : posK(S.Gt_col[e]); }
    ipx.resize(S.n); ipy.resize(S.p); ipz.resize(S.m); ipv.resize(S.nc); ipu.resize(S.nc);
    for (int j = 0; j < S.n; j++) ipx[j] = posK(j);
    for (int r = 0; r < S.p; r++) ipy[r] = posK(S.n + r);
    for (int i = 0; i < S.m; i++) ipz[i] = posK(S.n + S.p + zexp0[i]);
    for (int c = 0; c < S.nc; c++) { const int e0 = S.n + S.p + S.cone_off[c] + 2 * c + S.q[c]; ipv[c] = posK(e0); ipu[c] = posK(e0 + 1); }
    D.inst_stride = L.size;
    // second buffer set of the iterate (ShI::cur / best in kernels.hip): same spacing of y and z as in the instance slab -- the stacked
    // product [A' G'] gathers (y, z) through ONE index array relative to y
    D.w_lam = Wl.add(S.m); D.w_bx = Wl.add(S.n); D.w_by = Wl.add(S.p); D.w_bz = Wl.add(S.m); D.w_bs = Wl.add(S.m);
    if (D.w_bz - D.w_by != D.i_z - D.i_y) return fail(EICOS_E_INVALID, "internal: the two buffer sets of the iterate are laid out differently");
    D.w_rz = Wl.add(S.m);
    D.w_rhs1k = Wl.add((size_t)S.n + S.p + S.m); D.w_rhs2k = Wl.add((size_t)S.n + S.p + S.m);       // [x | y | z] order
    D.w_dx1 = Wl.add((size_t)S.n + S.p + S.m); D.w_dy1 = D.w_dx1 + S.n; D.w_dz1 = D.w_dy1 + S.p; // [dx | dy | dz]: one array each
    D.w_dx2 = Wl.add((size_t)S.n + S.p + S.m); D.w_dy2 = D.w_dx2 + S.n; D.w_dz2 = D.w_dy2 + S.p;
    D.w_dsw = Wl.add(S.m); D.w_wdz = Wl.add(S.m); D.w_dsa = Wl.add(S.m); D.w_t1 = Wl.add(S.m); D.w_t2 = Wl.add(S.m);
    D.w_lpw = Wl.add(S.l); D.w_lpv = Wl.add(S.l); D.w_csc = Wl.add((size_t)S.nc * CSC_STRIDE); D.w_qv = Wl.add(S.m);
    D.w_trace = Wl.add((size_t)TRACE_ROWS * TRACE_COLS);
    if (GT.on) { // G tile products: partial column sums per tile, G'z per column, G x per row; two right-hand sides
        D.w_gpart = Wl.add((size_t)GT.nt * 16 * 2); D.w_gx = Wl.add((size_t)S.n * 2); D.w_gz = Wl.add((size_t)S.m * 2);
    } else D.w_gpart = D.w_gx = D.w_gz = 0;
    // ---- the arrays of the factorisation / KKT solve ----
    D.w_xk = Wl.add((size_t)NV + 16); D.w_ek = Wl.add((size_t)NV + 16); D.w_dxr = Wl.add(NV);
    D.w_D = Wl.add(NV); D.w_invD = Wl.add((size_t)NV + 8); // (+ the always-zero slot fac_kpad of the deferred-L factorisation) // w_UF / w_UB are added once the slice plans are known
    return EICOS_OK;
}

int Planner::programs() {
    // ---- sliced-ELL plans of the two triangular sweeps (device_types.hpp: SliceMeta) ----
    // (tile mode: the sweeps and the factorisation run over the tile plan instead; the scalar plans stay empty)
    // A handle of at most one workgroup per CU gives NO level to a single wavefront: the idle wavefronts of such a part are issue slots for a
    // neighbour on the CU -- without one, every extra sweep call only adds a cold start (lp_bandm +2.2 %, lp_beaconfd +2.6 %, lp_blend +4 %,
    // lp_adlittle +2 %, lp_agg +0.6 %, lp_25fv47 +-0; MPC02 at three per CU -3 ... -7 %, which keeps its single-wavefront tree top)
    const bool solo_ok = batch > n_cu || profile == 1;
    if (!tile1) { planF = build_tri_plan(S, pl.threads, true, solo_ok, pl.apex); planB = build_tri_plan(S, pl.threads, false, solo_ok, pl.apex); }
    else { planF.idx.assign(1, NV); planB.idx.assign(1, NV); planF.pos.assign(S.nnzL, 0); planB.pos.assign(S.nnzL, 0); }
    D.nfs = planF.n_wide; D.nbs = planB.n_wide; D.nfs_solo = planF.n_solo; D.nbs_solo = planB.n_solo; D.nfs_ext = planF.n_ext; D.nUF = planF.slots; D.nUB = planB.slots;
    {   // the real slices of every section: its length without the trailing padding (empty slices)
        auto real = [](const std::vector<SliceMeta> &sl, int first, int count) { while (count > 0 && sl[(size_t)first + count - 1].cnt == 0) count--; return count; };
        // forward plan = [wide | solo | ext], backward plan = [solo | wide] (plans.cpp)
        D.nfs_r = real(planF.sl, 0, planF.n_wide); D.nfs_solo_r = real(planF.sl, planF.n_wide, planF.n_solo); D.nfs_ext_r = real(planF.sl, planF.n_wide + planF.n_solo, planF.n_ext);
        D.nbs_solo_r = real(planB.sl, 0, planB.n_solo); D.nbs_r = real(planB.sl, planB.n_solo, planB.n_wide);
    }
    // every section of a sweep plan is a whole number of queue-depth trips (tri_sweep's remainder loop executes full trips)
    if (D.nfs % TRI_DEPTH || D.nbs % TRI_DEPTH || D.nfs_ext % TRI_DEPTH || D.nfs_solo % TRI_DEPTH_SOLO || D.nbs_solo % TRI_DEPTH_SOLO)
        return fail(EICOS_E_INVALID, "internal: a section of a sweep plan is not padded to its queue depth");
    // (value arrays: the plan's slots + the dummy slot, then -- dense apex -- the folded image of the block's own entries (APEX_IMG doubles), zero wherever no
    // entry of L lands: the work slabs are zeroed at creation and the factor program only ever writes entry slots)
    D.w_UF = Wl.add((size_t)planF.ulen + 8); D.w_UB = Wl.add((size_t)planB.ulen + 8);
    const bool apex = !tile && pl.apex;
    D.apex_na = apex ? S.N - S.apex0 : 0; D.apex_n0 = apex ? S.apex0 : 0; D.apex_f = planF.apex_base; D.apex_b = planB.apex_base;
    D.apex_split_n = apex ? planF.split_n : 0; D.apex_split_slot = planF.split_slot0; D.apex_split_lane = planF.split_row - D.apex_n0;
    // (the parts' pseudo-rows N + 1 ... use the spare slots of the sweep vector: checked here against the plan's own bound and below, where the
    // vector's stride D.Npad is fixed, against that stride itself)
    if (D.apex_split_n > 0 && (tile || planF.split_slot0 + planF.split_n > scalar_npad(NV))) return fail(EICOS_E_INVALID, "internal: the split row of the apex does not fit the spare slots of the sweep vector");
    pl.posB = planB.pos; pl.ub_len = planB.ulen;
    // numeric factorisation program: reads L.*D through the backward (column) slots; slot nUB is the zero dummy
    if (!tile1) planX = build_factor_plan(S, pl.threads, planB.pos, planB.slots, planF.pos, planF.slots);
    else { planX.pa.assign(1, 0); planX.pb.assign(1, 0); planX.pbU.assign(1, 0); planX.pk.assign(1, 0); }
    D.fac_ns = (int)planX.sl.size(); D.fac_slots = planX.slots; D.fac_nt = (int)planX.target.size();
    if ((long long)planB.ulen + 1 >= IMG_BASE || (long long)S.N >= DIAG_POS / 2) return fail(EICOS_E_UNSUPPORTED, "pattern too large for the factor program's destination codes");
    {   // level 0 of the factor program: the leaves of the elimination tree have no pairs; the kernel streams over their targets
        // (diagonals first: the per-level task order is stable for equal pair counts) instead of walking their slices
        D.fac_s1 = 0; D.fac_nd0 = 0; D.fac_nt0 = 0;
        if (!tile1 && !planX.sl.empty()) {
            size_t s1 = 1;
            while (s1 < planX.sl.size() && !(planX.sl[s1].newlev & 1)) s1++;
            const int nt0 = s1 < planX.sl.size() ? planX.sl[s1].row0 : (int)planX.target.size();
            bool pairless = true, diag_first = true;
            int nd0 = 0;
            for (int t = 0; t < nt0; t++) {
                const int tgt = planX.target[t];
                if (S.tp[tgt + 1] != S.tp[tgt]) pairless = false;
                if (tgt < S.N) { if (t != nd0) diag_first = false; nd0++; }
            }
            if (pairless && diag_first) { D.fac_s1 = (int)s1; D.fac_nd0 = nd0; D.fac_nt0 = nt0; }
        }
    }
    // (shared factor operands: what the plan allows; the fields stay off here -- allocate() turns them on for the handles that take the path)
    if (!tile1) pl.shop = plan_shared_operands(S, planB, planX, D.fac_s1, D.fac_nd0, D.fac_nt0);
    D.ub0 = nullptr; D.kt0 = nullptr; D.ub0_off = 0x7fffffff; D.kt0_pass = 0;
    // KKT entries in target order: the factor's only per-target value stream; tile mode: the dense tile image
    D.w_Kt = Wl.add((tile1 ? (size_t)(TP.nb + TP.nt) * 256 : planX.target.size()) + 8);
    D.w_Kimg = tile1 ? D.w_Kt : (tile ? Wl.add((size_t)(TP.nb + TP.nt) * 256 + 8) : 0); // hybrid: the top block's image beside the scalar stream
    D.tile = S.tile; D.nb = TP.nb; D.nt = TP.nt; D.nblev = TP.nblev; D.tl_base = TP.n0;
    if (tile) { // unit-lower L tiles column-major (LC) and row-major (LR), the strictly lower part of the diagonal tiles (DL)
        D.w_LC = Wl.add((size_t)TP.nt * 256 + 256); D.w_LR = Wl.add((size_t)TP.nt * 256 + 256); // (+ one tile: the dummy loads of padding operations read tile 0)
        D.w_DL = Wl.add((size_t)TP.nb * 256);
    }
    D.w_dual_xk = Wl.add(2 * ((size_t)NV + 16)); D.w_dual_ek = Wl.add(2 * ((size_t)NV + 16)); // dual right-hand-side solves
    D.work_stride = Wl.size;
    col_of.resize(S.nnzL);
    for (int j = 0; j < S.N; j++) for (int e = S.Lp[j]; e < S.Lp[j + 1]; e++) col_of[e] = j;
    // the slice tables in device form (PackedSlice) and their 16-bit gather indices
    bool idx16_ok = true;
    const std::vector<int> f_o16 = lane_offsets(planF.sl, D.f_d16), b_o16 = lane_offsets(planB.sl, D.b_d16);
    const std::vector<int> cag_o16 = lane_offsets(pcag.sl, D.cag_d16), rA_o16 = lane_offsets(prA.sl, D.rA_d16), rG_o16 = lane_offsets(prG.sl, D.rG_d16);
    f_w16 = pack16(planF.sl, f_o16, D.f_d16, planF.idx, NV, &idx16_ok); b_w16 = pack16(planB.sl, b_o16, D.b_d16, planB.idx, NV, &idx16_ok);
    cag_k_w16 = pack16(pcag.sl, cag_o16, D.cag_d16, cag_idx_k, NV, &idx16_ok); cag_yz_w16 = pack16(pcag.sl, cag_o16, D.cag_d16, cag_idx_yz, 0, &idx16_ok);
    rA_w16 = pack16(prA.sl, rA_o16, D.rA_d16, rA_idx, 0, &idx16_ok); rA_k_w16 = pack16(prA.sl, rA_o16, D.rA_d16, rA_idx_k, NV, &idx16_ok);
    rG_w16 = pack16(prG.sl, rG_o16, D.rG_d16, rG_idx, 0, &idx16_ok); rG_k_w16 = pack16(prG.sl, rG_o16, D.rG_d16, rG_idx_k, NV, &idx16_ok);
    // factor program: the (pa, pb) slot pairs of a lane, 16 bytes per lane and slice (pa words then pb words)
    const std::vector<int> x_o16 = lane_offsets(planX.sl, D.fac_d16);
    {
        const std::vector<int> wa = pack16(planX.sl, x_o16, D.fac_d16, planX.pa, planB.slots, &idx16_ok), wb = pack16(planX.sl, x_o16, D.fac_d16, planX.pb, planF.slots, &idx16_ok);
        const std::vector<int> wu = pack16(planX.sl, x_o16, D.fac_d16, planX.pbU, planB.slots, &idx16_ok); // deferred-L form: both operands are UB slots
        fac_k16 = pack16(planX.sl, x_o16, D.fac_d16, planX.pk, S.N, &idx16_ok);                             // ... and the pivot column of every pair
        fac_w16.resize(wa.size() * 2); fac_w16d.resize(wa.size() * 2);
        for (size_t e = 0; e * 2 < wa.size(); e++) {
            fac_w16[4 * e] = wa[2 * e]; fac_w16[4 * e + 1] = wa[2 * e + 1]; fac_w16[4 * e + 2] = wb[2 * e]; fac_w16[4 * e + 3] = wb[2 * e + 1];
            fac_w16d[4 * e] = wa[2 * e]; fac_w16d[4 * e + 1] = wa[2 * e + 1]; fac_w16d[4 * e + 2] = wu[2 * e]; fac_w16d[4 * e + 3] = wu[2 * e + 1];
        }
    }
    D.idx16 = (idx16_ok && env_knob("EICOS_IDX16", 1, 0, 1)) ? 1 : 0;
    fsl_i = meta_ints(planF.sl, f_o16); bsl_i = meta_ints(planB.sl, b_o16); fac_sl_i = meta_ints(planX.sl, x_o16);
    for (size_t i = 0; i < pl.shop.slice_static.size(); i++) if (pl.shop.slice_static[i]) fac_sl_i[4 * i + 3] |= 1 << PS_STATIC; // (PackedSlice::bits)
    cag_sl_i = meta_ints(pcag.sl, cag_o16); rA_sl_i = meta_ints(prA.sl, rA_o16); rG_sl_i = meta_ints(prG.sl, rG_o16);
    return EICOS_OK;
}

// the pattern arrays, in the order they enter the pool (that order fixes pattern_bytes and the pool's contents)
void Planner::pool_image() {
    auto put = [&](const int *&field, const std::vector<int> &v) { pl.put(field, v); };
    std::vector<int> zdsign(S.m, 1), cone_vbase(S.nc), cone_small, cone_big;
    {
        int vb = S.l;
        for (int c = 0; c < S.nc; c++) {
            const int o = S.cone_off[c], d = S.q[c];
            zdsign[o + d - 1] = -1; // last cone row: -delta in the refinement operator (ref src/eicos.cpp:1552)
            cone_vbase[c] = vb; vb += 3 * d + 1;
            (d >= CONE_BIG ? cone_big : cone_small).push_back(c);
        }
    }
    put(D.Ajc, P.Ajc); put(D.Air, P.Air); put(D.At_ptr, S.At_ptr); put(D.At_pos, S.At_pos);
    put(D.Gjc, P.Gjc); put(D.Gir, P.Gir); put(D.Gt_ptr, S.Gt_ptr); put(D.Gt_pos, S.Gt_pos);
    {
        std::vector<int> Acol(S.nnzA), Gcol(S.nnzG);
        for (int j = 0; j < S.n; j++) { for (int k = P.Ajc[j]; k < P.Ajc[j + 1]; k++) Acol[k] = j; for (int k = P.Gjc[j]; k < P.Gjc[j + 1]; k++) Gcol[k] = j; }
        put(D.Acol, Acol); put(D.Gcol, Gcol);
    }
    put(D.cq, S.q); put(D.cone_off, S.cone_off); put(D.cone_vbase, cone_vbase); put(D.cone_small, cone_small); put(D.cone_big, cone_big);
    D.n_small = (int)cone_small.size(); D.n_big = (int)cone_big.size();
    {   // tiny cones (dimension <= TINY_D): descriptor table for the register-resident cone loops; the rest of the small cones
        std::vector<int> tiny_tab, cone_mid;
        for (int c : cone_small) {
            const int d = S.q[c], o = S.cone_off[c];
            if (d > TINY_D) { cone_mid.push_back(c); continue; }
            int rec[TINY_INTS] = {o, d, c, ipv[c], ipu[c], 0, 0, 0, 0, cone_vbase[c], 0, 0};
            for (int k = 0; k < TINY_D; k++) rec[5 + k] = ipz[o + std::min(k, d - 1)]; // (slots past the dimension repeat the last row: loads stay in range)
            tiny_tab.insert(tiny_tab.end(), rec, rec + TINY_INTS);
        }
        D.n_tiny = (int)tiny_tab.size() / TINY_INTS; D.n_mid = (int)cone_mid.size();
        put(D.cone_tiny, tiny_tab); put(D.cone_mid, cone_mid);
        std::vector<int> cone_wave, cone_huge;
        for (int c : cone_big) (S.q[c] <= 64 ? cone_wave : cone_huge).push_back(c);
        D.n_wave = (int)cone_wave.size(); D.n_huge = (int)cone_huge.size();
        put(D.cone_wave, cone_wave); put(D.cone_huge, cone_huge);
    }
    put(D.zdsign, zdsign);
    put(D.f_idx, planF.idx); put(D.b_idx, planB.idx);
    put(D.f_idx16, f_w16); put(D.b_idx16, b_w16); put(D.cag_k16, cag_k_w16); put(D.cag_yz16, cag_yz_w16);
    put(D.rA_16, rA_w16); put(D.rA_k16, rA_k_w16); put(D.rG_16, rG_w16); put(D.rG_k16, rG_k_w16);
    put(pl.fsl, fsl_i); put(pl.bsl, bsl_i); put(pl.cag_sl, cag_sl_i); put(pl.rA_sl, rA_sl_i); put(pl.rG_sl, rG_sl_i);
    put(D.cag_idx_k, cag_idx_k); put(D.cag_idx_yz, cag_idx_yz); put(D.cag_src, cag_src);
    put(D.rA_idx, rA_idx); put(D.rA_src, rA_src); put(D.rG_idx, rG_idx); put(D.rG_src, rG_src);
    put(D.rA_idx_k, rA_idx_k); put(D.rG_idx_k, rG_idx_k);
    {   // G tiles: columns of a tile as variable index and as elimination-order slot, slot of every row's z entry
        std::vector<int> gt_colk(GT.col.size()), gt_zslot((size_t)GT.nrb * 16, NV);
        for (size_t q = 0; q < GT.col.size(); q++) gt_colk[q] = GT.col[q] < 0 ? NV : posK(GT.col[q]);
        if (GT.on) for (int i = 0; i < S.m; i++) gt_zslot[i] = posK(S.n + S.p + zexp0[i]);
        put(D.gt_rbptr, GT.rbptr); put(D.gt_col, GT.col); put(D.gt_colk, gt_colk); put(D.gt_zslot, gt_zslot); put(D.gt_cidx, GT.cidx); put(D.gt_src, GT.src);
    }
    put(D.ipx, ipx); put(D.ipy, ipy); put(D.ipz, ipz); put(D.ipv, ipv); put(D.ipu, ipu);
    std::vector<int> ipk(ipx); ipk.insert(ipk.end(), ipy.begin(), ipy.end()); ipk.insert(ipk.end(), ipz.begin(), ipz.end());
    put(D.ipk, ipk);
    std::vector<int> zpos; // sweep-vector slots no x / y / z entry lands in: cone expansions, padding (inside the blocks in tile layouts)
    {
        std::vector<char> hit((size_t)D.Npad, 0);
        for (int o : ipk) hit[o] = 1;
        for (int i = 0; i < D.Npad; i++) if (!hit[i]) zpos.push_back(i);
    }
    D.nzpos = (int)zpos.size();
    put(D.zpos, zpos);
    // quasi-definite sign of pivot `pos` (elimination position): + for the x block and the u expansion of every cone
    // (ref setupKKT :1734-1890), - elsewhere; only used by the dynamic-regularisation extension
    auto pivot_positive = [&](int pos) {
        const int orig = S.perm[pos];
        if (orig < S.n) return true;
        int k = S.n + S.p + S.l;
        for (int c = 0; c < S.nc; c++) { if (orig == k + S.q[c] + 1) return true; k += S.q[c] + 2; }
        return false;
    };
    std::vector<int> fac_src(planX.target.size()), fac_dst(planX.target.size()), fac_dstF(planX.target.size()), fac_col(planX.target.size(), 0);
    for (size_t t = 0; t < planX.target.size(); t++) {
        const int tgt = planX.target[t];
        if (tgt < S.N) { fac_src[t] = srcoff(S.Dkind[tgt], S.Dsrc[tgt]); fac_dst[t] = -tgt - 1 - (pivot_positive(tgt) ? DIAG_POS : 0); fac_dstF[t] = 0; }
        else { const int e = tgt - S.N; fac_src[t] = srcoff(S.Lkind[e], S.Lsrc[e]); fac_dst[t] = planB.pos[e]; fac_dstF[t] = planF.pos[e]; fac_col[t] = col_of[e]; }
        // hybrid: the targets of the top block (their pairs stop at column n0) are the tile factorisation's input image
        if (S.tile == 2 && tgt < S.N && tgt >= S.n0) { fac_dst[t] = IMG_BASE + TP.D_img[tgt]; fac_dstF[t] = -1; }
        if (S.tile == 2 && tgt >= S.N && col_of[tgt - S.N] >= S.n0) { fac_dst[t] = IMG_BASE + TP.Le_img[tgt - S.N]; fac_dstF[t] = -1; }
    }
    std::vector<int> v2t(std::max(S.nV, 1), D.fac_nt); // entries that are no target (none by construction) -> spare slot
    for (size_t t = 0; t < planX.target.size(); t++)
        if (fac_src[t] >= D.i_Vv && fac_src[t] < D.i_Vv + S.nV) v2t[fac_src[t] - D.i_Vv] = (int)t;
    // ---- tile mode: where every KKT entry lands in the dense tile image, pivot signs, the tile program ----
    std::vector<int> img_dst, img_src, psign(tile ? NV : 0, 1);
    if (tile) {
        for (int j = 0; j < S.N; j++) psign[TP.slot[j]] = pivot_positive(j) ? 1 : -1;
        if (tile1) { // the image is filled straight from the instance slab (hybrid: by the scalar factor program)
            for (int j = 0; j < S.N; j++) {
                img_dst.push_back(TP.D_img[j]); img_src.push_back(srcoff(S.Dkind[j], S.Dsrc[j]));
                if (S.Dkind[j] == SRC_V) v2t[S.Dsrc[j]] = TP.D_img[j];
            }
            for (int e = 0; e < S.nnzL; e++) {
                if (S.Lkind[e] == SRC_ZERO) continue; // fill: stays 0 in the image
                img_dst.push_back(TP.Le_img[e]); img_src.push_back(srcoff(S.Lkind[e], S.Lsrc[e]));
                if (S.Lkind[e] == SRC_V) v2t[S.Lsrc[e]] = TP.Le_img[e];
            }
        }
        for (int d : TP.pad_img) { img_dst.push_back(d); img_src.push_back(D.i_cst + 3); } // padding nodes: identity rows
    }
    D.tl_nimg = (int)img_dst.size();
    put(D.tl_img_dst, img_dst); put(D.tl_img_src, img_src); put(D.tl_psign, psign);
    put(D.tl_blev, TP.blev_ptr); put(D.tl_tgt_lev, TP.tgt_lev_ptr); put(D.tl_tgt, TP.tgt); put(D.tl_tp, TP.tp_ptr);
    put(D.tl_pa, TP.pa); put(D.tl_pb, TP.pb); put(D.tl_pk, TP.pk); put(D.tl_fin_lev, TP.fin_lev_ptr); put(D.tl_fin, TP.fin);
    TileSweeps TSW;
    // (hybrid patterns whose vectors certainly live in LDS -- a serially swept block system relies on the in-order LDS accesses of one wavefront)
    if (tile) TSW = build_tile_sweeps(TP, pl.threads / 64, TILE_STRIP, (S.tile == 2 && TP.N16 <= 4096) ? env_knob("EICOS_TILE_SERIAL_MAX", 48, 0, 100000) : 0);
    put(D.tl_fops, TSW.fops); put(D.tl_bops, TSW.bops); put(D.tl_fptr, TSW.fptr); put(D.tl_bptr, TSW.bptr);
    put(D.tl_fsplit, TSW.fsplit); put(D.tl_bsplit, TSW.bsplit); put(D.tl_fend, TSW.fend); put(D.tl_bend, TSW.bend);
    TileFactorOps TFO;
    if (tile) {
        // pure tile mode: tiles of the K image no KKT entry lands in (targets that exist through fill only) start from zero without
        // a load; the image tile they would have read stays zero and is never touched (hybrid: the scalar program writes every tile)
        std::vector<char> img_zero((size_t)TP.nb + TP.nt, tile1 ? 1 : 0);
        for (int d : img_dst) img_zero[d / 256] = 0;
        TFO = build_tile_factor_ops(TP, pl.threads / 64, TILE_FTRIP, &img_zero);
    }
    put(D.tl_facops, TFO.ops); put(D.tl_facptr, TFO.ptr);
    put(D.tl_ident, TP.ident);
    put(D.tl_trow, TP.t_row); put(D.tl_tcol, TP.t_col); put(D.tl_tc_ptr, TP.tc_ptr); put(D.tl_tr_ptr, TP.tr_ptr); put(D.tl_tr_tile, TP.tr_tile);
    put(D.v2t, v2t);
    put(pl.fac_sl, fac_sl_i);
    // (stored-L / deferred-L forms of the factor operands: the launch shape chooses, allocate() points DevPat at one)
    put(D.fac_pa, planX.pa); put(pl.fac_pb_f, planX.pb); put(pl.fac_pb_u, planX.pbU); put(pl.fac_p16_f, fac_w16); put(pl.fac_p16_u, fac_w16d);
    put(D.fac_pk, planX.pk); put(D.fac_k16, fac_k16);
    put(D.fac_src, fac_src); put(D.fac_dst, fac_dst); put(D.fac_dstF, fac_dstF); put(D.fac_col, fac_col);
}

} // namespace

int analyse(const ProblemPattern &P, int batch, int n_cu, int profile, Analyses &A) {
    // (experiment knobs, envknob.hpp: honoured only under EICOS_EXPERIMENT=1, range-checked)
    const int order = env_knob("EICOS_ORDER", -1, 0, 16), tiles = env_knob("EICOS_TILES", -1, 0, 2);
    try {
        A.main.sym = analyze(P, order, tiles);
        if (A.main.sym.tile) A.main.tiles = build_tile_plan(A.main.sym);
    } catch (const std::invalid_argument &e) { return fail(EICOS_E_INVALID, e.what()); }
    catch (const std::runtime_error &e) { return fail(EICOS_E_UNSUPPORTED, e.what()); }
    catch (const std::exception &e) { return fail(EICOS_E_INVALID, e.what()); }
    const Symbolic &S = A.main.sym;
    // workgroup size by problem size (measured, batch 256: dim_K 129 -> 128, 1249 -> 256, >= 3815 -> 512 threads);
    // batches beyond one workgroup per CU are throughput-bound: 256 threads issue a third fewer wavefront-slices
    // per instance than 512 and fit three workgroups per CU (MPC02 pattern: 500 k vs 414 k iterations/s)
    const int dimK = P.n + P.p + P.m + 2 * P.nc;
    // (sparse factors only: with ~50 entries per row of L -- the dense-front config -- 512 threads stay ahead)
    // (arithmetic profile 1: every choice that shapes a PLAN -- and with it the order of the floating-point operations -- is made as for a
    // batch beyond one workgroup per CU, whatever the batch really is: workgroup size by pattern size alone, no dense apex, the
    // single-wavefront tree top; the launch shape itself -- grid, LDS residency, dual solves, which are bit-neutral -- follows the real batch)
    const bool as_large = profile == 1;
    const bool throughput_bound = (batch > n_cu || as_large) && (long long)S.nnzL < 16LL * S.N;
    // one workgroup per CU (batch <= CUs): latency-bound, more wavefronts per instance pay earlier (measured at batch 256 with
    // the 256-VGPR build of the 512-thread kernels: lp_blend / lp_adlittle, dim_K ~ 300: 256 threads +5..8 % over 128;
    // lp_beaconfd / lp_bandm / lp_agg, dim_K 763..1718: 512 threads +7..12 % over 256)
    const int dflt = throughput_bound ? (dimK < 400 ? 128 : 256) : (dimK < 250 ? 128 : (dimK < 700 ? 256 : 512));
    const int t = env_knob("EICOS_THREADS", dflt, 128, 512);
    if (t != 128 && t != 256 && t != 512) return fail(EICOS_E_INVALID, "EICOS_THREADS must be 128, 256 or 512");
    A.threads = t;
    // ---- dense apex: not under profile 1, not with 128-thread workgroups (small patterns; kernels.hip: apex_on) -- except in the
    // LDS-resident build, whose images then live in the LDS copy of the workspace slab; whether that build is taken is known from the
    // launch shape (eicos_batch_create) ----
    A.apex = profile == 0 && (t >= 256 || (t == 128 && env_knob("EICOS_LDSRES", 1, 0, 1) && batch <= n_cu));
    // small patterns whose narrow tree top would go to the tile path (hybrid): the level schedule + dense apex does better there -- a
    // handful of 16 x 16 blocks costs two workgroup-wide block levels each, the apex swallows the whole tail in 2 x 64 register steps
    // (lp_adlittle 1.13 -> 1.33 M, lp_blend 0.92 -> 1.08 M iter/s at batch 256; larger tops -- lp_bandm, lp_agg, lp_25fv47 -- stay hybrid:
    // their top blocks are dense and the MFMA factorisation of the block is what pays there)
    if (A.apex && S.tile == 2 && S.N < APEX_OVER_HYBRID_BELOW && t >= 256 && tiles < 0) {
        try {
            Symbolic alt = analyze(P, order, 0);
            if (alt.apex0 >= 0) { A.apex_alt.sym = std::move(alt); A.has_alt = true; }
        } catch (const std::exception &) { /* keep the hybrid analysis */ }
    }
    return EICOS_OK;
}

int build_plan(const ProblemPattern &P, Analyses &A, bool apex, int batch, int n_cu, int profile, Plan &pl) {
    Analysis &an = A.for_plan(apex);
    const Symbolic &S = an.sym;
    pl.an = &an; pl.apex = apex && S.apex0 >= 0; pl.threads = A.threads;
    if (S.npairs >= (int64_t)1 << 31) return fail(EICOS_E_UNSUPPORTED, "factor program exceeds 2^31 pairs");
    if (S.tile) { // the tile image, the tile arrays of L and their workspace offsets are indexed with 32-bit ints
        const long long img = ((long long)an.tiles.nb + an.tiles.nt) * 256;
        if (img >= IMG_BASE || (long long)S.N + img >= DIAG_POS / 2 || 3 * img * (long long)sizeof(double) > (8LL << 30))
            return fail(EICOS_E_UNSUPPORTED, "dense-front pattern too large: the tile image of L exceeds the per-workgroup workspace budget");
    }
    Planner pr(P, an, pl, batch, n_cu, profile);
    int rc = pr.layout_and_products();
    if (rc == EICOS_OK) rc = pr.programs();
    if (rc != EICOS_OK) return rc;
    DevPat &D = pl.dp;
    D.Npad = pr.tile ? pr.NV + 16 : (pr.NV + 1 + 15) & ~15; // >= N+1: slot N is the always-zero target of ELL padding (tile mode: a whole zero block)
    if (D.apex_split_n > 0 && D.apex_split_slot + D.apex_split_n > D.Npad) return fail(EICOS_E_INVALID, "internal: the split row of the apex runs past the sweep vector's stride");
    pr.pool_image();
    return EICOS_OK;
}

void lds_budget(Plan &pl, int batch, int n_cu, Shape &sh) {
    const Symbolic &S = pl.an->sym;
    DevPat &D = pl.dp;
    const bool tile = S.tile != 0, tile1 = S.tile == 1;
    const int NV = D.N, threads = pl.threads;
    // KKT-space vectors (solve vector, current solution, refinement residual) live in LDS when they fit:
    // 160 KiB per CU minus the static block (reductions + scalar state)
    D.lm_f = 0; D.lm_b = D.lm_f + D.nfs + D.nfs_solo + D.nfs_ext; D.lm_cag = D.lm_b + D.nbs + D.nbs_solo; D.lm_rA = D.lm_cag + D.cag_ns; D.lm_rG = D.lm_rA + D.rA_ns;
    D.lm_total = D.lm_rG + D.rG_ns;
    const size_t avail = LDS_PER_CU - LDS_STATIC, vec = (size_t)std::max(D.Npad, 16) * sizeof(double);
    // tile mode: one 16 x 17 fp64 scratch tile per wavefront (dense LDL' of the diagonal tiles), behind the tables
    // ... and the partial-sum slots of split blocks in the tile sweeps (TILE_PARTS x 16 rows x two right-hand sides)
    // dense apex: the packed image of the block's L (same place: the scalar path has no tile scratch)
    const size_t apex_img = (D.apex_na > 0 && threads >= 256) ? (size_t)APEX_IMG * sizeof(double) : 0; // (128 threads: the image IS the slab's, in LDS)
    const size_t scratch = tile ? ((size_t)(threads / 64) * TILE_SCR + (size_t)TILE_PARTS * 16 * KI_MAX_HOST) * sizeof(double) : apex_img;
    // workgroups per CU that 160 KB of LDS allow with one vector + tables of `slices` entries
    const int wgs_by_regs = (threads == 256 ? 3 : (threads == 512 ? 2 : 4)) * 4 / (threads / 64); // waves_per_eu<T>() of kernels.hip
    auto wgs_per_cu = [&](int slices) {
        return std::min(wgs_by_regs, (int)(LDS_PER_CU / (vec + (size_t)slices * sizeof(PackedSlice) + scratch + LDS_STATIC)));
    };
    // the factor program's table goes to LDS too when it is small and does not cost a resident workgroup
    if (D.fac_ns <= 512 && wgs_per_cu(D.lm_total + D.fac_ns) == wgs_per_cu(D.lm_total)) {
        D.lm_fac = D.lm_total; D.lm_total += D.fac_ns;
    } else D.lm_fac = -1;
    const size_t meta = (size_t)D.lm_total * sizeof(PackedSlice) + scratch;
    // NLDS >= 1 also stages both slice tables in LDS; if they do not fit beside one vector the
    // all-global variant (NLDS = 0, plain __syncthreads between levels) is used
    // KKT-space vectors in LDS: E (rhs / residual / solve vector) and X (current solution), + both slice tables
    int fit = 0;
    if (NV > 0 && meta + vec <= avail) fit = (meta + 2 * vec <= avail) ? 2 : 1;
    // more instances than CUs: keep only E in LDS so that several workgroups share a CU (measured)
    int want = fit;
    if (batch > n_cu && fit == 2 && 2 * (vec + meta + LDS_STATIC) <= LDS_PER_CU) want = 1;
    sh.nlds = std::max(0, std::min(fit, env_knob("EICOS_NLDS", want, 0, 2)));
    // Dual right-hand-side solves (the two independent systems of the initialisation and of every pass share one
    // sweep over the factor): needs two vectors in LDS.  Pure tile mode (bandwidth-bound on streaming L and G): always.
    // Scalar / hybrid programs: when the batch fits one workgroup per CU -- the sweeps are then a dependent chain of level
    // steps, and a step for two right-hand sides costs far less than two steps
    int dual = (fit == 2 && (tile1 || batch <= n_cu)) ? 1 : 0;
    dual = env_knob("EICOS_DUAL", dual, 0, 1);
    if (fit < 2) dual = 0;
    if (dual) sh.nlds = 1;
    D.dual = dual;
    const int nvec = dual ? 2 : sh.nlds; // vectors of Npad doubles at the start of the dynamic LDS
    D.meta_lds = sh.nlds >= 1 ? 1 : 0;
    // deferred-L factorisation (device_types.hpp: fac_defer): needs the idle LDS solve vector for the mirror of 1/D
    // It trades one LDS read per pair for a write + read of every L entry and one barrier per level: measured +1.5..3.3 % on MPC02 and
    // nine Netlib patterns (pairs/nnzL 1.7..7.5), -1 % on lp_25fv47 (10.1) -- profiles/r03_log_defer.log; the rule below is that fit.
    const int defer_auto = (double)S.npairs <= 8.0 * (double)S.nnzL ? 1 : 0;
    D.fac_defer = (!tile1 && sh.nlds >= 1 && env_knob("EICOS_FAC_DEFER", defer_auto, 0, 1)) ? 1 : 0;
    D.fac_kpad = S.N;
    sh.dyn_lds = sh.nlds >= 1 ? (size_t)nvec * vec + meta : (tile ? scratch : 0); // (no LDS vector: the apex sweeps read the global images, no LDS image)
    D.lds_tab = sh.nlds >= 1 ? nvec * D.Npad : 0;
    D.tl_scratch = sh.nlds >= 1 ? nvec * D.Npad + D.lm_total * 2 : 0; // in doubles from the start of the dynamic LDS
    D.tl_part = D.tl_scratch + (threads / 64) * TILE_SCR;
    D.apex_lds = (D.apex_na > 0 && sh.nlds >= 1) ? D.tl_scratch : -1; // (no LDS vector: the apex sweeps read the global images)
    D.apex_inplace = 0;
    // LDS-resident variant (small patterns, kernels_ldsres.hip): when the instance slab and the workspace slab fit LDS
    // beside the vectors and tables, k_solve works on LDS copies of both, so the elementwise stages and the products wait
    // for LDS instead of L2 (+12 % on lp_afiro at batch 256; the level-by-level sweeps are issue-bound and do not change:
    // DESIGN.md 5.1).  Only for batches that fit the grid in one round -- beyond that the eight small workgroups per CU
    // of the HBM-slab kernel hide more latency than the <= 3 that LDS holds here (measured, lp_afiro batch 2048).
    sh.ldsres = 0; D.lr_inst = D.lr_work = 0;
    if (!tile && sh.nlds >= 1 && threads == 128 && env_knob("EICOS_LDSRES", 1, 0, 1)) {
        const size_t base = (sh.dyn_lds + 15) & ~(size_t)15, islab = (D.inst_stride + 1) & ~(size_t)1, wslab = (D.work_stride + 1) & ~(size_t)1;
        const size_t total = base + (islab + wslab) * sizeof(double);
        const size_t per_cu = LDS_PER_CU / (total + LDS_STATIC); // workgroups per CU that LDS allows
        if (per_cu >= 1 && (size_t)batch <= per_cu * (size_t)n_cu) {
            sh.ldsres = 1; D.lr_inst = (int)(base / sizeof(double)); D.lr_work = D.lr_inst + (int)islab;
            sh.dyn_lds = total;
        }
    }
    if (D.apex_na > 0 && threads == 128) { // the apex of a 128-thread handle reads the forward image where it is: the LDS copy of the workspace slab
        if (!sh.ldsres) { sh.apex_unplaced = true; return; }
        D.apex_lds = D.lr_work + D.w_UF + D.apex_f; D.apex_inplace = 1;
    }
}

} // namespace eicos
