// The host-only self checks of the C ABI (eicos_debug_host_*: no GPU needed): the programs of the scalar, tile and hybrid paths executed
// sequentially exactly as the kernels index them.  No HIP call; compiled without a HIP include path.
#include "../../include/eicos_amd.h"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <stdexcept>
#include <vector>

#include "device_types.hpp"
#include "symbolic.hpp"
#include "plans.hpp"
#include "tiles.hpp"
#include "last_error.hpp"
#include "plan_step.hpp"

using namespace eicos;

// ---- the pieces the scalar and the tile / hybrid checks share ----
namespace {

// Pattern intake of a host-only entry: both halves back to back (no device to resolve between them), l derived.
int take_pattern(int n, int m, int p, int ncones, const int *q, const int *Gjc, const int *Gir, const int *Ajc, const int *Air, ProblemPattern &P) {
    const int rc = check_pattern_args(n, m, p, -1, ncones, q, Gjc, Gir, Ajc, Air, 1);
    return rc != EICOS_OK ? rc : take_csc(n, m, p, ncones, q, Gjc, Gir, Ajc, Air, P);
}

struct CheckRng { // the checks' random stream: the values of K first, then the right-hand side
    unsigned long long st;
    explicit CheckRng(unsigned seed) : st(seed * 2654435761ull + 12345) {}
    double operator()() { st = st * 6364136223846793005ull + 1442695040888963407ull; return ((st >> 11) & 0xFFFFFFFFFFFFull) / (double)(1ull << 48); }
};

// Random quasi-definite values on the KKT pattern (Kv per entry of K) and their scatter into P K P' (Lv per entry of L, Dv per
// diagonal).  false: an entry of K has no place in L.
bool random_kkt(const Symbolic &S, CheckRng &rnd, std::vector<double> &Kv, std::vector<double> &Lv, std::vector<double> &Dv) {
    Kv.assign(S.nnzK, 0.0); Lv.assign(S.nnzL, 0.0); Dv.assign(S.N, 0.0);
    for (int e = 0; e < S.nnzK; e++) {
        const int r = S.K_row[e], c = S.K_col[e];
        if (r == c) Kv[e] = (r < S.n ? 1.0 : -1.0) * (4.0 + rnd());
        else Kv[e] = 0.2 * (rnd() - 0.5);
    }
    for (int e = 0; e < S.nnzK; e++) {
        const int a = S.iperm[S.K_row[e]], b = S.iperm[S.K_col[e]];
        if (a == b) Dv[a] = Kv[e];
        else {
            const int i = std::max(a, b), j = std::min(a, b);
            auto it = std::lower_bound(S.Li.begin() + S.Lp[j], S.Li.begin() + S.Lp[j + 1], i);
            if (it == S.Li.begin() + S.Lp[j + 1] || *it != i) return false;
            Lv[it - S.Li.begin()] = Kv[e];
        }
    }
    return true;
}

// || K x - b ||_inf / || b ||_inf
double kkt_residual(const Symbolic &S, const std::vector<double> &Kv, const std::vector<double> &rhs, const std::vector<double> &x) {
    std::vector<double> r(rhs);
    for (int e = 0; e < S.nnzK; e++) {
        const int a = S.K_row[e], b = S.K_col[e];
        r[a] -= Kv[e] * x[b];
        if (a != b) r[b] -= Kv[e] * x[a];
    }
    double nr = 0, nb = 0;
    for (int i = 0; i < S.N; i++) { nr = std::max(nr, std::fabs(r[i])); nb = std::max(nb, std::fabs(rhs[i])); }
    return S.N ? nr / nb : 0.0;
}

// The sliced-ELL factor program of workgroup size T, lane by lane as stage_factor walks it: one level at a time, phase A (U into UB,
// D / invD), then phase B (L = U / D[col] into UF).  Targets in columns >= n0 -- a hybrid's top block -- go to the tile image `img` instead
// (the plan step's destination codes); n0 = N: none.  Returns what is wrong with a slice that the kernel could not run, else nullptr.
const char *walk_factor_program(const Symbolic &S, const FactorPlan &px, const TriPlan &pf, const TriPlan &pb, int T,
                                const std::vector<double> &Lv, const std::vector<double> &Dv, int n0, const TilePlan *TP, std::vector<double> *img,
                                std::vector<double> &UF, std::vector<double> &UB, std::vector<double> &D, std::vector<double> &invD) {
    const int N = S.N;
    std::vector<int> colof(S.nnzL);
    for (int j = 0; j < N; j++) for (int e = S.Lp[j]; e < S.Lp[j + 1]; e++) colof[e] = j;
    size_t s0 = 0;
    std::vector<double> carry;
    while (s0 < px.sl.size()) {
        size_t s1 = s0 + 1;
        while (s1 < px.sl.size() && !(px.sl[s1].newlev & 1)) s1++;
        for (size_t si = s0; si < s1; si++) {
            const SliceMeta &m = px.sl[si];
            const int g = 1 << m.lg, lanes = m.cnt * g;
            if (lanes > T) return "factor slice wider than the workgroup";
            if (m.K > ELL_KMAX) return "factor slice deeper than the prefetch depth";
            if (!m.cont) carry.assign(m.cnt, 0.0);
            for (int r = 0; r < m.cnt; r++) {
                double acc = carry[r];
                for (int q = 0; q < g; q++)
                    for (int kk = 0; kk < m.K; kk++) { const int slot = m.off + kk * lanes + r * g + q; acc += UB[px.pa[slot]] * UF[px.pb[slot]]; }
                if (m.more) { carry[r] = acc; continue; } // sub-slices of one set of targets accumulate
                const int tgt = px.target[m.row0 + r];
                if (tgt < N) {
                    if (tgt >= n0) (*img)[TP->D_img[tgt]] = Dv[tgt] - acc;
                    else { D[tgt] = Dv[tgt] - acc; invD[tgt] = 1.0 / D[tgt]; }
                } else {
                    const int e = tgt - N;
                    if (colof[e] >= n0) (*img)[TP->Le_img[e]] = Lv[e] - acc;
                    else UB[pb.pos[e]] = Lv[e] - acc;
                }
            }
        }
        for (size_t si = s0; si < s1; si++)
            for (int r = 0; r < px.sl[si].cnt && !px.sl[si].more; r++) {
                const int tgt = px.target[px.sl[si].row0 + r];
                if (tgt >= N && colof[tgt - N] < n0) { const int e = tgt - N; UF[pf.pos[e]] = UB[pb.pos[e]] * invD[colof[e]]; }
            }
        s0 = s1;
    }
    return nullptr;
}

// One sweep of a sliced-ELL triangular plan over ws, slice by slice as tri_sweep runs it: L y = b forward, x = (y - U' x) / D backward.
// Returns what is wrong with a slice that the kernel could not run, else nullptr.
const char *ell_sweep(const TriPlan &pl, const std::vector<double> &val, bool fwd, int T, std::vector<double> &ws, const std::vector<double> &invD) {
    for (const SliceMeta &m : pl.sl) {
        const int g = 1 << m.lg, lanes = m.cnt * g;
        if (lanes > T) return "slice wider than the workgroup";
        if (m.K > ELL_KMAX) return "slice deeper than the prefetch depth";
        std::vector<double> acc(m.cnt, 0.0);
        for (int t = 0; t < lanes; t++)
            for (int kk = 0; kk < m.K; kk++) { const int slot = m.off + kk * lanes + t; acc[t / g] += val[slot] * ws[pl.idx[slot]]; }
        for (int r = 0; r < m.cnt; r++) {
            const int i = m.row0 + r;
            ws[i] = (fwd || m.more) ? ws[i] - acc[r] : (ws[i] - acc[r]) * invD[i];
        }
    }
    return nullptr;
}

// developer aid (EICOS_PLAN_STATS): shape of the three programs for workgroup size T
void print_plan_stats(const Symbolic &S, int T, const TriPlan &pf, const TriPlan &pb, const FactorPlan &px) {
    auto stat = [&](const char *nm, const std::vector<SliceMeta> &sl, int slots) {
        int lev = 0, kmax = 0; long lanes = 0, kl = 0;
        for (const SliceMeta &m : sl) { lev += m.newlev & 1; kmax = std::max(kmax, m.K); lanes += (long)m.cnt << m.lg; kl += (long)m.K; }
        fprintf(stderr, "[plan T=%d] %-8s slices %zu levels %d slots %d sum(K) %ld maxK %d active-lane slices %.2f\n", T, nm,
                sl.size(), lev, slots, kl, kmax, (double)lanes / T);
    };
    stat("forward", pf.sl, pf.slots); stat("backward", pb.sl, pb.slots); stat("factor", px.sl, px.slots);
    fprintf(stderr, "[plan T=%d] factor targets %zu pairs %lld\n", T, px.target.size(), (long long)S.tp.back());
    if (T == 512 || (T == 256 && getenv("EICOS_PLAN_STATS")[0] == '2')) {
        fprintf(stderr, "[plan] level sizes:");
        for (int v = 0; v < S.nlev; v++) fprintf(stderr, " %d", S.lev_ptr[v + 1] - S.lev_ptr[v]);
        fprintf(stderr, "\n[plan T=%d] backward slices (lanes x K):", T);
        for (const SliceMeta &m : pb.sl) fprintf(stderr, " %d%sx%d", m.cnt << m.lg, (m.newlev & 1) ? "*" : "", m.K);
        fprintf(stderr, "\n[plan T=%d] forward slices (lanes x K):", T);
        for (const SliceMeta &m : pf.sl) fprintf(stderr, " %d%sx%d", m.cnt << m.lg, (m.newlev & 1) ? "*" : "", m.K);
        fprintf(stderr, "\n");
    }
}

} // namespace

extern "C" {

// Host-only self check of the symbolic analysis (no GPU needed): random quasi-definite values
// on the KKT pattern, the factor program and the level-scheduled gather solves executed
// sequentially exactly as the kernels index them, then || K x - b ||_inf / || b ||_inf.
double eicos_debug_host_check(int n, int m, int p, int ncones, const int *q, const int *Gjc, const int *Gir,
                              const int *Ajc, const int *Air, unsigned seed, int order_mode, int *stats /*[8] or NULL*/) {
    try {
        ProblemPattern P;
        if (take_pattern(n, m, p, ncones, q, Gjc, Gir, Ajc, Air, P) != EICOS_OK) return -2.0;
        Symbolic S = analyze(P, order_mode, 0); // the scalar programs (the tile and hybrid paths have their own checks)
        const int N = S.N;
        if (stats) { stats[0] = N; stats[1] = S.nnzK; stats[2] = S.nnzL; stats[3] = S.nlev; stats[4] = (int)std::min<int64_t>(S.npairs, 2147483647); stats[5] = S.order_mode; stats[6] = S.max_row_len; stats[7] = S.max_col_len; }
        // permutation sanity
        std::vector<char> seen(N, 0);
        for (int k = 0; k < N; k++) { if (S.perm[k] < 0 || S.perm[k] >= N || seen[S.perm[k]]) return -1.0; seen[S.perm[k]] = 1; }
        CheckRng rnd(seed);
        std::vector<double> Kv, Lv, Dv;
        if (!random_kkt(S, rnd, Kv, Lv, Dv)) return -4.0;
        // reference factorisation: the symbolic factor program, task by task
        std::vector<double> U(S.nnzL, 0.0), D(N, 0.0), invD(N, 0.0);
        for (int v = 0; v < S.nlev; v++)
            for (int t = S.ftask_ptr[v]; t < S.ftask_ptr[v + 1]; t++) {
                const int tgt = S.ftask[t];
                double s = 0;
                for (int64_t k = S.tp[tgt]; k < S.tp[tgt + 1]; k++) s += U[S.pa[k]] * U[S.pb[k]] * invD[S.pk[k]];
                if (tgt < N) { D[tgt] = Dv[tgt] - s; invD[tgt] = 1.0 / D[tgt]; }
                else { const int e = tgt - N; U[e] = Lv[e] - s; }
            }
        std::vector<double> rhs(N), x(N);
        for (int i = 0; i < N; i++) rhs[i] = rnd() - 0.5;
        // the factor program and the two sweeps exactly as the kernel walks its sliced-ELL plans (lane by lane)
        double plan_err = 0;
        for (int T : {128, 256, 512}) {
            TriPlan pf = build_tri_plan(S, T, true), pb = build_tri_plan(S, T, false);
            std::vector<double> UF(pf.ulen, 0.0), UB(pb.ulen, 0.0), ws(scalar_npad(N), 0.0);
            {
                FactorPlan px = build_factor_plan(S, T, pb.pos, pb.slots, pf.pos, pf.slots);
                if (getenv("EICOS_PLAN_STATS")) print_plan_stats(S, T, pf, pb, px);
                std::vector<double> D2(N, 0.0), iD2(N, 0.0);
                if (const char *bad = walk_factor_program(S, px, pf, pb, T, Lv, Dv, N, nullptr, nullptr, UF, UB, D2, iD2)) throw std::logic_error(bad);
                for (int e = 0; e < S.nnzL; e++) plan_err = std::max(plan_err, std::fabs(UB[pb.pos[e]] - U[e]) / (1.0 + std::fabs(U[e])));
                for (int jn = 0; jn < N; jn++) plan_err = std::max(plan_err, std::fabs(D2[jn] - D[jn]) / (1.0 + std::fabs(D[jn])));
            }
            for (int i = 0; i < N; i++) ws[i] = rhs[S.perm[i]];
            if (const char *bad = ell_sweep(pf, UF, true, T, ws, invD)) throw std::logic_error(bad);
            if (S.apex0 >= 0) { // the dense apex as apex_solve walks it: a column of the block per forward step, a row per backward step
                const int n0 = S.apex0, na = N - n0;
                for (int q_ = 0; q_ < pf.split_n; q_++) { ws[pf.split_row] += ws[pf.split_slot0 + q_]; ws[pf.split_slot0 + q_] = 0.; } // the parts of the split row
                if (na > APEX_MAX || pf.n_ext % TRI_DEPTH) throw std::logic_error("apex: bad shape");
                for (int k = 0; k < na; k++) for (int i = k + 1; i < na; i++) ws[n0 + i] -= UF[pf.apex_base + apex_img_at(i, k)] * ws[n0 + k];
                for (int i = na - 1; i >= 0; i--) {
                    ws[n0 + i] *= invD[n0 + i];
                    for (int k = 0; k < i; k++) ws[n0 + k] -= UB[pb.apex_base + apex_img_at(i, k)] * ws[n0 + i];
                }
            }
            if (const char *bad = ell_sweep(pb, UB, false, T, ws, invD)) throw std::logic_error(bad);
            std::vector<double> xt(N);
            for (int j = 0; j < N; j++) xt[S.perm[j]] = ws[j];
            if (T == 128) x = xt;
            for (int j = 0; j < N; j++) plan_err = std::max(plan_err, std::fabs(xt[j] - x[j]));
        }
        if (plan_err > 1e-9) return -3.0;
        return kkt_residual(S, Kv, rhs, x);
    } catch (const std::exception &e) { g_err = e.what(); return -2.0; }
}


// Host-only self check of the TILE path (no GPU needed): random quasi-definite values on the KKT pattern, the block
// factorisation and the two tile sweeps executed exactly as the kernels index them (tile image, pair lists, finalise
// lists, CSR / CSC tile views, column- / row-major tile copies, inverse diagonal tiles), then ||K x - b|| / ||b||.
// stats[8] = {dim_K, nnzK, nnzL, block levels, tile pairs, order_mode, blocks, off-diagonal tiles}.
static double host_check_tiles_impl(int n, int m, int p, int ncones, const int *q, const int *Gjc, const int *Gir,
                                    const int *Ajc, const int *Air, unsigned seed, int order_mode, int *stats, int mode) {
    try {
        ProblemPattern P;
        if (take_pattern(n, m, p, ncones, q, Gjc, Gir, Ajc, Air, P) != EICOS_OK) return -2.0;
        Symbolic S = analyze(P, order_mode, mode);
        if (S.tile != mode) return -10.0; // (hybrid requested, but the schedule has no tail worth handing to the tile path)
        TilePlan TP = build_tile_plan(S);
        const int n0 = TP.n0;
        if (getenv("EICOS_PLAN_STATS")) (void)build_tile_sweeps(TP, 8, TILE_PF);
        const int N = S.N, nb = TP.nb, nt = TP.nt, N16 = TP.N16;
        if (stats) { stats[0] = N; stats[1] = S.nnzK; stats[2] = S.nnzL; stats[3] = TP.nblev; stats[4] = (int)std::min<int64_t>(TP.npairs, 2147483647); stats[5] = S.order_mode; stats[6] = nb; stats[7] = nt; }
        CheckRng rnd(seed);
        std::vector<double> Kv, Lv, Dv; // values of P K P' per entry of L / per diagonal
        if (!random_kkt(S, rnd, Kv, Lv, Dv)) return -4.0;
        // the tile image: pure tile mode -- P K P' itself (what the solve prologue scatters from the instance slab);
        // hybrid -- written by the scalar factor program below (K minus the updates from the columns under the top block)
        std::vector<double> img((size_t)(nb + nt) * 256, 0.0);
        for (int d : TP.pad_img) img[d] = 1.0;
        std::vector<double> LC((size_t)nt * 256 + 1, 0.0), LR((size_t)nt * 256 + 1, 0.0), DC((size_t)nb * 256, 0.0), DR((size_t)nb * 256, 0.0), Dall(N16 + 1, 0.0), invDall(N16 + 1, 0.0);
        double *D = Dall.data() + n0, *invD = invDall.data() + n0; // block-relative views (DevPat::tl_base)
        constexpr int TW = 256; // workgroup size the scalar plans of the hybrid are laid out for in this check
        TriPlan pf, pb;
        std::vector<double> UF, UB;
        if (mode == 1) {
            for (int j = 0; j < N; j++) img[TP.D_img[j]] = Dv[j];
            for (int e = 0; e < S.nnzL; e++) img[TP.Le_img[e]] = Lv[e];
        } else { // hybrid: the scalar factor program below the cut, its top-block targets into the image
            pf = build_tri_plan(S, TW, true); pb = build_tri_plan(S, TW, false);
            FactorPlan px = build_factor_plan(S, TW, pb.pos, pb.slots, pf.pos, pf.slots);
            UF.assign(pf.slots + 1, 0.0); UB.assign(pb.slots + 1, 0.0);
            if (walk_factor_program(S, px, pf, pb, TW, Lv, Dv, n0, &TP, &img, UF, UB, Dall, invDall)) return -6.0;
        }
        for (int v = 0; v < TP.nblev; v++) {
            for (int qi = TP.tgt_lev_ptr[v]; qi < TP.tgt_lev_ptr[v + 1]; qi++) { // phase 1
                const int tg = TP.tgt[qi];
                double Tt[16][16];
                for (int r = 0; r < 16; r++) for (int c = 0; c < 16; c++) Tt[r][c] = img[(size_t)tg * 256 + tile_res(r, c)];
                for (int e = TP.tp_ptr[qi]; e < TP.tp_ptr[qi + 1]; e++) {
                    const double *A = LC.data() + (size_t)TP.pa[e] * 256, *B = LC.data() + (size_t)TP.pb[e] * 256, *d = D + TP.pk[e] * 16;
                    for (int r = 0; r < 16; r++) for (int c = 0; c < 16; c++) { double sacc = 0; for (int k = 0; k < 16; k++) sacc += A[tile_op(r, k)] * (B[tile_op(c, k)] * d[k]); Tt[r][c] -= sacc; }
                }
                if (tg >= nb) { double *o = LC.data() + (size_t)(tg - nb) * 256; for (int r = 0; r < 16; r++) for (int c = 0; c < 16; c++) o[tile_op(r, c)] = Tt[r][c]; continue; }
                const int J = tg;
                for (int j = 0; j < 16; j++) {
                    const double dj = Tt[j][j];
                    for (int c = j + 1; c < 16; c++) for (int r = c; r < 16; r++) Tt[r][c] -= (Tt[r][j] / dj) * Tt[c][j];
                    for (int r = j + 1; r < 16; r++) Tt[r][j] /= dj;
                }
                for (int c = 0; c < 16; c++) {
                    D[J * 16 + c] = Tt[c][c]; invD[J * 16 + c] = 1.0 / Tt[c][c];
                    double mc[16];
                    for (int r = 0; r < 16; r++) { double sacc = (r == c) ? 1.0 : 0.0; for (int k = 0; k < r; k++) sacc -= Tt[r][k] * mc[k]; mc[r] = (r < c) ? 0.0 : sacc; }
                    for (int r = 0; r < 16; r++) { DC[(size_t)J * 256 + tile_op(r, c)] = mc[r]; DR[(size_t)J * 256 + tile_res(r, c)] = mc[r]; }
                }
            }
            for (int qi = TP.fin_lev_ptr[v]; qi < TP.fin_lev_ptr[v + 1]; qi++) { // phase 2
                const int t = TP.fin[qi], J = TP.t_col[t];
                double Tt[16][16];
                for (int r = 0; r < 16; r++) for (int c = 0; c < 16; c++) {
                    double sacc = 0;
                    for (int k = 0; k < 16; k++) sacc += LC[(size_t)t * 256 + tile_op(r, k)] * DC[(size_t)J * 256 + tile_op(c, k)]; // T[r][k] * Linv[c][k]
                    Tt[r][c] = sacc * invD[J * 16 + c];
                }
                for (int r = 0; r < 16; r++) for (int c = 0; c < 16; c++) { LR[(size_t)t * 256 + tile_res(r, c)] = Tt[r][c]; LC[(size_t)t * 256 + tile_op(r, c)] = Tt[r][c]; }
            }
        }
        std::vector<double> rhs(N), wsall(N16 + 17, 0.0);
        for (int i = 0; i < N; i++) rhs[i] = rnd() - 0.5;
        for (int i = 0; i < N; i++) wsall[TP.slot[i]] = rhs[S.perm[i]];
        double *ws = wsall.data() + n0; // block-relative view
        if (mode == 2 && ell_sweep(pf, UF, true, TW, wsall, invDall)) return -6.0; // levels under the top block, then its rows against them (the plan's extra level)
        auto block = [&](int B, const std::vector<int> &tiles_of, int e0, int e1, const std::vector<double> &val, const std::vector<double> &dia, bool fwd) {
            double acc[16] = {0};
            for (int e = e0; e < e1; e++) {
                const int t = fwd ? tiles_of[e] : e, vb = fwd ? TP.t_col[t] : TP.t_row[t];
                // forward: LC in operand order, out[r] += L[r][k] y[k]; backward: LR in result order read as the transposed operand, out[c] += L[r][c] x[r]
                for (int c = 0; c < 16; c++) for (int k = 0; k < 16; k++) acc[c] += val[(size_t)t * 256 + tile_op(c, k)] * ws[vb * 16 + k];
            }
            double r[16], o[16] = {0};
            for (int c = 0; c < 16; c++) r[c] = (fwd ? ws[B * 16 + c] : ws[B * 16 + c] * invD[B * 16 + c]) - acc[c];
            if (TP.ident[B]) { for (int c = 0; c < 16; c++) ws[B * 16 + c] = r[c]; return; } // identity diagonal tile: skipped by the kernel
            for (int c = 0; c < 16; c++) for (int k = 0; k < 16; k++) o[c] += dia[(size_t)B * 256 + tile_op(c, k)] * r[k];
            for (int c = 0; c < 16; c++) ws[B * 16 + c] = o[c];
        };
        for (int v = 0; v < TP.nblev; v++) for (int B = TP.blev_ptr[v]; B < TP.blev_ptr[v + 1]; B++) block(B, TP.tr_tile, TP.tr_ptr[B], TP.tr_ptr[B + 1], LC, DC, true);
        for (int v = TP.nblev - 1; v >= 0; v--) for (int B = TP.blev_ptr[v]; B < TP.blev_ptr[v + 1]; B++) block(B, TP.tr_tile, TP.tc_ptr[B], TP.tc_ptr[B + 1], LR, DR, false);
        if (mode == 2 && ell_sweep(pb, UB, false, TW, wsall, invDall)) return -6.0;
        std::vector<double> x(N);
        for (int j = 0; j < N; j++) x[S.perm[j]] = wsall[TP.slot[j]];
        for (int s_ = 0; s_ < N16; s_++) { bool real = false; for (int j = 0; j < N && !real; j++) real = TP.slot[j] == s_; if (!real && wsall[s_] != 0.0) return -5.0; if (N > 4000) break; } // padding slots stay 0
        return kkt_residual(S, Kv, rhs, x);
    } catch (const std::exception &e) { g_err = e.what(); return -2.0; }
}


// Host-only: the elimination order and block partition the tile path would use (perm[new] = KKT index, blk_ptr[nblk + 1]); returns the
// number of blocks, < 0 on error.  Development aid for ordering studies (tools/dev), no GPU needed.
int eicos_debug_host_tile_order(int n, int m, int p, int ncones, const int *q, const int *Gjc, const int *Gir,
                                const int *Ajc, const int *Air, int order_mode, int *perm, int *blk_ptr, int *stats, int *Lp, int *Li) {
    try {
        ProblemPattern P;
        if (take_pattern(n, m, p, ncones, q, Gjc, Gir, Ajc, Air, P) != EICOS_OK) return -2;
        Symbolic S = analyze(P, order_mode, 1);
        TilePlan TP = build_tile_plan(S);
        if (perm) std::copy(S.perm.begin(), S.perm.end(), perm);
        if (blk_ptr) std::copy(S.blk_ptr.begin(), S.blk_ptr.end(), blk_ptr);
        if (Lp) std::copy(S.Lp.begin(), S.Lp.end(), Lp);
        if (Li) std::copy(S.Li.begin(), S.Li.end(), Li);
        if (stats) { stats[0] = S.N; stats[1] = S.nnzL; stats[2] = TP.nb; stats[3] = TP.nt; stats[4] = TP.nblev; stats[5] = (int)std::min<int64_t>(TP.npairs, 2147483647); stats[6] = S.order_mode; stats[7] = S.cone_order; }
        return S.nblk;
    } catch (const std::exception &e) { g_err = e.what(); return -2; }
}

double eicos_debug_host_check_tiles(int n, int m, int p, int ncones, const int *q, const int *Gjc, const int *Gir,
                                    const int *Ajc, const int *Air, unsigned seed, int order_mode, int *stats) {
    return host_check_tiles_impl(n, m, p, ncones, q, Gjc, Gir, Ajc, Air, seed, order_mode, stats, 1);
}
// hybrid: scalar programs under the cut + tile path on the top block; returns -10 when the pattern does not qualify
double eicos_debug_host_check_hybrid(int n, int m, int p, int ncones, const int *q, const int *Gjc, const int *Gir,
                                     const int *Ajc, const int *Air, unsigned seed, int order_mode, int *stats) {
    return host_check_tiles_impl(n, m, p, ncones, q, Gjc, Gir, Ajc, Air, seed, order_mode, stats, 2);
}

} // extern "C"
