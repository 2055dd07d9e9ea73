// Host check of eicos_amd/csrc/rollout_layout.hpp (tests/test_rollout_layout.py builds this with -fsanitize=address,undefined and runs
// it): the layout of a rollout's three device buffers over the shapes below, every part written whole inside a block of exactly the
// buffer's total, so that the address sanitizer sees a part that leaves the block; the totals against the sums the buffers had while
// api.cpp laid them out by hand, restated here as plain arithmetic; the refusal of a batch * steps beyond an int; and the rule of the
// held trajectory with its three messages.  Exit status 0 = all checks passed.
#include "rollout_layout.hpp"

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

using namespace eicos;

static int g_failed = 0, g_cases = 0;
#define CHECK(cond)                                                                   \
    do {                                                                              \
        g_cases++;                                                                    \
        if (!(cond)) { std::printf("line %d: %s\n", __LINE__, #cond); g_failed++; }   \
    } while (0)

static const size_t HEADER = 128, D = sizeof(double), I = sizeof(int);

struct Piece { size_t at, bytes, align; bool wanted; }; // wanted: the shape gives the part a width

// One buffer: every wanted part inside [0, total), aligned, none overlapping another, each written whole inside a block of exactly
// `total` bytes; a part without width takes no bytes; total in [sum, sum + 64 per part]
static void check_buffer(const std::vector<Piece> &parts, size_t total, size_t sum) {
    char *block = static_cast<char *>(std::malloc(total ? total : 1));
    std::vector<Piece> placed;
    for (const Piece &q : parts) {
        CHECK(q.wanted == (q.bytes != 0));
        if (!q.bytes) continue;
        CHECK(q.at < total && q.at + q.bytes <= total);
        CHECK(q.at % q.align == 0 && reinterpret_cast<uintptr_t>(block + q.at) % q.align == 0);
        std::memset(block + q.at, 0x5a, q.bytes);
        placed.push_back(q);
    }
    std::sort(placed.begin(), placed.end(), [](const Piece &a, const Piece &b) { return a.at < b.at; });
    for (size_t i = 1; i < placed.size(); i++) CHECK(placed[i - 1].at + placed[i - 1].bytes <= placed[i].at);
    CHECK(total >= sum && total <= sum + 64 * parts.size());
    std::free(block);
}

static Piece piece(const RolloutLayout::Part &q, size_t align, bool wanted) { return Piece{q.at, q.bytes, align, wanted}; }

// The six parts of `rows` recorded rows: widths, order, packed from R.at[0]; rows = 0: none, and no bytes
static void record_pieces(const RecordLayout &R, size_t rows, const RolloutShape &s, size_t from, std::vector<Piece> &out) {
    const size_t width[6] = {s.r * s.n, s.r * s.m, s.r * s.p, s.n, s.p, s.m};
    CHECK(R.rows == rows && R.at[0] == from);
    size_t at = from;
    for (int q = 0; q < 6; q++) {
        CHECK(R.width[q] == width[q] && R.at[q] == at);
        out.push_back(Piece{R.at[q], rows * width[q] * D, D, rows * width[q] != 0});
        at += rows * width[q] * D;
    }
    CHECK(R.end == at);
}

// The pointers rollout_run takes: each the part's place in its buffer, NULL where the part has no bytes; written through whole, in
// three blocks of exactly the totals
static void check_pointers(const RolloutLayout &L) {
    char *blk[3];
    const size_t total[3] = {L.roll_bytes, L.rollJ_bytes, L.rollW_bytes};
    for (int q = 0; q < 3; q++) blk[q] = static_cast<char *>(std::malloc(total[q] ? total[q] : 1));
    const RolloutArrays a = L.in(blk[0], blk[1], blk[2]);
    const struct { const void *p; const RolloutLayout::Part &part; int buf; } want[12] = {
        {a.roll_rec, L.roll_rec, 0}, {a.theta, L.theta, 0}, {a.u, L.u, 0}, {a.w, L.w, 0}, {a.cur, L.cur, 0}, {a.codes, L.codes, 0}, {a.iters, L.iters, 0},
        {a.adj_rec, L.adj_rec, 1}, {a.J, L.J, 1}, {a.res, L.res, 1}, {a.J1, L.J1, 1}, {a.res1, L.res1, 1}};
    for (const auto &w : want) {
        CHECK(w.p == (w.part.bytes ? blk[w.buf] + w.part.at : nullptr));
        if (w.p) std::memset(const_cast<void *>(w.p), 0x5a, w.part.bytes);
    }
    for (const auto &rows : {std::make_pair(&a.W, &L.record), std::make_pair(&a.W1, &L.step)})
        for (int q = 0; q < 6; q++) {
            if (!rows.second->rows) { CHECK(rows.first->part(q) == nullptr); continue; }
            CHECK(reinterpret_cast<char *>(rows.first->part(q)) == blk[2] + rows.second->at[q] && rows.first->width[q] == rows.second->width[q]);
            std::memset(rows.first->part(q), 0x5a, rows.second->rows * rows.second->width[q] * D);
        }
    for (char *b : blk) std::free(b);
}

static void check_shape(const RolloutShape &s) {
    CHECK(rollout_shape_fault(s).empty());
    const RolloutLayout L(s);
    check_pointers(L);
    const size_t B = s.B, T = s.T, k = s.k, r = s.r;
    {   // d_roll, as it was summed: MAP_HEADER + (n_th + n_u + n_w + n_cur) * 8 + 2 * n_rec * 4
        const size_t n_th = B * (T + 1) * k, n_u = B * T * r, n_w = s.w ? B * T * k : 0, n_cur = 2 * B * k, n_rec = B * T;
        const std::vector<Piece> parts = {piece(L.roll_rec, 8, true), piece(L.theta, D, true), piece(L.u, D, true), piece(L.w, D, s.w),
                                          piece(L.cur, D, true), piece(L.codes, I, true), piece(L.iters, I, true)};
        check_buffer(parts, L.roll_bytes, HEADER + (n_th + n_u + n_w + n_cur) * D + 2 * n_rec * I);
        CHECK(L.roll_rec.at == 0 && L.roll_rec.bytes == HEADER && L.theta.bytes == n_th * D && L.u.bytes == n_u * D && L.w.bytes == n_w * D &&
              L.cur.bytes == n_cur * D && L.codes.bytes == n_rec * I && L.iters.bytes == n_rec * I);
        double probe[1];
        CHECK((L.w.in<double>(probe) != nullptr) == s.w); // a part without width has no address
    }
    {   // d_rollJ: MAP_HEADER + (n_J + n_res + n_J1 + n_res1) * 8, made by a rollout with sens alone
        const size_t n_J = B * T * r * k, n_res = B * T * r, n_J1 = B * r * k, n_res1 = B * r;
        const std::vector<Piece> parts = {piece(L.adj_rec, 8, s.sens), piece(L.J, D, s.sens), piece(L.res, D, s.sens), piece(L.J1, D, s.sens), piece(L.res1, D, s.sens)};
        check_buffer(parts, L.rollJ_bytes, s.sens ? HEADER + (n_J + n_res + n_J1 + n_res1) * D : 0);
        if (s.sens) CHECK(L.adj_rec.at == 0 && L.J.bytes == n_J * D && L.res.bytes == n_res * D && L.J1.bytes == n_J1 * D && L.res1.bytes == n_res1 * D);
        else CHECK(L.rollJ_bytes == 0);
    }
    {   // d_rollW: (B T + (fused ? 0 : B)) * (r + 1) * (n + m + p) * 8 -- the number its refusal names, so the total is exactly that
        const size_t sum = s.recording ? (B * T + (s.fused ? 0 : B)) * (r + 1) * (s.n + s.m + s.p) * D : 0;
        std::vector<Piece> parts;
        if (s.recording) {
            record_pieces(L.record, B * T, s, 0, parts);
            record_pieces(L.step, s.fused ? 0 : B, s, L.record.end, parts);
        }
        check_buffer(parts, L.rollW_bytes, sum);
        CHECK(L.rollW_bytes == sum);
        CHECK((L.step.rows != 0) == (s.recording && !s.fused)); // the one step's rows exist exactly there
        if (!s.recording) { CHECK(L.record.rows == 0 && L.record.end == 0 && L.step.end == 0); return; }
        // "row t of instance b" of the whole record: where eicos_batch_rollout_records reads it -- part q copied out whole as
        // [B][T][width[q]] --, where the per-step move puts it -- from row t of instance 0, instances T rows apart --, and
        // inside its part
        std::vector<double> block(L.rollW_bytes / D + 1);
        const RecordRows W = L.record.in(block.data());
        for (int q = 0; q < 6; q++) {
            CHECK(W.width[q] == L.record.width[q] && reinterpret_cast<char *>(W.part(q)) == reinterpret_cast<char *>(block.data()) + L.record.at[q]);
            for (size_t b = 0; b < B; b++)
                for (size_t t = 0; t < T; t++) {
                    const size_t at = L.record.row_at(q, b, t, T);
                    CHECK(at == L.record.at[q] + ((b * T + t) * W.width[q]) * D);
                    CHECK(reinterpret_cast<char *>(W.part(q) + t * W.width[q] + b * T * W.width[q]) == reinterpret_cast<char *>(block.data()) + at);
                    CHECK(at + W.width[q] * D <= L.record.at[q] + B * T * W.width[q] * D);
                }
        }
        if (L.step.rows) { // the step's rows start where the record ends, parts of no width keep an address
            const RecordRows W1 = L.step.in(block.data());
            CHECK(reinterpret_cast<char *>(W1.Wc) == reinterpret_cast<char *>(block.data()) + L.record.end);
            for (int q = 0; q < 6; q++) CHECK(W1.part(q) != nullptr && W.part(q) != nullptr);
        }
    }
}

struct Plant { int nnz = 0; };

int main() {
    // (a) the smallest shape: nothing optional
    check_shape(RolloutShape{1, 1, 1, 1, 1, 0, 0, false, false, false, true});
    check_shape(RolloutShape{1, 1, 1, 1, 1, 0, 0, false, false, false, false});
    // (b) B T k odd, p = 0: Wb and y of no width; (c) the same with p = 2 -- w given, sens on, recording off and on, fused and not
    for (size_t p : {(size_t)0, (size_t)2})
        for (int recording = 0; recording < 2; recording++)
            for (int fused = 0; fused < 2; fused++) check_shape(RolloutShape{3, 2, 3, 2, 5, 4, p, true, true, recording != 0, fused != 0});
    check_shape(RolloutShape{3, 2, 3, 2, 5, 4, 0, false, true, true, false}); // ... and without w
    {   // ---- batch * steps beyond an int: refused with sens, by arithmetic alone (no layout is built)
        RolloutShape s{65536, 32768, 3, 2, 5, 4, 0, false, true, false, true};
        CHECK(rollout_shape_fault(s) == "rollout_jacobian: batch * steps must fit an int");
        s.T = 32767;
        CHECK(rollout_shape_fault(s).empty()); // 2^31 - 65536
        s.T = 32768; s.sens = false;
        CHECK(rollout_shape_fault(s).empty()); // (a plain rollout has no such rows)
    }
    {   // ---- the held trajectory
        const std::string none = "w: the handle holds no Jacobian trajectory (eicos_batch_rollout_jacobian records one)";
        const std::string stale = "w: a parameter, matrix, output, plant or fallback map was installed after the rollout whose Jacobians the handle holds (setting or clearing per-instance plant values counts as one): run eicos_batch_rollout_jacobian again";
        const std::string norows = "w: the handle holds no recorded rows: recording was off for the rollout it holds (eicos_batch_set_rollout_recording, then eicos_batch_rollout_jacobian)";
        HeldTrajectory<Plant> H;
        CHECK(H.steps == 0 && H.fault("w", 0, false) == none && H.fault("w", 0, true, false) == none); // a fresh struct
        double J[4], res[2], rows[8];
        const RecordRows R = lay_records(0, 2, 1, 1, 1, 0).in(rows);
        H.hold(2, 1, 2, 1, Plant{7}, 5, J, res, nullptr); // a record without rows, at generation 5
        CHECK(H.steps == 1 && H.k == 2 && H.r == 1 && H.rows == 2 && H.plant.nnz == 7 && H.J() == J && H.res() == res);
        CHECK(H.fault("w", 5, false).empty() && H.fault("w", 5, true) == norows && H.fault("w", 5, true, false) == norows);
        CHECK(H.fault("w", 6, false) == stale && H.fault("w", 6, false, false).empty()); // a generation bump, current true and false
        CHECK(H.fault("w", 6, true) == stale && H.fault("w", 6, true, false) == norows);  // (the stale map is reported first)
        H.hold(2, 1, 2, 1, Plant{7}, 6, J, res, &R); // ... with rows
        CHECK(H.fault("w", 6, true).empty() && H.records().Wc == R.Wc && H.records().z == R.z && H.records().width[1] == 1);
        CHECK(H.fault("w", 7, true) == stale && H.fault("w", 7, true, false).empty()); // the record is still read after an install
        H.drop_rows(); // recording switched off: J stays
        CHECK(H.fault("w", 6, false).empty() && H.fault("w", 6, true) == norows);
        H.hold(2, 1, 2, 1, Plant{7}, 6, J, res, &R);
        H.invalidate(); // until the next rollout has been enqueued whole
        CHECK(H.steps == 0 && H.fault("w", 6, false) == none && H.fault("w", 6, true, false) == none);
        CHECK(H.fault("eicos_batch_rollout_gradient", 6, false).rfind("eicos_batch_rollout_gradient: the handle holds", 0) == 0);
    }
    if (g_failed) { std::printf("%d check(s) failed\n", g_failed); return 1; }
    std::printf("rollout_layout_check: %d cases, all passed\n", g_cases);
    return 0;
}
