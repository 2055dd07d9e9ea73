// Host check of eicos_amd/csrc/chunk_plan.hpp (tests/test_chunk_plan.py builds this with -fsanitize=address,undefined and runs it): the
// packed layout of a chunk under both padding rules, the three area sizes and the chunk-size rules, against numbers laid out by hand
// here and against the pointer walks api.cpp held before the rules had a home of their own, restated below.  Exit status 0 = all passed.
//   chunk_plan_check                          the checks
//   chunk_plan_check in PER COUNT             prints bounce_in_chunk (PER = doubles per instance over the given arrays)
//   chunk_plan_check out ROW_BYTES COUNT      prints bounce_out_chunk and whether the result is a small one
//   chunk_plan_check matrix ROW COUNT CAP     prints matrix_stage_chunk (ROW = matrix_stage_row, CAP in doubles)
// -- the latter three so that a test can say from the header itself how many chunks its shape gives (tests/test_chunked_transfers.py).
#include "chunk_plan.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>

using namespace eicos;

static int g_failed = 0, g_cases = 0;
#define CHECK(cond)                                                                   \
    do {                                                                              \
        g_cases++;                                                                    \
        if (!(cond)) { std::printf("line %d: %s\n", __LINE__, #cond); g_failed++; }   \
    } while (0)

// The walks as the call sites wrote them.  update_in_chunks and the staged branch of update_solve:
//     packed[q] = at; ...; at += (size_t)cnt * in.w[q] + 8;          (stage_need += (size_t)h->batch * in.w[k] + 8)
// param_range:
//     arr[g] = at; ...; at += ((size_t)cnt * w[g] + 7) / 8 * 8;      (per += (size_t)w[g] + 8; reserve chunk * per)
static size_t old_walk(const size_t w[5], const bool given[5], size_t rows, bool round_up, size_t off[5]) {
    size_t at = 0;
    for (int q = 0; q < 5; q++) {
        if (!given[q]) continue;
        off[q] = at;
        at += round_up ? (rows * w[q] + 7) / 8 * 8 : rows * w[q] + 8;
    }
    return at;
}

static void check_layout(const size_t w[5], unsigned subset, size_t rows) {
    bool given[5];
    size_t per = 0;
    int ngiven = 0;
    for (int q = 0; q < 5; q++) { given[q] = (subset >> q) & 1; if (given[q]) { per += w[q]; ngiven++; } }
    for (ChunkPad pad : {ChunkPad::Gap8, ChunkPad::RoundUp8}) {
        const bool up = pad == ChunkPad::RoundUp8;
        const PackedChunk pk = pack_chunk(w, given, rows, pad);
        size_t old_off[5] = {0, 0, 0, 0, 0};
        const size_t old_total = old_walk(w, given, rows, up, old_off);
        bool same = pk.total == old_total, inside = true, apart = true, aligned = true;
        size_t end = 0; // of the array before
        bool first = true;
        for (int q = 0; q < 5; q++) {
            if (!given[q]) { same = same && pk.off[q] == 0; continue; }
            same = same && pk.off[q] == old_off[q];
            inside = inside && pk.off[q] + rows * w[q] <= pk.total;
            // in order, no overlap; eight doubles between two arrays under Gap8
            apart = apart && (first || pk.off[q] >= end + (up ? 0 : 8));
            aligned = aligned && pk.off[q] % 8 == 0;
            end = pk.off[q] + rows * w[q];
            first = false;
        }
        CHECK(same);
        CHECK(inside);
        CHECK(apart);
        if (up) CHECK(aligned); // RoundUp8 aligns every array, whatever rows * w is; Gap8 promises it for the first alone (spelled out in main)
        // the areas as they are reserved today hold the chunk
        if (up) CHECK(matrix_stage_row(w, given) == per + 8 * (size_t)ngiven && pk.total <= rows * matrix_stage_row(w, given));
        else {
            CHECK(pk.total == rows * per + 8 * (size_t)ngiven); // (what the staged fused update reserves for the whole batch, exactly)
            if (rows >= 1) CHECK(pk.total <= staging_doubles(per, (int)rows));
            if (rows == 1 && ngiven == 5) CHECK(pk.total == staging_doubles(per, 1)); // five gaps per instance: tight for one instance with all five given
        }
    }
}

static int print_rule(int argc, char **argv) {
    const size_t a = std::strtoull(argv[2], nullptr, 10);
    const int count = std::atoi(argv[3]);
    if (argc == 4 && std::strcmp(argv[1], "in") == 0) std::printf("%d\n", bounce_in_chunk(a, count));
    else if (argc == 4 && std::strcmp(argv[1], "out") == 0) std::printf("%d %d\n", bounce_out_chunk(a, count), (int)small_result(a * (size_t)count));
    else if (argc == 5 && std::strcmp(argv[1], "matrix") == 0) std::printf("%d\n", matrix_stage_chunk(a, count, std::strtoull(argv[4], nullptr, 10)));
    else return 2;
    return 0;
}

int main(int argc, char **argv) {
    if (argc >= 4) return print_rule(argc, argv);
    // ---- the packed layout
    const size_t widths[][5] = {{7, 3, 5, 4, 2}, {7, 0, 5, 0, 2}, {0, 0, 0, 0, 0}, {8, 16, 24, 8, 40}, {131072, 1, 999, 0, 63}};
    int layouts = 0;
    for (const auto &w : widths)
        for (unsigned subset = 0; subset < 32; subset++)
            for (size_t rows : {0, 1, 3, 8, 16, 17, 257}) { check_layout(w, subset, rows); layouts++; }
    // by hand: w = 7, 3, 5, 4, 2, three rows, all given.  Gap8: 21 + 8, 9 + 8, 15 + 8, 12 + 8, 6 + 8
    const bool all[5] = {true, true, true, true, true}, gcb[5] = {true, false, true, false, true};
    {
        const size_t w[5] = {7, 3, 5, 4, 2};
        PackedChunk p = pack_chunk(w, all, 3, ChunkPad::Gap8);
        CHECK(p.off[0] == 0 && p.off[1] == 29 && p.off[2] == 46 && p.off[3] == 69 && p.off[4] == 89 && p.total == 103);
        CHECK(p.off[1] % 8 != 0); // rows * w = 21 is no multiple of 8: the second array is NOT 64-byte aligned under Gap8 ...
        p = pack_chunk(w, all, 8, ChunkPad::Gap8); // ... and eight rows are: 56 + 8, 24 + 8, 40 + 8, 32 + 8, 16 + 8
        CHECK(p.off[0] == 0 && p.off[1] == 64 && p.off[2] == 96 && p.off[3] == 144 && p.off[4] == 184 && p.total == 208);
        // RoundUp8, three rows: 21 -> 24, 9 -> 16, 15 -> 16, 12 -> 16, 6 -> 8; eight rows: nothing to round
        p = pack_chunk(w, all, 3, ChunkPad::RoundUp8);
        CHECK(p.off[0] == 0 && p.off[1] == 24 && p.off[2] == 40 && p.off[3] == 56 && p.off[4] == 72 && p.total == 80);
        p = pack_chunk(w, all, 8, ChunkPad::RoundUp8);
        CHECK(p.off[0] == 0 && p.off[1] == 56 && p.off[2] == 80 && p.off[3] == 120 && p.off[4] == 152 && p.total == 168);
        // G, c, b given
        p = pack_chunk(w, gcb, 3, ChunkPad::Gap8);
        CHECK(p.off[0] == 0 && p.off[1] == 0 && p.off[2] == 29 && p.off[3] == 0 && p.off[4] == 52 && p.total == 66);
        p = pack_chunk(w, gcb, 3, ChunkPad::RoundUp8);
        CHECK(p.off[0] == 0 && p.off[2] == 24 && p.off[4] == 40 && p.total == 48);
        CHECK(matrix_stage_row(w, all) == 61 && matrix_stage_row(w, gcb) == 38);
    }
    { // widths of 0 (a pattern without A: nnzA = p = 0), given all the same: an address of its own under Gap8, the next array's under RoundUp8
        const size_t w[5] = {7, 0, 5, 0, 2};
        PackedChunk p = pack_chunk(w, all, 3, ChunkPad::Gap8);
        CHECK(p.off[0] == 0 && p.off[1] == 29 && p.off[2] == 37 && p.off[3] == 60 && p.off[4] == 68 && p.total == 82);
        p = pack_chunk(w, all, 3, ChunkPad::RoundUp8);
        CHECK(p.off[0] == 0 && p.off[1] == 24 && p.off[2] == 24 && p.off[3] == 40 && p.off[4] == 40 && p.total == 48);
    }
    CHECK(staging_doubles(1000, 2016) == 2096640 && staging_doubles(0, 1) == 40 && staging_doubles(14, 0) == 0);

    // ---- host arrays in: 16 MB / ((per + 40) * 8 bytes).  per = 1000: 16777216 / 8320 = 2016
    {
        const int chunk = 2016;
        CHECK(bounce_in_chunk(1000, 0) == 0 && bounce_in_chunk(1000, 1) == 1 && bounce_in_chunk(1000, 15) == 15 && bounce_in_chunk(1000, 16) == 16 &&
              bounce_in_chunk(1000, 17) == 17);
        CHECK(bounce_in_chunk(1000, chunk - 1) == 2015 && bounce_in_chunk(1000, chunk) == 2016);
        // two even chunks on (chunk, 2 * chunk): both ends and the middle of the interval, and the counts next to it
        CHECK(bounce_in_chunk(1000, chunk + 1) == 1009 && bounce_in_chunk(1000, 3000) == 1500 && bounce_in_chunk(1000, 3001) == 1501 &&
              bounce_in_chunk(1000, 2 * chunk - 1) == 2016);
        CHECK(bounce_in_chunk(1000, 2 * chunk) == 2016 && bounce_in_chunk(1000, 2 * chunk + 1) == 2016 && bounce_in_chunk(1000, 100000) == 2016);
        // a row so wide that the floor of 16 decides (200040 * 8 bytes: 10 rows in 16 MB) -- the even split applies to it too
        CHECK(bounce_in_chunk(200000, 15) == 15 && bounce_in_chunk(200000, 16) == 16 && bounce_in_chunk(200000, 17) == 9 && bounce_in_chunk(200000, 31) == 16 &&
              bounce_in_chunk(200000, 32) == 16 && bounce_in_chunk(200000, 1000) == 16);
        // a row so narrow that count decides (41 * 8 bytes: 51150 rows)
        CHECK(bounce_in_chunk(1, 100) == 100 && bounce_in_chunk(1, 51150) == 51150 && bounce_in_chunk(1, 51151) == 25576 && bounce_in_chunk(1, 102300) == 51150);
    }
    // ---- results out: 4 MB / row bytes.  1000 doubles a row: 4194304 / 8000 = 524
    {
        const int chunk = 524;
        for (int count : {0, 1, 15, 16, 17, chunk - 1, chunk}) CHECK(bounce_out_chunk(8000, count) == count);
        for (int count : {chunk + 1, 2 * chunk - 1, 2 * chunk, 100000}) CHECK(bounce_out_chunk(8000, count) == 524);
        CHECK(bounce_out_chunk(400000, 15) == 15 && bounce_out_chunk(400000, 16) == 16 && bounce_out_chunk(400000, 17) == 16 && bounce_out_chunk(400000, 1000) == 16); // (10 rows in 4 MB: the floor)
        CHECK(bounce_out_chunk(8, 100) == 100 && bounce_out_chunk(8, 524288) == 524288 && bounce_out_chunk(8, 524289) == 524288);
        CHECK(small_result(0) && small_result(262143) && !small_result(262144) && !small_result(262145));
    }
    // ---- the staged fused update: 12 MB / (per * 8 bytes), at least 8, at most the batch.  per = 1000: 12582912 / 8000 = 1572
    {
        const int chunk = 1572;
        CHECK(fused_stage_chunk(1000, 0) == 8 && fused_stage_chunk(1000, 1) == 8 && fused_stage_chunk(1000, 7) == 8 && fused_stage_chunk(1000, 8) == 8); // (the floor holds against the batch too)
        for (int batch : {15, 16, 17, chunk - 1, chunk}) CHECK(fused_stage_chunk(1000, batch) == batch);
        for (int batch : {chunk + 1, 2 * chunk - 1, 2 * chunk, 100000}) CHECK(fused_stage_chunk(1000, batch) == 1572);
        CHECK(fused_stage_chunk(400000, 100) == 8 && fused_stage_chunk(400000, 5) == 8); // (3 rows in 12 MB: the floor)
        CHECK(fused_stage_chunk(1, 100) == 100 && fused_stage_chunk(0, 100) == 100);     // (nothing staged: a divisor of 1 byte)
        CHECK(chunk_count(0, 8) == 0 && chunk_count(1, 8) == 1 && chunk_count(8, 8) == 1 && chunk_count(9, 8) == 2 && chunk_count(100, 8) == 13);
        CHECK(chunk_count(chunk, chunk) == 1 && chunk_count(chunk + 1, chunk) == 2 && chunk_count(2 * chunk - 1, chunk) == 2 && chunk_count(2 * chunk, chunk) == 2 &&
              chunk_count(2 * chunk + 1, chunk) == 3);
    }
    // ---- the matrix-map staging: cap / row, at least 1, at most count.  64 MB = 8388608 doubles, row = 1000: 8388
    {
        const size_t cap = 8388608;
        const int chunk = 8388;
        CHECK(matrix_stage_chunk(1000, 0, cap) == 1); // (the caller returns before it asks, for count 0)
        for (int count : {1, 15, 16, 17, chunk - 1, chunk}) CHECK(matrix_stage_chunk(1000, count, cap) == count);
        for (int count : {chunk + 1, 2 * chunk - 1, 2 * chunk, 100000}) CHECK(matrix_stage_chunk(1000, count, cap) == 8388);
        CHECK(matrix_stage_chunk(10000000, 100, cap) == 1 && matrix_stage_chunk(8388608, 100, cap) == 1 && matrix_stage_chunk(4194304, 100, cap) == 2); // (the floor of 1)
        CHECK(matrix_stage_chunk(8, 100, cap) == 100);
        CHECK(matrix_stage_chunk(1000, 1000, 131072) == 131); // (a cap of 1 MB)
    }
    CHECK(PEER_CHUNK == 256 && PIN_CHUNK_BYTES == 16777216);

    if (layouts != 5 * 32 * 7) { std::printf("walked %d layouts, expected %d\n", layouts, 5 * 32 * 7); g_failed++; }
    if (g_failed) { std::printf("%d check(s) failed\n", g_failed); return 1; }
    std::printf("chunk_plan_check: %d cases, all passed\n", g_cases);
    return 0;
}
