// Host check of eicos_amd/csrc/host_copy.hpp / host_copy.cpp (tests/test_host_copy.py builds this program with host_copy.cpp, once with
// -fsanitize=address,undefined and once with -fsanitize=thread, and runs it once per setting of the pool -- the pool is a singleton of
// the process and reads its knobs once).
//   host_copy_check pieces            the piece rule alone, as arithmetic
//   host_copy_check copy THREADS      the pool must have THREADS helpers (EICOS_COPY_THREADS under EICOS_EXPERIMENT=1 in the environment);
//                                     four host threads then call CopyPool::copy concurrently -- thread t with sources t-th offset
//                                     from a 16-byte boundary, every size, every destination offset
// Exit status 0 = all checks passed.
#include "host_copy.hpp"

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <atomic>
#include <thread>
#include <vector>

using namespace eicos;

static std::atomic<int> g_failed{0}, g_cases{0};
#define CHECK(cond)                                                                   \
    do {                                                                              \
        g_cases++;                                                                    \
        if (!(cond)) { std::printf("line %d: %s\n", __LINE__, #cond); g_failed++; }   \
    } while (0)

static const size_t MB = 1u << 20;
static const size_t SIZES[] = {0, 1, 15, 4095, 4096, 4097, MB - 1, MB + 1, 3 * MB + 17, 12 * MB + 5};
static const size_t OFFSETS[] = {0, 1, 7, 15};

// the pieces of one copy: piece 0 starts at 0, each piece starts where the one before ended, none runs backwards, the last ends at
// `bytes`; every piece but empty ones starts on a multiple of 64; returns how many pieces are empty
static int check_pieces(size_t bytes, int threads) {
    const CopyPieces pc = copy_pieces(bytes, threads);
    CHECK(pc.parts >= 1 && pc.parts <= threads + 1 && pc.bytes == bytes);
    size_t at = 0;
    int empty = 0;
    bool ok = true;
    for (int k = 0; k < pc.parts; k++) {
        const size_t a = pc.begin(k), b = pc.end(k);
        ok = ok && a == at && b >= a && b <= bytes && (a == b || a % 64 == 0);
        empty += a == b;
        at = b;
    }
    CHECK(ok);
    CHECK(at == bytes);
    return empty;
}

static void pieces_mode() {
    for (size_t bytes : SIZES)
        for (int threads : {0, 1, 3, 10, 64}) {
            const int empty = check_pieces(bytes, threads);
            // with the 0 ... 64 helpers the knob allows a piece is >= 1 MB and the rounding to 64 bytes cannot use one up: only the
            // one piece of an empty copy is empty
            CHECK(empty == (bytes == 0 ? 1 : 0));
        }
    // the numbers of the rule, by hand.  Below 1 MB + 1, or without helpers: one piece, the whole copy.
    CHECK(copy_pieces(MB, 10).parts == 1 && copy_pieces(MB, 10).end(0) == MB);
    CHECK(copy_pieces(12 * MB + 5, 0).parts == 1 && copy_pieces(12 * MB + 5, 0).end(0) == 12 * MB + 5);
    // 1 MB + 1 over 3 helpers: ceil = 2 parts, 524289 bytes each rounded up to 524352
    { const CopyPieces p = copy_pieces(MB + 1, 3); CHECK(p.parts == 2 && p.per == 524352 && p.begin(1) == 524352 && p.end(1) == MB + 1); }
    // 3 MB + 17 over 3 helpers: 4 parts of ceil(3145745 / 4) = 786437 -> 786496; over 1 helper: 2 parts of 1572873 -> 1572928
    { const CopyPieces p = copy_pieces(3 * MB + 17, 3); CHECK(p.parts == 4 && p.per == 786496 && p.begin(3) == 2359488 && p.end(3) == 3145745); }
    { const CopyPieces p = copy_pieces(3 * MB + 17, 1); CHECK(p.parts == 2 && p.per == 1572928 && p.end(1) == 3145745); }
    // 12 MB + 5 over 10 helpers: 11 parts of ceil(12582917 / 11) = 1143902 -> 1143936; over 64: 13 parts of 967917 -> 967936
    { const CopyPieces p = copy_pieces(12 * MB + 5, 10); CHECK(p.parts == 11 && p.per == 1143936 && p.begin(10) == 11439360 && p.end(10) == 12582917); }
    { const CopyPieces p = copy_pieces(12 * MB + 5, 64); CHECK(p.parts == 13 && p.per == 967936 && p.begin(12) == 11615232); }
    // Empty last pieces need more parts than the knob allows -- the rule as arithmetic, nothing is copied: 65536 parts of 1 MB + 1 byte
    // round up to 1 MB + 64, so 65533 pieces hold the copy and the last three are empty (32768 parts: the last one).
    CHECK(check_pieces((size_t)65536 * (MB + 1), 65535) == 3);
    CHECK(check_pieces((size_t)32768 * (MB + 1), 32767) == 1);
    { const CopyPieces p = copy_pieces((size_t)65536 * (MB + 1), 65535); CHECK(p.parts == 65536 && p.per == MB + 64 && p.begin(65533) == p.bytes && p.end(65535) == p.bytes); }
}

// one caller: source offset `soff`, every size, every destination offset.  The source is a block of exactly soff + size bytes (a read
// past its end is the address sanitizer's to report); the destination has GUARD bytes of 0xA5 on both sides.
static void caller(int t, const std::vector<unsigned char> &pattern) {
    const size_t GUARD = 64, soff = OFFSETS[t];
    for (size_t size : SIZES) {
        unsigned char *sblock = (unsigned char *)std::malloc(soff + size + 1), *dblock = (unsigned char *)std::malloc(GUARD + 15 + size + GUARD);
        if (!sblock || !dblock) { std::printf("out of memory\n"); g_failed++; std::free(sblock); std::free(dblock); return; }
        // (malloc blocks are 16-byte aligned; the source ends at the block's end but for one byte that keeps size 0 a valid malloc)
        unsigned char *src = sblock + soff;
        CHECK(((uintptr_t)sblock & 15) == 0 && ((uintptr_t)dblock & 15) == 0);
        std::memcpy(src, pattern.data() + t, size);
        for (size_t doff : OFFSETS) {
            unsigned char *dst = dblock + GUARD + doff;
            std::memset(dblock, 0xA5, GUARD + 15 + size + GUARD);
            CopyPool::get().copy(dst, src, size);
            CHECK(std::memcmp(dst, src, size) == 0 && std::memcmp(dst, pattern.data() + t, size) == 0);
            bool guards = true;
            for (size_t i = 0; i < GUARD + doff; i++) guards = guards && dblock[i] == 0xA5;
            for (size_t i = 0; i < GUARD; i++) guards = guards && dst[size + i] == 0xA5;
            CHECK(guards);
        }
        std::free(sblock); std::free(dblock);
    }
}

static void copy_mode(int threads) {
    CHECK(CopyPool::get().threads() == threads); // (the knob reached the pool: the run tests the setting it says it tests)
    CHECK(usable_cores() >= 1);
    std::vector<unsigned char> pattern(12 * MB + 5 + 4);
    for (size_t i = 0; i < pattern.size(); i++) pattern[i] = (unsigned char)(i * 131u + (i >> 12)); // (no period of a power of two: a piece copied to the wrong place shows)
    std::vector<std::thread> callers;
    for (int t = 0; t < 4; t++) callers.emplace_back(caller, t, std::cref(pattern));
    for (auto &c : callers) c.join();
    // stream_copy on its own, below and above its 4096-byte switch, from the caller's thread
    for (size_t size : {(size_t)4095, (size_t)4096, (size_t)65536 + 3}) {
        std::vector<unsigned char> d(size + 2, 0xA5);
        stream_copy(d.data() + 1, pattern.data(), size);
        CHECK(std::memcmp(d.data() + 1, pattern.data(), size) == 0 && d[0] == 0xA5 && d[size + 1] == 0xA5);
    }
}

int main(int argc, char **argv) {
    if (argc == 2 && std::strcmp(argv[1], "pieces") == 0) pieces_mode();
    else if (argc == 3 && std::strcmp(argv[1], "copy") == 0) copy_mode(std::atoi(argv[2]));
    else { std::printf("usage: host_copy_check pieces | copy THREADS\n"); return 2; }
    if (g_failed) { std::printf("%d check(s) failed\n", g_failed.load()); return 1; }
    std::printf("host_copy_check %s: %d cases, all passed\n", argv[1], g_cases.load());
    return 0;
}
