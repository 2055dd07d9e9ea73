// Host check of eicos_amd/csrc/affine_pack.hpp (tests/test_affine_pack.py builds this with -fsanitize=address,undefined and runs it):
// the validation ladder's messages, word for word and in the order the setters have always reported them, and the layout of the packed
// allocation, offset by offset, against a device base address that is never dereferenced.  Exit status 0 = all checks passed.
#include "affine_pack.hpp"
#include "eicos_amd.h"

#include <cstdint>
#include <cstdio>
#include <cstring>

using namespace eicos;

static int g_failed = 0;
#define CHECK(cond)                                                                   \
    do {                                                                              \
        if (!(cond)) { std::printf("line %d: %s\n", __LINE__, #cond); g_failed++; }   \
    } while (0)

struct Dev { const double *base; const int *rowptr, *col; const double *val; }; // (the members of launch.hpp's AffineDev)

// 3 rows, columns in [0, 4): what `a` must be refused with
static void expect_fault(const eicos_affine_map &a, const char *text) {
    const AffineGroup g = {&a, 3, 4, "parameter map of c: ", "[0, k)"};
    std::string msg = "untouched";
    const bool bad = affine_fault(g, msg);
    if (!bad || msg != text) { std::printf("expected \"%s\", got %s \"%s\"\n", text, bad ? "fault" : "no fault", msg.c_str()); g_failed++; }
}

static void fault_cases() {
    const double base[3] = {1., 2., 3.}, val[3] = {.5, .25, .125};
    const int rowptr[4] = {0, 1, 2, 3}, col[3] = {0, 3, 2};
    std::string msg = "untouched";
    const eicos_affine_map good = {base, rowptr, col, val};
    CHECK(!affine_fault(AffineGroup{&good, 3, 4, "parameter map of c: ", "[0, k)"}, msg) && msg == "untouched");
    CHECK(!affine_fault(AffineGroup{nullptr, 3, 4, "parameter map of c: ", "[0, k)"}, msg) && msg == "untouched"); // (an absent group)
    const int empty[4] = {0, 0, 0, 0};
    const eicos_affine_map no_entries = {base, empty, nullptr, nullptr};
    CHECK(!affine_fault(AffineGroup{&no_entries, 3, 4, "parameter map of c: ", "[0, k)"}, msg) && msg == "untouched");

    expect_fault({nullptr, rowptr, col, val}, "parameter map of c: base or rowptr is NULL");
    expect_fault({base, nullptr, col, val}, "parameter map of c: base or rowptr is NULL");
    const int from1[4] = {1, 1, 2, 3};
    expect_fault({base, from1, col, val}, "parameter map of c: rowptr[0] must be 0");
    const int down[4] = {0, 2, 1, 3};
    expect_fault({base, down, col, val}, "parameter map of c: rowptr decreases at row 1");
    expect_fault({base, rowptr, nullptr, val}, "parameter map of c: col or val is NULL");
    expect_fault({base, rowptr, col, nullptr}, "parameter map of c: col or val is NULL");
    const int minus[3] = {0, -1, 2}, four[3] = {0, 3, 4};
    expect_fault({base, rowptr, minus, val}, "parameter map of c: column -1 of entry 1 is outside [0, k)");
    expect_fault({base, rowptr, four, val}, "parameter map of c: column 4 of entry 2 is outside [0, k)");
    // two faults: the earlier rung of the ladder is the one reported
    expect_fault({base, from1, four, val}, "parameter map of c: rowptr[0] must be 0");
    expect_fault({base, down, nullptr, val}, "parameter map of c: rowptr decreases at row 1");
    expect_fault({base, rowptr, minus, nullptr}, "parameter map of c: col or val is NULL");
    const int both[3] = {4, -1, 2};
    expect_fault({base, rowptr, both, val}, "parameter map of c: column 4 of entry 0 is outside [0, k)");
    // the prefix and the name of the bound are the group's
    const AffineGroup s = {&good, 3, 2, "shift map of s: ", "[0, rows)"};
    CHECK(affine_fault(s, msg) && msg == "shift map of s: column 3 of entry 1 is outside [0, rows)");
}

// groups of (rows, nnz) = (3, 4), absent, (1, 0), (5, 5) behind a 128-byte header and `gap` bytes
static void pack_case(size_t gap) {
    const size_t header = 128;
    const double b0[3] = {1., 2., 3.}, v0[4] = {10., 11., 12., 13.}, b2[1] = {-7.}, b3[5] = {.1, .2, .3, .4, .5}, v3[5] = {21., 22., 23., 24., 25.};
    const int r0[4] = {0, 2, 2, 4}, c0[4] = {1, 1, 0, 3}, r2[2] = {0, 0}, r3[6] = {0, 1, 2, 3, 4, 5}, c3[5] = {4, 3, 2, 1, 0};
    const eicos_affine_map m0 = {b0, r0, c0, v0}, m2 = {b2, r2, nullptr, nullptr}, m3 = {b3, r3, c3, v3};
    const AffineGroup g[4] = {{&m0, 3, 4, "a: ", "[0, 4)"}, {nullptr, 9, 4, "b: ", "[0, 4)"}, {&m2, 1, 4, "c: ", "[0, 4)"}, {&m3, 5, 5, "d: ", "[0, 5)"}};
    std::string msg;
    for (const AffineGroup &q : g) CHECK(!affine_fault(q, msg));

    const AffineLayout L = affine_layout(g, 4, header, gap);
    const size_t nd = 3 + 4 + 1 + 0 + 5 + 5, ni = 4 + 4 + 2 + 0 + 6 + 5;
    CHECK(L.nd == nd && L.ni == ni);
    CHECK(L.bytes() == header + gap + 8 * nd + 4 * ni);

    const char *dev = reinterpret_cast<const char *>(uintptr_t(0x7f0000100000)); // (never dereferenced)
    Dev out[4];
    std::memset(out, 0xff, sizeof out);
    const std::vector<char> image = affine_pack(g, 4, L, dev, out);
    CHECK(image.size() == L.bytes() - gap);

    // [header | gap | base[rows] val[nnz] per group | rowptr[rows + 1] col[nnz] per group], the offsets written out
    const size_t D = header + gap, I = D + 8 * nd;
    const auto at = [&](const void *p) { return size_t(reinterpret_cast<uintptr_t>(p) - reinterpret_cast<uintptr_t>(dev)); };
    CHECK(at(out[0].base) == D + 0 && at(out[0].val) == D + 24);
    CHECK(at(out[2].base) == D + 56 && at(out[2].val) == D + 64);
    CHECK(at(out[3].base) == D + 64 && at(out[3].val) == D + 104);
    CHECK(at(out[0].rowptr) == I + 0 && at(out[0].col) == I + 16);
    CHECK(at(out[2].rowptr) == I + 32 && at(out[2].col) == I + 40);
    CHECK(at(out[3].rowptr) == I + 40 && at(out[3].col) == I + 64);
    CHECK(I + 84 == L.bytes());
    CHECK(!out[1].base && !out[1].rowptr && !out[1].col && !out[1].val); // (the absent group)
    for (int q : {0, 2, 3}) CHECK(reinterpret_cast<uintptr_t>(out[q].base) % 8 == 0 && reinterpret_cast<uintptr_t>(out[q].val) % 8 == 0);
    CHECK((reinterpret_cast<uintptr_t>(dev) + D) % 8 == 0);

    // the image holds everything but the gap: a device offset behind the header lies `gap` bytes earlier in it
    const auto same = [&](const void *devp, const void *src, size_t bytes) {
        const size_t o = at(devp) - gap;
        return o >= header && o + bytes <= image.size() && std::memcmp(image.data() + o, src, bytes) == 0;
    };
    CHECK(same(out[0].base, b0, sizeof b0) && same(out[0].val, v0, sizeof v0) && same(out[0].rowptr, r0, sizeof r0) && same(out[0].col, c0, sizeof c0));
    CHECK(same(out[2].base, b2, sizeof b2) && same(out[2].rowptr, r2, sizeof r2));
    CHECK(same(out[3].base, b3, sizeof b3) && same(out[3].val, v3, sizeof v3) && same(out[3].rowptr, r3, sizeof r3) && same(out[3].col, c3, sizeof c3));
    for (size_t o = 0; o < header; o++) CHECK(image[o] == 0); // (the descriptor's place)
}

int main() {
    fault_cases();
    pack_case(0);
    pack_case(24);
    if (g_failed) { std::printf("%d check(s) failed\n", g_failed); return 1; }
    std::printf("affine_pack: ok\n");
    return 0;
}
