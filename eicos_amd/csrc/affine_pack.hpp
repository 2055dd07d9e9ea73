// Affine maps on the host, one path for all of them (parameter, output, plant, matrix, shift and fallback map): every map is a handful of groups
// "base vector + CSR matrix" (eicos_affine_map) that is validated by affine_fault and packed by affine_pack into ONE device allocation
//     [header | gap | base, val of every present group (doubles) | rowptr, col of every present group (ints)]
// whose header takes the map's descriptor.  Host only: no HIP, so that the sanitizer check under tests/host compiles it on its own.
#pragma once
#include "../../include/eicos_amd.h"

#include <algorithm>
#include <cstddef>
#include <string>
#include <vector>

namespace eicos {
// One group of a map as its setter describes it: the caller's arrays (NULL: the group is absent), its row count, its column bound, and the
// two strings that vary in the messages -- the prefix ("shift map of s: ") and the name of the bound ("[0, k)").
struct AffineGroup { const eicos_affine_map *map; int rows, cols; std::string who; const char *bound; };

// The validation ladder.  true, with the message in msg, at the first fault of a present group.
inline bool affine_fault(const AffineGroup &g, std::string &msg) {
    const eicos_affine_map *a = g.map;
    if (!a) return false;
    const auto fault = [&](const std::string &what) { msg = g.who + what; return true; };
    if (!a->base || !a->rowptr) return fault("base or rowptr is NULL");
    if (a->rowptr[0] != 0) return fault("rowptr[0] must be 0");
    for (int r = 0; r < g.rows; r++)
        if (a->rowptr[r + 1] < a->rowptr[r]) return fault("rowptr decreases at row " + std::to_string(r));
    const int nnz = a->rowptr[g.rows];
    if (nnz > 0 && (!a->col || !a->val)) return fault("col or val is NULL");
    for (int t = 0; t < nnz; t++)
        if (a->col[t] < 0 || a->col[t] >= g.cols)
            return fault("column " + std::to_string(a->col[t]) + " of entry " + std::to_string(t) + " is outside " + g.bound);
    return false;
}

// The layout of n VALIDATED groups behind `header` bytes and a gap of `gap` bytes (both multiples of 8: the doubles stay aligned).
struct AffineLayout {
    size_t header = 0, gap = 0, nd = 0, ni = 0; // nd doubles, then ni ints
    size_t doubles_at() const { return header + gap; }
    size_t ints_at() const { return doubles_at() + nd * sizeof(double); }
    size_t bytes() const { return ints_at() + ni * sizeof(int); } // the device allocation
};
inline AffineLayout affine_layout(const AffineGroup *g, int n, size_t header, size_t gap) {
    AffineLayout L;
    L.header = header; L.gap = gap;
    for (int q = 0; q < n; q++) {
        if (!g[q].map) continue;
        const size_t rows = (size_t)g[q].rows, nnz = (size_t)g[q].map->rowptr[g[q].rows];
        L.nd += rows + nnz; L.ni += rows + 1 + nnz;
    }
    return L;
}

// The host image of everything but the gap ([header, zeroed | doubles | ints], L.bytes() - L.gap bytes), and in out[q] the addresses the
// arrays of group q get in an allocation that starts at dev_base (all NULL for an absent group).  Dev: launch.hpp's AffineDev, or any
// struct with its four members.
template <class Dev>
std::vector<char> affine_pack(const AffineGroup *g, int n, const AffineLayout &L, const void *dev_base, Dev *out) {
    std::vector<char> image(L.bytes() - L.gap);
    double *hd = reinterpret_cast<double *>(image.data() + L.header);
    int *hi = reinterpret_cast<int *>(image.data() + L.header + L.nd * sizeof(double));
    const double *dd = reinterpret_cast<const double *>(static_cast<const char *>(dev_base) + L.doubles_at());
    const int *di = reinterpret_cast<const int *>(static_cast<const char *>(dev_base) + L.ints_at());
    size_t od = 0, oi = 0;
    for (int q = 0; q < n; q++) {
        out[q] = Dev{};
        const eicos_affine_map *a = g[q].map;
        if (!a) continue;
        const size_t rows = (size_t)g[q].rows, nnz = (size_t)a->rowptr[g[q].rows];
        out[q].base = dd + od; std::copy(a->base, a->base + rows, hd + od); od += rows;
        out[q].val = dd + od; if (nnz) std::copy(a->val, a->val + nnz, hd + od); od += nnz;
        out[q].rowptr = di + oi; std::copy(a->rowptr, a->rowptr + rows + 1, hi + oi); oi += rows + 1;
        out[q].col = di + oi; if (nnz) std::copy(a->col, a->col + nnz, hi + oi); oi += nnz;
    }
    return image;
}
} // namespace eicos
