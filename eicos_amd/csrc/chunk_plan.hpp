// Transfers that go through a staging area, described once: how the given arrays of a chunk of instances are packed into the area, how
// large the area is, and how many instances a chunk holds on each path.  Functions of plain integers: no HIP, no eicos_batch, no
// environment (the callers in api.cpp read the knobs, own the areas and issue the copies and launches).  tests/host/chunk_plan_check.cpp
// checks every rule against numbers laid out by hand.
#pragma once

#include <algorithm>
#include <cstddef>

namespace eicos {
#pragma GCC visibility push(hidden) // (internal to the library: not part of its exported symbols)

// ---- the packed chunk -----------------------------------------------------------------------------------------------------
// The (up to) five arrays of an updateData -- G, A, c, h, b; `w` doubles per instance each -- of `rows` instances, the given ones behind
// each other in one area.  Two padding rules are in use.  They place the arrays at different addresses, and those are addresses the
// kernels read over PCIe, so each path keeps the rule it was measured with (docs/HISTORY.md A.34: merging them is an open item).
enum class ChunkPad {
    // 8 doubles of slack behind every given array.  What it guarantees: two arrays never share a 64-byte line, and an array of no width
    // still has an address of its own.  What it does NOT guarantee: an array behind the first starts on a 64-byte boundary only where
    // rows * w of every array in front of it is a multiple of 8.  (The host bounce, the peer staging, the staged fused update.)
    Gap8,
    // every given array rounded up to a multiple of 8 doubles.  What it guarantees: in a 64-byte aligned area EVERY given array starts
    // on a 64-byte boundary, for any rows and w.  Arrays of no width take no room and share the next array's address.  (The matrix-map
    // staging, whose arrays the expansion kernel writes and updateData reads in device memory.)
    RoundUp8,
};
struct PackedChunk {
    size_t off[5]; // of the given arrays, in doubles from the start of the area (0 where not given)
    size_t total;  // doubles from the start of the area to the end of the last array's padding
};
inline PackedChunk pack_chunk(const size_t w[5], const bool given[5], size_t rows, ChunkPad pad) {
    PackedChunk p{{0, 0, 0, 0, 0}, 0};
    for (int q = 0; q < 5; q++) {
        if (!given[q]) continue;
        p.off[q] = p.total;
        p.total += pad == ChunkPad::Gap8 ? rows * w[q] + 8 : (rows * w[q] + 7) / 8 * 8;
    }
    return p;
}

// ---- how large an area is ----------------------------------------------------------------------------------------------------
// None of the three is the packed total: each is what its path has always reserved, an upper bound of it for every chunk >= 1.
// The bounce buffers and the peer staging buffer, `per` = doubles per instance over the given arrays: room for five gaps per INSTANCE.
inline size_t staging_doubles(size_t per, int chunk) { return (size_t)chunk * (per + 5 * 8); }
// The matrix-map staging buffer holds `chunk` instances of matrix_stage_row doubles: one gap per given array and instance.
inline size_t matrix_stage_row(const size_t w[5], const bool given[5]) {
    size_t per = 0;
    for (int q = 0; q < 5; q++) if (given[q]) per += w[q] + 8;
    return per;
}
// (the staging buffer of the staged fused update holds the whole batch as ONE packed chunk: pack_chunk(..., batch, Gap8).total)

// ---- how many instances a chunk holds ------------------------------------------------------------------------------------------
constexpr size_t PIN_CHUNK_BYTES = 16u << 20; // bounce buffer size aimed at (per buffer)
inline int chunk_count(int rows, int chunk) { return (rows + chunk - 1) / chunk; }
// host arrays in, through the bounce buffers: ~16 MB of rows with their share of the gaps, at least 16 instances, at most all of them
inline int bounce_in_chunk(size_t per, int count) {
    int chunk = (int)std::max<size_t>(16, PIN_CHUNK_BYTES / (staging_doubles(per, 1) * sizeof(double)));
    chunk = std::min(chunk, count);
    if (count > chunk && count < 2 * chunk) chunk = (count + 1) / 2; // two even chunks rather than a long one and a stub
    return chunk;
}
// results out, through the bounce buffers: ~4 MB -- small enough that the device-to-host copy of one chunk and the host copy of the
// previous one overlap on a result of a few MB
inline int bounce_out_chunk(size_t row_bytes, int count) {
    return std::min((int)std::max<size_t>(16, (PIN_CHUNK_BYTES / 4) / row_bytes), count);
}
// a result this small takes one strided copy instead, wherever it goes
inline bool small_result(size_t bytes) { return bytes < (256u << 10); }
// the staged fused update, `per` = doubles per instance over the STAGED arrays: ~12 MB -- the copy pool splits an array's share of a chunk
// into pieces of >= 1 MB over its threads, so a chunk must be large enough to keep them busy and small enough that the first workgroups
// start after a fraction of the whole copy; at least 8 instances
inline int fused_stage_chunk(size_t per, int batch) {
    return (int)std::max<size_t>(8, std::min<size_t>((size_t)batch, (12u << 20) / std::max<size_t>(per * sizeof(double), 1)));
}
// the matrix-map staging: what fits `cap` doubles, at least one instance
inline int matrix_stage_chunk(size_t row, int count, size_t cap) { return (int)std::max<size_t>(1, std::min<size_t>((size_t)count, cap / row)); }
// peer copies without peer access: one stream synchronisation per chunk
constexpr int PEER_CHUNK = 256;

#pragma GCC visibility pop
} // namespace eicos
