// The host's copies between pageable and pinned memory: a memcpy with non-temporal stores, the rule that cuts a large copy into pieces,
// and the few persistent threads the pieces go to.  The only multithreaded host code of the library.  Pure host code: no HIP call, no
// eicos_batch.  host_copy.cpp is compiled without a HIP include path, and tests/host/host_copy_check.cpp runs it under the address,
// undefined-behaviour and thread sanitizers.
#pragma once

#include <algorithm>
#include <condition_variable>
#include <cstddef>
#include <functional>
#include <mutex>
#include <thread>
#include <vector>

namespace eicos {
#pragma GCC visibility push(hidden) // (internal to the library: not part of its exported symbols)

// memcpy with non-temporal stores: the destination of a bounce copy is read next by the GPU over PCIe (or is the caller's result array), never
// by this core -- regular stores would first read every destination line into the cache (read-for-ownership: a third more memory traffic)
// and evict the caller's working set.  glibc switches to such stores only above a few MB per call; the pool's pieces are ~1.5 MB.
// Ends with an sfence: the bytes are visible before any store the caller issues next.  EICOS_COPY_NT=0 (experiments): plain memcpy.
void stream_copy(void *dst, const void *src, size_t bytes);

// The piece rule: a copy of `bytes` over `threads` helpers and the caller is cut into `parts` pieces of `per` bytes, a multiple of 64 (so a
// piece of a 64-byte aligned destination starts on a cache line); piece k is [begin(k), end(k)).  At least 1 MB a piece: parts = 1 below
// 2 MB or without helpers -- then the caller copies alone.  The rounding up can leave the last pieces empty (begin == end == bytes).
struct CopyPieces {
    size_t bytes, per;
    int parts;
    size_t begin(int k) const { return std::min(bytes, (size_t)k * per); }
    size_t end(int k) const { return std::min(bytes, ((size_t)k + 1) * per); }
};
inline CopyPieces copy_pieces(size_t bytes, int threads) {
    const size_t piece = 1u << 20;
    const int parts = (int)std::min<size_t>((size_t)threads + 1, (bytes + piece - 1) / piece);
    if (parts <= 1) return {bytes, bytes, 1};
    return {bytes, ((bytes + parts - 1) / parts + 63) & ~(size_t)63, parts};
}

// cores this process may really use: the affinity mask, capped by the cgroup CPU quota (a container's hardware_concurrency() is the host's)
int usable_cores();

// A few persistent host threads that split large memcpy calls between pageable and pinned memory (one core copies ~10 GB/s, a PCIe 5
// x16 link moves ~50 GB/s: a single-threaded bounce copy would be the slowest stage of a host-pointer updateData).  Shared by every
// handle of the process -- the shards of an eicos_multi call copy() from parallel host threads --, started on first use, joined at exit.
class CopyPool {
  public:
    static CopyPool &get();
    // dst[0, bytes) = src[0, bytes), cut by copy_pieces over the pool's threads and the caller; returns when every piece is copied
    void copy(void *dst, const void *src, size_t bytes);
    int threads() const { return nthreads_; }
  private:
    CopyPool();
    ~CopyPool();
    void push(std::function<void()> f);
    void run();
    int nthreads_ = 0; bool stop_ = false;
    std::vector<std::thread> th_;
    std::vector<std::function<void()>> q_;
    std::mutex mu_; std::condition_variable cv_;
};

#pragma GCC visibility pop
} // namespace eicos
