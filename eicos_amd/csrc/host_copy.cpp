// The host's copies between pageable and pinned memory (host_copy.hpp).  No HIP.
#include "host_copy.hpp"

#include <emmintrin.h>
#include <sched.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "envknob.hpp"

namespace eicos {

void stream_copy(void *dst, const void *src, size_t bytes) {
    static const bool nt = env_knob("EICOS_COPY_NT", 1, 0, 1) != 0;
    char *d = (char *)dst; const char *s = (const char *)src;
    if (!nt || bytes < 4096) { std::memcpy(d, s, bytes); return; }
    // (the stores need a 16-byte aligned destination: the bytes in front of the first such address, then blocks of 64, then the rest)
    const size_t head = std::min(bytes, (size_t)((16 - ((uintptr_t)d & 15)) & 15));
    std::memcpy(d, s, head); d += head; s += head; bytes -= head;
    const size_t blocks = bytes / 64;
    for (size_t i = 0; i < blocks; i++, d += 64, s += 64) {
        const __m128i a = _mm_loadu_si128((const __m128i *)s), b = _mm_loadu_si128((const __m128i *)(s + 16));
        const __m128i c = _mm_loadu_si128((const __m128i *)(s + 32)), e = _mm_loadu_si128((const __m128i *)(s + 48));
        _mm_stream_si128((__m128i *)d, a); _mm_stream_si128((__m128i *)(d + 16), b);
        _mm_stream_si128((__m128i *)(d + 32), c); _mm_stream_si128((__m128i *)(d + 48), e);
    }
    _mm_sfence();
    std::memcpy(d, s, bytes - blocks * 64);
}

int usable_cores() {
    int n = (int)std::max(1u, std::thread::hardware_concurrency());
    cpu_set_t set;
    if (sched_getaffinity(0, sizeof set, &set) == 0) n = std::max(1, CPU_COUNT(&set));
    if (FILE *f = std::fopen("/sys/fs/cgroup/cpu.max", "r")) {
        char q[32] = {0}; long period = 0;
        if (std::fscanf(f, "%31s %ld", q, &period) == 2 && std::strcmp(q, "max") != 0 && period > 0) n = std::max(1, std::min(n, (int)(std::atol(q) / period)));
        std::fclose(f);
    }
    return n;
}

CopyPool &CopyPool::get() { static CopyPool p; return p; }

void CopyPool::copy(void *dst, const void *src, size_t bytes) {
    const CopyPieces pc = copy_pieces(bytes, nthreads_);
    if (pc.parts <= 1) { stream_copy(dst, src, bytes); return; }
    // completion state on the caller's stack: the count is changed and the caller notified INSIDE the lock, so a helper's last access to
    // these objects is its unlock, which the caller's wait cannot overtake
    int left = pc.parts - 1;
    std::mutex done_mu; std::condition_variable done_cv;
    for (int k = 1; k < pc.parts; k++) {
        const size_t a = pc.begin(k), b = pc.end(k);
        push([=, &left, &done_mu, &done_cv] {
            if (b > a) stream_copy((char *)dst + a, (const char *)src + a, b - a);
            std::lock_guard<std::mutex> lk(done_mu);
            if (--left == 0) done_cv.notify_one();
        });
    }
    stream_copy(dst, src, pc.end(0));
    std::unique_lock<std::mutex> lk(done_mu);
    done_cv.wait(lk, [&] { return left == 0; });
}

CopyPool::CopyPool() {
    // the bounce copy of a host-pointer updateData must keep up with the PCIe link (~50 GB/s; one core copies ~10 GB/s): up to ten
    // helper threads, two cores left to the caller and the runtime; EICOS_COPY_THREADS overrides (experiments)
    const int cores = usable_cores();
    nthreads_ = env_knob("EICOS_COPY_THREADS", std::max(0, std::min(10, cores - 2)), 0, 64);
    for (int i = 0; i < nthreads_; i++) th_.emplace_back([this] { run(); });
}
CopyPool::~CopyPool() {
    { std::lock_guard<std::mutex> lk(mu_); stop_ = true; }
    cv_.notify_all();
    for (auto &t : th_) t.join();
}
void CopyPool::push(std::function<void()> f) { { std::lock_guard<std::mutex> lk(mu_); q_.push_back(std::move(f)); } cv_.notify_one(); }
void CopyPool::run() {
    for (;;) {
        std::function<void()> f;
        {
            std::unique_lock<std::mutex> lk(mu_);
            cv_.wait(lk, [&] { return stop_ || !q_.empty(); });
            if (q_.empty()) return;
            f = std::move(q_.front()); q_.erase(q_.begin());
        }
        f();
    }
}

} // namespace eicos
