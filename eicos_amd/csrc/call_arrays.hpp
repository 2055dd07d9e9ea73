// The caller's arrays of one sensitivity or rollout call (api.cpp: adjoint_run, rollout_gradient, rollout_data_gradient, ...), declared
// once each: all in host memory, or all in device memory for the call's _device form.  The host form stages them in one device buffer
// -- copied in, the launch, copied out --, the device form hands the caller's pointers through.  From the one declaration come the kind
// fault, the bytes of the staging, every array's device pointer and the copies, so that none of them can disagree with another.
// Host only, and no HIP symbol, as resources.hpp: the memory-kind query and the two copies come from a policy (api.cpp: StageMem).
//   Mem: error_t, stream_t, ok;  on_device(const void *) -> bool;
//        to_device(void *dst, const void *src, size_t bytes, stream_t) -> error_t;  to_host(the same) -> error_t, both asynchronous
#pragma once

#include <cstddef>
#include <string>

namespace eicos {

template <class Mem> struct CallArrays {
    using error_t = typename Mem::error_t;
    static constexpr int CAP = 16;
    enum Dir { FIXED, IN, OUT };
    struct Part { const char *name; void *host; size_t bytes, at; Dir dir; bool staged; };
    Part part[CAP];
    int n = 0;
    size_t end = 0;          // of the last staged part: what the staging needs
    char *base = nullptr;    // place()
    bool device, overflow = false;

    explicit CallArrays(bool device_form) : device(device_form) {}

    // Each returns the part's handle for at().  Every staged part starts on a 64-byte boundary.
    // fixed: a part of the buffer that both forms have and nobody copies (the launch's record, an index list, the kernel's own rows)
    int fixed(size_t bytes) { return add(nullptr, nullptr, bytes, FIXED); }
    // in / out: `count` doubles at p, named as the C header names them.  NULL or no width: no device array, no copy, no bytes.
    int in(const char *name, const double *p, size_t count) { return add(name, const_cast<double *>(p), count * sizeof(double), IN); }
    int out(const char *name, double *p, size_t count) { return add(name, p, count * sizeof(double), OUT); }

    // The first declared array that does not live where the form takes its arrays, as a message; empty: none.  paired: the entry
    // point has a form of the other kind to point to.
    std::string kind_fault(const char *who, bool paired = true) const {
        if (overflow) return std::string(who) + ": more than " + std::to_string(CAP) + " arrays declared";
        for (int i = 0; i < n; i++) {
            const Part &q = part[i];
            if (q.dir == FIXED || !q.host || Mem::on_device(q.host) == device) continue;
            return std::string(who) + ": " + q.name +
                   (device ? " must live in device memory (the form without _device takes host pointers)"
                           : paired ? " lives in device memory: this form takes host pointers (use the _device form)"
                                    : " lives in device memory: this form takes host pointers");
        }
        return std::string();
    }
    size_t bytes() const { return end; }
    void place(void *buffer) { base = static_cast<char *>(buffer); }
    // The device pointer of a part: its place in the buffer, the caller's own pointer in the device form, NULL where there is no array
    void *at(int i) const {
        const Part &q = part[i];
        if (q.staged) return base + q.at;
        return device && q.dir != FIXED && q.bytes ? q.host : nullptr;
    }
    double *dbl(int i) const { return static_cast<double *>(at(i)); }
    // The host form's copies, enqueued in declaration order
    error_t copy_in(typename Mem::stream_t stream) const { return copy(IN, stream); }
    error_t copy_out(typename Mem::stream_t stream) const { return copy(OUT, stream); }

private:
    int add(const char *name, void *host, size_t bytes, Dir dir) {
        if (n == CAP) { overflow = true; return 0; } // (kind_fault refuses the call)
        Part &q = part[n];
        q = Part{name, host, bytes, 0, dir, dir == FIXED || (!device && host && bytes)};
        if (q.staged) { q.at = (end + 63) & ~(size_t)63; end = q.at + bytes; }
        return n++;
    }
    error_t copy(Dir dir, typename Mem::stream_t stream) const {
        for (int i = 0; i < n; i++) {
            const Part &q = part[i];
            if (q.dir != dir || !q.staged) continue;
            const error_t e = dir == IN ? Mem::to_device(base + q.at, q.host, q.bytes, stream) : Mem::to_host(q.host, base + q.at, q.bytes, stream);
            if (e != Mem::ok) return e;
        }
        return Mem::ok;
    }
};

} // namespace eicos
