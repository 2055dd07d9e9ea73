// Who owns a handle's memory: one move-only buffer type and one "pinned buffer + event of its last GPU use" type.  Every allocation of
// eicos_batch (api.cpp) is a member of one of the two, so that freeing is what the handle's destructor does and "grow on demand" is one
// rule.  Host only, and no HIP symbol: the memory and event calls come from small policy structs (api.cpp: DeviceMem, PinnedMem,
// HipEvent), so that the check under tests/host compiles this header on its own, with policies that record what they are asked to do.
//   Mem: error_t, stream_t, ok;  alloc(void **, size_t) -> error_t;  free(void *);  sync(stream_t) -> error_t
//   Ev : event_t (a pointer type);  create(event_t *) -> error_t, timing disabled;  destroy(event_t);
//        record(event_t, stream_t) -> error_t;  sync(event_t) -> error_t
#pragma once

#include <cstddef>

namespace eicos {

template <class Mem> struct Buffer {
    using error_t = typename Mem::error_t;
    void *p = nullptr;
    size_t bytes = 0;

    Buffer() = default;
    Buffer(const Buffer &) = delete;
    Buffer &operator=(const Buffer &) = delete;
    Buffer(Buffer &&o) noexcept : p(o.p), bytes(o.bytes) { o.p = nullptr; o.bytes = 0; }
    Buffer &operator=(Buffer &&o) noexcept {
        if (this != &o) { reset(); p = o.p; bytes = o.bytes; o.p = nullptr; o.bytes = 0; }
        return *this;
    }
    ~Buffer() { reset(); }

    // Frees; no synchronisation: the caller knows that nothing on the GPU uses the memory any more.
    void reset() {
        if (p) Mem::free(p);
        p = nullptr; bytes = 0;
    }
    // Exactly `bytes` into an empty buffer (the allocations made once); a failure leaves it empty.
    error_t alloc(size_t n) {
        reset();
        const error_t e = Mem::alloc(&p, n);
        if (e != Mem::ok) { p = nullptr; return e; }
        bytes = n;
        return Mem::ok;
    }
    // The grow rule: at least `n` bytes.  Large enough already: nothing happens and the contents stay.  Else work on `stream` may still
    // use the allocation that goes away, so the stream is waited for first -- only when there is one to free --, and the buffer gets
    // exactly `n` bytes: never smaller, no slack.  *grew: the contents are new.  A failure leaves the buffer empty.
    error_t reserve(size_t n, typename Mem::stream_t stream, bool *grew = nullptr) {
        if (grew) *grew = false;
        if (n <= bytes) return Mem::ok;
        if (p) { const error_t e = Mem::sync(stream); if (e != Mem::ok) return e; }
        const error_t e = alloc(n);
        if (grew) *grew = e == Mem::ok;
        return e;
    }
    template <class T> T *as() const { return static_cast<T *>(p); }
    explicit operator bool() const { return p != nullptr; }
};

// A pinned buffer the GPU reads or writes asynchronously, the event of its last such use and whether that use may still be running.
// The protocol: wait(), use the buffer on the host, enqueue the GPU work that touches it, mark(stream).
template <class Mem, class Ev> struct PinnedSlot {
    using error_t = typename Mem::error_t;
    Buffer<Mem> buf;
    typename Ev::event_t ev = nullptr; // created by the first mark()
    bool busy = false;

    PinnedSlot() = default;
    PinnedSlot(const PinnedSlot &) = delete;
    PinnedSlot &operator=(const PinnedSlot &) = delete;
    ~PinnedSlot() { if (ev) Ev::destroy(ev); }

    error_t wait() {
        if (!busy) return Mem::ok;
        const error_t e = Ev::sync(ev);
        if (e == Mem::ok) busy = false;
        return e;
    }
    error_t mark(typename Mem::stream_t stream) {
        if (!ev) { const error_t e = Ev::create(&ev); if (e != Mem::ok) { ev = nullptr; return e; } }
        const error_t e = Ev::record(ev, stream);
        if (e == Mem::ok) busy = true;
        return e;
    }
    // Buffer::reserve, except that what is waited for is the slot's own event, not the stream
    error_t reserve(size_t n) {
        if (n <= buf.bytes) return Mem::ok;
        const error_t e = wait();
        return e != Mem::ok ? e : buf.alloc(n);
    }
    template <class T> T *as() const { return buf.template as<T>(); }
};

} // namespace eicos
