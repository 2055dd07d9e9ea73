// Host check of eicos_amd/csrc/resources.hpp (tests/test_resources.py builds this with -fsanitize=address,undefined and runs it):
// Buffer and PinnedSlot over policies that allocate with malloc and write every call they get into a log, so that the order of
// synchronise / free / allocate is what is asserted, and the address sanitizer sees every leak and double free.  Exit status 0 = all
// checks passed.
#include "resources.hpp"

#include <cstdio>
#include <cstdlib>
#include <initializer_list>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

using namespace eicos;

static int g_failed = 0, g_cases = 0;
#define CHECK(cond)                                                                   \
    do {                                                                              \
        g_cases++;                                                                    \
        if (!(cond)) { std::printf("line %d: %s\n", __LINE__, #cond); g_failed++; }   \
    } while (0)

static std::vector<std::string> g_log; // "alloc", "free", "sync", "ev_create", "ev_destroy", "ev_record", "ev_sync", in call order
static bool g_fail_alloc = false;
static int g_live = 0;                 // allocations not yet freed
static int g_events = 0;               // events not yet destroyed

struct Stream { int id; };
struct RecMem {
    using error_t = int; using stream_t = Stream *;
    static constexpr int ok = 0;
    static int alloc(void **p, size_t bytes) {
        g_log.push_back("alloc");
        if (g_fail_alloc) { *p = reinterpret_cast<void *>(0x10); return 2; } // (a failing allocator may leave garbage behind: the buffer must not keep it)
        *p = std::malloc(bytes ? bytes : 1);
        g_live++;
        return 0;
    }
    static void free(void *p) { g_log.push_back("free"); std::free(p); g_live--; }
    static int sync(Stream *) { g_log.push_back("sync"); return 0; }
};
struct RecEvent {
    using event_t = int *;
    static int create(int **e) { g_log.push_back("ev_create"); *e = new int(0); g_events++; return 0; }
    static void destroy(int *e) { g_log.push_back("ev_destroy"); delete e; g_events--; }
    static int record(int *e, Stream *) { g_log.push_back("ev_record"); ++*e; return 0; }
    static int sync(int *) { g_log.push_back("ev_sync"); return 0; }
};
using Buf = Buffer<RecMem>;
using Slot = PinnedSlot<RecMem, RecEvent>;

static int count(const char *what) { int c = 0; for (const std::string &s : g_log) c += s == what; return c; }
static bool log_is(std::initializer_list<const char *> want) {
    if (want.size() != g_log.size()) return false;
    size_t i = 0;
    for (const char *w : want) if (g_log[i++] != w) return false;
    return true;
}

static_assert(!std::is_copy_constructible<Buf>::value && !std::is_copy_assignable<Buf>::value, "Buffer is move-only");
static_assert(!std::is_copy_constructible<Slot>::value && !std::is_move_constructible<Slot>::value, "PinnedSlot stays where it is");

int main() {
    Stream st{1};
    {   // ---- growth from empty, no growth, growth from non-empty
        Buf b;
        bool grew = true;
        CHECK(!b && b.p == nullptr && b.bytes == 0);
        CHECK(b.reserve(0, &st, &grew) == 0 && !grew && g_log.empty()); // (nothing asked for: nothing done)
        CHECK(b.reserve(100, &st, &grew) == 0 && grew);
        CHECK(log_is({"alloc"})); // from empty: no sync, nothing to free
        CHECK(b && b.bytes == 100);
        void *p0 = b.p;
        static_cast<char *>(b.p)[99] = 1; // (the whole extent is ours: ASan would object)
        g_log.clear();
        CHECK(b.reserve(100, &st, &grew) == 0 && !grew && b.p == p0 && g_log.empty()); // equal
        CHECK(b.reserve(7, &st, &grew) == 0 && !grew && b.p == p0 && b.bytes == 100 && g_log.empty()); // smaller: never shrinks
        CHECK(b.reserve(7, &st) == 0 && g_log.empty()); // (grew is optional)
        CHECK(b.reserve(101, &st, &grew) == 0 && grew);
        CHECK(log_is({"sync", "free", "alloc"})); // strictly in this order
        CHECK(b.bytes == 101 && g_live == 1); // exactly the request, and the old allocation is gone
        CHECK(b.as<double>() == static_cast<double *>(b.p) && b.as<const int>() == static_cast<const int *>(b.p));
        g_log.clear();
        // ---- reset: a free and no sync
        b.reset();
        CHECK(log_is({"free"}) && !b && b.bytes == 0 && g_live == 0);
        b.reset();
        CHECK(log_is({"free"})); // (an empty buffer frees nothing)
        g_log.clear();
    }
    CHECK(g_log.empty()); // (the destructor of an empty buffer makes no call)
    {   // ---- the destructor frees exactly once
        { Buf b; CHECK(b.alloc(32) == 0 && b.bytes == 32 && log_is({"alloc"})); }
        CHECK(log_is({"alloc", "free"}) && g_live == 0);
        g_log.clear();
    }
    {   // ---- a failing allocation leaves the buffer empty and returns the policy's error; the next one works
        Buf b;
        bool grew = true;
        g_fail_alloc = true;
        CHECK(b.reserve(64, &st, &grew) == 2 && !grew && !b && b.p == nullptr && b.bytes == 0);
        CHECK(b.alloc(64) == 2 && b.p == nullptr && b.bytes == 0);
        g_fail_alloc = false;
        CHECK(b.reserve(64, &st, &grew) == 0 && grew && b.bytes == 64);
        g_fail_alloc = true; g_log.clear(); // growth of a NON-empty buffer fails: the old allocation is gone (once), nothing is kept
        CHECK(b.reserve(128, &st, &grew) == 2 && !grew && !b && b.bytes == 0);
        CHECK(log_is({"sync", "free", "alloc"}) && g_live == 0);
        g_fail_alloc = false;
        CHECK(b.reserve(16, &st, &grew) == 0 && grew && b.bytes == 16 && g_live == 1);
        g_log.clear();
    }
    CHECK(log_is({"free"}) && g_live == 0);
    g_log.clear();
    {   // ---- moves: the source is left empty, the destination's old allocation is freed exactly once
        Buf a, b;
        CHECK(a.alloc(10) == 0 && b.alloc(20) == 0);
        void *pa = a.p;
        g_log.clear();
        Buf c(std::move(a));
        CHECK(g_log.empty() && c.p == pa && c.bytes == 10 && !a && a.bytes == 0);
        b = std::move(c);
        CHECK(log_is({"free"}) && b.p == pa && b.bytes == 10 && !c && c.bytes == 0 && g_live == 1);
        Buf &self = b;
        b = std::move(self); // (self-assignment keeps the allocation)
        CHECK(log_is({"free"}) && b.p == pa && b.bytes == 10);
        g_log.clear();
        Buf empty;
        b = std::move(empty); // (an empty source: the destination is freed and left empty)
        CHECK(log_is({"free"}) && !b && g_live == 0);
        g_log.clear();
    }
    CHECK(g_log.empty() && g_live == 0); // (three empty buffers went away)
    {   // ---- PinnedSlot
        Slot s;
        CHECK(s.wait() == 0 && g_log.empty()); // never marked: no event call
        CHECK(s.reserve(0) == 0 && g_log.empty());
        CHECK(s.reserve(48) == 0 && log_is({"alloc"}) && s.buf.bytes == 48 && s.as<char>() == s.buf.p); // (not busy: no event call, and never the stream)
        g_log.clear();
        CHECK(s.mark(&st) == 0 && s.busy && log_is({"ev_create", "ev_record"})); // the event is created by the first mark
        CHECK(s.wait() == 0 && !s.busy && log_is({"ev_create", "ev_record", "ev_sync"}));
        CHECK(s.wait() == 0 && count("ev_sync") == 1); // the next wait makes no call
        CHECK(s.mark(&st) == 0 && s.busy && count("ev_create") == 1 && count("ev_record") == 2);
        g_log.clear();
        CHECK(s.reserve(48) == 0 && s.busy && g_log.empty()); // large enough: a busy slot is left alone
        CHECK(s.reserve(49) == 0 && !s.busy && s.buf.bytes == 49);
        CHECK(log_is({"ev_sync", "free", "alloc"})); // the slot's own event, before the free; no stream sync
        CHECK(s.mark(&st) == 0 && s.busy);
        g_log.clear();
    }
    CHECK(count("ev_destroy") == 1 && count("free") == 1 && count("ev_sync") == 0 && g_log.size() == 2); // (destruction waits for nothing)
    CHECK(g_live == 0 && g_events == 0);
    g_log.clear();
    { Slot s; }
    CHECK(g_log.empty()); // (a slot that was never marked has no event to destroy)
    if (g_failed) { std::printf("%d check(s) failed\n", g_failed); return 1; }
    std::printf("resources_check: %d cases, all passed\n", g_cases);
    return 0;
}
