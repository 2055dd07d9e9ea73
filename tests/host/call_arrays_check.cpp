// Host check of eicos_amd/csrc/call_arrays.hpp (tests/test_call_arrays.py builds this with -fsanitize=address,undefined and runs it):
// CallArrays over a policy that answers the memory-kind query from a table, performs every copy it is asked for and writes it into a
// log.  The cases declare what the real calls of api.cpp declare, in their order and with widths of their kind; every placed part is
// written whole inside a block of exactly bytes(), so that the address sanitizer sees a part that leaves the block.  Exit status 0 =
// all checks passed.
#include "call_arrays.hpp"

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

using namespace eicos;

static int g_failed = 0, g_cases = 0;
#define CHECK(cond)                                                                   \
    do {                                                                              \
        g_cases++;                                                                    \
        if (!(cond)) { std::printf("line %d: %s\n", __LINE__, #cond); g_failed++; }   \
    } while (0)

struct Copy {
    char dir; const void *dst, *src; size_t bytes;
    bool operator==(const Copy &o) const { return dir == o.dir && dst == o.dst && src == o.src && bytes == o.bytes; }
};
static std::vector<Copy> g_copies;          // 'i' host to device, 'o' device to host, in call order
static std::vector<const void *> g_device;  // the pointers that live in "device memory"
static int g_queries = 0;

struct RecMem {
    using error_t = int; using stream_t = int *;
    static constexpr int ok = 0;
    static bool on_device(const void *p) { g_queries++; return std::find(g_device.begin(), g_device.end(), p) != g_device.end(); }
    static int to_device(void *dst, const void *src, size_t bytes, int *) { g_copies.push_back({'i', dst, src, bytes}); std::memcpy(dst, src, bytes); return 0; }
    static int to_host(void *dst, const void *src, size_t bytes, int *) { g_copies.push_back({'o', dst, src, bytes}); std::memcpy(dst, src, bytes); return 0; }
};
using Arr = CallArrays<RecMem>;

// What a case declared, beside the type's own bookkeeping: 'f' fixed, 'i' in, 'o' out
struct Decl { int handle; char dir; double *host; size_t bytes; };
struct Case {
    Arr a;
    std::vector<Decl> d;
    std::vector<std::vector<double>> mem; // the caller's arrays
    explicit Case(bool device) : a(device) { mem.reserve(Arr::CAP + 1); }
    void fixed(size_t bytes) { d.push_back({a.fixed(bytes), 'f', nullptr, bytes}); }
    // present: the caller gave the array (of `count` doubles, possibly none)
    void in(const char *name, bool present, size_t count) { double *p = host(present, count); d.push_back({a.in(name, p, count), 'i', p, count * sizeof(double)}); }
    void out(const char *name, bool present, size_t count) { double *p = host(present, count); d.push_back({a.out(name, p, count), 'o', p, count * sizeof(double)}); }
    double *host(bool present, size_t count) {
        if (!present) return nullptr;
        mem.emplace_back(count + 1, 1.5); // (+ 1: an array of no width still has an address)
        return mem.back().data();
    }
};

static bool wanted(const Decl &q) { return q.dir == 'f' || (q.host && q.bytes); }

// The host form: placement inside a block of exactly bytes(), then the copies
static void check_host_form(Case &c) {
    Arr &a = c.a;
    int st = 0;
    char *block = static_cast<char *>(std::malloc(a.bytes() ? a.bytes() : 1));
    a.place(block);
    size_t end = 0;
    std::vector<Copy> want_in, want_out;
    for (const Decl &q : c.d) {
        char *p = static_cast<char *>(a.at(q.handle));
        if (!wanted(q)) { CHECK(p == nullptr); continue; } // an absent array and one of no width: no device array ...
        CHECK(p != nullptr && a.dbl(q.handle) == static_cast<void *>(p));
        const size_t at = (size_t)(p - block);
        CHECK(at % 64 == 0);
        CHECK(at >= end); // declaration order, no overlap
        std::memset(p, 0x5a, q.bytes);
        end = at + q.bytes;
        if (q.dir == 'i') want_in.push_back({'i', p, q.host, q.bytes});
        if (q.dir == 'o') want_out.push_back({'o', q.host, p, q.bytes});
    }
    CHECK(end <= a.bytes());
    if (!c.d.empty() && wanted(c.d.back())) CHECK(end == a.bytes());
    size_t sum = 0; // ... and no bytes: the wanted parts alone, each rounded up to its boundary, reach bytes()
    for (const Decl &q : c.d) if (wanted(q)) sum = ((sum + 63) & ~(size_t)63) + q.bytes;
    CHECK(sum == a.bytes());
    g_copies.clear();
    CHECK(a.copy_in(&st) == 0 && g_copies == want_in);   // one per wanted input, in declaration order, none for anything else
    g_copies.clear();
    CHECK(a.copy_out(&st) == 0 && g_copies == want_out);
    g_copies.clear();
    std::free(block);
}

// The device form: the fixed parts alone take bytes, every array is the caller's own, nothing is copied
static void check_device_form(Case &c) {
    Arr &a = c.a;
    int st = 0;
    char *block = static_cast<char *>(std::malloc(a.bytes() ? a.bytes() : 1));
    a.place(block);
    size_t sum = 0;
    for (const Decl &q : c.d) {
        if (q.dir == 'f') {
            char *p = static_cast<char *>(a.at(q.handle));
            CHECK(p >= block && (size_t)(p - block) % 64 == 0 && (size_t)(p - block) >= sum);
            std::memset(p, 0x5a, q.bytes);
            sum = (size_t)(p - block) + q.bytes;
        } else CHECK(a.at(q.handle) == (q.bytes ? q.host : nullptr));
    }
    CHECK(sum == a.bytes());
    g_copies.clear();
    CHECK(a.copy_in(&st) == 0 && a.copy_out(&st) == 0 && g_copies.empty());
    std::free(block);
}

// ---- the real calls' declarations (api.cpp), with a pattern of lp_afiro's kind: odd widths, none a multiple of 8 doubles
static const size_t B = 8, N = 51, M = 51, P = 27, NNZG = 51, NNZA = 102, K = 3, R = 2, T = 3, HEADER = 128;

// adjoint_run: [record | ids | J | g | grad_c | grad_h | grad_b | grad_G | grad_A | res]
static void adjoint(Case &c, size_t rows, size_t k, bool g, bool J, bool grads, bool gG, bool gA, bool res) {
    c.fixed(HEADER); c.fixed(B * sizeof(int));
    c.out("J", J, rows * k); c.in("g", g, rows * N);
    c.out("grad_c", grads, rows * N); c.out("grad_h", grads, rows * M); c.out("grad_b", grads, rows * P);
    c.out("grad_G", gG, rows * NNZG); c.out("grad_A", gA, rows * NNZA); c.out("res", res, rows);
}
// rollout_gradient, the plant-gradient form: gu, gtheta, grad_theta0, grad_w, u_traj, theta_traj, grad_f0, grad_val
static void plant_gradient(Case &c, bool g0, size_t nnzF) {
    c.in("gu", true, B * T * R); c.in("gtheta", true, B * (T + 1) * K); c.out("grad_theta0", g0, B * K); c.out("grad_w", true, B * T * K);
    c.in("u_traj", true, B * T * R); c.in("theta_traj", true, B * (T + 1) * K); c.out("grad_f0", true, B * K); c.out("grad_val", true, B * nnzF);
}
// rollout_data_gradient: the sweep's own rows, three inputs, ten outputs (a parameter map without an h group: no grad_Hval, no width)
static void data_gradient(Case &c) {
    c.fixed(4 * (N + M + P) * sizeof(double));
    c.in("gu", false, B * T * R); c.in("gtheta", true, B * (T + 1) * K); c.in("theta_traj", true, B * (T + 1) * K);
    c.out("grad_c", true, B * N); c.out("grad_h", true, B * M); c.out("grad_b", false, B * P); c.out("grad_G", true, B * NNZG); c.out("grad_A", true, B * NNZA);
    c.out("grad_Cval", true, B * 7); c.out("grad_Hval", false, 0); c.out("grad_Bval", true, B * 5); c.out("grad_u0", true, B * R); c.out("grad_Uval", true, B * 4);
}

int main() {
    for (int device = 0; device < 2; device++) {
        auto check = device ? check_device_form : check_host_form;
        { Case c(device); adjoint(c, 5 * 2, 0, true, false, true, true, false, true); check(c); }   // the gradient form: grad_G and no grad_A
        { Case c(device); adjoint(c, 5 * 2, 0, true, false, true, false, true, false); check(c); }  // ... grad_A last, no res
        { Case c(device); adjoint(c, 3 * R, K, false, true, false, false, false, false); check(c); } // the contracted form (the output map's rows): J and no res
        { Case c(device); adjoint(c, 3 * 2, K, true, true, false, false, false, true); check(c); }   // ... nrhs rows of g, grad_theta and res
        { Case c(device); plant_gradient(c, false, 0); check(c); }                                   // no grad_theta0, a plant map without stored entries
        { Case c(device); plant_gradient(c, true, 9); check(c); }
        { Case c(device); data_gradient(c); check(c); }
    }
    {   // ---- a device form without a fixed part needs no buffer at all
        Case c(true); plant_gradient(c, true, 9);
        CHECK(c.a.bytes() == 0);
        Case e(false);
        CHECK(e.a.bytes() == 0 && e.a.kind_fault("f").empty());
    }
    {   // ---- the kind fault: the first offender in declaration order, by name; absent arrays are not asked about; fixed parts never
        Case c(false); adjoint(c, 4, 0, true, false, true, true, false, true);
        g_queries = 0;
        CHECK(c.a.kind_fault("eicos_batch_adjoint_data", false).empty() && g_queries == 6); // (g, three gradients, grad_G, res)
        g_device = {c.d[7].host, c.d[5].host}; // grad_G and grad_h
        CHECK(c.a.kind_fault("eicos_batch_adjoint_data", false) == "eicos_batch_adjoint_data: grad_h lives in device memory: this form takes host pointers");
        CHECK(c.a.kind_fault("w") == "w: grad_h lives in device memory: this form takes host pointers (use the _device form)");
        g_device = {c.d[7].host};
        CHECK(c.a.kind_fault("w").find("w: grad_G lives in device memory") == 0);
    }
    {   // ... the device form: the first array that is NOT in device memory; an array of no width is still the caller's and is asked about
        Case c(true); plant_gradient(c, false, 0);
        g_device.clear();
        for (const Decl &q : c.d) if (q.host) g_device.push_back(q.host);
        CHECK(c.a.kind_fault("eicos_batch_rollout_plant_gradient_device").empty());
        g_device.pop_back(); // grad_val, of no width
        CHECK(c.a.kind_fault("w_device") == "w_device: grad_val must live in device memory (the form without _device takes host pointers)");
        g_device.erase(g_device.begin() + 1); // gtheta
        CHECK(c.a.kind_fault("w_device").find("w_device: gtheta must live in device memory") == 0);
        g_device.clear();
    }
    {   // ---- more declarations than the type holds: refused, and nothing is written past the entries
        Case c(false);
        for (int q = 0; q < Arr::CAP; q++) c.in("a", true, 3);
        CHECK(c.a.kind_fault("w").empty() && c.a.n == Arr::CAP);
        const size_t bytes = c.a.bytes();
        c.in("b", true, 3);
        CHECK(c.a.n == Arr::CAP && c.a.bytes() == bytes && c.a.kind_fault("w") == "w: more than 16 arrays declared");
    }
    if (g_failed) { std::printf("%d check(s) failed\n", g_failed); return 1; }
    std::printf("call_arrays_check: %d cases, all passed\n", g_cases);
    return 0;
}
