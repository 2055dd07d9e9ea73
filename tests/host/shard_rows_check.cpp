// Stand-alone check (tests/test_shard_rows.py builds it with the address and undefined-behaviour sanitizers) of the row routing of the
// multi-GPU layer: eicos_amd/csrc/shard_rows.hpp, the header multi.cpp includes -- no HIP, no threads.  The shard is played by a callable
// that writes, for local id i of shard s, values derived from first[s] + i and from the packed input rows; the expected answer is a plain
// loop over the caller's list.
//   shard_rows_check layout | routing | refusals | failing | rules | sweep
// Exit status 0: everything held.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <memory>
#include <random>
#include <string>
#include <vector>

#include "eicos_amd.h"
#include "shard_rows.hpp"

using namespace eicos;

namespace {

int failures = 0, checks = 0;
std::string where; // the case under check, for the messages
#define EXPECT(cond, ...)                                                               \
    do {                                                                                \
        checks++;                                                                       \
        if (!(cond)) { failures++; std::printf("FAIL [%s] %s: ", where.c_str(), #cond); std::printf(__VA_ARGS__); std::printf("\n"); } \
    } while (0)

enum Type { DBL, INT, INFO };
size_t esize(Type t) { return t == DBL ? sizeof(double) : t == INT ? sizeof(int) : sizeof(eicos_info); }
void put(Type t, void *base, size_t i, double v) {
    if (t == DBL) static_cast<double *>(base)[i] = v;
    else if (t == INT) static_cast<int *>(base)[i] = (int)v;
    else { eicos_info r; std::memset(&r, 0, sizeof r); r.pcost = v; r.exitcode = (int)v; r.iter = (int)v + 1; static_cast<eicos_info *>(base)[i] = r; }
}
double get(Type t, const void *base, size_t i) { return t == DBL ? static_cast<const double *>(base)[i] : (double)static_cast<const int *>(base)[i]; }

// One column of a case.  given = false: the caller passes NULL.  Inputs are DBL or INT.
struct Spec { Type t; int w; bool input, given; Column::Rule rule; };
const unsigned char SENTINEL = 0xA5;

// The caller's array of a column: exactly rows * w elements on the heap, so that the sanitizer sees every byte beyond it; a given array
// without bytes is a pointer that must not be dereferenced (the end of a 16-byte block).
struct Array {
    std::unique_ptr<char[]> mem;
    size_t bytes = 0;
    char *ptr = nullptr;
    void make(const Spec &sp, size_t rows) {
        bytes = rows * (size_t)sp.w * esize(sp.t);
        if (!sp.given) return;
        mem.reset(new char[bytes ? bytes : 16]);
        ptr = bytes ? mem.get() : mem.get() + 16;
        std::memset(mem.get(), SENTINEL, bytes);
    }
};
Column column(const Spec &sp, char *ptr) {
    if (sp.t == DBL) return sp.input ? in((const double *)ptr, sp.w) : out((double *)ptr, sp.w, sp.rule);
    if (sp.t == INT) return sp.input ? in((const int *)ptr, sp.w) : out((int *)ptr, sp.w, sp.rule);
    return out((eicos_info *)ptr, sp.w, sp.rule);
}
// what the inputs of a row contribute to every output of that row: all values are small integers, so every type holds them exactly
double input_sum(const std::vector<Spec> &spec, void *const *ptr, size_t row) {
    double sum = 0;
    for (size_t c = 0; c < spec.size(); c++)
        for (int e = 0; spec[c].input && ptr[c] && e < spec[c].w; e++) sum += (double)(c + e + 1) * get(spec[c].t, ptr[c], row * spec[c].w + e);
    return sum;
}
double out_value(int gid, size_t c, int e, double insum) { return 100.0 * gid + 10.0 * (double)c + e + insum; }

struct Result { int rc = EICOS_OK, calls = 0; std::string refusal; std::vector<int> called; };

// One list-indexed call over `ns` shards of `batch` instances as multi.cpp makes it: the split, then every shard's share through
// serve_share, the first failing shard's code returned.  Checks the pointers the shard sees against the column rules and every byte of
// every output against the plain loop.  fail_shard >= 0: that shard writes its scratch, then returns EICOS_E_INVALID.
Result run_case(int batch, int ns, const int *idx, int count, bool prefix_form, const std::vector<Spec> &spec, int fail_shard = -1) {
    Result res;
    std::vector<int> first, cnt;
    shard_layout(batch, ns, first, cnt);
    const size_t rows = (size_t)std::max(count, 0), nc = spec.size();
    std::vector<Array> arr(nc);
    std::vector<Column> cols;
    std::vector<void *> caller(nc);
    for (size_t c = 0; c < nc; c++) {
        arr[c].make(spec[c], rows);
        caller[c] = arr[c].ptr;
        for (size_t i = 0; spec[c].input && spec[c].given && i < rows * (size_t)spec[c].w; i++) put(spec[c].t, arr[c].ptr, i, (double)((i * 7 + c * 3) % 50 + 1));
        cols.push_back(column(spec[c], arr[c].ptr));
    }
    // the expected outputs: sentinels, overwritten below by the plain loop where the call succeeds
    std::vector<std::vector<char>> want(nc);
    for (size_t c = 0; c < nc; c++) if (spec[c].given && !spec[c].input) want[c].assign(arr[c].bytes, (char)SENTINEL);

    Shares sh;
    res.refusal = split_list(first, batch, idx, count, "who", prefix_form, sh);
    if (!res.refusal.empty()) res.rc = EICOS_E_INVALID;
    for (int s = 0; res.refusal.empty() && s < ns; s++) {
        const int rc = serve_share(sh.ids[s], sh.pos[s], cols.data(), (int)nc, [&](const int *ids, int k, void *const *p) {
            res.calls++; res.called.push_back(s);
            EXPECT(k > 0 && k == (int)sh.pos[s].size(), "shard %d got k = %d", s, k);
            for (size_t c = 0; c < nc; c++) {
                const Spec &sp = spec[c];
                if (!sp.given) EXPECT(p[c] == nullptr, "column %zu was not given", c);
                else if (sp.w > 0) EXPECT(p[c] != nullptr && p[c] != caller[c], "column %zu: the shard gets scratch", c);
                else if (sp.input || sp.rule == Column::GIVEN) EXPECT(p[c] == caller[c], "column %zu: given at width 0 stays the caller's pointer", c);
                else if (sp.rule == Column::AT_LEAST_ONE) EXPECT(p[c] != nullptr && p[c] != caller[c], "column %zu: at least one element", c);
                else EXPECT(p[c] == nullptr, "column %zu: width 0, exact", c);
                if (sp.given && !sp.input && sp.w == 0 && sp.rule == Column::AT_LEAST_ONE) put(sp.t, p[c], 0, 1.0); // (one writable element: the sanitizer judges)
            }
            for (int q = 0; q < k; q++) {
                EXPECT(ids[q] >= 0 && ids[q] < cnt[s], "shard %d got local id %d", s, ids[q]);
                const double insum = input_sum(spec, p, (size_t)q);
                for (size_t c = 0; c < nc; c++)
                    for (int e = 0; !spec[c].input && p[c] && e < spec[c].w; e++) put(spec[c].t, p[c], (size_t)q * spec[c].w + e, out_value(first[s] + ids[q], c, e, insum));
            }
            return s == fail_shard ? (int)EICOS_E_INVALID : (int)EICOS_OK;
        });
        if (rc != EICOS_OK && res.rc == EICOS_OK) res.rc = rc;
    }
    // the plain loop over the caller's list
    for (size_t q = 0; res.refusal.empty() && q < rows; q++) {
        const int gid = idx ? idx[q] : (int)q;
        int s = 0;
        while (!(first[s] <= gid && gid < first[s] + cnt[s])) s++;
        if (s == fail_shard) continue;
        const double insum = input_sum(spec, caller.data(), q);
        for (size_t c = 0; c < nc; c++)
            for (int e = 0; !want[c].empty() && e < spec[c].w; e++) put(spec[c].t, want[c].data(), q * spec[c].w + e, out_value(gid, c, e, insum));
    }
    for (size_t c = 0; c < nc; c++) {
        if (!spec[c].given || spec[c].input) continue;
        size_t bad = 0;
        while (bad < arr[c].bytes && arr[c].ptr[bad] == want[c][bad]) bad++;
        EXPECT(bad == arr[c].bytes, "output column %zu differs from the plain loop at element %zu", c, bad / esize(spec[c].t));
    }
    return res;
}

const std::vector<Spec> FIVE = {{DBL, 3, true, true, Column::GIVEN},   {DBL, 0, true, true, Column::GIVEN}, {DBL, 2, true, false, Column::GIVEN},
                                {DBL, 3, false, true, Column::EXACT},  {INT, 1, false, true, Column::EXACT}, {INFO, 1, false, true, Column::EXACT}};

void layout() {
    struct { int batch, ns; std::vector<int> first, count; } cases[] = {
        {5, 2, {0, 3}, {3, 2}}, {7, 3, {0, 3, 5}, {3, 2, 2}}, {3, 3, {0, 1, 2}, {1, 1, 1}}, {4, 1, {0}, {4}}};
    for (auto &c : cases) {
        where = "layout " + std::to_string(c.batch) + " over " + std::to_string(c.ns);
        std::vector<int> first, count;
        shard_layout(c.batch, c.ns, first, count);
        EXPECT(first == c.first && count == c.count, "first[0] %d count[0] %d", first[0], count[0]);
    }
}

void routing() {
    where = "5 over 2, [4, 0, 3]";
    const int l1[] = {4, 0, 3};
    Result r = run_case(5, 2, l1, 3, false, FIVE);
    EXPECT(r.rc == EICOS_OK && r.calls == 2, "rc %d calls %d", r.rc, r.calls);
    where = "3 over 3, [1]";
    const int l2[] = {1};
    r = run_case(3, 3, l2, 1, false, FIVE);
    EXPECT(r.rc == EICOS_OK && r.calls == 1 && r.called == std::vector<int>{1}, "rc %d calls %d", r.rc, r.calls);
    where = "4 over 1, [2, 0, 3, 1]";
    const int l3[] = {2, 0, 3, 1};
    r = run_case(4, 1, l3, 4, false, FIVE);
    EXPECT(r.rc == EICOS_OK && r.calls == 1, "rc %d calls %d", r.rc, r.calls);
    where = "count 0";
    r = run_case(5, 2, l1, 0, false, FIVE);
    EXPECT(r.rc == EICOS_OK && r.calls == 0, "rc %d calls %d", r.rc, r.calls);
    r = run_case(5, 2, nullptr, 0, false, FIVE);
    EXPECT(r.rc == EICOS_OK && r.calls == 0, "rc %d calls %d", r.rc, r.calls);
    for (int count : {0, 2, 5}) {
        where = "idx NULL, count " + std::to_string(count);
        r = run_case(5, 2, nullptr, count, true, FIVE);
        EXPECT(r.rc == EICOS_OK && r.calls == (count == 0 ? 0 : count <= 3 ? 1 : 2), "rc %d calls %d", r.rc, r.calls);
    }
    where = "idx given in the prefix form";
    r = run_case(5, 2, l1, 3, true, FIVE);
    EXPECT(r.rc == EICOS_OK && r.calls == 2, "rc %d calls %d", r.rc, r.calls);
}

void refusals() {
    const int batch = 5;
    struct { const char *name; std::vector<int> idx; bool null_idx; int count; bool prefix_form; } cases[] = {
        {"duplicate", {4, 0, 4}, false, 3, false},      {"index -1", {0, -1}, false, 2, false},        {"index = batch", {1, 5, 2}, false, 3, false},
        {"count > batch", {0, 1, 2, 3, 4, 0}, false, 6, false}, {"NULL idx, count > 0", {}, true, 2, false},
        {"prefix form, count = batch + 1", {}, true, 6, true}, {"duplicate in the prefix form", {2, 2}, false, 2, true}};
    for (auto &c : cases) {
        where = std::string("refusal: ") + c.name;
        const int *idx = c.null_idx ? nullptr : c.idx.data();
        const Result r = run_case(batch, 2, idx, c.count, c.prefix_form, FIVE); // (compares every output with its sentinels)
        const std::string want = c.null_idx && c.prefix_form ? "who: count must lie in [0, batch] when idx is NULL (instances 0 .. count-1)"
                                                             : "who: " + index_list_fault(idx, c.count, batch);
        EXPECT(r.rc == EICOS_E_INVALID && r.calls == 0, "rc %d calls %d", r.rc, r.calls);
        EXPECT(want.size() > 5 && r.refusal == want, "got '%s', want '%s'", r.refusal.c_str(), want.c_str());
    }
}

void failing() {
    where = "shard 1 of 2 fails";
    const int list[] = {4, 0, 3, 1};
    const Result r = run_case(5, 2, list, 4, false, FIVE, 1); // (rows 0 and 2 of the outputs must keep their sentinels, rows 1 and 3 be written)
    EXPECT(r.rc == EICOS_E_INVALID && r.calls == 2, "rc %d calls %d", r.rc, r.calls);
    where = "shard 0 of 2 fails";
    const Result r0 = run_case(5, 2, list, 4, false, FIVE, 0);
    EXPECT(r0.rc == EICOS_E_INVALID && r0.calls == 2, "rc %d calls %d", r0.rc, r0.calls);
}

void rules() {
    const int list[] = {3, 1, 4};
    for (Type t : {DBL, INT, INFO})
        for (Column::Rule rule : {Column::EXACT, Column::GIVEN, Column::AT_LEAST_ONE}) {
            where = "rules, type " + std::to_string(t) + " rule " + std::to_string(rule);
            // an output of width 0 under the rule (given, and not), a given input of width 0, an input that was not given, one real output
            const std::vector<Spec> spec = {{t, 0, false, true, rule}, {t, 0, false, false, rule}, {DBL, 0, true, true, Column::GIVEN},
                                            {INT, 2, true, false, Column::GIVEN}, {t, 2, false, true, rule}};
            const Result r = run_case(5, 2, list, 3, false, spec); // (the pointer rules are checked inside the callable)
            EXPECT(r.rc == EICOS_OK && r.calls == 2, "rc %d calls %d", r.rc, r.calls);
        }
}

void sweep() {
    for (unsigned seed = 0; seed < 200; seed++) {
        std::mt19937 rng(seed);
        auto draw = [&](int lo, int hi) { return lo + (int)(rng() % (unsigned)(hi - lo + 1)); };
        const int batch = draw(1, 9), ns = draw(1, std::min(4, batch)), count = draw(0, batch);
        std::vector<int> list(batch);
        for (int i = 0; i < batch; i++) list[i] = i;
        std::shuffle(list.begin(), list.end(), rng);
        const bool prefix_form = draw(0, 4) == 0, null_idx = prefix_form && draw(0, 1) == 0;
        std::vector<Spec> spec((size_t)draw(1, 4));
        for (Spec &sp : spec) {
            sp.input = draw(0, 2) == 0;
            sp.t = (Type)draw(0, sp.input ? 1 : 2);
            sp.w = draw(0, 3);
            sp.given = draw(0, 4) != 0;
            sp.rule = sp.input ? Column::GIVEN : (Column::Rule)draw(0, 2);
        }
        const int fail_shard = draw(0, 5) == 0 ? draw(0, ns - 1) : -1;
        where = "seed " + std::to_string(seed);
        const Result r = run_case(batch, ns, null_idx ? nullptr : list.data(), count, prefix_form, spec, fail_shard);
        const bool failed = fail_shard >= 0 && std::count(r.called.begin(), r.called.end(), fail_shard) > 0;
        EXPECT(r.refusal.empty() && r.rc == (failed ? (int)EICOS_E_INVALID : (int)EICOS_OK), "rc %d '%s'", r.rc, r.refusal.c_str());
    }
}

} // namespace

int main(int argc, char **argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "layout") layout();
    else if (mode == "routing") routing();
    else if (mode == "refusals") refusals();
    else if (mode == "failing") failing();
    else if (mode == "rules") rules();
    else if (mode == "sweep") sweep();
    else { std::fprintf(stderr, "usage: shard_rows_check layout | routing | refusals | failing | rules | sweep\n"); return 2; }
    std::printf("%s: %d checks, %d failures\n", mode.c_str(), checks, failures);
    return failures ? 1 : 0;
}
