// Row routing of the multi-GPU layer (multi.cpp), free of threads, devices and HIP: where the shards lie in the batch, which shard
// serves which entry of a caller's list of global instance ids, and how one shard's share of a list-indexed call is served -- its rows
// of the inputs packed behind each other, the call, its rows of the outputs back at their positions in the caller's list.
// tests/host/shard_rows_check.cpp runs this header under the sanitizers.
#pragma once
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "internal.hpp"

#pragma GCC visibility push(hidden) // (internal to the library: not part of its exported symbols)
namespace eicos {

// Contiguous shards, the first `batch % ns` one instance longer (= eicos_amd.generate.shard_range).
inline void shard_layout(int batch, int ns, std::vector<int> &first, std::vector<int> &count) {
    const int base = batch / ns, rem = batch % ns;
    first.resize(ns); count.resize(ns);
    for (int s = 0; s < ns; s++) { first[s] = s * base + std::min(s, rem); count[s] = base + (s < rem ? 1 : 0); }
}

// A caller's list split by shard: per shard its ids, reduced by the shard's first instance, and their positions in the caller's list.
struct Shares { std::vector<std::vector<int>> ids, pos; };

// Checks the list as a whole (so that a refused list reaches no shard), then splits it over the layout `first` (ascending from 0).
// Returns what is wrong with the list behind "who: ", or nothing.  prefix_form: idx == NULL means instances 0 .. count-1.
inline std::string split_list(const std::vector<int> &first, int batch, const int *idx, int count, const char *who, bool prefix_form, Shares &sh) {
    std::vector<int> all;
    if (prefix_form && !idx) {
        if (count < 0 || count > batch) return std::string(who) + ": count must lie in [0, batch] when idx is NULL (instances 0 .. count-1)";
        all.resize((size_t)count);
        for (int q = 0; q < count; q++) all[q] = q;
        idx = all.data();
    }
    const std::string msg = index_list_fault(idx, count, batch);
    if (!msg.empty()) return std::string(who) + ": " + msg;
    sh.ids.assign(first.size(), {}); sh.pos.assign(first.size(), {});
    for (int q = 0; q < count; q++) {
        const int s = (int)(std::upper_bound(first.begin(), first.end(), idx[q]) - first.begin()) - 1;
        sh.ids[s].push_back(idx[q] - first[s]); sh.pos[s].push_back(q);
    }
    return std::string();
}

// One list-ordered array of a call: row q belongs to entry q of the caller's list.  A column that is NULL reaches the shard as NULL.
// What the shard gets where a given column has no bytes (width 0) is the column's rule:
//   EXACT         NULL
//   GIVEN         the caller's pointer: a given group stays given (the h / b rules and "no output map" look at pointers)
//   AT_LEAST_ONE  one element of scratch, so that the shard's own refusal and message come back (a handle without its maps)
struct Column {
    enum Rule { EXACT, GIVEN, AT_LEAST_ONE };
    void *ptr;
    size_t row, elem; // bytes of a row and of one element
    bool input;
    Rule rule;
};
template <class T> Column in(const T *p, int width) { return {const_cast<T *>(p), (size_t)std::max(width, 0) * sizeof(T), sizeof(T), true, Column::GIVEN}; }
template <class T> Column out(T *p, int width, Column::Rule rule = Column::EXACT) { return {p, (size_t)std::max(width, 0) * sizeof(T), sizeof(T), false, rule}; }

constexpr int MAX_COLUMNS = 8;

// Serves one shard's share (ids, pos: the shard's entries of a Shares): packs the input columns, sizes zeroed scratch for the output
// columns, hands call(ids, k, p) the per-shard pointers p[0 .. ncol) in column order and, on EICOS_OK and only then, copies every
// output row to its position in the caller's array.  An empty share is EICOS_OK without a call.
template <class F> int serve_share(const std::vector<int> &ids, const std::vector<int> &pos, const Column *cols, int ncol, F &&call) {
    const size_t k = pos.size();
    if (k == 0) return EICOS_OK;
    if (ncol > MAX_COLUMNS) return EICOS_E_INVALID;
    std::vector<char> buf[MAX_COLUMNS];
    void *p[MAX_COLUMNS];
    for (int c = 0; c < ncol; c++) {
        const Column &col = cols[c];
        size_t bytes = col.ptr ? k * col.row : 0;
        if (col.ptr && bytes == 0 && col.rule == Column::AT_LEAST_ONE) bytes = col.elem;
        if (bytes == 0) { p[c] = col.ptr && col.rule == Column::GIVEN ? col.ptr : nullptr; continue; }
        buf[c].assign(bytes, 0);
        for (size_t q = 0; col.input && q < k; q++) std::memcpy(buf[c].data() + q * col.row, (const char *)col.ptr + (size_t)pos[q] * col.row, col.row);
        p[c] = buf[c].data();
    }
    const int rc = call(ids.data(), (int)k, (void *const *)p);
    if (rc != EICOS_OK) return rc;
    for (int c = 0; c < ncol; c++) {
        const Column &col = cols[c];
        if (col.input || !col.ptr || col.row == 0) continue;
        for (size_t q = 0; q < k; q++) std::memcpy((char *)col.ptr + (size_t)pos[q] * col.row, buf[c].data() + q * col.row, col.row);
    }
    return EICOS_OK;
}
template <size_t N, class F> int serve_share(const std::vector<int> &ids, const std::vector<int> &pos, const Column (&cols)[N], F &&call) {
    static_assert(N <= (size_t)MAX_COLUMNS, "more columns than serve_share holds scratch for");
    return serve_share(ids, pos, cols, (int)N, call);
}

} // namespace eicos
#pragma GCC visibility pop
