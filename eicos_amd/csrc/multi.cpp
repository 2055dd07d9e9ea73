// Multi-GPU layer of the C ABI (include/eicos_amd.h: eicos_multi_*): one sparsity pattern, `batch` instances in contiguous
// shards over a list of devices -- one eicos_batch handle (own stream) per list entry, no data-path collective (instances are
// independent: SURVEY.md 8e).  Host C++ only: no torch, no RCCL; inputs reach a shard over its own GPU's PCIe link (host
// pointers) or by peer copies over xGMI (inputs resident on one GPU).  A device may be listed more than once: its shards then
// run concurrently on separate streams of that GPU (what a single-GPU box can exercise, tests/test_gpu_parity.py).
#include "../../include/eicos_amd.h"

#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstdio>
#include <condition_variable>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "internal.hpp"
#include "shard_rows.hpp"

namespace {
// One persistent host thread per shard: blocking calls of the shards (symbolic analysis at creation, the chunked host-pointer
// updateData, result copies) overlap across GPUs without a thread being created per call.  post() hands the worker one job, wait()
// blocks until it has run.
class Worker {
  public:
    Worker() : th_([this] { run(); }) {}
    ~Worker() {
        { std::lock_guard<std::mutex> lk(mu_); stop_ = true; }
        cv_.notify_all();
        th_.join();
    }
    void post(std::function<void()> f) { { std::lock_guard<std::mutex> lk(mu_); job_ = std::move(f); has_ = true; done_ = false; } cv_.notify_all(); }
    void wait() { std::unique_lock<std::mutex> lk(mu_); cv_.wait(lk, [&] { return done_; }); }
  private:
    void run() {
        for (;;) {
            std::function<void()> f;
            { std::unique_lock<std::mutex> lk(mu_); cv_.wait(lk, [&] { return stop_ || has_; }); if (!has_) return; f = std::move(job_); has_ = false; }
            f();
            { std::lock_guard<std::mutex> lk(mu_); done_ = true; }
            cv_.notify_all();
        }
    }
    std::mutex mu_; std::condition_variable cv_;
    std::function<void()> job_;
    bool has_ = false, done_ = true, stop_ = false;
    std::thread th_; // (last member: the thread starts after the state above is initialised)
};
} // namespace

struct eicos_multi {
    int batch = 0, n = 0, m = 0, p = 0, nnzG = 0, nnzA = 0;
    std::vector<eicos_batch *> shard;
    std::vector<int> first, count, device;
    std::vector<std::unique_ptr<Worker>> worker; // one per shard (none for a single shard: the caller's thread does the work)
    std::mutex call_mu;                          // one fan-out at a time (the workers hold one job each)
};

namespace {
thread_local std::string g_merr;
int mfail(int code, const std::string &msg) { g_merr = msg; return code; }
// run fn(s) for every shard on the shard's host thread; returns the first failing shard's code and message
template <class F> int for_shards(eicos_multi *mh, F &&fn) {
    const int ns = (int)mh->shard.size();
    std::vector<int> rc(ns, EICOS_OK);
    std::vector<std::string> msg(ns);
    auto body = [&](int s) { rc[s] = fn(s); if (rc[s] != EICOS_OK) msg[s] = eicos_last_error(); };
    if (ns == 1 || mh->worker.empty()) { for (int s = 0; s < ns; s++) body(s); }
    else {
        std::lock_guard<std::mutex> lk(mh->call_mu);
        for (int s = 0; s < ns; s++) mh->worker[s]->post([&body, s] { body(s); });
        for (int s = 0; s < ns; s++) mh->worker[s]->wait();
    }
    for (int s = 0; s < ns; s++) if (rc[s] != EICOS_OK) return mfail(rc[s], "shard " + std::to_string(s) + " (device " + std::to_string(mh->device[s]) + "): " + msg[s]);
    return EICOS_OK;
}
// shards that intersect the instance range [first, first + count): fn(s, first index inside the shard, count, offset in the caller's arrays)
template <class F> int for_range(eicos_multi *mh, int first, int count, F &&fn) {
    if (!mh) return mfail(EICOS_E_INVALID, "NULL handle");
    if (first < 0 || count < 0 || first + count > mh->batch) return mfail(EICOS_E_INVALID, "instance range out of bounds");
    return for_shards(mh, [&](int s) {
        const int a = std::max(first, mh->first[s]), b = std::min(first + count, mh->first[s] + mh->count[s]);
        if (a >= b) return (int)EICOS_OK;
        return fn(s, a - mh->first[s], b - a, (size_t)(a - first));
    });
}
// fn(s) for every shard in turn on the caller's thread (calls that only enqueue, and settings); the first failure ends the loop.
// name_shard: the shard's message behind "shard s: ", else as it is
template <class F> int in_turn(eicos_multi *mh, bool name_shard, F &&fn) {
    if (!mh) return mfail(EICOS_E_INVALID, "NULL handle");
    for (size_t s = 0; s < mh->shard.size(); s++) {
        const int rc = fn((int)s);
        if (rc != EICOS_OK) return mfail(rc, (name_shard ? "shard " + std::to_string(s) + ": " : std::string()) + eicos_last_error());
    }
    return EICOS_OK;
}
// row `row` of an array of `width` elements per row; NULL stays NULL
template <class T> T *at(T *p, size_t row, size_t width) { return p ? p + row * width : nullptr; }
} // namespace

extern "C" {

const char *eicos_multi_last_error(void) { return g_merr.c_str(); }

int eicos_multi_create(int n, int m, int p, int l, int ncones, const int *q, const int *Gjc, const int *Gir, const int *Ajc, const int *Air,
                       int batch, const int *device_ids, int ndev, eicos_multi **out) {
    if (!out) return mfail(EICOS_E_INVALID, "out is NULL");
    *out = nullptr;
    if (ndev < 1 || !device_ids) return mfail(EICOS_E_INVALID, "need at least one device id");
    if (batch < ndev) return mfail(EICOS_E_INVALID, "batch smaller than the number of shards");
    eicos_multi *mh = new eicos_multi();
    mh->batch = batch;
    mh->shard.assign(ndev, nullptr); mh->device.assign(device_ids, device_ids + ndev);
    // a negative id means "the caller's current device": resolved HERE, on the calling thread (a worker thread's current device is 0)
    {
        int cur = 0, nvis = 0;
        if (hipGetDeviceCount(&nvis) != hipSuccess || nvis == 0) {
            const int d0 = mh->device[0];
            delete mh;
            return mfail(EICOS_E_NOGPU, "shard 0 (device " + std::to_string(d0) + "): no HIP device visible: the solver has no CPU fallback");
        }
        if (hipGetDevice(&cur) != hipSuccess) cur = 0;
        for (int &d : mh->device) { if (d < 0) d = cur; if (d >= nvis) { delete mh; return mfail(EICOS_E_INVALID, "device index out of range (" + std::to_string(nvis) + " visible)"); } }
    }
    if (ndev > 1) for (int s = 0; s < ndev; s++) mh->worker.emplace_back(new Worker());
    eicos::shard_layout(batch, ndev, mh->first, mh->count);
    // every shard analyses the pattern and sets up its device on its own host thread (the analysis is deterministic: identical plans)
    const int rc = for_shards(mh, [&](int s) {
        return eicos_batch_create(n, m, p, l, ncones, q, Gjc, Gir, Ajc, Air, mh->count[s], mh->device[s], &mh->shard[s]);
    });
    if (rc != EICOS_OK) { const std::string keep = g_merr; eicos_multi_destroy(mh); g_merr = keep; return rc; }
    eicos_dims d;
    eicos_batch_dims(mh->shard[0], &d);
    mh->n = d.n; mh->m = d.m; mh->p = d.p; mh->nnzG = d.nnzG; mh->nnzA = d.nnzA;
    // Peer access between every pair of distinct devices of the list, both directions: eicos_multi_update_device then reads inputs that
    // live on one GPU in place over xGMI.  A pair without it (or a failure to enable it) falls back to staged peer copies -- noted once.
    int caller_dev = 0;
    if (hipGetDevice(&caller_dev) != hipSuccess) caller_dev = 0;
    for (int a = 0; a < ndev; a++)
        for (int b = 0; b < ndev; b++) {
            const int da = mh->device[a], db = mh->device[b];
            if (da == db) continue;
            int can = 0;
            if (hipDeviceCanAccessPeer(&can, da, db) != hipSuccess) { (void)hipGetLastError(); can = 0; }
            hipError_t e = hipErrorUnknown;
            if (can && hipSetDevice(da) == hipSuccess) e = hipDeviceEnablePeerAccess(db, 0);
            (void)hipGetLastError();
            if (!can || (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled)) {
                static bool noted = false;
                if (!noted) { noted = true; std::fprintf(stderr, "[eicos_amd] no peer access from device %d to device %d: eicos_multi_update_device will stage peer copies\n", da, db); }
            }
        }
    (void)hipSetDevice(caller_dev); // (enabling peer access switched devices: the caller's current device is restored)
    *out = mh;
    return EICOS_OK;
}

int eicos_multi_destroy(eicos_multi *mh) {
    if (!mh) return EICOS_OK;
    for (eicos_batch *h : mh->shard) eicos_batch_destroy(h);
    delete mh;
    return EICOS_OK;
}

int eicos_multi_num_shards(eicos_multi *mh) { return mh ? (int)mh->shard.size() : mfail(EICOS_E_INVALID, "NULL handle"); }

int eicos_multi_shard(eicos_multi *mh, int s, eicos_batch **handle, int *first, int *count, int *device) {
    if (!mh || s < 0 || s >= (int)mh->shard.size()) return mfail(EICOS_E_INVALID, "bad shard index");
    if (handle) *handle = mh->shard[s];
    if (first) *first = mh->first[s];
    if (count) *count = mh->count[s];
    if (device) *device = mh->device[s];
    return EICOS_OK;
}

int eicos_multi_update(eicos_multi *mh, int first, int count, const double *Gpr, const double *Apr, const double *c, const double *h, const double *b) {
    return for_range(mh, first, count, [&](int s, int f, int cnt, size_t off) {
        return eicos_batch_update(mh->shard[s], f, cnt, at(Gpr, off, mh->nnzG), at(Apr, off, mh->nnzA), at(c, off, mh->n), at(h, off, mh->m), at(b, off, mh->p));
    });
}

int eicos_multi_update_device(eicos_multi *mh, int src_device, int first, int count, const double *dGpr, const double *dApr, const double *dc,
                              const double *dh, const double *db) {
    if (src_device < 0) return mfail(EICOS_E_INVALID, "src_device must name the GPU that holds the inputs");
    return for_range(mh, first, count, [&](int s, int f, int cnt, size_t off) {
        const double *G = at(dGpr, off, mh->nnzG), *A = at(dApr, off, mh->nnzA), *cc = at(dc, off, mh->n), *hh = at(dh, off, mh->m), *bb = at(db, off, mh->p);
        // (experiment knob, honoured like the others only under EICOS_EXPERIMENT=1 and read on EVERY call: take the other-GPU path even on
        // the source GPU, so that a single-GPU box exercises it; eicos_batch_last_update_path tells which path a shard took)
        const char *e_ = std::getenv("EICOS_EXPERIMENT"), *k_ = std::getenv("EICOS_MULTI_FORCE_PEER");
        const bool force_peer = e_ && !std::strcmp(e_, "1") && k_ && !std::strcmp(k_, "1");
        if (mh->device[s] == src_device && !force_peer) return eicos_batch_update_device(mh->shard[s], f, cnt, G, A, cc, hh, bb); // already in this GPU's HBM: no copy
        return eicos_internal_update_staged(mh->shard[s], f, cnt, G, A, cc, hh, bb, src_device, 0);               // peer copies (xGMI), then the same kernel
    });
}

int eicos_multi_update_rhs(eicos_multi *mh, int first, int count, const double *c, const double *h, const double *b) {
    return for_range(mh, first, count, [&](int s, int f, int cnt, size_t off) {
        return eicos_batch_update_rhs(mh->shard[s], f, cnt, at(c, off, mh->n), at(h, off, mh->m), at(b, off, mh->p));
    });
}

int eicos_multi_update_rhs_device(eicos_multi *mh, int src_device, int first, int count, const double *dc, const double *dh, const double *db) {
    if (src_device < 0) return mfail(EICOS_E_INVALID, "src_device must name the GPU that holds the inputs");
    return for_range(mh, first, count, [&](int s, int f, int cnt, size_t off) {
        const double *cc = at(dc, off, mh->n), *hh = at(dh, off, mh->m), *bb = at(db, off, mh->p);
        if (mh->device[s] == src_device) return eicos_batch_update_rhs_device(mh->shard[s], f, cnt, cc, hh, bb);
        return eicos_internal_update_staged(mh->shard[s], f, cnt, nullptr, nullptr, cc, hh, bb, src_device, 1);
    });
}

int eicos_multi_set_param_map(eicos_multi *mh, int k, const eicos_affine_map *c, const eicos_affine_map *h, const eicos_affine_map *b) {
    if (!mh) return mfail(EICOS_E_INVALID, "NULL handle");
    return for_shards(mh, [&](int s) { return eicos_batch_set_param_map(mh->shard[s], k, c, h, b); });
}

int eicos_multi_param_count(eicos_multi *mh) { return mh ? eicos_batch_param_count(mh->shard[0]) : mfail(EICOS_E_INVALID, "NULL handle"); }

int eicos_multi_update_param(eicos_multi *mh, int first, int count, const double *theta) {
    if (!mh) return mfail(EICOS_E_INVALID, "NULL handle");
    const int k = eicos_batch_param_count(mh->shard[0]); // (0: every shard refuses, "no parameter map")
    return for_range(mh, first, count, [&](int s, int f, int cnt, size_t off) {
        return eicos_batch_update_param(mh->shard[s], f, cnt, at(theta, off, k));
    });
}

int eicos_multi_update_param_device(eicos_multi *mh, int src_device, int first, int count, const double *dtheta) {
    if (!mh) return mfail(EICOS_E_INVALID, "NULL handle");
    if (src_device < 0) return mfail(EICOS_E_INVALID, "src_device must name the GPU that holds the inputs");
    const int k = eicos_batch_param_count(mh->shard[0]);
    return for_range(mh, first, count, [&](int s, int f, int cnt, size_t off) {
        if (mh->device[s] == src_device) return eicos_batch_update_param_device(mh->shard[s], f, cnt, at(dtheta, off, k));
        return eicos_internal_update_param_staged(mh->shard[s], f, cnt, at(dtheta, off, k), src_device);
    });
}

int eicos_multi_set_output_map(eicos_multi *mh, int r, const eicos_affine_map *u) {
    if (!mh) return mfail(EICOS_E_INVALID, "NULL handle");
    return for_shards(mh, [&](int s) { return eicos_batch_set_output_map(mh->shard[s], r, u); });
}

int eicos_multi_output_count(eicos_multi *mh) { return mh ? eicos_batch_output_count(mh->shard[0]) : mfail(EICOS_E_INVALID, "NULL handle"); }

int eicos_multi_outputs(eicos_multi *mh, int first, int count, double *u) {
    if (!mh) return mfail(EICOS_E_INVALID, "NULL handle");
    const int r = eicos_batch_output_count(mh->shard[0]); // (0: every shard refuses, "no output map")
    return for_range(mh, first, count, [&](int s, int f, int cnt, size_t off) { return eicos_batch_outputs(mh->shard[s], f, cnt, at(u, off, r)); });
}

// enqueue only: every shard's kernels start on its own stream, the call returns at once
int eicos_multi_solve_async(eicos_multi *mh) { return in_turn(mh, true, [&](int s) { return eicos_batch_solve_async(mh->shard[s]); }); }

int eicos_multi_sync(eicos_multi *mh) { return in_turn(mh, true, [&](int s) { return eicos_batch_sync(mh->shard[s]); }); }

int eicos_multi_info(eicos_multi *mh, eicos_info *info) {
    if (!mh || !info) return mfail(EICOS_E_INVALID, "NULL argument");
    return for_shards(mh, [&](int s) { return eicos_batch_info(mh->shard[s], info + mh->first[s]); });
}

int eicos_multi_solve(eicos_multi *mh, int *exitcodes) {
    int rc = eicos_multi_solve_async(mh);
    if (rc == EICOS_OK) rc = eicos_multi_sync(mh);
    if (rc != EICOS_OK || !exitcodes) return rc;
    std::vector<eicos_info> info(mh->batch);
    rc = eicos_multi_info(mh, info.data());
    if (rc != EICOS_OK) return rc;
    for (int i = 0; i < mh->batch; i++) exitcodes[i] = info[i].exitcode;
    return EICOS_OK;
}

} // extern "C"

// ---- Calls that take a list of GLOBAL instance ids with host arrays in list order (the eicos_batch_* namesake per shard).  Each is its
// argument checks, a table of its list-ordered arrays (eicos::Column) and the namesake call; the routing is shard_rows.hpp's.  The list
// is checked as a whole before any shard sees its share, so a refused call changes no shard; shards with an empty share are skipped; a
// failing shard's rows of the caller's outputs stay as they were.
namespace {
using eicos::Column;
using eicos::Shares;
using eicos::in;
using eicos::out;
// prefix_form: idx == NULL means instances 0 .. count-1 (the adjoint family)
int split(eicos_multi *mh, const int *idx, int count, const char *who, Shares &sh, bool prefix_form = false) {
    if (!mh) return mfail(EICOS_E_INVALID, "NULL handle");
    const std::string msg = eicos::split_list(mh->first, mh->batch, idx, count, who, prefix_form, sh);
    return msg.empty() ? (int)EICOS_OK : mfail(EICOS_E_INVALID, msg);
}
// every shard serves its share on its host thread: call(s, ids, k, p) with the shard's ids and the per-shard pointers, in column order
template <size_t N, class F> int route(eicos_multi *mh, const Shares &sh, const Column (&cols)[N], F &&call) {
    return for_shards(mh, [&](int s) {
        return eicos::serve_share(sh.ids[s], sh.pos[s], cols, [&](const int *ids, int k, void *const *p) { return call(s, ids, k, p); });
    });
}
// ... but a handle of ONE shard hands the caller's list and arrays on as they are: pinned arrays stay pinned, so the step over a subset
// keeps its one-launch path (the five indexed updates and reads and the subset step)
template <size_t N, class F> int route_or_pass(eicos_multi *mh, const Shares &sh, const int *idx, int count, const Column (&cols)[N], F &&call) {
    if (mh->shard.size() != 1) return route(mh, sh, cols, call);
    void *p[N];
    for (size_t c = 0; c < N; c++) p[c] = cols[c].ptr;
    return for_shards(mh, [&](int) { return call(0, idx, count, (void *const *)p); });
}
double *D(void *p) { return static_cast<double *>(p); }
int *I(void *p) { return static_cast<int *>(p); }
// the widths the maps give (0 without the map: the shard refuses)
int param_k(eicos_multi *mh) { return std::max(0, eicos_batch_param_count(mh->shard[0])); }
int output_r(eicos_multi *mh) { return std::max(0, eicos_batch_output_count(mh->shard[0])); }
// k of the contracted forms: the parameter map's, or -- without one -- the one the matrix map was installed for
int contracted_k(eicos_multi *mh) { return param_k(mh) ? param_k(mh) : std::max(0, eicos_batch_matrix_map_count(mh->shard[0])); }
// the refusals of the adjoint family behind the list's, in this order: nrhs, a NULL g, a NULL J / grad_theta
int check_nrhs(const char *who, int nrhs) {
    if (nrhs >= 1 && nrhs <= EICOS_ADJOINT_MAX_RHS) return EICOS_OK;
    return mfail(EICOS_E_INVALID, std::string(who) + ": nrhs must lie in [1, " + std::to_string(EICOS_ADJOINT_MAX_RHS) + "], got " + std::to_string(nrhs));
}
int check_given(const char *who, const char *name, const void *p, bool needed) {
    return p || !needed ? (int)EICOS_OK : mfail(EICOS_E_INVALID, std::string(who) + ": " + name + " is NULL");
}
int check_g(eicos_multi *mh, const char *who, int nrhs, const double *g, int count) {
    const int rc = check_nrhs(who, nrhs);
    return rc != EICOS_OK ? rc : check_given(who, "g", g, count > 0 && mh->n > 0);
}
int check_mask(eicos_multi *mh, unsigned mask, const char *who) {
    if (!mh) return mfail(EICOS_E_INVALID, "NULL handle");
    const std::string msg = eicos::class_mask_fault(mask);
    return msg.empty() ? (int)EICOS_OK : mfail(EICOS_E_INVALID, std::string(who) + ": " + msg);
}
// per shard: the ids a mask call selected (local) and their exit codes; concatenated in shard order they are the ascending global list
int concat_selected(eicos_multi *mh, const std::vector<std::vector<int>> &ids, const std::vector<int> &cnt, const std::vector<std::vector<int>> *codes,
                    int *idx_out, int *count_out, int *exitcodes) {
    int at = 0;
    for (size_t s = 0; s < mh->shard.size(); s++)
        for (int q = 0; q < cnt[s]; q++, at++) {
            if (idx_out) idx_out[at] = ids[s][q] + mh->first[s];
            if (exitcodes && codes) exitcodes[at] = (*codes)[s][q];
        }
    if (count_out) *count_out = at;
    return EICOS_OK;
}
} // namespace

extern "C" {

int eicos_multi_select(eicos_multi *mh, unsigned mask, int *idx_out, int *count_out) {
    int rc = check_mask(mh, mask, "eicos_multi_select");
    if (rc != EICOS_OK) return rc;
    const size_t ns = mh->shard.size();
    std::vector<std::vector<int>> ids(ns);
    std::vector<int> cnt(ns, 0);
    rc = for_shards(mh, [&](int s) { ids[s].resize(mh->count[s]); return eicos_batch_select(mh->shard[s], mask, ids[s].data(), &cnt[s]); });
    return rc != EICOS_OK ? rc : concat_selected(mh, ids, cnt, nullptr, idx_out, count_out, nullptr);
}

int eicos_multi_solve_subset_async(eicos_multi *mh, const int *idx, int count) {
    Shares sh;
    const int rc = split(mh, idx, count, "eicos_multi_solve_subset", sh);
    if (rc != EICOS_OK) return rc;
    return in_turn(mh, true, [&](int s) { // enqueue only, as eicos_multi_solve_async
        return sh.ids[s].empty() ? (int)EICOS_OK : eicos_batch_solve_subset_async(mh->shard[s], sh.ids[s].data(), (int)sh.ids[s].size());
    });
}

int eicos_multi_solve_subset(eicos_multi *mh, const int *idx, int count, int *exitcodes) {
    Shares sh;
    const int rc = split(mh, idx, count, "eicos_multi_solve_subset", sh);
    if (rc != EICOS_OK) return rc;
    const Column cols[] = {out(exitcodes, 1)};
    return route(mh, sh, cols, [&](int s, const int *ids, int k, void *const *p) { return eicos_batch_solve_subset(mh->shard[s], ids, k, I(p[0])); });
}

int eicos_multi_solve_where(eicos_multi *mh, unsigned mask, int *idx_out, int *count_out, int *exitcodes) {
    int rc = check_mask(mh, mask, "eicos_multi_solve_where");
    if (rc != EICOS_OK) return rc;
    const size_t ns = mh->shard.size();
    std::vector<std::vector<int>> ids(ns), codes(ns);
    std::vector<int> cnt(ns, 0);
    rc = for_shards(mh, [&](int s) {
        ids[s].resize(mh->count[s]); codes[s].resize(mh->count[s]);
        return eicos_batch_solve_where(mh->shard[s], mask, ids[s].data(), &cnt[s], codes[s].data());
    });
    return rc != EICOS_OK ? rc : concat_selected(mh, ids, cnt, &codes, idx_out, count_out, exitcodes);
}

// (a column of width 0 -- n, p or m = 0 -- copies nothing and reaches the shard as NULL)
int eicos_multi_gather(eicos_multi *mh, const int *idx, int count, double *x, double *y, double *z, double *sl, eicos_info *info) {
    Shares sh;
    const int rc = split(mh, idx, count, "eicos_multi_gather", sh);
    if (rc != EICOS_OK) return rc;
    const Column cols[] = {out(x, mh->n), out(y, mh->p), out(z, mh->m), out(sl, mh->m), out(info, 1)};
    return route(mh, sh, cols, [&](int s, const int *ids, int k, void *const *p) {
        return eicos_batch_gather(mh->shard[s], ids, k, D(p[0]), D(p[1]), D(p[2]), D(p[3]), static_cast<eicos_info *>(p[4]));
    });
}

// Index-list updates, output rows and the closed-loop step over a subset.  An input group the caller gave stays given for the shard
// even where its width is 0 (eicos::in); so does u, so that a handle without its output map refuses with its own words.
int eicos_multi_update_indexed(eicos_multi *mh, const int *idx, int count, const double *G, const double *A, const double *c, const double *hh,
                               const double *b) {
    Shares sh;
    const int rc = split(mh, idx, count, "eicos_multi_update_indexed", sh);
    if (rc != EICOS_OK) return rc;
    const Column cols[] = {in(G, mh->nnzG), in(A, mh->nnzA), in(c, mh->n), in(hh, mh->m), in(b, mh->p)};
    return route_or_pass(mh, sh, idx, count, cols, [&](int s, const int *ids, int k, void *const *p) {
        return eicos_batch_update_indexed(mh->shard[s], ids, k, D(p[0]), D(p[1]), D(p[2]), D(p[3]), D(p[4]));
    });
}

int eicos_multi_update_rhs_indexed(eicos_multi *mh, const int *idx, int count, const double *c, const double *hh, const double *b) {
    Shares sh;
    const int rc = split(mh, idx, count, "eicos_multi_update_rhs_indexed", sh);
    if (rc != EICOS_OK) return rc;
    const Column cols[] = {in(c, mh->n), in(hh, mh->m), in(b, mh->p)};
    return route_or_pass(mh, sh, idx, count, cols, [&](int s, const int *ids, int k, void *const *p) {
        return eicos_batch_update_rhs_indexed(mh->shard[s], ids, k, D(p[0]), D(p[1]), D(p[2]));
    });
}

int eicos_multi_update_param_indexed(eicos_multi *mh, const int *idx, int count, const double *theta) {
    Shares sh;
    const int rc = split(mh, idx, count, "eicos_multi_update_param_indexed", sh);
    if (rc != EICOS_OK) return rc;
    const Column cols[] = {in(theta, param_k(mh))};
    return route_or_pass(mh, sh, idx, count, cols, [&](int s, const int *ids, int k, void *const *p) {
        return eicos_batch_update_param_indexed(mh->shard[s], ids, k, D(p[0]));
    });
}

int eicos_multi_set_iterate_indexed(eicos_multi *mh, const int *idx, int count, const double *x, const double *y, const double *z, const double *sl) {
    Shares sh;
    const int rc = split(mh, idx, count, "eicos_multi_set_iterate_indexed", sh);
    if (rc != EICOS_OK) return rc;
    const Column cols[] = {in(x, mh->n), in(y, mh->p), in(z, mh->m), in(sl, mh->m)};
    return route_or_pass(mh, sh, idx, count, cols, [&](int s, const int *ids, int k, void *const *p) {
        return eicos_batch_set_iterate_indexed(mh->shard[s], ids, k, D(p[0]), D(p[1]), D(p[2]), D(p[3]));
    });
}

int eicos_multi_outputs_indexed(eicos_multi *mh, const int *idx, int count, double *u) {
    Shares sh;
    const int rc = split(mh, idx, count, "eicos_multi_outputs_indexed", sh);
    if (rc != EICOS_OK) return rc;
    const Column cols[] = {out(u, output_r(mh), Column::GIVEN)};
    return route_or_pass(mh, sh, idx, count, cols, [&](int s, const int *ids, int k, void *const *p) {
        return eicos_batch_outputs_indexed(mh->shard[s], ids, k, D(p[0]));
    });
}

// (x_out with n = 0 reaches the shard as NULL)
int eicos_multi_update_param_solve_subset(eicos_multi *mh, const int *idx, int count, const double *theta, double *u_out, double *x_out,
                                          int *exitcodes) {
    Shares sh;
    const int rc = split(mh, idx, count, "eicos_multi_update_param_solve_subset", sh);
    if (rc != EICOS_OK) return rc;
    const Column cols[] = {in(theta, param_k(mh)), out(u_out, output_r(mh), Column::GIVEN), out(x_out, mh->n), out(exitcodes, 1)};
    return route_or_pass(mh, sh, idx, count, cols, [&](int s, const int *ids, int k, void *const *p) {
        return eicos_batch_update_param_solve_subset(mh->shard[s], ids, k, D(p[0]), D(p[1]), D(p[2]), I(p[3]));
    });
}

// Adjoint sensitivities (eicos_batch_adjoint / _output_jacobian / _adjoint_data / _param_jacobian / _param_gradient per shard); idx ==
// NULL: instances 0 .. count-1.  The calls change no state, so a shard's refusal (no maps, a matrix map, nrhs) leaves nothing behind
// either.  They pack on a handle of one shard too.  J, its res and grad_theta are AT_LEAST_ONE: a handle without its maps gives them
// width 0, and the shard's own refusal and message come back.
int eicos_multi_adjoint(eicos_multi *mh, const int *idx, int count, int nrhs, const double *g, double *grad_c, double *grad_h, double *grad_b,
                        double *res) {
    const char *who = "eicos_multi_adjoint";
    Shares sh;
    int rc = split(mh, idx, count, who, sh, true);
    if (rc == EICOS_OK) rc = check_g(mh, who, nrhs, g, count);
    if (rc != EICOS_OK) return rc;
    const Column cols[] = {in(g, nrhs * mh->n), out(grad_c, nrhs * mh->n), out(grad_h, nrhs * mh->m), out(grad_b, nrhs * mh->p), out(res, nrhs)};
    return route(mh, sh, cols, [&](int s, const int *ids, int k, void *const *p) {
        return eicos_batch_adjoint(mh->shard[s], ids, k, nrhs, D(p[0]), D(p[1]), D(p[2]), D(p[3]), D(p[4]));
    });
}

int eicos_multi_adjoint_data(eicos_multi *mh, const int *idx, int count, int nrhs, const double *g, double *grad_c, double *grad_h, double *grad_b,
                             double *grad_G, double *grad_A, double *res) {
    const char *who = "eicos_multi_adjoint_data";
    Shares sh;
    int rc = split(mh, idx, count, who, sh, true);
    if (rc == EICOS_OK) rc = check_g(mh, who, nrhs, g, count);
    if (rc != EICOS_OK) return rc;
    const Column cols[] = {in(g, nrhs * mh->n), out(grad_c, nrhs * mh->n), out(grad_h, nrhs * mh->m), out(grad_b, nrhs * mh->p),
                           out(grad_G, nrhs * mh->nnzG), out(grad_A, nrhs * mh->nnzA), out(res, nrhs)};
    return route(mh, sh, cols, [&](int s, const int *ids, int k, void *const *p) {
        return eicos_batch_adjoint_data(mh->shard[s], ids, k, nrhs, D(p[0]), D(p[1]), D(p[2]), D(p[3]), D(p[4]), D(p[5]), D(p[6]));
    });
}

int eicos_multi_output_jacobian(eicos_multi *mh, const int *idx, int count, double *J, double *res) {
    const char *who = "eicos_multi_output_jacobian";
    Shares sh;
    int rc = split(mh, idx, count, who, sh, true);
    if (rc == EICOS_OK) rc = check_given(who, "J", J, count > 0);
    if (rc != EICOS_OK) return rc;
    const int r = output_r(mh);
    const Column cols[] = {out(J, r * param_k(mh), Column::AT_LEAST_ONE), out(res, r, Column::AT_LEAST_ONE)};
    return route(mh, sh, cols, [&](int s, const int *ids, int k, void *const *p) { return eicos_batch_output_jacobian(mh->shard[s], ids, k, D(p[0]), D(p[1])); });
}

int eicos_multi_param_jacobian(eicos_multi *mh, const int *idx, int count, double *J, double *res) {
    const char *who = "eicos_multi_param_jacobian";
    Shares sh;
    int rc = split(mh, idx, count, who, sh, true);
    if (rc == EICOS_OK) rc = check_given(who, "J", J, count > 0);
    if (rc != EICOS_OK) return rc;
    const int r = output_r(mh);
    const Column cols[] = {out(J, r * contracted_k(mh), Column::AT_LEAST_ONE), out(res, r, Column::AT_LEAST_ONE)};
    return route(mh, sh, cols, [&](int s, const int *ids, int k, void *const *p) { return eicos_batch_param_jacobian(mh->shard[s], ids, k, D(p[0]), D(p[1])); });
}

int eicos_multi_param_gradient(eicos_multi *mh, const int *idx, int count, int nrhs, const double *g, double *grad_theta, double *res) {
    const char *who = "eicos_multi_param_gradient";
    Shares sh;
    int rc = split(mh, idx, count, who, sh, true);
    if (rc == EICOS_OK) rc = check_g(mh, who, nrhs, g, count);
    if (rc == EICOS_OK) rc = check_given(who, "grad_theta", grad_theta, count > 0);
    if (rc != EICOS_OK) return rc;
    const Column cols[] = {in(g, nrhs * mh->n), out(grad_theta, nrhs * contracted_k(mh), Column::AT_LEAST_ONE), out(res, nrhs)};
    return route(mh, sh, cols, [&](int s, const int *ids, int k, void *const *p) {
        return eicos_batch_param_gradient(mh->shard[s], ids, k, nrhs, D(p[0]), D(p[1]), D(p[2]));
    });
}

// updateData + solve in one call over every shard (eicos_batch_update_solve per shard on its rows, the shards concurrently)
int eicos_multi_update_solve(eicos_multi *mh, const double *G, const double *A, const double *c, const double *hh, const double *b,
                             double *x_out, int *exitcodes) {
    if (!mh) return mfail(EICOS_E_INVALID, "NULL handle");
    return for_shards(mh, [&](int s) {
        const size_t r = (size_t)mh->first[s];
        return eicos_batch_update_solve(mh->shard[s], at(G, r, mh->nnzG), at(A, r, mh->nnzA), at(c, r, mh->n), at(hh, r, mh->m), at(b, r, mh->p),
                                        at(x_out, r, mh->n), at(exitcodes, r, 1));
    });
}

int eicos_multi_update_rhs_solve(eicos_multi *mh, const double *c, const double *hh, const double *b, double *x_out, int *exitcodes) {
    if (!mh) return mfail(EICOS_E_INVALID, "NULL handle");
    return for_shards(mh, [&](int s) {
        const size_t r = (size_t)mh->first[s];
        return eicos_batch_update_rhs_solve(mh->shard[s], at(c, r, mh->n), at(hh, r, mh->m), at(b, r, mh->p), at(x_out, r, mh->n), at(exitcodes, r, 1));
    });
}

// the closed-loop step over every shard (eicos_batch_update_param_solve per shard on its rows of theta, u_out and x_out, the shards concurrently)
int eicos_multi_update_param_solve(eicos_multi *mh, const double *theta, double *u_out, double *x_out, int *exitcodes) {
    if (!mh) return mfail(EICOS_E_INVALID, "NULL handle");
    const int k = eicos_batch_param_count(mh->shard[0]), ro = eicos_batch_output_count(mh->shard[0]);
    return for_shards(mh, [&](int s) {
        const size_t r = (size_t)mh->first[s];
        return eicos_batch_update_param_solve(mh->shard[s], at(theta, r, k), at(u_out, r, ro), at(x_out, r, mh->n), at(exitcodes, r, 1));
    });
}

// plant map and rollout over every shard (eicos_batch_rollout per shard on its rows, the shards concurrently): with [batch][steps][...]
// arrays the rows of a shard are contiguous, so every shard gets plain offsets into the caller's arrays
int eicos_multi_set_plant_map(eicos_multi *mh, const eicos_affine_map *f) {
    if (!mh) return mfail(EICOS_E_INVALID, "NULL handle");
    return for_shards(mh, [&](int s) { return eicos_batch_set_plant_map(mh->shard[s], f); });
}

int eicos_multi_set_matrix_map(eicos_multi *mh, const eicos_affine_map *G, const eicos_affine_map *A) {
    if (!mh) return mfail(EICOS_E_INVALID, "NULL handle");
    return for_shards(mh, [&](int s) { return eicos_batch_set_matrix_map(mh->shard[s], G, A); });
}
int eicos_multi_matrix_map_count(eicos_multi *mh) { return mh ? eicos_batch_matrix_map_count(mh->shard[0]) : mfail(EICOS_E_INVALID, "NULL handle"); }
int eicos_multi_has_matrix_map(eicos_multi *mh) { return mh ? eicos_batch_has_matrix_map(mh->shard[0]) : mfail(EICOS_E_INVALID, "NULL handle"); }

int eicos_multi_set_shift_map(eicos_multi *mh, const eicos_affine_map *x, const eicos_affine_map *y, const eicos_affine_map *z, const eicos_affine_map *s) {
    if (!mh) return mfail(EICOS_E_INVALID, "NULL handle");
    return for_shards(mh, [&](int sh) { return eicos_batch_set_shift_map(mh->shard[sh], x, y, z, s); });
}
int eicos_multi_has_shift_map(eicos_multi *mh) { return mh ? eicos_batch_has_shift_map(mh->shard[0]) : mfail(EICOS_E_INVALID, "NULL handle"); }

// rows in global instance order: every shard takes its own
int eicos_multi_set_iterate(eicos_multi *mh, int first, int count, const double *x, const double *y, const double *z, const double *s) {
    return for_range(mh, first, count, [&](int sh, int f, int cnt, size_t off) {
        return eicos_batch_set_iterate(mh->shard[sh], f, cnt, at(x, off, mh->n), at(y, off, mh->p), at(z, off, mh->m), at(s, off, mh->m));
    });
}

int eicos_multi_has_plant_map(eicos_multi *mh) { return mh ? eicos_batch_has_plant_map(mh->shard[0]) : mfail(EICOS_E_INVALID, "NULL handle"); }

int eicos_multi_rollout(eicos_multi *mh, int steps, const double *theta0, const double *w, double *u_traj, double *theta_traj,
                        int *exitcodes, int *iters) {
    if (!mh) return mfail(EICOS_E_INVALID, "NULL handle");
    if (steps < 1) return mfail(EICOS_E_INVALID, "rollout: steps must be at least 1");
    const size_t k = (size_t)eicos_batch_param_count(mh->shard[0]), ro = (size_t)eicos_batch_output_count(mh->shard[0]), T = (size_t)steps;
    return for_shards(mh, [&](int s) {
        const size_t f = (size_t)mh->first[s];
        return eicos_batch_rollout(mh->shard[s], steps, at(theta0, f, k), at(w, f, T * k), at(u_traj, f, T * ro), at(theta_traj, f, (T + 1) * k),
                                   at(exitcodes, f, T), at(iters, f, T));
    });
}

// the rollout that records its Jacobians, and the gradient over it: rows by shard, as eicos_multi_rollout's
int eicos_multi_rollout_jacobian(eicos_multi *mh, int steps, const double *theta0, const double *w, double *u_traj, double *theta_traj,
                                 int *exitcodes, int *iters, double *J_traj, double *res_traj) {
    if (!mh) return mfail(EICOS_E_INVALID, "NULL handle");
    if (steps < 1) return mfail(EICOS_E_INVALID, "rollout: steps must be at least 1");
    if (!J_traj) return mfail(EICOS_E_INVALID, "rollout_jacobian: J_traj is NULL");
    const size_t k = (size_t)eicos_batch_param_count(mh->shard[0]), ro = (size_t)eicos_batch_output_count(mh->shard[0]), T = (size_t)steps;
    return for_shards(mh, [&](int s) {
        const size_t f = (size_t)mh->first[s];
        return eicos_batch_rollout_jacobian(mh->shard[s], steps, at(theta0, f, k), at(w, f, T * k), at(u_traj, f, T * ro), at(theta_traj, f, (T + 1) * k),
                                            at(exitcodes, f, T), at(iters, f, T), at(J_traj, f, T * ro * k), at(res_traj, f, T * ro));
    });
}
// (T = the step count of the trajectory the shards hold: every shard ran the same eicos_multi_rollout_jacobian)
int eicos_multi_rollout_gradient(eicos_multi *mh, const double *gu, const double *gtheta, double *grad_theta0, double *grad_w) {
    if (!mh) return mfail(EICOS_E_INVALID, "NULL handle");
    if (!gu && !gtheta) return mfail(EICOS_E_INVALID, "rollout_gradient: gu and gtheta are both NULL");
    if (!grad_theta0) return mfail(EICOS_E_INVALID, "rollout_gradient: grad_theta0 is NULL");
    const int steps = eicos_batch_rollout_jacobian_steps(mh->shard[0]);
    for (int s = 0; s < (int)mh->shard.size(); s++)
        if (steps < 1 || eicos_batch_rollout_jacobian_steps(mh->shard[s]) != steps)
            return mfail(EICOS_E_INVALID, "rollout_gradient: shard " + std::to_string(s) + " holds no Jacobian trajectory, or one of another length (eicos_multi_rollout_jacobian records one)");
    const size_t k = (size_t)eicos_batch_param_count(mh->shard[0]), ro = (size_t)eicos_batch_output_count(mh->shard[0]), T = (size_t)steps;
    return for_shards(mh, [&](int s) {
        const size_t f = (size_t)mh->first[s];
        return eicos_batch_rollout_gradient(mh->shard[s], at(gu, f, T * ro), at(gtheta, f, (T + 1) * k), at(grad_theta0, f, k), at(grad_w, f, T * k));
    });
}

// per-instance plant values: rows by global instance id, every shard takes the part of the range it owns.  The row widths are those of
// the plant map shard 0 holds (eicos_internal_plant_dims: the k it was installed for and its stored entries)
namespace {
void plant_dims(eicos_multi *mh, size_t &k, size_t &nnz) {
    int k_ = 0, nnz_ = 0;
    (void)eicos_internal_plant_dims(mh->shard[0], &k_, &nnz_);
    k = (size_t)k_; nnz = (size_t)nnz_;
}
} // namespace
int eicos_multi_set_plant_values(eicos_multi *mh, int first, int count, const double *f0, const double *val) {
    if (!mh) return mfail(EICOS_E_INVALID, "NULL handle");
    if (!eicos_batch_has_plant_map(mh->shard[0])) return mfail(EICOS_E_INVALID, "set_plant_values: no plant map (eicos_multi_set_plant_map installs one)");
    if (!f0 && !val) return mfail(EICOS_E_INVALID, "set_plant_values: f0 and val are both NULL");
    size_t k, nnz;
    plant_dims(mh, k, nnz);
    const int rc = for_range(mh, first, count, [&](int s, int f, int cnt, size_t off) {
        return eicos_batch_set_plant_values(mh->shard[s], f, cnt, at(f0, off, k), at(val, off, nnz));
    });
    if (rc != EICOS_OK) return rc;
    // the shards the range missed hold the group too, filled with the shared values: every shard answers has_plant_values alike
    return for_shards(mh, [&](int s) { return eicos_batch_set_plant_values(mh->shard[s], 0, 0, f0, val); });
}
int eicos_multi_plant_values(eicos_multi *mh, int first, int count, double *f0_out, double *val_out) {
    if (!mh) return mfail(EICOS_E_INVALID, "NULL handle");
    if (!eicos_batch_has_plant_map(mh->shard[0])) return mfail(EICOS_E_INVALID, "plant_values: no plant map (eicos_multi_set_plant_map installs one)");
    if (!f0_out && !val_out) return mfail(EICOS_E_INVALID, "plant_values: f0_out and val_out are both NULL");
    size_t k, nnz;
    plant_dims(mh, k, nnz);
    return for_range(mh, first, count, [&](int s, int f, int cnt, size_t off) {
        return eicos_batch_plant_values(mh->shard[s], f, cnt, at(f0_out, off, k), at(val_out, off, nnz));
    });
}
int eicos_multi_has_plant_values(eicos_multi *mh) { return mh ? eicos_batch_has_plant_values(mh->shard[0]) : mfail(EICOS_E_INVALID, "NULL handle"); }
int eicos_multi_clear_plant_values(eicos_multi *mh) {
    if (!mh) return mfail(EICOS_E_INVALID, "NULL handle");
    return for_shards(mh, [&](int s) { return eicos_batch_clear_plant_values(mh->shard[s]); });
}
// (rows by shard, T = the step count of the trajectory the shards hold: eicos_multi_rollout_gradient)
int eicos_multi_rollout_plant_gradient(eicos_multi *mh, const double *gu, const double *gtheta, const double *u_traj, const double *theta_traj,
                                       double *grad_theta0, double *grad_w, double *grad_f0, double *grad_val) {
    if (!mh) return mfail(EICOS_E_INVALID, "NULL handle");
    if (!gu && !gtheta) return mfail(EICOS_E_INVALID, "rollout_plant_gradient: gu and gtheta are both NULL");
    if (!u_traj || !theta_traj) return mfail(EICOS_E_INVALID, "rollout_plant_gradient: u_traj or theta_traj is NULL");
    if (!grad_theta0 && !grad_w && !grad_f0 && !grad_val) return mfail(EICOS_E_INVALID, "rollout_plant_gradient: grad_theta0, grad_w, grad_f0 and grad_val are all NULL");
    const int steps = eicos_batch_rollout_jacobian_steps(mh->shard[0]);
    for (int s = 0; s < (int)mh->shard.size(); s++)
        if (steps < 1 || eicos_batch_rollout_jacobian_steps(mh->shard[s]) != steps)
            return mfail(EICOS_E_INVALID, "rollout_plant_gradient: shard " + std::to_string(s) + " holds no Jacobian trajectory, or one of another length (eicos_multi_rollout_jacobian records one)");
    const size_t k = (size_t)eicos_batch_param_count(mh->shard[0]), ro = (size_t)eicos_batch_output_count(mh->shard[0]), T = (size_t)steps;
    size_t k_plant, nnz;
    plant_dims(mh, k_plant, nnz);
    return for_shards(mh, [&](int s) {
        const size_t f = (size_t)mh->first[s];
        return eicos_batch_rollout_plant_gradient(mh->shard[s], at(gu, f, T * ro), at(gtheta, f, (T + 1) * k), at(u_traj, f, T * ro), at(theta_traj, f, (T + 1) * k),
                                                  at(grad_theta0, f, k), at(grad_w, f, T * k), at(grad_f0, f, k), at(grad_val, f, nnz));
    });
}

// recording on every shard; records and the data gradient are rows by shard, T = the step count of the trajectory the shards hold
int eicos_multi_set_rollout_recording(eicos_multi *mh, int on) {
    return in_turn(mh, false, [&](int s) { return eicos_batch_set_rollout_recording(mh->shard[s], on); });
}
int eicos_multi_rollout_recording(eicos_multi *mh) { return mh ? eicos_batch_rollout_recording(mh->shard[0]) : mfail(EICOS_E_INVALID, "NULL handle"); }
namespace {
int shard_steps(eicos_multi *mh, const char *who, int &steps) {
    steps = eicos_batch_rollout_jacobian_steps(mh->shard[0]);
    for (int s = 0; s < (int)mh->shard.size(); s++)
        if (steps < 1 || eicos_batch_rollout_jacobian_steps(mh->shard[s]) != steps)
            return mfail(EICOS_E_INVALID, std::string(who) + ": shard " + std::to_string(s) + " holds no Jacobian trajectory, or one of another length (eicos_multi_rollout_jacobian records one)");
    return EICOS_OK;
}
} // namespace
int eicos_multi_rollout_records(eicos_multi *mh, double *Wc, double *Wh, double *Wb, double *x_rec, double *y_rec, double *z_rec) {
    if (!mh) return mfail(EICOS_E_INVALID, "NULL handle");
    int steps = 0;
    const int rc = shard_steps(mh, "rollout_records", steps);
    if (rc != EICOS_OK) return rc;
    const size_t T = (size_t)steps, ro = (size_t)eicos_batch_output_count(mh->shard[0]);
    return for_shards(mh, [&](int s) {
        const size_t f = (size_t)mh->first[s];
        return eicos_batch_rollout_records(mh->shard[s], at(Wc, f, T * ro * mh->n), at(Wh, f, T * ro * mh->m), at(Wb, f, T * ro * mh->p),
                                           at(x_rec, f, T * mh->n), at(y_rec, f, T * mh->p), at(z_rec, f, T * mh->m));
    });
}
int eicos_multi_rollout_data_gradient(eicos_multi *mh, const double *gu, const double *gtheta, const double *theta_traj, const eicos_data_gradient *out) {
    if (!mh) return mfail(EICOS_E_INVALID, "NULL handle");
    if (!gu && !gtheta) return mfail(EICOS_E_INVALID, "rollout_data_gradient: gu and gtheta are both NULL");
    if (!theta_traj || !out) return mfail(EICOS_E_INVALID, "rollout_data_gradient: theta_traj or out is NULL");
    int steps = 0;
    const int rc = shard_steps(mh, "rollout_data_gradient", steps);
    if (rc != EICOS_OK) return rc;
    const size_t k = (size_t)eicos_batch_param_count(mh->shard[0]), ro = (size_t)eicos_batch_output_count(mh->shard[0]), T = (size_t)steps;
    int nnz[3] = {0, 0, 0}, nnzU = 0;
    (void)eicos_internal_map_nnz(mh->shard[0], nnz, &nnzU);
    return for_shards(mh, [&](int s) {
        const size_t f = (size_t)mh->first[s];
        const eicos_data_gradient o = {at(out->grad_c, f, mh->n), at(out->grad_h, f, mh->m), at(out->grad_b, f, mh->p), at(out->grad_G, f, mh->nnzG),
                                       at(out->grad_A, f, mh->nnzA), at(out->grad_Cval, f, nnz[0]), at(out->grad_Hval, f, nnz[1]),
                                       at(out->grad_Bval, f, nnz[2]), at(out->grad_u0, f, ro), at(out->grad_Uval, f, nnzU)};
        return eicos_batch_rollout_data_gradient(mh->shard[s], at(gu, f, T * ro), at(gtheta, f, (T + 1) * k), at(theta_traj, f, (T + 1) * k), &o);
    });
}

int eicos_multi_solution(eicos_multi *mh, double *x) {
    if (!mh || !x) return mfail(EICOS_E_INVALID, "NULL argument");
    if (mh->n == 0) return EICOS_OK;
    return for_shards(mh, [&](int s) { return eicos_batch_solution(mh->shard[s], at(x, (size_t)mh->first[s], mh->n)); });
}

int eicos_multi_duals(eicos_multi *mh, double *y, double *z, double *sl) {
    if (!mh) return mfail(EICOS_E_INVALID, "NULL handle");
    return for_shards(mh, [&](int s) {
        const size_t f = (size_t)mh->first[s];
        return eicos_batch_duals(mh->shard[s], at(y, f, mh->p), at(z, f, mh->m), at(sl, f, mh->m));
    });
}

int eicos_multi_set_warm_start(eicos_multi *mh, double shift) {
    return in_turn(mh, false, [&](int s) { return eicos_batch_set_warm_start(mh->shard[s], shift); });
}

int eicos_multi_set_dynamic_regularization(eicos_multi *mh, double delta, double eps) {
    return in_turn(mh, false, [&](int s) { return eicos_batch_set_dynamic_regularization(mh->shard[s], delta, eps); });
}

// (validation does not depend on the shard: the first shard refuses what any would, before one of them has changed)
int eicos_multi_set_settings(eicos_multi *mh, const eicos_settings *st) {
    return in_turn(mh, false, [&](int s) { return eicos_batch_set_settings(mh->shard[s], st); });
}

// the cone scaling of the adjoint (the mode is validated alike by every shard: the first refuses before any has changed)
int eicos_multi_set_adjoint_scaling(eicos_multi *mh, int mode) {
    return in_turn(mh, false, [&](int s) { return eicos_batch_set_adjoint_scaling(mh->shard[s], mode); });
}
int eicos_multi_adjoint_scaling(eicos_multi *mh) { return mh ? eicos_batch_adjoint_scaling(mh->shard[0]) : mfail(EICOS_E_INVALID, "NULL handle"); }

int eicos_multi_get_settings(eicos_multi *mh, eicos_settings *out) {
    if (!mh) return mfail(EICOS_E_INVALID, "NULL handle");
    const int rc = eicos_batch_get_settings(mh->shard[0], out);
    return rc != EICOS_OK ? mfail(rc, eicos_last_error()) : EICOS_OK;
}

// retry policy (validation does not depend on the shard either: every shard refuses what any would, before it has changed anything; the
// record is written on each shard's own stream, so on the shard's host thread like the maps)
int eicos_multi_set_retry(eicos_multi *mh, const eicos_retry *r) {
    if (!mh) return mfail(EICOS_E_INVALID, "NULL handle");
    return for_shards(mh, [&](int s) { return eicos_batch_set_retry(mh->shard[s], r); });
}

int eicos_multi_get_retry(eicos_multi *mh, eicos_retry *out) {
    if (!mh) return mfail(EICOS_E_INVALID, "NULL handle");
    const int rc = eicos_batch_get_retry(mh->shard[0], out);
    return rc != EICOS_OK ? mfail(rc, eicos_last_error()) : EICOS_OK;
}

// fallback map (validated against the shard's own maps, which are the same on every shard: all refuse what any would)
int eicos_multi_set_fallback_map(eicos_multi *mh, unsigned mask, const eicos_affine_map *v) {
    if (!mh) return mfail(EICOS_E_INVALID, "NULL handle");
    return for_shards(mh, [&](int s) { return eicos_batch_set_fallback_map(mh->shard[s], mask, v); });
}

int eicos_multi_fallback_mask(eicos_multi *mh) { return mh ? eicos_batch_fallback_mask(mh->shard[0]) : mfail(EICOS_E_INVALID, "NULL handle"); }

int eicos_multi_fallback_counts(eicos_multi *mh, int first, int count, int *fired, int reset) {
    if (!mh) return mfail(EICOS_E_INVALID, "NULL handle");
    if (count > 0 && !fired) return mfail(EICOS_E_INVALID, "fallback counts: fired is NULL");
    return for_range(mh, first, count, [&](int s, int f, int cnt, size_t off) {
        return eicos_batch_fallback_counts(mh->shard[s], f, cnt, fired + off, reset);
    });
}

int eicos_multi_retry_counts(eicos_multi *mh, int first, int count, int *retries, int reset) {
    if (!mh) return mfail(EICOS_E_INVALID, "NULL handle");
    if (count > 0 && !retries) return mfail(EICOS_E_INVALID, "retry counts: retries is NULL");
    return for_range(mh, first, count, [&](int s, int f, int cnt, size_t off) {
        return eicos_batch_retry_counts(mh->shard[s], f, cnt, retries + off, reset);
    });
}

int eicos_multi_last_solve_ms(eicos_multi *mh, float *ms_max, float *per_shard) {
    if (!mh || !ms_max) return mfail(EICOS_E_INVALID, "NULL argument");
    *ms_max = 0.f;
    const size_t ns = mh->shard.size();
    for (size_t s = 0; s < ns; s++) {
        float ms = 0.f;
        const int rc = eicos_batch_last_solve_ms(mh->shard[s], &ms);
        if (rc != EICOS_OK) return mfail(rc, eicos_last_error());
        if (per_shard) per_shard[s] = ms;
        *ms_max = std::max(*ms_max, ms);
    }
    // A device that holds several shards runs their launches partly one after the other: its solve lasted from the first start to the last
    // end over ITS shards (HIP events of one device are comparable across streams), not as long as its slowest shard alone.
    for (size_t a = 0; a < ns; a++)
        for (size_t b = 0; b < ns; b++) {
            if (a == b || mh->device[a] != mh->device[b]) continue;
            float span = 0.f;
            if (eicos_internal_solve_span_ms(mh->shard[a], mh->shard[b], &span) == EICOS_OK) *ms_max = std::max(*ms_max, span);
        }
    return EICOS_OK;
}

} // extern "C"
