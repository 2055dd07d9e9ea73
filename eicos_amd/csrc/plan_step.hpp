// The host-only steps of handle creation: pattern intake, analysis, plan and LDS budget -- everything that turns a
// symbolic analysis into the offsets and indices a kernel addresses.  Pure host code: no HIP call, no eicos_batch.  plan_step.cpp is
// compiled without a HIP include path, and tests/host/plan_step_check.cpp runs it under the address and undefined-behaviour sanitizers.
#pragma once

#include <cstddef>
#include <vector>

#include "device_types.hpp"
#include "symbolic.hpp"
#include "plans.hpp"
#include "tiles.hpp"

namespace eicos {
#pragma GCC visibility push(hidden) // (internal to the library: not part of its exported symbols)

// LDS of a CU, and the part of it a solve workgroup's static block takes: struct Sh + the per-instance states of kernels.hip (reductions +
// scalar state), rounded up -- kernels.hip asserts sizeof(Sh) against its own copy of the figure.
constexpr size_t LDS_PER_CU = 160 * 1024;
constexpr size_t LDS_STATIC = 4096;

struct IntPool { // one int32 buffer for every pattern array
    std::vector<int> data;
    size_t add(const std::vector<int> &v) {
        size_t off = data.size();
        data.insert(data.end(), v.begin(), v.end());
        while (data.size() % 4) data.push_back(0); // keep 16-byte alignment of every array
        if (v.empty()) { data.insert(data.end(), 4, 0); }
        return off;
    }
};

struct Analysis { Symbolic sym; TilePlan tiles; }; // a symbolic analysis (+ the dense-front plan of the tile and hybrid paths)

// What the analysis step decides: the workgroup size, whether plans carry the dense apex, and which analysis a plan is built from.
struct Analyses {
    Analysis main;         // EICOS_ORDER / EICOS_TILES as set
    Analysis apex_alt;     // small hybrid patterns at 256 / 512 threads: the scalar analysis with a dense apex (has_alt)
    bool has_alt = false;
    int threads = 256;
    bool apex = false;     // the dense apex is allowed (profile 0, and a workgroup size / batch that can carry it)
    Analysis &for_plan(bool with_apex) { return with_apex && has_alt ? apex_alt : main; }
};

// Everything the plan step produces: the DevPat offsets and counts, the backward value slots, and the pattern image with the places its
// arrays' device addresses go (filled by the allocation step).  `slots` points into this object, so a Plan is never copied or moved.
struct Plan {
    Analysis *an = nullptr;  // the analysis it was built from
    bool apex = false;       // the sweeps end in the dense apex (Symbolic::apex0)
    int threads = 256;
    DevPat dp{};
    std::vector<int> posB;   // CSC entry of L -> slot in the backward value array
    int ub_len = 1;
    IntPool pool;
    struct Slot { const int **dst; size_t off; };
    std::vector<Slot> slots;
    // pool arrays whose DevPat fields are typed (slice tables) or chosen by the launch shape (stored-L / deferred-L factor operands)
    const int *fsl = nullptr, *bsl = nullptr, *cag_sl = nullptr, *rA_sl = nullptr, *rG_sl = nullptr, *fac_sl = nullptr;
    const int *fac_pb_f = nullptr, *fac_pb_u = nullptr, *fac_p16_f = nullptr, *fac_p16_u = nullptr;
    SharedOperands shop;     // which factor operands a batch that shares its matrices may read from one copy (plans.hpp); allocate() decides
    Plan() = default;
    Plan(const Plan &) = delete;
    Plan &operator=(const Plan &) = delete;
    void put(const int *&field, const std::vector<int> &v) { slots.push_back({&field, pool.add(v)}); }
};

// The launch shape of a plan (api.cpp: launch_shape; its LDS part: lds_budget).
struct Shape {
    int nlds = 0, ldsres = 0, w2 = 0, ubl = 0;
    size_t dyn_lds = 0;
    int bpc = 1, grid = 0, order_min = 0;
    int upd_grid = 0, upd_vals_lds = 1; size_t upd_lds = 0;
    bool apex_unplaced = false; // a 128-thread plan with the apex that does not get the LDS-resident build: it cannot run (no probes done)
};

// Pattern intake, in two halves: eicos_batch_create resolves its device between them, so that a machine without a GPU answers
// EICOS_E_NOGPU after the argument checks and before the CSC checks; the host-only debug entries call them back to back.
// check_pattern_args: the argument checks.  Groups given as NULL are empty: m, p and ncones come back as the pattern will have them.
int check_pattern_args(int n, int &m, int &p, int l, int &ncones, const int *q, const int *Gjc, const int *Gir, const int *Ajc, const int *Air,
                       int batch);
// take_csc: the CSC checks, and the checked arguments as a ProblemPattern.
int take_csc(int n, int m, int p, int ncones, const int *q, const int *Gjc, const int *Gir, const int *Ajc, const int *Air, ProblemPattern &P);

// Analysis step: the pattern's symbolic analysis, the workgroup size, whether plans may carry the dense apex, and -- small hybrid patterns
// -- the scalar analysis with a dense apex that such a plan uses instead.  `profile` = eicos_set_arithmetic_profile at creation.
int analyse(const ProblemPattern &P, int batch, int n_cu, int profile, Analyses &A);
// Plan step.  `apex`: the plan carries the dense apex when its analysis has one.
int build_plan(const ProblemPattern &P, Analyses &A, bool apex, int batch, int n_cu, int profile, Plan &pl);
// The LDS budget of a plan: which KKT-space vectors and slice tables live in LDS, dual right-hand sides, the deferred-L factorisation, the
// LDS-resident build.  Fills the LDS fields of the plan's DevPat.
void lds_budget(Plan &pl, int batch, int n_cu, Shape &sh);
// Workgroups per CU for a batch, at most `max_r`: the cheapest estimate of the launch's duration wins.
int launch_blocks_per_cu(int batch, int n_cu, int max_r, int threads);

#pragma GCC visibility pop
} // namespace eicos
