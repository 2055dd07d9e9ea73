// C ABI of the batched solver (include/eicos_amd.h): host-side setup, memory, launches.
// There is deliberately NO CPU fallback: without a HIP device every compute entry point fails
// with EICOS_E_NOGPU.
#include "../../include/eicos_amd.h"

#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <climits>
#include <cstring>
#include <atomic>
#include <functional>
#include <map>
#include <mutex>
#include <stdexcept>
#include <string>
#include <vector>

#include "device_types.hpp"
#include "launch.hpp"
#include "symbolic.hpp"
#include "plans.hpp"
#include "tiles.hpp"
#include "envknob.hpp"
#include "internal.hpp"
#include "affine_pack.hpp"
#include "fused_fit.hpp"
#include "exit_class.hpp"
#include "resources.hpp"
#include "call_arrays.hpp"
#include "rollout_layout.hpp"
#include "last_error.hpp"
#include "plan_step.hpp"
#include "host_copy.hpp"
#include "chunk_plan.hpp"

using namespace eicos;

// eicos_set_arithmetic_profile: 0 = plans shaped by the launch (default), 1 = plans shaped by the pattern alone (batch-independent bits)
static std::atomic<int> g_arith_profile{0};
static std::mutex g_slot_mu;
static std::map<int, std::vector<char>> g_slot_used; // per device: which constant-memory descriptor slots are taken (under g_slot_mu)
// HIP_TRY_AS: the message names the HIP call `what` -- for calls made through the handle's buffers (resources.hpp), so that their
// failures read as they did when the call stood here itself ("hipMalloc...: out of memory").  HIP_TRY: the expression is the name.
#define HIP_TRY_AS(what, expr)                                                                     \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess) return fail(EICOS_E_HIP, std::string(what) + ": " + hipGetErrorString(e_)); \
    } while (0)
#define HIP_TRY(expr) HIP_TRY_AS(#expr, expr)

// The memory and event policies of the handle's buffers (resources.hpp): the only places that allocate or free for a handle.
struct HipPolicy {
    using error_t = hipError_t; using stream_t = hipStream_t;
    static constexpr hipError_t ok = hipSuccess;
    static hipError_t sync(hipStream_t s) { return hipStreamSynchronize(s); }
};
struct DeviceMem : HipPolicy {
    static hipError_t alloc(void **p, size_t bytes) { return hipMalloc(p, bytes); }
    static void free(void *p) { (void)hipFree(p); }
};
struct PinnedMem : HipPolicy {
    static hipError_t alloc(void **p, size_t bytes) { return hipHostMalloc(p, bytes, hipHostMallocDefault); }
    static void free(void *p) { (void)hipHostFree(p); }
};
struct HipEvent {
    using event_t = hipEvent_t;
    static hipError_t create(hipEvent_t *e) { return hipEventCreateWithFlags(e, hipEventDisableTiming); }
    static void destroy(hipEvent_t e) { (void)hipEventDestroy(e); }
    static hipError_t record(hipEvent_t e, hipStream_t s) { return hipEventRecord(e, s); }
    static hipError_t sync(hipEvent_t e) { return hipEventSynchronize(e); }
};
using DevBuf = Buffer<DeviceMem>;
using PinBuf = Buffer<PinnedMem>;
using PinSlot = PinnedSlot<PinnedMem, HipEvent>;

struct eicos_batch {
    ProblemPattern pat;
    Symbolic sym;
    DevPat dp{};
    int batch = 0, device = 0, threads = 256, grid = 0, upd_grid = 0;
    int order_min = 0;        // batches up to this size (one instance per CU) are solved in identity order, larger ones longest-first
    bool last_ordered = false; // how the most recent solve was launched (eicos_debug_trace)
    bool last_subset = false; int last_count = 0; // ... whether it took a chosen subset (eicos_batch_solve_subset / _solve_where), and how many instances
    size_t upd_lds = 0;       // > 0: updateData runs the entry-parallel kernel with this much dynamic LDS (values + maxima)
    int upd_vals_lds = 1;     // 1: its working copy of the values is in LDS too; 0: streamed in place in the instance slab
    DevBuf d_pattern;        // the pattern image (int32 arrays; DevPat points into it)
    int pslot = -1; // slot of this handle's DevPat in the kernels' constant-memory table
    size_t dyn_lds = 0;
    int nlds = 0;
    int w2 = 0;               // 1: solves run the two-waves-per-SIMD build of the 256-thread kernel (w2::solve_entries)
    int ubl = 0;              // 1: solves run the build with the factor operand array U in LDS (ubl256:: / ubl512::solve_entries; one workgroup per CU)
    int ldsres = 0;           // 1: solves run the LDS-resident kernel (ldsres::solve_entries), slabs copied in and out per instance
    size_t pattern_ints = 0;
    DevBuf d_inst, d_work, d_scratch; // the instance slabs, the workspace slabs of the resident workgroups, the updateData scratch
    DevBuf d_queue; // instance queue of the solve kernel (reset per launch): [16-int header | launch order [batch] | candidates of a subset launch [batch] | row map of a step over a subset [batch]]
    // (what the enqueue path reads of them: a member load each)
    double *inst() const { return d_inst.as<double>(); }
    double *work() const { return d_work.as<double>(); }
    int *queue() const { return d_queue.as<int>(); }
    // subset calls: a host index list travels through one pinned buffer of `batch` ints; the row gather packs the chosen instances' rows
    // into d_gather = [ids | rows]
    PinSlot sub;
    DevBuf d_gather;
    // index-list updates and outputs (eicos_batch_*_indexed): their validated ids in device memory, `batch` ints of their own -- the
    // candidates behind the launch order belong to the subset launches, and one that is queued still reads them
    DevBuf d_upd_ids;
    DevBuf d_stage; // peer-copy updateData without peer access: staging buffer (one chunk)
    // host-pointer updateData / results (the reference's real signature: updateData(double *...), solution() on the host): two PINNED
    // bounce buffers (hipHostMalloc).  Input chunk k is copied into pin[k & 1] by the host while the GPU's updateData kernel reads chunk
    // k - 1 straight out of the other one over PCIe (the kernel's loads are the transfer: no device-side staging copy, no per-chunk
    // stream synchronisation); results come back through the same buffers, the strided device-to-host copy of chunk k + 1 in flight
    // while the host copies chunk k out.
    PinSlot pin[2];
    int last_update_path = 0; // how the most recent host/peer updateData moved its inputs: 1 pinned bounce, 2 zero-copy (pinned source), 3 peer zero-copy, 4 peer staged copies, 5 fused into the solve launch, 6 the same with pageable arrays staged while the kernel runs
    DevBuf d_flag;           // debug hooks
    double warm_shift = 0.; // > 0: warm start (eicos_batch_set_warm_start)
    double dyn_delta = 0., dyn_eps = 0.; // > 0: dynamic regularisation (eicos_batch_set_dynamic_regularization)
    SolveCfg cfg = solve_cfg_default(); // runtime settings (eicos_batch_set_settings): every solve launch carries a copy by value
    hipStream_t own_stream = nullptr, stream = nullptr;
    // HIP events around every solve launch / every updateData call, on the handle's stream.  A RING of pairs: the durations of the last
    // EV_RING launches can be read after the fact (eicos_batch_ms_history), so that a caller timing K back-to-back steps need not
    // synchronise with the GPU inside its loop to learn each launch's duration.  ev_* = the most recent pair of each ring.
    static constexpr int EV_RING = 64;
    hipEvent_t ring_s[EV_RING][2] = {}, ring_u[EV_RING][2] = {};
    hipEvent_t ring_step0[EV_RING] = {}; // per solve slot: start event of the updateData call that preceded it (the start of the caller's "step")
    long n_solve_rec = 0, n_update_rec = 0;
    hipEvent_t ev_s0 = nullptr, ev_s1 = nullptr, ev_u0 = nullptr, ev_u1 = nullptr;
    bool solve_timed = false, update_timed = false;
    int64_t npairs = 0;
    std::vector<int> posB; // CSC entry of L -> slot in the backward value array
    int ub_len = 1;        // length of that array (plan slots + dummy, + the dense apex image)
    int bpc = 1, n_cu = 256; // workgroups per CU of the solve launch; CUs of the device
    int arith_profile = 0;   // eicos_set_arithmetic_profile at creation
    // eicos_batch_update_solve from pageable host memory: one pinned staging buffer for the whole batch (+ one ready flag per chunk), filled while the kernel runs
    PinBuf stage_pin, stage_flags; unsigned stage_seq = 0;
    DevBuf d_err;
    // parametric right-hand sides (eicos_batch_set_param_map): the map's arrays in one device allocation, param.k = 0 while none is installed
    // (d_param starts with a device copy of `param` itself, MAP_HEADER bytes: what the fused step's workgroups read -- launch.hpp: UpdArgs)
    ParamMapDev param{}; DevBuf d_param;
    // output map (eicos_batch_set_output_map): one device allocation [OutMapDev | u rows of the batch | base, val | rowptr, col], out.r = 0
    // while none is installed; d_u = the [batch][r] rows the range kernel fills for a host destination
    OutMapDev out{}; DevBuf d_out; double *d_u = nullptr;
    // plant map (eicos_batch_set_plant_map): one device allocation [PlantMapDev (MAP_HEADER bytes) | base, val | rowptr, col], plant.k = 0 while none is installed
    PlantMapDev plant{}; DevBuf d_plant;
    // per-instance plant values (eicos_batch_set_plant_values): one allocation per group, [batch][k] and [batch][plant.nnz], made and filled
    // with the shared values by the group's first call; plant.ibase / plant.ival point at them (NULL: the group is the shared one)
    DevBuf d_plant_f0, d_plant_val;
    // rollout (eicos_batch_rollout): d_roll, d_rollJ and d_rollW as rollout_layout.hpp lays them out -- the trajectories of the most
    // recent rollout; with eicos_batch_rollout_jacobian its Jacobians, kept for the backward sweeps; the rows of a recording rollout
    // (eicos_batch_set_rollout_recording), made by the first recording rollout and freed, with d_rollD, when recording is switched off.
    // All three grow on demand.  roll = the host copy of the record of the most recent call; held = the trajectory the handle holds
    // for the calls that read it back; map_gen counts the installs of the parameter, matrix, output, plant and fallback maps.
    RolloutDev roll{}; DevBuf d_roll, d_rollJ, d_rollW; int rollout_launches = 0; bool roll_recording = false;
    HeldTrajectory<PlantMapDev> held; unsigned long map_gen = 0;
    // matrix map (eicos_batch_set_matrix_map): one device allocation [MatrixMapDev (MAP_HEADER bytes) | base, val | rowptr, col], mat.k = 0
    // while none is installed; d_mstage = the device staging buffer the range path expands [Gpr | Apr | c | h | b] of a chunk of instances
    // into (param_range), up to MSTAGE_CAP_MB
    MatrixMapDev mat{}; DevBuf d_mat, d_mstage;
    // shift map (eicos_batch_set_shift_map): one device allocation [ShiftMapDev (MAP_HEADER bytes) | base, val | rowptr, col]; every solve
    // launch of the handle carries its address (UpdArgs::smap), d_shift empty while none is installed
    ShiftMapDev shift{}; DevBuf d_shift;
    // retry policy (eicos_batch_set_retry): one device allocation [RetryDev (MAP_HEADER bytes) | counts [batch]], made by the first policy
    // and kept; retry = the host copy of the record (its source for the copy on the handle's stream), retry.mask = 0 while no policy is
    // installed -- then no launch carries the record's address (UpdArgs::retry)
    RetryDev retry{0u, 0., 0., 0., solve_cfg_default(), nullptr}; DevBuf d_retry;
    // fallback map (eicos_batch_set_fallback_map): one device allocation [FallbackDev (MAP_HEADER bytes) | counts [batch] | base, val |
    // rowptr, col], fb.mask = 0 while none is installed -- then no launch carries the record's address (UpdArgs::fb); d_fb_theta = the
    // [batch][k] device copy of a step's pageable theta rows, which the range kernel reads behind a step that is not fused
    FallbackDev fb{}; DevBuf d_fb, d_fb_theta;
    TilePlan tiles;      // tile mode (Symbolic::tile): the dense-front plan
    // Shared product values (eicos_batch_shared_values): ONE device word.  -1: every instance streams the product values of
    // its own slab.  0: the last writer of matrix values was a full updateData over [0, batch) from arrays the GPU addresses, and its
    // kernel found every row of Gpr / Apr bit-identical to row 0 -- the solve's products then all stream instance 0's copies.  ONE place
    // sets it (shared_detect, in front of that launch); every other launch that writes matrix values of any instance (i_Av, i_Gv, i_cag,
    // i_rA, i_rG, i_Gt: a sub-range or group-keeping updateData, the chunked paths, the matrix map, the fused forms) is preceded by
    // shared_clear on the handle's stream.  shared_on: EICOS_SHARED_VALUES (default 1) and not the LDS-resident build, whose values are
    // in LDS already; shared_maybe: the word may be 0 (spares the clearing memset of a handle that never shares).
    DevBuf d_shared; bool shared_on = false, shared_maybe = false;
    // Shared factor operands (DevPat::kt0 / ub0): one allocation [kt0 | ub0], filled from instance 0 on the handle's stream behind
    // every launch that may leave the word above at 0 (launch_range) -- so its contents are valid exactly while the word is 0, and only the
    // stages' PLAIN instantiations, which run exactly then, read it.  Empty: not on this handle (eicos_dims.shared_operands = 0).
    DevBuf d_shop;
    // Adjoint sensitivities (eicos_batch_adjoint, _adjoint_data, _output_jacobian, _param_jacobian, _param_gradient): one device
    // allocation, made by the first call and grown on demand: the record of the launch (AdjointDev, MAP_HEADER bytes), its index list and
    // the staging of the host forms' arrays, as adjoint_run declares them (call_arrays.hpp)
    DevBuf d_adj; AdjointDev adj{}; // (adj: the host copy of the most recent launch's record, the source of its copy on the handle's stream)
    // the staging of eicos_batch_rollout_gradient and of eicos_batch_rollout_data_gradient, as rollout_gradient and rollout_data_gradient
    // declare their arrays (call_arrays.hpp): the latter also the workgroups' contracted rows
    DevBuf d_rollG, d_rollD;
    int param_nnz[3] = {0, 0, 0}, out_nnz = 0; // stored entries of the installed parameter map's groups and of the output map (the widths of their slope gradients)
    int adjoint_scaling = EICOS_ADJOINT_NT; // eicos_batch_set_adjoint_scaling: what adjoint_record puts into AdjointDev::centred
    hipEvent_t ev_a0 = nullptr, ev_a1 = nullptr; bool adjoint_timed = false; // HIP events around the most recent adjoint launch (eicos_batch_last_adjoint_ms)

    // The events and the stream the handle made; the buffers free themselves after this body.  eicos_batch_destroy has set the device and
    // waited for both streams: nothing here synchronises.
    ~eicos_batch() {
        if (own_stream) (void)hipStreamDestroy(own_stream);
        for (int i = 0; i < EV_RING; i++)
            for (hipEvent_t e : {ring_s[i][0], ring_s[i][1], ring_u[i][0], ring_u[i][1]}) if (e) (void)hipEventDestroy(e);
        for (hipEvent_t e : {ev_a0, ev_a1}) if (e) (void)hipEventDestroy(e);
    }
};

// ---- handle creation ----
// eicos_batch_create runs five steps, each once: pattern intake (check_pattern_args, device resolution, take_csc), analysis (analyse), plan
// (build_plan), launch shape (launch_shape: LDS budget, occupancy probes, kernel build) and allocation (allocate: the only step that makes
// device resources).  The first three and the LDS budget are pure host code and live in plan_step.cpp; what follows here is what talks
// to HIP.  Only the last two steps hold the per-device creation lock, so the shards of an eicos_multi -- created on parallel host threads
// -- overlap their analyses and plans.

// One creation lock PER DEVICE: the shards of an eicos_multi that live on different GPUs set their devices up in parallel, two handles on
// one GPU take turns (the occupancy probes and hipFuncSetAttribute calls of one device must not interleave).
static std::mutex &create_mutex(int device) {
    static std::mutex map_mu;
    static std::map<int, std::mutex> mus;
    std::lock_guard<std::mutex> lk(map_mu);
    return mus[device];
}

// Launch-shape step: the LDS budget, then -- under the device's creation lock -- the occupancy probes and the choice of the kernel build
// (w2 / U in LDS), the LDS head of the refinement residual, the grid and the updateData kernel.  Allocates nothing.
static int launch_shape(Plan &pl, int batch, int device, Shape &sh) {
    std::lock_guard<std::mutex> create_lock(create_mutex(device));
    HIP_TRY(hipSetDevice(device));
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    const int n_cu = prop.multiProcessorCount, threads = pl.threads;
    lds_budget(pl, batch, n_cu, sh);
    if (sh.apex_unplaced) return EICOS_OK;
    const Symbolic &S = pl.an->sym;
    DevPat &D = pl.dp;
    const int idx16 = D.idx16;
    int bpc = 1;
    {
        const SolveBuild sb = solve_build(threads, sh.ldsres, false);
        HIP_TRY(sb.set_max_lds(threads, sh.nlds, idx16, sh.dyn_lds));
        HIP_TRY(sb.occupancy(threads, sh.nlds, idx16, sh.dyn_lds, &bpc));
    }
    bpc = std::max(1, std::min(bpc, 8));
    HIP_TRY(update_set_max_lds()); // (per handle = per device, after hipSetDevice: the entry-parallel updateData kernels use up to 160 KB of dynamic LDS)
    bpc = launch_blocks_per_cu(batch, n_cu, bpc, threads); // workgroups per CU for this batch: the cheapest estimate (measured constants)
    bpc = std::max(1, std::min(bpc, env_knob("EICOS_BLOCKS_PER_CU", bpc, 1, 8)));
    // 256 threads at <= 2 workgroups per CU: the build with 256 VGPRs per thread (the default one is held to 168 so that three fit)
    sh.w2 = 0;
    if (!sh.ldsres && threads == 256 && bpc <= 2 && env_knob("EICOS_W2", 1, 0, 1)) {
        const SolveBuild wb = solve_build(threads, false, true);
        int got = 0;
        HIP_TRY(wb.set_max_lds(threads, sh.nlds, idx16, sh.dyn_lds));
        HIP_TRY(wb.occupancy(threads, sh.nlds, idx16, sh.dyn_lds, &got));
        if (got >= bpc) sh.w2 = 1;
    }
    // One workgroup per CU (batch <= CUs) and the factor operand array U = L.*D fits the LDS that the lone workgroup leaves idle: the build that
    // keeps it there (kernels_ubl*.hip).  The numeric factorisation of a deep pattern is a chain of levels that each wait for operand gathers
    // and for their stores to land -- L2 round trips with U in the workspace slab, LDS round trips here; bit-identical results.
    sh.ubl = 0; D.ub_lds = -1; D.ub_len = pl.ub_len;
    if (!sh.ldsres && (threads == 256 || threads == 512) && bpc == 1 && batch <= n_cu && sh.nlds >= 1 && D.fac_defer && S.tile != 1 &&
        !(D.apex_na > 0 && D.apex_lds < 0) && env_knob("EICOS_UBL", 1, 0, 1)) {
        const size_t base = (sh.dyn_lds + 15) & ~(size_t)15, need = base + ((size_t)pl.ub_len + 8) * sizeof(double);
        if (need + LDS_STATIC <= LDS_PER_CU) { // (the static block, as lds_budget counts it)
            const SolveBuild ub = solve_build(threads, false, false, true);
            int got = 0;
            HIP_TRY(ub.set_max_lds(threads, sh.nlds, idx16, need));
            HIP_TRY(ub.occupancy(threads, sh.nlds, idx16, need, &got));
            if (got >= 1) { sh.ubl = 1; sh.w2 = 0; D.ub_lds = (int)(base / sizeof(double)); sh.dyn_lds = need; }
        }
    }
    const SolveBuild sbuild = solve_build(threads, sh.ldsres, sh.w2, sh.ubl);
    // The two-waves-per-SIMD build with one LDS vector and one right-hand side keeps the parked refinement iterate in registers of the owning
    // threads (device_types.hpp: xpark) when a thread's share fits; larger patterns park it in the workspace slab as every other build does.
    D.xpark = (sh.w2 && sh.nlds == 1 && !D.dual && D.N <= XPARK_CAP * threads && env_knob("EICOS_XPARK", 1, 0, 1)) ? 1 : 0;
    // The LDS that `bpc` resident workgroups leave free takes the head of the refinement residual E (device_types.hpp: e_lds): its
    // scattered stores and the read-back stay on chip.  Verified against the runtime's occupancy for the enlarged allocation.
    D.e_lds = 0; D.e_off = 0;
    if (!sh.ldsres && sh.nlds == 1 && !D.dual && S.tile != 1) {
        const size_t base = (sh.dyn_lds + 15) & ~(size_t)15, room = LDS_PER_CU / (size_t)bpc;
        size_t xs = room > base + LDS_STATIC + 1024 ? std::min<size_t>((size_t)D.N, (room - base - LDS_STATIC - 1024) / sizeof(double)) & ~(size_t)15 : 0;
        while (xs > 0) {
            int got = 0;
            HIP_TRY(sbuild.set_max_lds(threads, sh.nlds, idx16, base + xs * sizeof(double)));
            HIP_TRY(sbuild.occupancy(threads, sh.nlds, idx16, base + xs * sizeof(double), &got));
            if (got >= bpc) break;
            xs = (xs * 3 / 4) & ~(size_t)15;
        }
        if (xs > 0) { D.e_lds = (int)xs; D.e_off = (int)(base / sizeof(double)); sh.dyn_lds = base + xs * sizeof(double); }
    }
    sh.bpc = bpc;
    sh.grid = std::min(batch, n_cu * bpc);
    sh.order_min = n_cu;
    sh.upd_grid = std::min(batch, n_cu * 4);
    {   // entry-parallel updateData: needs the A / G values and the row / column maxima in LDS and <= 8 vector entries per thread
        const size_t need = ((size_t)S.nnzA + S.nnzG + S.n + S.p + S.m + 8) * sizeof(double);
        const size_t need_max = ((size_t)S.n + S.p + S.m + 8) * sizeof(double); // the row / column maxima alone
        const bool small_vecs = update_vectors_fit(S.n, S.p, S.m);
        const int mode = env_knob("EICOS_UPDATE_LDS", 1, 0, 2); // 0: thread-per-column kernel, 2: force the streamed-values variant
        if (need <= 156 * 1024 && small_vecs && mode == 1) { sh.upd_lds = need; sh.upd_vals_lds = 1; sh.upd_grid = std::min(batch, n_cu); }
        else if (need_max <= 156 * 1024 && small_vecs && mode >= 1) { // values streamed in place, maxima in LDS: as many 512-thread workgroups per CU as fit (<= 4)
            sh.upd_lds = need_max; sh.upd_vals_lds = 0;
            const int per_cu = (int)std::max<size_t>(1, std::min<size_t>(4, LDS_PER_CU / (need_max + 1024)));
            sh.upd_grid = std::min(batch, n_cu * per_cu);
        }
    }
    return EICOS_OK;
}

// Allocation step: the only code that gives a handle device resources -- the pattern image, the descriptor slot (uploaded to the default
// build and to the chosen one), the slabs, the instance queue, the updateData scratch and the stream.  One cleanup path:
// eicos_batch_destroy takes a partly set-up handle, whose members free what was made.
static int allocate(ProblemPattern &&P, Plan &pl, const Shape &sh, int batch, int device, int n_cu, int profile, eicos_batch **out) {
    std::lock_guard<std::mutex> create_lock(create_mutex(device));
    eicos_batch *h = new eicos_batch();
    h->batch = batch; h->device = device; h->n_cu = n_cu; h->arith_profile = profile;
    h->threads = pl.threads; h->posB = std::move(pl.posB); h->ub_len = pl.ub_len; h->npairs = pl.an->sym.npairs;
    h->nlds = sh.nlds; h->ldsres = sh.ldsres; h->w2 = sh.w2; h->ubl = sh.ubl; h->dyn_lds = sh.dyn_lds;
    h->bpc = sh.bpc; h->grid = sh.grid; h->order_min = sh.order_min;
    h->upd_grid = sh.upd_grid; h->upd_lds = sh.upd_lds; h->upd_vals_lds = sh.upd_vals_lds;
    h->pattern_ints = pl.pool.data.size();
    const Symbolic &S = pl.an->sym;
    const int rc = [&]() -> int {
        HIP_TRY(hipSetDevice(device));
        HIP_TRY_AS("hipMalloc", h->d_pattern.alloc(pl.pool.data.size() * sizeof(int)));
        HIP_TRY(hipMemcpy(h->d_pattern.p, pl.pool.data.data(), pl.pool.data.size() * sizeof(int), hipMemcpyHostToDevice));
        DevPat &D = pl.dp;
        for (auto &s : pl.slots) *s.dst = h->d_pattern.as<int>() + s.off;
        D.fac_pb = D.fac_defer ? pl.fac_pb_u : pl.fac_pb_f; D.fac_p16 = D.fac_defer ? pl.fac_p16_u : pl.fac_p16_f;
        D.fsl = reinterpret_cast<const PackedSlice *>(pl.fsl); D.bsl = reinterpret_cast<const PackedSlice *>(pl.bsl);
        D.cag_sl = reinterpret_cast<const PackedSlice *>(pl.cag_sl); D.rA_sl = reinterpret_cast<const PackedSlice *>(pl.rA_sl);
        D.rG_sl = reinterpret_cast<const PackedSlice *>(pl.rG_sl);
        D.fac_sl = reinterpret_cast<const PackedSlice *>(pl.fac_sl);
        h->shared_on = !h->ldsres && env_knob("EICOS_SHARED_VALUES", 1, 0, 1) != 0;
        // shared factor operands: the scalar factor path of the builds that keep U in the workspace slab and the sweep vector in LDS
        if (h->shared_on && !h->ubl && sh.nlds >= 1 && S.tile == 0 && pl.shop.any() && env_knob("EICOS_SHARED_OPERANDS", 1, 0, 1)) {
            const bool ub0 = pl.shop.ub0_off != 0x7fffffff;
            const size_t kt_len = ((size_t)D.fac_nt + 8 + 7) & ~(size_t)7, ub_len = ub0 ? (size_t)(D.nUB + 1 - pl.shop.ub0_off) + 8 : 0;
            HIP_TRY_AS("hipMalloc", h->d_shop.alloc((kt_len + ub_len) * sizeof(double)));
            HIP_TRY(hipMemset(h->d_shop.p, 0, h->d_shop.bytes)); // (the padding slots and the dummy slot of ub0 stay 0)
            D.kt0 = h->d_shop.as<double>(); D.kt0_pass = pl.shop.pass;
            if (ub0) { D.ub0 = h->d_shop.as<double>() + kt_len; D.ub0_off = pl.shop.ub0_off; }
        }
        h->dp = D;
        {
            std::lock_guard<std::mutex> lk(g_slot_mu);
            std::vector<char> &used = g_slot_used[device];
            used.resize((size_t)max_patterns(), 0);
            for (int q = 0; q < max_patterns(); q++) if (!used[q]) { h->pslot = q; used[q] = 1; break; }
        }
        if (h->pslot < 0) return fail(EICOS_E_INVALID, "too many live handles on this device (64)");
        const SolveBuild main_build = solve_entries(), sbuild = solve_build(h->threads, h->ldsres, h->w2, h->ubl);
        HIP_TRY(main_build.upload(h->pslot, h->dp)); // (the default namespace always: updateData and the debug kernels live there)
        if (!(sbuild == main_build)) HIP_TRY(sbuild.upload(h->pslot, h->dp));
        HIP_TRY_AS("hipMalloc", h->d_inst.alloc((size_t)batch * D.inst_stride * sizeof(double)));
        HIP_TRY(hipMemset(h->d_inst.p, 0, h->d_inst.bytes));
        HIP_TRY_AS("hipMalloc", h->d_work.alloc((size_t)h->grid * D.work_stride * sizeof(double)));
        HIP_TRY(hipMemset(h->d_work.p, 0, h->d_work.bytes));
        HIP_TRY_AS("hipMalloc", h->d_queue.alloc((16 + 3 * (size_t)batch) * sizeof(int))); // [0] queue head, [1] the count of a selection, [16..] launch order, [16 + batch..] candidates, [16 + 2 batch..] row map
        HIP_TRY_AS("hipMalloc", h->d_shared.alloc(64));
        HIP_TRY(hipMemset(h->d_shared.p, 0xFF, 64)); // (-1: nothing shared)
        HIP_TRY_AS("hipMalloc", h->d_scratch.alloc((size_t)h->upd_grid * (size_t)(S.n + S.p + S.m + 8) * sizeof(double)));
        HIP_TRY(hipStreamCreateWithFlags(&h->own_stream, hipStreamNonBlocking));
        h->stream = h->own_stream;
        // (the event pairs of the timing rings are created on first use: next_events)
        HIP_TRY(hipDeviceSynchronize());
        return EICOS_OK;
    }();
    if (rc != EICOS_OK) { eicos_batch_destroy(h); return rc; }
    h->pat = std::move(P); h->sym = std::move(pl.an->sym); h->tiles = std::move(pl.an->tiles);
    *out = h;
    return EICOS_OK;
}

// ---- affine maps (no reference counterpart): parameter, output, plant, matrix, shift and fallback map through one path ----
// A setter states its own preconditions and its groups (affine_pack.hpp: AffineGroup); affine_fault validates a group, install_map packs
// the groups into ONE device allocation [descriptor (MAP_HEADER bytes) | gap | base, val per group | rowptr, col per group] and swaps it
// for the one in the handle.  A later call replaces a map; DESIGN.md, "Affine maps: one path".
static constexpr size_t MAP_HEADER = 128; // bytes kept for the descriptor in front of a map's arrays (keeps the doubles aligned)
static_assert(sizeof(ParamMapDev) <= MAP_HEADER && sizeof(OutMapDev) <= MAP_HEADER && sizeof(PlantMapDev) <= MAP_HEADER &&
              sizeof(RolloutDev) <= MAP_HEADER && sizeof(MatrixMapDev) <= MAP_HEADER && sizeof(ShiftMapDev) <= MAP_HEADER &&
              sizeof(FallbackDev) <= MAP_HEADER && ROLLOUT_HEADER == MAP_HEADER,
              "map descriptor larger than its header");

// The map in `slot` (its device allocation) and `cur` (the handle's copy of its descriptor) goes away; M != NULL: the n validated groups
// g take its place -- *M is the new descriptor and `out` its AffineDev array of n, filled here; `gap` bytes behind the header stay
// uninitialised (the output map's u rows).
template <class Desc>
static int install_map(eicos_batch *h, DevBuf &slot, Desc &cur, const char *name, const AffineGroup *g, int n, size_t gap, Desc *M, AffineDev *out) {
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream)); // (a launch in flight may still read the map that goes away)
    slot.reset(); // (first, so that the old and the new map never coexist; a failure below leaves the handle without this map)
    if (&slot != &h->d_shift) h->map_gen++; // (HeldTrajectory::fault: a recorded rollout belongs to the maps it ran under; the shift map is not one of them)
    cur = Desc{};
    if (!M) return EICOS_OK;
    const AffineLayout lay = affine_layout(g, n, MAP_HEADER, gap);
    DevBuf dev;
    HIP_TRY_AS("hipMalloc", dev.alloc(lay.bytes()));
    std::vector<char> image = affine_pack(g, n, lay, dev.p, out);
    std::memcpy(image.data(), M, sizeof *M);
    char *dc = dev.as<char>();
    hipError_t e = hipMemcpy(dc, image.data(), gap ? MAP_HEADER : image.size(), hipMemcpyHostToDevice);
    if (e == hipSuccess && gap) e = hipMemcpy(dc + MAP_HEADER + gap, image.data() + MAP_HEADER, image.size() - MAP_HEADER, hipMemcpyHostToDevice);
    if (e != hipSuccess) return fail(EICOS_E_HIP, std::string("hipMemcpy of the ") + name + " map: " + hipGetErrorString(e));
    slot = std::move(dev); cur = *M;
    return EICOS_OK;
}

extern "C" {

const char *eicos_last_error(void) { return g_err.c_str(); }

int eicos_set_arithmetic_profile(int profile) {
    if (profile != 0 && profile != 1) return fail(EICOS_E_INVALID, "arithmetic profile must be 0 or 1");
    g_arith_profile.store(profile);
    return EICOS_OK;
}
int eicos_get_arithmetic_profile(void) { return g_arith_profile.load(); }

int eicos_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

// The dense apex (symbolic.hpp) keeps an image of its block in LDS.  Whether that costs the launch a resident workgroup per CU is only
// known from the launch shape.  So: plan and shape with the apex; plan and shape once more without it when the apex cannot run (128
// threads without the LDS-resident build) or when the batch is one that would run one more workgroup per CU than came out, and keep
// the shape with more workgroups per CU (MPC02 on 256 CUs: batches 513 ... 768 run three per CU without the apex, two with it:
// launch_blocks_per_cu).  Only the kept plan is allocated.
int eicos_batch_create(int n, int m, int p, int l, int ncones, const int *q,
                       const int *Gjc, const int *Gir, const int *Ajc, const int *Air,
                       int batch, int device, eicos_batch **out) {
    if (!out) return fail(EICOS_E_INVALID, "out is NULL");
    *out = nullptr;
    // pattern intake: argument checks, then the device, then the CSC checks -- a machine without a GPU answers EICOS_E_NOGPU in between
    int rc = check_pattern_args(n, m, p, l, ncones, q, Gjc, Gir, Ajc, Air, batch);
    if (rc != EICOS_OK) return rc;
    {
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
            return fail(EICOS_E_NOGPU, "no HIP device visible: the solver has no CPU fallback");
        if (device < 0) { if (hipGetDevice(&device) != hipSuccess) device = 0; }
        if (device >= ndev) return fail(EICOS_E_INVALID, "device index out of range");
    }
    ProblemPattern P;
    if ((rc = take_csc(n, m, p, ncones, q, Gjc, Gir, Ajc, Air, P)) != EICOS_OK) return rc;
    const int profile = g_arith_profile.load();
    int n_cu = 256;
    { hipDeviceProp_t pr; if (hipGetDeviceProperties(&pr, device) == hipSuccess) n_cu = pr.multiProcessorCount; }
    Analyses A;
    if ((rc = analyse(P, batch, n_cu, profile, A)) != EICOS_OK) return rc;
    Plan with, without;
    Shape sw, so;
    if ((rc = build_plan(P, A, A.apex, batch, n_cu, profile, with)) != EICOS_OK) return rc;
    if ((rc = launch_shape(with, batch, device, sw)) != EICOS_OK) return rc;
    const bool try_without = with.apex && (sw.apex_unplaced || launch_blocks_per_cu(batch, n_cu, sw.bpc + 1, with.threads) > sw.bpc);
    if (!try_without) return allocate(std::move(P), with, sw, batch, device, n_cu, profile, out);
    rc = build_plan(P, A, false, batch, n_cu, profile, without);
    if (rc == EICOS_OK) rc = launch_shape(without, batch, device, so);
    if (sw.apex_unplaced) return rc != EICOS_OK ? rc : allocate(std::move(P), without, so, batch, device, n_cu, profile, out);
    const bool take_without = rc == EICOS_OK && so.bpc > sw.bpc; // (a plan without the apex that fails keeps the one with it)
    return take_without ? allocate(std::move(P), without, so, batch, device, n_cu, profile, out)
                        : allocate(std::move(P), with, sw, batch, device, n_cu, profile, out);
}

// ---- single-instance surface: a batch of one (reference include/eicos.hpp:151-163, test/ecos.h:11-34)
int eicos_create(int n, int m, int p, int l, int ncones, const int *q, const double *Gpr, const int *Gjc, const int *Gir,
                 const double *Apr, const int *Ajc, const int *Air, const double *c, const double *h, const double *b,
                 int device, eicos_batch **out) {
    if (!out) return fail(EICOS_E_INVALID, "out is NULL");
    const bool haveG = Gpr && Gjc && Gir, haveA = Apr && Ajc && Air; // NULL groups as in src/eicos.cpp:103-117
    if (n > 0 && !c) return fail(EICOS_E_INVALID, "c is NULL");
    eicos_batch *hd = nullptr;
    (void)l; // ignored exactly as by the reference's constructor (src/eicos.cpp:91): derived as m - sum(q)
    int rc = eicos_batch_create(n, m, p, -1, ncones, q, haveG ? Gjc : nullptr, haveG ? Gir : nullptr,
                                haveA ? Ajc : nullptr, haveA ? Air : nullptr, 1, device, &hd);
    if (rc != EICOS_OK) return rc;
    rc = eicos_batch_update(hd, 0, 1, haveG ? Gpr : nullptr, haveA ? Apr : nullptr, c, haveG ? h : nullptr, haveA ? b : nullptr);
    if (rc != EICOS_OK) { eicos_batch_destroy(hd); return rc; }
    *out = hd;
    return EICOS_OK;
}
int eicos_update(eicos_batch *hd, const double *Gpr, const double *Apr, const double *c, const double *h, const double *b) {
    return eicos_batch_update(hd, 0, 1, Gpr, Apr, c, h, b);
}
int eicos_solve(eicos_batch *hd, int *exitcode) {
    if (hd && hd->batch != 1) return fail(EICOS_E_INVALID, "eicos_solve needs a handle made by eicos_create (batch of one)");
    return eicos_batch_solve(hd, exitcode);
}
int eicos_solution(eicos_batch *hd, double *x) { return eicos_batch_solution(hd, x); }
int eicos_info_get(eicos_batch *hd, eicos_info *info) { return eicos_batch_info(hd, info); }
int eicos_destroy(eicos_batch *hd) { return eicos_batch_destroy(hd); }

int eicos_batch_destroy(eicos_batch *h) {
    if (!h) return EICOS_OK;
    (void)hipSetDevice(h->device);
    // in-flight work may sit on a caller stream (eicos_batch_set_stream): wait for it before the slabs go away
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    if (h->own_stream) (void)hipStreamSynchronize(h->own_stream);
    // the constant-memory descriptor slot is handed out again only after nothing can read it any more
    if (h->pslot >= 0) { std::lock_guard<std::mutex> lk(g_slot_mu); g_slot_used[h->device][h->pslot] = 0; }
    delete h; // (~eicos_batch: events and stream, then every buffer)
    return EICOS_OK;
}

int eicos_batch_set_warm_start(eicos_batch *h, double shift) {
    if (!h || !(shift >= 0.)) return fail(EICOS_E_INVALID, "bad argument");
    h->warm_shift = shift;
    return EICOS_OK;
}

int eicos_batch_set_dynamic_regularization(eicos_batch *h, double delta, double eps) {
    if (!h || !(delta >= 0.) || !(eps >= 0.)) return fail(EICOS_E_INVALID, "bad argument");
    h->dyn_delta = delta; h->dyn_eps = eps;
    return EICOS_OK;
}

// ---- runtime settings (include/eicos_amd.h: eicos_settings).  SolveCfg (launch.hpp) is the same ten fields in the same order.
static_assert(sizeof(eicos_settings) == sizeof(SolveCfg), "eicos_settings and SolveCfg mirror each other");
void eicos_settings_default(eicos_settings *out) {
    if (!out) return;
    const SolveCfg d = solve_cfg_default();
    *out = eicos_settings{d.feastol, d.abstol, d.reltol, d.feastol_inacc, d.abstol_inacc, d.reltol_inacc, d.linsysacc, d.irerrfact, d.iter_max, d.nitref};
}
size_t eicos_settings_size(void) { return sizeof(eicos_settings); }

// NULL when `s` is acceptable, else the message naming the refused field
static const char *settings_fault(const eicos_settings &s, std::string &msg) {
    const struct { const char *name; double v; } pos[] = {
        {"feastol", s.feastol}, {"abstol", s.abstol}, {"reltol", s.reltol}, {"feastol_inacc", s.feastol_inacc},
        {"abstol_inacc", s.abstol_inacc}, {"reltol_inacc", s.reltol_inacc}, {"linsysacc", s.linsysacc}, {"irerrfact", s.irerrfact}};
    for (const auto &f : pos)
        if (!(std::isfinite(f.v) && f.v > 0.)) { msg = std::string("settings: ") + f.name + " must be finite and positive"; return msg.c_str(); }
    // (the per-pass trace rows -- DevPat::w_trace, eicos_debug_trace's out[102][12] -- are sized for 100 passes, and only pass 0 creates the
    // best iterate that the iteration-cap exit may restore; nothing in the KKT solve is sized by nitref: 100 bounds the loop, no more)
    if (s.iter_max < 1 || s.iter_max > 100) { msg = "settings: iter_max must lie in [1, 100]"; return msg.c_str(); }
    if (s.nitref < 0 || s.nitref > 100) { msg = "settings: nitref must lie in [0, 100]"; return msg.c_str(); }
    return nullptr;
}

int eicos_batch_set_settings(eicos_batch *h, const eicos_settings *s) {
    if (!h) return fail(EICOS_E_INVALID, "NULL handle");
    if (!s) return fail(EICOS_E_INVALID, "settings: NULL struct");
    std::string msg;
    if (settings_fault(*s, msg)) return fail(EICOS_E_INVALID, msg);
    h->cfg = SolveCfg{s->feastol, s->abstol, s->reltol, s->feastol_inacc, s->abstol_inacc, s->reltol_inacc, s->linsysacc, s->irerrfact, s->iter_max, s->nitref};
    return EICOS_OK;
}

int eicos_batch_get_settings(eicos_batch *h, eicos_settings *out) {
    if (!h) return fail(EICOS_E_INVALID, "NULL handle");
    if (!out) return fail(EICOS_E_INVALID, "settings: NULL struct");
    const SolveCfg &c = h->cfg;
    *out = eicos_settings{c.feastol, c.abstol, c.reltol, c.feastol_inacc, c.abstol_inacc, c.reltol_inacc, c.linsysacc, c.irerrfact, c.iter_max, c.nitref};
    return EICOS_OK;
}

// ---- retry policy (include/eicos_amd.h: eicos_retry; launch.hpp: RetryDev) ----
static_assert(sizeof(RetryDev) <= MAP_HEADER, "the retry record larger than its header");
static eicos_settings settings_from(const SolveCfg &c) {
    return eicos_settings{c.feastol, c.abstol, c.reltol, c.feastol_inacc, c.abstol_inacc, c.reltol_inacc, c.linsysacc, c.irerrfact, c.iter_max, c.nitref};
}
void eicos_retry_default(eicos_retry *out) {
    if (!out) return;
    *out = eicos_retry{0u, 0., 0., 0., settings_from(solve_cfg_default())};
}
size_t eicos_retry_size(void) { return sizeof(eicos_retry); }

// the counters of the handle's retry record, behind its header
static int *retry_counts_dev(const eicos_batch *h) { return reinterpret_cast<int *>(h->d_retry.as<char>() + MAP_HEADER); }

int eicos_batch_set_retry(eicos_batch *h, const eicos_retry *r) {
    if (!h) return fail(EICOS_E_INVALID, "NULL handle");
    RetryDev next{0u, 0., 0., 0., solve_cfg_default(), h->retry.counts};
    if (r && r->mask != 0) {
        if (r->mask & ~(unsigned)EICOS_SEL_ALL) return fail(EICOS_E_INVALID, "retry: mask has bits above bit 11 (EICOS_SEL_UNSOLVED)");
        // (beside other classes the bit is idle and accepted: EICOS_SEL_NOT_OPTIMAL, the mask of most policies, holds it)
        if (r->mask == EICOS_SEL_UNSOLVED) return fail(EICOS_E_INVALID, "retry: mask is EICOS_SEL_UNSOLVED alone, and an attempted instance is never in that class");
        if (!(r->warm >= 0.)) return fail(EICOS_E_INVALID, "retry: warm must be >= 0");
        if (!(r->dyn_delta >= 0.) || !(r->dyn_eps >= 0.)) return fail(EICOS_E_INVALID, "retry: dyn_delta and dyn_eps must be >= 0");
        std::string msg;
        if (settings_fault(r->settings, msg)) return fail(EICOS_E_INVALID, "retry: " + msg);
        const eicos_settings &s = r->settings;
        next.mask = r->mask; next.warm = r->warm; next.dyn_delta = r->dyn_delta; next.dyn_eps = r->dyn_eps;
        next.cfg = SolveCfg{s.feastol, s.abstol, s.reltol, s.feastol_inacc, s.abstol_inacc, s.reltol_inacc, s.linsysacc, s.irerrfact, s.iter_max, s.nitref};
    }
    if (next.mask == 0 && !h->d_retry) { h->retry = next; return EICOS_OK; } // (no policy before, none now: nothing on the GPU)
    HIP_TRY(hipSetDevice(h->device));
    if (!h->d_retry) { // the first policy of the handle: the record and the counters, zeroed
        DevBuf dev;
        HIP_TRY_AS("hipMalloc", dev.alloc(MAP_HEADER + (size_t)h->batch * sizeof(int)));
        HIP_TRY(hipMemsetAsync(dev.p, 0, dev.bytes, h->stream));
        h->d_retry = std::move(dev);
        next.counts = retry_counts_dev(h);
    }
    // (on the handle's stream, behind every launch that is enqueued: those keep the record they were enqueued with; a launch enqueued
    // while the mask is 0 does not carry the record's address at all)
    h->retry = next;
    HIP_TRY(hipMemcpyAsync(h->d_retry.p, &h->retry, sizeof(RetryDev), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream)); // (the source is a member: the copy has left it when the call returns)
    return EICOS_OK;
}

int eicos_batch_get_retry(eicos_batch *h, eicos_retry *out) {
    if (!h) return fail(EICOS_E_INVALID, "NULL handle");
    if (!out) return fail(EICOS_E_INVALID, "retry: NULL struct");
    const RetryDev &r = h->retry;
    *out = eicos_retry{r.mask, r.warm, r.dyn_delta, r.dyn_eps, settings_from(r.cfg)};
    return EICOS_OK;
}

int eicos_batch_retry_counts(eicos_batch *h, int first, int count, int *retries, int reset) {
    if (!h) return fail(EICOS_E_INVALID, "NULL handle");
    if (first < 0 || count < 0 || first > h->batch - count) return fail(EICOS_E_INVALID, "retry counts: instance range out of bounds");
    if (count > 0 && !retries) return fail(EICOS_E_INVALID, "retry counts: retries is NULL");
    if (count == 0) return EICOS_OK;
    if (!h->d_retry) { std::fill(retries, retries + count, 0); return EICOS_OK; } // (never had a policy: nothing was retried)
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream));
    HIP_TRY(hipMemcpy(retries, retry_counts_dev(h) + first, (size_t)count * sizeof(int), hipMemcpyDeviceToHost));
    if (reset) {
        HIP_TRY(hipMemsetAsync(retry_counts_dev(h) + first, 0, (size_t)count * sizeof(int), h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
    }
    return EICOS_OK;
}

int eicos_batch_set_stream(eicos_batch *h, void *hip_stream) {
    if (!h) return fail(EICOS_E_INVALID, "NULL handle");
    h->stream = hip_stream ? (hipStream_t)hip_stream : h->own_stream;
    return EICOS_OK;
}

// the next event pair of a timing ring (created on first use) becomes the handle's current pair
static int next_events(hipEvent_t (*ring)[2], long &count, hipEvent_t &e0, hipEvent_t &e1) {
    hipEvent_t *slot = ring[count % eicos_batch::EV_RING];
    for (int i = 0; i < 2; i++) if (!slot[i]) HIP_TRY(hipEventCreate(&slot[i]));
    e0 = slot[0]; e1 = slot[1]; count++;
    return EICOS_OK;
}
// One updateData call = one pair of the update ring: ev_u0, the call's kernels, ev_u1 on the handle's stream.  The public entry points and
// the chunk loops wrap their whole body in this pair; the function that launches the kernel for a row range (launch_range) records nothing.
static int begin_update_timing(eicos_batch *h) {
    int rc = next_events(h->ring_u, h->n_update_rec, h->ev_u0, h->ev_u1);
    if (rc != EICOS_OK) return rc;
    HIP_TRY(hipEventRecord(h->ev_u0, h->stream));
    return EICOS_OK;
}
// rc: what the body between the two gave (a failed call records no end and leaves update_timed as it was)
static int end_update_timing(eicos_batch *h, int rc) {
    if (rc != EICOS_OK) return rc;
    HIP_TRY(hipEventRecord(h->ev_u1, h->stream));
    h->update_timed = true;
    return EICOS_OK;
}

// ---- host memory helpers -------------------------------------------------------------------------------------------------
// (the host's own copies -- stream_copy, the copy pool -- are host_copy.hpp; what follows asks the runtime)
namespace {
// What kind of memory the extent [p, p + bytes) is -- the one place that asks the runtime:
//   MEM_DEVICE  : the first byte is device memory
//   MEM_PINNED  : the WHOLE extent is host memory the GPU addresses directly (hipHostMalloc / hipHostRegister / eicos_host_alloc): kernels read
//                 or write it in place over PCIe and no bounce copy is needed
//   MEM_PAGEABLE: everything else (managed memory is host-addressable: it takes the bounce path like pageable memory), partly pinned extents included
// The kernels read (updateData) or the copy engine writes (results) every byte of a pinned extent in place, so the first byte alone does not
// decide: a pointer into a registered buffer with a count that runs past its end, or a buffer registered a second time with a larger size
// (hipHostRegister reports "already registered" and maps nothing new), would be a GPU page fault instead of an error code.  First byte,
// last byte and one probe per 2 MB in between (a lookup costs about a microsecond).
enum MemKind { MEM_PAGEABLE = 0, MEM_PINNED = 1, MEM_DEVICE = 2 };
MemKind memory_kind(const void *p, size_t bytes) {
    auto probe = [](const void *q) {
        hipPointerAttribute_t a;
        if (hipPointerGetAttributes(&a, q) != hipSuccess) { (void)hipGetLastError(); return MEM_PAGEABLE; } // (plain malloc memory: "invalid value")
        if (a.type == hipMemoryTypeHost) return MEM_PINNED;
        return (a.type == hipMemoryTypeDevice || a.type == hipMemoryTypeArray) ? MEM_DEVICE : MEM_PAGEABLE;
    };
    if (!p) return MEM_PAGEABLE;
    const MemKind first = probe(p);
    if (first != MEM_PINNED || bytes <= 1) return first;
    const char *b = (const char *)p;
    if (probe(b + bytes - 1) != MEM_PINNED) return MEM_PAGEABLE;
    for (size_t o = 2u << 20; o < bytes - 1; o += 2u << 20) if (probe(b + o) != MEM_PINNED) return MEM_PAGEABLE;
    return MEM_PINNED;
}
// The policy of a call's arrays (call_arrays.hpp; beside DeviceMem and PinnedMem, above): where an array lives, and the two copies
struct StageMem : HipPolicy {
    static bool on_device(const void *p) { return memory_kind(p, 1) == MEM_DEVICE; }
    static hipError_t to_device(void *dst, const void *src, size_t bytes, hipStream_t s) { return hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, s); }
    static hipError_t to_host(void *dst, const void *src, size_t bytes, hipStream_t s) { return hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, s); }
};
using Arrays = CallArrays<StageMem>;
// the handle's two pinned bounce buffers hold at least `doubles` each
int ensure_pin(eicos_batch *h, size_t doubles) {
    for (PinSlot &s : h->pin) HIP_TRY_AS("hipHostMalloc", s.reserve(doubles * sizeof(double)));
    return EICOS_OK;
}
} // namespace

void *eicos_host_alloc(size_t bytes) {
    void *p = nullptr;
    if (hipHostMalloc(&p, bytes ? bytes : 8, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); g_err = "hipHostMalloc failed"; return nullptr; }
    return p;
}
int eicos_host_free(void *p) {
    if (!p) return EICOS_OK;
    HIP_TRY(hipHostFree(p));
    return EICOS_OK;
}
// Pin arrays the caller already owns (std::vector storage, numpy arrays, ...) IN PLACE: hipHostRegister.  From then on updateData / solution
// treat them like eicos_host_alloc memory (no bounce copy).  Registering costs about as much as a few bounce copies of the same
// bytes, so it pays for arrays that are reused across calls -- the sample-by-sample rewrite of an MPC loop; the caller unregisters
// before freeing them.
int eicos_host_register(void *p, size_t bytes) {
    if (!p || bytes == 0) return fail(EICOS_E_INVALID, "bad argument");
    const hipError_t e = hipHostRegister(p, bytes, hipHostRegisterDefault);
    if (e == hipErrorHostMemoryAlreadyRegistered) { // fine only if the existing registration covers the whole range asked for
        (void)hipGetLastError();
        if (memory_kind(p, bytes) == MEM_PINNED) return EICOS_OK;
        return fail(EICOS_E_INVALID, "eicos_host_register: the pointer is already registered with a SMALLER extent (unregister it first)");
    }
    if (e != hipSuccess) return fail(EICOS_E_HIP, std::string("hipHostRegister: ") + hipGetErrorString(e));
    return EICOS_OK;
}
int eicos_host_unregister(void *p) {
    if (!p) return EICOS_OK;
    const hipError_t e = hipHostUnregister(p);
    if (e != hipSuccess) { (void)hipGetLastError(); return fail(EICOS_E_HIP, std::string("hipHostUnregister: ") + hipGetErrorString(e)); }
    return EICOS_OK;
}

// ---- updateData: one description of a call's inputs ----------------------------------------------------------------------
// Everything an updateData call is given, validated once (take_inputs): the five groups as the kernels read them, their widths, and --
// for the entry points that decide by it -- what kind of memory each given array is.  Whoever holds one needs to know neither the
// h / b rule nor the widths nor how kinds are found.
namespace {
struct UpdateInputs {
    eicos_batch *h;
    int first, count;
    bool rhs;             // the right-hand-side-only update (G, A not given)
    bool param;           // the parametric update (take_theta): the ONE given group is theta, [count][k], in the slot of c
    const double *src[5]; // G, A, c, h, b, rows of `count` instances; NULL keeps the group
    size_t w[5];          // doubles per instance
    MemKind kind[5];      // of the arrays that hold data, when the entry point asked for kinds
    size_t per;           // doubles per instance over the given groups
    bool iterate = false; // a starting point (take_iterate): the groups are x, y, z, s in the slots of G, A, c, h
    const int *ids = nullptr; // the index-list forms (eicos_batch_*_indexed): `count` ids in device memory -- row q of the arrays belongs to
                              // instance ids[q], first = 0 counts positions of the list; NULL: the range [first, first + count)
    bool detect = false;  // eicos_batch_update_device: arrays in the GPU's own memory, where reading row 0 once more per instance is an L2 hit (pinned host
                          // rows and another GPU's would cross the link twice) -- its launch may set the shared-values word
    bool holds_data(int k) const { return src[k] && w[k]; }
    // the arrays of `rows` instances packed into a staging area (chunk_plan.hpp): every given array has a place, one of no width too
    PackedChunk packed(size_t rows) const {
        const bool given[5] = {src[0] != nullptr, src[1] != nullptr, src[2] != nullptr, src[3] != nullptr, src[4] != nullptr};
        return pack_chunk(w, given, rows, ChunkPad::Gap8);
    }
    bool any(MemKind m) const { for (int k = 0; k < 5; k++) if (holds_data(k) && kind[k] == m) return true; return false; }
    bool all(MemKind m) const { for (int k = 0; k < 5; k++) if (holds_data(k) && kind[k] != m) return false; return true; }
};
struct Staging { // where the two staged paths (update_in_chunks) differ
    std::function<int(int k, double *&area)> area;                        // the staging area of chunk k, free to be overwritten
    std::function<int(double *dst, const double *src, size_t bytes)> put; // rows of one array into it
    std::function<int(int k)> launched;                                   // behind chunk k's launch: what orders the reuse of its area
};
} // namespace

// kinds: classify the given arrays (the host entry points and eicos_batch_update_solve; the device and peer forms take the caller's word)
static int take_inputs(UpdateInputs &in, eicos_batch *h, int first, int count, const double *G, const double *A,
                       const double *c, const double *hh, const double *b, bool rhs, bool kinds) {
    if (!h) return fail(EICOS_E_INVALID, "NULL handle");
    if (first < 0 || count < 0 || first + count > h->batch) return fail(EICOS_E_INVALID, "instance range out of bounds");
    const DevPat &D = h->dp;
    if (G && !hh && D.m > 0) return fail(EICOS_E_INVALID, "Gpr given without h");
    if (A && !b && D.p > 0) return fail(EICOS_E_INVALID, "Apr given without b");
    HIP_TRY(hipSetDevice(h->device));
    // (h is read only with Gpr, b only with Apr: reference src/eicos.cpp:2053-2074; the right-hand-side-only update reads them on their own)
    in = UpdateInputs{h, first, count, rhs, false, {G, A, c, (G || rhs) ? hh : nullptr, (A || rhs) ? b : nullptr},
                      {(size_t)D.nnzG, (size_t)D.nnzA, (size_t)D.n, (size_t)D.m, (size_t)D.p}, {}, 0};
    for (int k = 0; k < 5; k++) {
        if (in.src[k]) in.per += in.w[k];
        if (kinds && in.holds_data(k)) in.kind[k] = memory_kind(in.src[k], (size_t)count * in.w[k] * sizeof(double));
    }
    return EICOS_OK;
}

// A matrix map (eicos_batch_set_matrix_map) against the parameter map installed NOW -- checked where the map is installed and again by
// every call that consumes theta, because the parameter map can be replaced in between: the same k, and the vector updateData reads with
// a matrix (h with Gpr, b with Apr: take_inputs) mapped too.
static int matrix_map_fits(const eicos_batch *h) {
    if (h->mat.k == 0) return EICOS_OK;
    if (h->mat.k != h->param.k)
        return fail(EICOS_E_INVALID, "matrix map: installed for k = " + std::to_string(h->mat.k) + ", the parameter map now installed has k = " +
                                         std::to_string(h->param.k) + ": install it again");
    if (h->mat.g[0].base && h->dp.m > 0 && !h->param.g[1].base)
        return fail(EICOS_E_INVALID, "matrix map of G: the parameter map has no h group (updateData reads h with Gpr)");
    if (h->mat.g[1].base && h->dp.p > 0 && !h->param.g[2].base)
        return fail(EICOS_E_INVALID, "matrix map of A: the parameter map has no b group (updateData reads b with Apr)");
    return EICOS_OK;
}

// The inputs of a parametric update (eicos_batch_update_param*): one more kind of UpdateInputs -- a single group, theta, `k` doubles per
// instance -- so that the rows travel over the very paths of the other updates (bounce, pinned in place, device, peer in place / staged).
static int take_theta(UpdateInputs &in, eicos_batch *h, int first, int count, const double *theta, bool kinds) {
    if (!h) return fail(EICOS_E_INVALID, "NULL handle");
    if (h->param.k == 0) return fail(EICOS_E_INVALID, "no parameter map (eicos_batch_set_param_map installs one)");
    if (first < 0 || count < 0 || first + count > h->batch) return fail(EICOS_E_INVALID, "instance range out of bounds");
    if (!theta) return fail(EICOS_E_INVALID, "theta is NULL");
    { const int rc = matrix_map_fits(h); if (rc != EICOS_OK) return rc; }
    HIP_TRY(hipSetDevice(h->device));
    const size_t k = (size_t)h->param.k;
    in = UpdateInputs{h, first, count, false, true, {nullptr, nullptr, theta, nullptr, nullptr}, {0, 0, k, 0, 0}, {}, k};
    if (kinds) in.kind[2] = memory_kind(theta, (size_t)count * k * sizeof(double));
    return EICOS_OK;
}

// the updateData kernel (full, right-hand-side-only -- kernels.hip: rhs_instance -- or parametric: k_update_param_range) of rows [first, first + count) on five pointers the GPU addresses
// The parametric update of instances [first, first + count) from rows of theta the GPU addresses, on the handle's stream.  Without a
// matrix map: the right-hand-side kernel.  With one the update is a FULL updateData whose inputs are formed on the GPU: chunk by chunk,
// the mapped groups [Gpr | Apr | c | h | b] are expanded into the handle's device staging buffer (launch_expand_affine; h only with G, b
// only with A, as updateData reads them) and the unchanged launch_update runs on those pointers -- stream order keeps a chunk's expansion
// behind the previous chunk's updateData; the buffer grows on demand up to MSTAGE_CAP_MB.  A vector mapped without its matrix then goes
// through the right-hand-side kernel, which divides by the scalings that updateData has just stored.
// The shared-values word (eicos_batch::d_shared), on the handle's stream.  shared_clear: in front of every launch that writes matrix values
// of any instance and is not the detecting one.  shared_detect: in front of the ONE launch that may leave it set.
static int shared_clear(eicos_batch *h) {
    if (!h->shared_maybe) return EICOS_OK;
    HIP_TRY(hipMemsetAsync(h->d_shared.p, 0xFF, sizeof(int), h->stream));
    h->shared_maybe = false;
    return EICOS_OK;
}
static int shared_detect(eicos_batch *h) {
    HIP_TRY(hipMemsetAsync(h->d_shared.p, 0, sizeof(int), h->stream));
    h->shared_maybe = true;
    return EICOS_OK;
}

static constexpr int MSTAGE_CAP_MB = 64; // (EICOS_MATRIX_STAGE_MB under EICOS_EXPERIMENT=1: tests reach several chunks with a small batch)
// list != NULL (UpdateInputs::ids + the position the rows start at): row q belongs to instance list[q] and `first` is unused.
static int param_range(eicos_batch *h, int first, int count, const double *theta, const int *list) {
    const DevPat &D = h->dp;
    const ParamMapDev &M = h->param;
    if (h->mat.k == 0) {
        const int width = (M.g[0].base ? D.n : 0) + (M.g[1].base ? D.m : 0) + (M.g[2].base ? D.p : 0);
        HIP_TRY(launch_update_param(h->pslot, h->inst(), first, count, M, theta, width, h->stream, list));
        return EICOS_OK;
    }
    if (count == 0) return EICOS_OK;
    { const int rc = shared_clear(h); if (rc != EICOS_OK) return rc; } // (every instance gets matrices of its own theta)
    const bool mG = h->mat.g[0].base != nullptr, mA = h->mat.g[1].base != nullptr;
    const AffineDev *src[5] = {mG ? &h->mat.g[0] : nullptr, mA ? &h->mat.g[1] : nullptr, M.g[0].base ? &M.g[0] : nullptr,
                               mG && D.m > 0 ? &M.g[1] : nullptr, mA && D.p > 0 ? &M.g[2] : nullptr};
    const size_t w[5] = {(size_t)D.nnzG, (size_t)D.nnzA, (size_t)D.n, (size_t)D.m, (size_t)D.p};
    const bool given[5] = {src[0] != nullptr, src[1] != nullptr, src[2] != nullptr, src[3] != nullptr, src[4] != nullptr};
    const size_t row = matrix_stage_row(w, given);
    const size_t cap = (size_t)env_knob("EICOS_MATRIX_STAGE_MB", MSTAGE_CAP_MB, 1, 4096) * ((1u << 20) / sizeof(double));
    const int chunk = matrix_stage_chunk(row, count, cap);
    HIP_TRY_AS("hipMalloc", h->d_mstage.reserve((size_t)chunk * row * sizeof(double), h->stream));
    for (int o = 0; o < count; o += chunk) {
        const int cnt = std::min(chunk, count - o);
        const PackedChunk pk = pack_chunk(w, given, (size_t)cnt, ChunkPad::RoundUp8); // (every array of a chunk starts 64-byte aligned)
        const double *arr[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
        for (int g = 0; g < 5; g++) {
            if (!src[g]) continue;
            double *at = h->d_mstage.as<double>() + pk.off[g];
            arr[g] = at;
            HIP_TRY(launch_expand_affine(*src[g], (int)w[g], M.k, theta + (size_t)o * M.k, cnt, at, h->stream));
        }
        HIP_TRY(launch_update(h->pslot, h->inst(), first + o, cnt, arr[0], arr[1], arr[2], arr[3], arr[4], h->d_scratch.as<double>(), std::min(cnt, h->upd_grid),
                              h->upd_lds, h->upd_vals_lds, h->stream, nullptr, list ? list + o : nullptr));
    }
    ParamMapDev rest{};
    rest.k = M.k;
    if (!mG) rest.g[1] = M.g[1];
    if (!mA) rest.g[2] = M.g[2];
    const int width = (rest.g[1].base ? D.m : 0) + (rest.g[2].base ? D.p : 0);
    HIP_TRY(launch_update_param(h->pslot, h->inst(), first, count, rest, theta, width, h->stream, list));
    return EICOS_OK;
}

// in_place: the launch reads the caller's own arrays (update_in_place) -- with UpdateInputs::detect, the whole batch and every matrix the
// pattern has among them it is the launch that compares every row of Gpr / Apr with row 0 (launch.hpp: launch_update)
static int launch_range(const UpdateInputs &in, int first, int count, const double *const p[5], bool in_place = false) {
    eicos_batch *h = in.h;
    const int *list = in.ids ? in.ids + first : nullptr; // (an index list: `first` is the position in it the rows start at)
    if (in.iterate) HIP_TRY(launch_set_iterate(h->pslot, h->inst(), first, count, p[0], p[1], p[2], p[3], (int)in.per, h->stream, list));
    else if (in.param) {
        const int rc = param_range(h, first, count, p[2], list);
        if (rc != EICOS_OK) return rc;
    } else if (in.rhs) HIP_TRY(launch_update_rhs(h->pslot, h->inst(), first, count, p[2], p[3], p[4], (int)in.per, h->stream, list));
    else {
        const DevPat &D = h->dp;
        const bool detect = in_place && in.detect && !list && h->shared_on && first == 0 && count == h->batch && D.nnzG + D.nnzA > 0 &&
                            (p[0] || D.nnzG == 0) && (p[1] || D.nnzA == 0);
        const int rc = detect ? shared_detect(h) : (count > 0 ? shared_clear(h) : EICOS_OK);
        if (rc != EICOS_OK) return rc;
        HIP_TRY(launch_update(h->pslot, h->inst(), first, count, p[0], p[1], p[2], p[3], p[4], h->d_scratch.as<double>(), std::min(count, h->upd_grid), h->upd_lds, h->upd_vals_lds, h->stream,
                              detect ? h->d_shared.as<int>() : nullptr, list));
        // (the one launch that may leave the word at 0: the shared factor operands follow it on the stream, from instance 0's fresh values)
        if (detect && h->d_shop) HIP_TRY(launch_shared_operands(h->pslot, h->inst(), h->d_shop.as<double>(), const_cast<double *>(D.ub0), h->stream));
    }
    return EICOS_OK;
}

// one launch on the caller's pointers; path > 0 is left as the witness of eicos_batch_last_update_path
static int update_in_place(const UpdateInputs &in, int path) {
    if (path) in.h->last_update_path = path;
    int rc = begin_update_timing(in.h);
    if (rc == EICOS_OK) rc = launch_range(in, in.first, in.count, in.src, true);
    return end_update_timing(in.h, rc);
}

// The two staged paths: rows travel in chunks of `chunk` instances through a staging area the GPU addresses, the given arrays of a chunk
// packed behind each other (UpdateInputs::packed: 8 doubles between two arrays, which keeps them on lines of their own but aligns only
// the first to 64 bytes), one launch per chunk on the packed pointers; an area holds staging_doubles(in.per, chunk) (chunk_plan.hpp).
static int update_in_chunks(const UpdateInputs &in, int chunk, const Staging &st) {
    int rc = begin_update_timing(in.h), k = 0;
    for (int o = 0; o < in.count && rc == EICOS_OK; o += chunk, k++) {
        const int cnt = std::min(chunk, in.count - o);
        const PackedChunk pk = in.packed((size_t)cnt);
        const double *packed[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
        double *area = nullptr;
        rc = st.area(k, area);
        for (int q = 0; q < 5 && rc == EICOS_OK; q++) {
            if (!in.src[q]) continue;
            packed[q] = area + pk.off[q];
            if (in.w[q]) rc = st.put(area + pk.off[q], in.src[q] + (size_t)o * in.w[q], (size_t)cnt * in.w[q] * sizeof(double));
        }
        if (rc == EICOS_OK) rc = launch_range(in, in.first + o, cnt, packed);
        if (rc == EICOS_OK) rc = st.launched(k);
    }
    return end_update_timing(in.h, rc);
}

//   peer, access on: the kernel reads the other GPU's HBM in place over xGMI (asynchronous, like eicos_batch_update_device)
//   peer, no access: hipMemcpyPeerAsync into a device staging buffer, chunk by chunk
static int peer_update(const UpdateInputs &in, int src_dev) {
    eicos_batch *h = in.h;
    int can = 0;
    if (src_dev == h->device) can = 1;
    else if (hipDeviceCanAccessPeer(&can, h->device, src_dev) != hipSuccess) { (void)hipGetLastError(); can = 0; }
    if (can && src_dev != h->device) {
        const hipError_t e = hipDeviceEnablePeerAccess(src_dev, 0);
        if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) can = 0;
        (void)hipGetLastError();
    }
    if (can && !env_knob("EICOS_PEER_STAGED", 0, 0, 1)) return update_in_place(in, 3);
    // no peer access: staged peer copies, one chunk at a time through the device staging buffer
    h->last_update_path = 4;
    const int chunk = PEER_CHUNK;
    HIP_TRY_AS("hipMalloc", h->d_stage.reserve(staging_doubles(in.per, std::min(in.count, chunk)) * sizeof(double), h->stream));
    Staging st;
    st.area = [&](int, double *&area) -> int { area = h->d_stage.as<double>(); return EICOS_OK; };
    st.put = [&](double *dst, const double *src, size_t bytes) -> int {
        return hipMemcpyPeerAsync(dst, h->device, src, src_dev, bytes, h->stream) == hipSuccess ? EICOS_OK : fail(EICOS_E_HIP, "hipMemcpyPeerAsync failed");
    };
    st.launched = [&](int) -> int { // the staging buffer is reused by the next chunk
        return hipStreamSynchronize(h->stream) == hipSuccess ? EICOS_OK : fail(EICOS_E_HIP, "stream sync failed in update");
    };
    return update_in_chunks(in, chunk, st);
}

//   host, pageable : rows go through the two pinned bounce buffers in chunks -- the host copies chunk k + 1 in (CopyPool) while the
//                    updateData kernel of chunk k reads its inputs straight from the other buffer over PCIe; returns when the last chunk
//                    has been COPIED (the caller's arrays are free again), the kernels are still in flight on the handle's stream
//   host, pinned   : (every given array addressable by the GPU) ONE kernel launch reads the caller's arrays in place; the call
//                    waits for it, so that the caller may overwrite them on return -- the reference's updateData is synchronous too
static int host_update(const UpdateInputs &in) {
    eicos_batch *h = in.h;
    // a device pointer handed to the HOST-pointer entry point must not reach the bounce copy (a host memcpy from it would fault)
    if (in.any(MEM_DEVICE)) return fail(EICOS_E_INVALID, in.iterate ? "eicos_batch_set_iterate takes host pointers: an array lives in device memory (use eicos_batch_set_iterate_device)"
                                                         : in.param ? "eicos_batch_update_param takes a host pointer: theta lives in device memory (use eicos_batch_update_param_device)"
                                                         : in.rhs ? "eicos_batch_update_rhs takes host pointers: an array lives in device memory (use eicos_batch_update_rhs_device)"
                                                                 : "eicos_batch_update takes host pointers: an array lives in device memory (use eicos_batch_update_device)");
    // pinned in place only when EVERY byte the kernel will read is mapped (else the bounce path, which reads with the host's own loads)
    if (in.all(MEM_PINNED) && !env_knob("EICOS_HOST_BOUNCE", 0, 0, 1)) {
        const int rc = update_in_place(in, 2);
        if (rc != EICOS_OK) return rc;
        HIP_TRY(hipStreamSynchronize(h->stream)); // the caller may overwrite its arrays on return
        return EICOS_OK;
    }
    h->last_update_path = 1;
    const int chunk = bounce_in_chunk(in.per, in.count);
    const int rc = ensure_pin(h, staging_doubles(in.per, chunk));
    if (rc != EICOS_OK) return rc;
    CopyPool &pool = CopyPool::get();
    Staging st;
    st.area = [&](int k, double *&area) -> int { // the kernel that read this buffer two chunks ago (or an earlier call's) must have finished
        if (h->pin[k & 1].wait() != hipSuccess) return fail(EICOS_E_HIP, "event sync failed in update");
        area = h->pin[k & 1].as<double>();
        return EICOS_OK;
    };
    st.put = [&](double *dst, const double *src, size_t bytes) -> int { pool.copy(dst, src, bytes); return EICOS_OK; };
    st.launched = [&](int k) -> int { // (the launch reads the pinned buffer in place)
        return h->pin[k & 1].mark(h->stream) == hipSuccess ? EICOS_OK : fail(EICOS_E_HIP, "event record failed in update");
    };
    return update_in_chunks(in, chunk, st);
}

// updateData from buffers that are not in the handle's HBM: host memory (src_dev < 0; `in` with kinds) or the HBM of another GPU
// (src_dev = that device, eicos_multi_update_device), over the paths above.
static int staged_update(const UpdateInputs &in, int src_dev) {
    if (in.count == 0) return EICOS_OK;
    // nothing given: everything is kept -- still a valid updateData (re-equilibrates what is there; the right-hand-side-only one changes nothing)
    if (in.per == 0) return update_in_place(in, 0);
    return src_dev >= 0 ? peer_update(in, src_dev) : host_update(in);
}

int eicos_batch_last_update_path(eicos_batch *h) { return h ? h->last_update_path : fail(EICOS_E_INVALID, "NULL handle"); }

int eicos_batch_update_device(eicos_batch *h, int first, int count, const double *dG, const double *dA,
                              const double *dc, const double *dh, const double *db) {
    UpdateInputs in;
    const int rc = take_inputs(in, h, first, count, dG, dA, dc, dh, db, false, false);
    in.detect = true;
    return rc != EICOS_OK ? rc : update_in_place(in, 0);
}

// right-hand-side-only updateData (kernels.hip: rhs_instance): the given vectors divided by every instance's stored scalings; A, G and the
// equilibration stay as they are
int eicos_batch_update_rhs_device(eicos_batch *h, int first, int count, const double *dc, const double *dh, const double *db) {
    UpdateInputs in;
    const int rc = take_inputs(in, h, first, count, nullptr, nullptr, dc, dh, db, true, false);
    return rc != EICOS_OK ? rc : update_in_place(in, 0);
}

// rhs = 1: the right-hand-side-only update (G, A must be NULL; h and b are read on their own) over the same paths.
int eicos_internal_update_staged(eicos_batch *h, int first, int count, const double *G, const double *A,
                                 const double *c, const double *hh, const double *b, int src_dev, int rhs) {
    UpdateInputs in;
    const int rc = take_inputs(in, h, first, count, G, A, c, hh, b, rhs != 0, src_dev < 0);
    return rc != EICOS_OK ? rc : staged_update(in, src_dev);
}

int eicos_batch_update(eicos_batch *h, int first, int count, const double *G, const double *A,
                       const double *c, const double *hh, const double *b) {
    return eicos_internal_update_staged(h, first, count, G, A, c, hh, b, -1, 0);
}

int eicos_batch_update_rhs(eicos_batch *h, int first, int count, const double *c, const double *hh, const double *b) {
    return eicos_internal_update_staged(h, first, count, nullptr, nullptr, c, hh, b, -1, 1);
}

// ---- a caller-supplied starting point (no reference counterpart) ----
// One more kind of UpdateInputs: up to four groups, x [n], y [p], z [m], s [m] per instance, in the slots of G, A, c, h -- so that the rows
// travel over the very paths of the updates (bounce, pinned in place, device) into k_set_iterate_range, which stores them in the slabs as
// they are and marks the instances warm-startable.
static int take_iterate(UpdateInputs &in, eicos_batch *h, int first, int count, const double *x, const double *y, const double *z,
                        const double *s, bool kinds) {
    if (!h) return fail(EICOS_E_INVALID, "NULL handle");
    if (first < 0 || count < 0 || first + count > h->batch) return fail(EICOS_E_INVALID, "instance range out of bounds");
    if (!x && !y && !z && !s) return fail(EICOS_E_INVALID, "set_iterate: x, y, z and s are all NULL");
    const DevPat &D = h->dp;
    if (y && D.p == 0) return fail(EICOS_E_INVALID, "set_iterate: y given, but the pattern has no equality rows (p = 0)");
    if (z && D.m == 0) return fail(EICOS_E_INVALID, "set_iterate: z given, but the pattern has no cone rows (m = 0)");
    if (s && D.m == 0) return fail(EICOS_E_INVALID, "set_iterate: s given, but the pattern has no cone rows (m = 0)");
    HIP_TRY(hipSetDevice(h->device));
    in = UpdateInputs{h, first, count, false, false, {x, y, z, s, nullptr}, {(size_t)D.n, (size_t)D.p, (size_t)D.m, (size_t)D.m, 0}, {}, 0};
    in.iterate = true;
    for (int k = 0; k < 4; k++) {
        if (in.src[k]) in.per += in.w[k];
        if (kinds && in.holds_data(k)) in.kind[k] = memory_kind(in.src[k], (size_t)count * in.w[k] * sizeof(double));
    }
    return EICOS_OK;
}

// host arrays: pageable through the bounce buffers, pinned / registered read in place; synchronous like eicos_batch_update_rhs
int eicos_batch_set_iterate(eicos_batch *h, int first, int count, const double *x, const double *y, const double *z, const double *s) {
    UpdateInputs in;
    const int rc = take_iterate(in, h, first, count, x, y, z, s, true);
    return rc != EICOS_OK ? rc : staged_update(in, -1);
}

// device arrays: one launch on the handle's stream, asynchronous
int eicos_batch_set_iterate_device(eicos_batch *h, int first, int count, const double *dx, const double *dy, const double *dz, const double *ds) {
    UpdateInputs in;
    const int rc = take_iterate(in, h, first, count, dx, dy, dz, ds, false);
    return rc != EICOS_OK ? rc : update_in_place(in, 0);
}

// ---- parametric right-hand sides: c, h, b affine in a short parameter row theta (an affine map: install_map, above) ----
// The range kernel takes the descriptor by value, the fused
// step reads its device copy through a pointer.  All groups NULL or k = 0 removes the map.
int eicos_batch_set_param_map(eicos_batch *h, int k, const eicos_affine_map *c, const eicos_affine_map *hh, const eicos_affine_map *b) {
    if (!h) return fail(EICOS_E_INVALID, "NULL handle");
    if (k < 0) return fail(EICOS_E_INVALID, "parameter map: k must not be negative");
    const DevPat &D = h->dp;
    const AffineGroup g[3] = {{c, D.n, k, "parameter map of c: ", "[0, k)"}, {hh, D.m, k, "parameter map of h: ", "[0, k)"},
                              {b, D.p, k, "parameter map of b: ", "[0, k)"}};
    const bool remove = k == 0 || (!c && !hh && !b);
    std::string msg;
    for (int q = 0; q < 3 && !remove; q++) {
        if (!g[q].map) continue;
        if (g[q].rows == 0) return fail(EICOS_E_INVALID, g[q].who + "the pattern has no such group (its size is 0)");
        if (affine_fault(g[q], msg)) return fail(EICOS_E_INVALID, msg);
    }
    ParamMapDev M{};
    M.k = k;
    const int rc = install_map(h, h->d_param, h->param, "parameter", g, 3, 0, remove ? nullptr : &M, M.g);
    for (int q = 0; q < 3; q++) h->param_nnz[q] = h->param.g[q].base ? g[q].map->rowptr[g[q].rows] : 0;
    return rc;
}

int eicos_batch_param_count(eicos_batch *h) { return h ? h->param.k : fail(EICOS_E_INVALID, "NULL handle"); }

// theta from buffers that are not in the handle's HBM (host: src_dev < 0; another GPU: eicos_multi_update_param_device)
int eicos_internal_update_param_staged(eicos_batch *h, int first, int count, const double *theta, int src_dev) {
    UpdateInputs in;
    const int rc = take_theta(in, h, first, count, theta, src_dev < 0);
    return rc != EICOS_OK ? rc : staged_update(in, src_dev);
}

int eicos_batch_update_param(eicos_batch *h, int first, int count, const double *theta) {
    return eicos_internal_update_param_staged(h, first, count, theta, -1);
}

int eicos_batch_update_param_device(eicos_batch *h, int first, int count, const double *dtheta) {
    UpdateInputs in;
    const int rc = take_theta(in, h, first, count, dtheta, false);
    return rc != EICOS_OK ? rc : update_in_place(in, 0);
}

// ---- output map: u = u0 + U x, the few numbers of x a controller applies ----
// The allocation keeps the u rows of the batch between the descriptor and the arrays (d_u: what the range kernel fills for a host
// destination).  The range kernel takes the descriptor by value, the fused step through a pointer to its device copy.
int eicos_batch_set_output_map(eicos_batch *h, int r, const eicos_affine_map *u) {
    if (!h) return fail(EICOS_E_INVALID, "NULL handle");
    if (r < 0) return fail(EICOS_E_INVALID, "output map: r must not be negative");
    const AffineGroup g = {u, r, h->dp.n, "output map: ", "[0, n)"};
    const bool remove = r == 0 || !u;
    std::string msg;
    if (!remove) {
        if (h->dp.n == 0) return fail(EICOS_E_INVALID, g.who + "the pattern has no variables (n = 0)");
        if (affine_fault(g, msg)) return fail(EICOS_E_INVALID, msg);
    }
    OutMapDev M{};
    M.r = r;
    const int rc = install_map(h, h->d_out, h->out, "output", &g, 1, (size_t)h->batch * r * sizeof(double), remove ? nullptr : &M, &M.a);
    h->d_u = h->d_out ? reinterpret_cast<double *>(h->d_out.as<char>() + MAP_HEADER) : nullptr;
    h->out_nnz = h->out.r ? u->rowptr[r] : 0;
    return rc;
}

int eicos_batch_output_count(eicos_batch *h) { return h ? h->out.r : fail(EICOS_E_INVALID, "NULL handle"); }

static int fetch_strided(eicos_batch *h, double *dst, const double *src, size_t pitch, int width, int count); // (with the result paths, below)
static int take_output_range(eicos_batch *h, int first, int count, const double *u) {
    if (!h) return fail(EICOS_E_INVALID, "NULL handle");
    if (h->out.r == 0) return fail(EICOS_E_INVALID, "no output map (eicos_batch_set_output_map installs one)");
    if (first < 0 || count < 0 || first + count > h->batch) return fail(EICOS_E_INVALID, "instance range out of bounds");
    if (!u && count > 0) return fail(EICOS_E_INVALID, "u is NULL");
    HIP_TRY(hipSetDevice(h->device));
    return EICOS_OK;
}

// ---- fallback map (eicos_batch_set_fallback_map, with the plant map below): what the steps that hold theta need of it ----
// Every such step checks the map against the maps installed NOW: the parameter or the output map may have been replaced
static int fallback_fits(const eicos_batch *h) {
    if (h->fb.mask == 0 || (h->fb.k == h->param.k && h->fb.r == h->out.r)) return EICOS_OK;
    return fail(EICOS_E_INVALID, "fallback map: installed for (k, r) = (" + std::to_string(h->fb.k) + ", " + std::to_string(h->fb.r) +
                                     "), the maps now installed have (" + std::to_string(h->param.k) + ", " + std::to_string(h->out.r) + "): install it again");
}
// The theta rows [count][k] of a step that is not fused, where launch_fallback can read them: pinned and device memory as it is,
// pageable memory through the handle's device copy (on the handle's stream; the step waits for the stream before it returns)
static int fallback_theta(eicos_batch *h, const double *theta, MemKind kind, int count, const double *&out) {
    out = theta;
    if (kind != MEM_PAGEABLE) return EICOS_OK;
    const size_t bytes = (size_t)count * h->fb.k * sizeof(double);
    HIP_TRY_AS("hipMalloc", h->d_fb_theta.reserve(bytes, h->stream));
    HIP_TRY(hipMemcpyAsync(h->d_fb_theta.p, theta, bytes, hipMemcpyHostToDevice, h->stream));
    out = h->d_fb_theta.as<const double>();
    return EICOS_OK;
}

// the output rows of instances [first, first + count) into `u` [count][r], wherever it lives: device memory is written by the range kernel
// itself (asynchronous), host memory gets the handle's rows d_u over the paths of fetch_strided (synchronous)
// list != NULL (device memory, `count` ids): row q is the output row of instance list[q] and `first` is unused
// fb_theta != NULL (a step under a fallback map whose launch did not write these rows): theta [count][k] the GPU addresses, row q beside
// row q of u -- the fallback kernel follows the output kernel on the same rows (launch.hpp: launch_fallback)
static int outputs_to(eicos_batch *h, int first, int count, double *u, MemKind kind, const int *list = nullptr, const double *fb_theta = nullptr) {
    if (count == 0) return EICOS_OK;
    if (kind == MEM_DEVICE) {
        HIP_TRY(launch_outputs(h->pslot, h->inst(), first, count, h->out, u, h->stream, list));
        if (fb_theta) HIP_TRY(launch_fallback(h->pslot, h->inst(), first, count, h->fb, fb_theta, u, h->stream, list));
        return EICOS_OK;
    }
    double *rows = h->d_u + (list ? 0 : (size_t)first * h->out.r);
    HIP_TRY(launch_outputs(h->pslot, h->inst(), first, count, h->out, rows, h->stream, list));
    if (fb_theta) HIP_TRY(launch_fallback(h->pslot, h->inst(), first, count, h->fb, fb_theta, rows, h->stream, list));
    const int rc = fetch_strided(h, u, rows, (size_t)h->out.r * sizeof(double), h->out.r, count);
    if (rc != EICOS_OK) return rc;
    HIP_TRY(hipStreamSynchronize(h->stream));
    return EICOS_OK;
}

int eicos_batch_outputs(eicos_batch *h, int first, int count, double *u) {
    const int rc = take_output_range(h, first, count, u);
    if (rc != EICOS_OK) return rc;
    if (count > 0 && memory_kind(u, 1) == MEM_DEVICE) return fail(EICOS_E_INVALID, "eicos_batch_outputs takes a host pointer: u lives in device memory (use eicos_batch_outputs_device)");
    HIP_TRY(hipStreamSynchronize(h->stream));
    return outputs_to(h, first, count, u, MEM_PAGEABLE);
}

int eicos_batch_outputs_device(eicos_batch *h, int first, int count, double *du) {
    const int rc = take_output_range(h, first, count, du);
    return rc != EICOS_OK ? rc : outputs_to(h, first, count, du, MEM_DEVICE);
}

// the candidate ids of a subset launch, in device memory behind the launch order
static int *subset_ids(const eicos_batch *h) { return h->queue() + 16 + h->batch; }
// the row map of a step over a subset (launch.hpp: UpdArgs::rows_at), behind the candidates: its place in the queue allocation, in ints
static int subset_rows_at(const eicos_batch *h) { return 16 + 2 * h->batch; }
// the launch record of a handle's solves (launch.hpp); subset >= 0: a launch over the `subset` ids in subset_ids(h) instead of the batch
static SolveLaunch solve_launch(const eicos_batch *h, int subset) {
    SolveLaunch L{};
    L.ps = h->pslot; L.inst = h->inst(); L.work = h->work(); L.B = h->batch; L.queue = h->queue(); L.order = h->queue() + 16;
    L.grid = h->grid; L.threads = h->threads; L.nlds = h->nlds; L.idx16 = h->dp.idx16; L.order_min = h->order_min;
    L.warm = h->warm_shift; L.dyn_delta = h->dyn_delta; L.dyn_eps = h->dyn_eps; L.cfg = h->cfg; L.dyn_lds = h->dyn_lds;
    L.batch = h->batch; L.full_grid = h->grid;
    if (subset >= 0) { L.list = subset_ids(h); L.B = subset; L.grid = std::min(h->grid, subset); }
    return L;
}
// The one place that enqueues k_solve on the handle's stream.  step: the update fused into this launch (update_solve, the rollout), NULL
// for a plain solve; it lives for this call only.  subset >= 0: the launch takes that many chosen instances (solve_launch).
// sens != NULL (the rollout that records its Jacobians): the build's k_roll_sens takes the launch, with that adjoint record.
static int enqueue_solve(eicos_batch *h, const UpdArgs *step, int subset = -1, const AdjointDev *sens = nullptr) {
    HIP_TRY(hipSetDevice(h->device));
    { const int rc = next_events(h->ring_s, h->n_solve_rec, h->ev_s0, h->ev_s1); if (rc != EICOS_OK) return rc; }
    h->ring_step0[(h->n_solve_rec - 1) % eicos_batch::EV_RING] = h->update_timed ? h->ev_u0 : h->ev_s0;
    HIP_TRY(hipEventRecord(h->ev_s0, h->stream));
    UpdArgs args = step ? *step : UpdArgs{};
    // (a shift map and the shared-values word travel with EVERY launch, the ones without a fused update included: instance_begin reads them)
    args.smap = h->d_shift.as<const ShiftMapDev>();
    args.retry = h->retry.mask ? h->d_retry.as<const RetryDev>() : nullptr; // (eicos_batch_set_retry: every launch of the handle, like the shift map)
    if (writes_matrix_values(args)) { const int rc = shared_clear(h); if (rc != EICOS_OK) return rc; } // (the step drops the shared values)
    args.shared = h->shared_on ? h->d_shared.as<int>() : nullptr;
    SolveLaunch L = solve_launch(h, subset);
    if (args.rows_at) L.rows = h->queue() + args.rows_at; // (a step in list order: the selection kernel of this launch fills the row map it reads)
    HIP_TRY(solve_build(h->threads, h->ldsres, h->w2, h->ubl).launch(L, h->stream, args, sens));
    HIP_TRY(hipEventRecord(h->ev_s1, h->stream));
    h->solve_timed = true;
    h->last_subset = subset >= 0; h->last_count = subset >= 0 ? subset : h->batch;
    h->last_ordered = h->last_subset || h->batch > h->order_min; // (a subset launch always goes through the order array)
    return EICOS_OK;
}

int eicos_batch_solve_async(eicos_batch *h) { return h ? enqueue_solve(h, nullptr) : fail(EICOS_E_INVALID, "NULL handle"); }

int eicos_batch_sync(eicos_batch *h) {
    if (!h) return fail(EICOS_E_INVALID, "NULL handle");
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return EICOS_OK;
}

// rows [off, off + width) of every instance slab -> dst[batch][width] on the host.  Pinned destination: one strided device-to-host copy
// straight into it.  Pageable destination: chunks through the two pinned bounce buffers, the copy of chunk k + 1 in flight while the
// host copies chunk k out (a strided hipMemcpy2D into pageable memory is staged by the runtime row by row).
// fetch_strided: `count` rows of `width` doubles, `pitch` bytes apart in device memory at src (the output rows of eicos_batch_outputs too).
static int fetch_strided(eicos_batch *h, double *dst, const double *src, size_t pitch, int width, int count) {
    if (!dst || width == 0 || count == 0) return EICOS_OK;
    const size_t wb = (size_t)width * sizeof(double), stride = pitch / sizeof(double);
    // (a small result takes the one strided copy as well, unless it starts in pinned memory that ends before it does)
    if (memory_kind(dst, (size_t)count * wb) == MEM_PINNED || (small_result((size_t)count * wb) && memory_kind(dst, 1) != MEM_PINNED)) {
        HIP_TRY(hipMemcpy2DAsync(dst, wb, src, pitch, wb, (size_t)count, hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
        return EICOS_OK;
    }
    const int chunk = bounce_out_chunk(wb, count);
    int rc = ensure_pin(h, (size_t)chunk * width);
    if (rc != EICOS_OK) return rc;
    for (PinSlot &s : h->pin) HIP_TRY_AS("hipEventSynchronize", s.wait());
    CopyPool &pool = CopyPool::get();
    auto issue = [&](int o, int bi) -> int {
        const int cnt = std::min(chunk, count - o);
        HIP_TRY(hipMemcpy2DAsync(h->pin[bi].as<void>(), wb, src + (size_t)o * stride, pitch, wb, (size_t)cnt, hipMemcpyDeviceToHost, h->stream));
        HIP_TRY_AS("hipEventRecord", h->pin[bi].mark(h->stream));
        return EICOS_OK;
    };
    rc = issue(0, 0);
    int k = 0;
    for (int o = 0; o < count && rc == EICOS_OK; o += chunk, k++) {
        const int cnt = std::min(chunk, count - o), bi = k & 1;
        if (o + chunk < count) rc = issue(o + chunk, bi ^ 1);
        if (rc != EICOS_OK) break;
        HIP_TRY_AS("hipEventSynchronize", h->pin[bi].wait());
        pool.copy(dst + (size_t)o * width, h->pin[bi].as<void>(), (size_t)cnt * wb);
    }
    return rc;
}
static int fetch_rows(eicos_batch *h, double *dst, int off, int width) {
    return fetch_strided(h, dst, h->inst() + off, h->dp.inst_stride * sizeof(double), width, h->batch);
}

// the public form of an instance's info record
static void info_from(const DevInfo &d, eicos_info &o) {
        o.pcost = d.pcost; o.dcost = d.dcost; o.pres = d.pres; o.dres = d.dres; o.gap = d.gap; o.relgap = d.relgap;
        o.sigma = d.sigma; o.mu = d.mu; o.step = d.step; o.step_aff = d.step_aff; o.kapovert = d.kapovert;
        o.pinfres = d.pinfres; o.dinfres = d.dinfres; o.tau = d.tau; o.kap = d.kap;
        o.has_relgap = d.has_relgap; o.has_pinfres = d.has_pinfres; o.has_dinfres = d.has_dinfres;
        o.pinf = d.pinf; o.dinf = d.dinf; o.iter = d.iter; o.nitref1 = d.nitref1; o.nitref2 = d.nitref2;
        o.nitref3 = d.nitref3; o.exitcode = d.exitcode; o.n_factor = d.n_factor; o.n_ldlsolve = d.n_ldlsolve;
        o.n_sweep = d.n_sweep; o.reserved_ = 0; o.solve_us = d.solve_us;
}

int eicos_batch_info(eicos_batch *h, eicos_info *info) {
    if (!h || !info) return fail(EICOS_E_INVALID, "NULL argument");
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream));
    std::vector<DevInfo> tmp(h->batch);
    HIP_TRY(hipMemcpy2D(tmp.data(), sizeof(DevInfo), h->inst() + h->dp.i_info, h->dp.inst_stride * sizeof(double),
                        sizeof(DevInfo), (size_t)h->batch, hipMemcpyDeviceToHost));
    for (int i = 0; i < h->batch; i++) info_from(tmp[i], info[i]);
    return EICOS_OK;
}

// the exit codes of the batch out of eicos_batch_info (out: optional)
static int exit_codes(eicos_batch *h, int *out) {
    if (!out) return EICOS_OK;
    std::vector<eicos_info> info(h->batch);
    const int rc = eicos_batch_info(h, info.data());
    for (int i = 0; rc == EICOS_OK && i < h->batch; i++) out[i] = info[i].exitcode;
    return rc;
}

int eicos_batch_solve(eicos_batch *h, int *exitcodes) {
    int rc = eicos_batch_solve_async(h);
    if (rc != EICOS_OK) return rc;
    rc = eicos_batch_sync(h);
    if (rc != EICOS_OK) return rc;
    return exit_codes(h, exitcodes);
}

// ---- subset solves: by index list or by exit class (include/eicos_amd.h) ----
// A subset solve is an ordinary launch (enqueue_solve) whose order array the selection kernel fills from subset_ids(h); the exit codes
// and rows of chosen instances come back through the row-gather kernel and ONE copy of its compact buffer (fetch_strided).
int eicos_exit_class(int exitcode, int n_factor) { return (int)exit_class(exitcode, n_factor); }

// the checks every subset call makes before anything is enqueued: a refused list or mask changes no state
static int take_index_list(const eicos_batch *h, const int *idx, int count, const char *who) {
    if (!h) return fail(EICOS_E_INVALID, "NULL handle");
    const std::string msg = index_list_fault(idx, count, h->batch);
    return msg.empty() ? EICOS_OK : fail(EICOS_E_INVALID, std::string(who) + ": " + msg);
}
static int take_class_mask(const eicos_batch *h, unsigned mask, const char *who) {
    if (!h) return fail(EICOS_E_INVALID, "NULL handle");
    const std::string msg = class_mask_fault(mask);
    return msg.empty() ? EICOS_OK : fail(EICOS_E_INVALID, std::string(who) + ": " + msg);
}
// `count` validated ids from the host into device memory at dst, on the handle's stream, through the pinned list buffer
static int upload_ids(eicos_batch *h, const int *idx, int count, int *dst) {
    HIP_TRY_AS("hipHostMalloc", h->sub.reserve((size_t)h->batch * sizeof(int))); // (once: every list fits)
    HIP_TRY_AS("hipEventSynchronize", h->sub.wait()); // (the previous list may still be on its way)
    std::memcpy(h->sub.as<int>(), idx, (size_t)count * sizeof(int));
    HIP_TRY(hipMemcpyAsync(dst, h->sub.as<int>(), (size_t)count * sizeof(int), hipMemcpyHostToDevice, h->stream));
    HIP_TRY_AS("hipEventRecord", h->sub.mark(h->stream));
    return EICOS_OK;
}
// the compact buffer of the row gather: [ids of `count` instances | count rows of `width` doubles]
static size_t gather_rows_at(int count) { return (((size_t)count * sizeof(int)) + 63) & ~(size_t)63; }
static int grow_gather(eicos_batch *h, int count, int width) {
    HIP_TRY_AS("hipMalloc", h->d_gather.reserve(gather_rows_at(count) + (size_t)count * width * sizeof(double), h->stream));
    return EICOS_OK;
}
// rows of the instances d_list[0 .. count) (device memory; NULL: the ids already at the head of d_gather) into the caller's arrays, any
// NULL: the gather kernel, one copy of the compact buffer, and the split into groups on the host.  Complete on return.
static int gather_rows(eicos_batch *h, const int *d_list, int count, double *x, double *y, double *z, double *s, eicos_info *info, int *codes) {
    const DevPat &D = h->dp;
    const int want = (x && D.n ? GATHER_X : 0) | (y && D.p ? GATHER_Y : 0) | (z && D.m ? GATHER_Z : 0) | (s && D.m ? GATHER_S : 0) | (info || codes ? GATHER_INFO : 0);
    if (count == 0 || want == 0) return EICOS_OK;
    const int width = gather_width(want, D.n, D.p, D.m);
    const int rc = grow_gather(h, count, width);
    if (rc != EICOS_OK) return rc;
    double *rows = reinterpret_cast<double *>(h->d_gather.as<char>() + gather_rows_at(count));
    HIP_TRY(launch_gather_rows(h->pslot, h->inst(), d_list ? d_list : h->d_gather.as<const int>(), count, want, rows, h->stream));
    std::vector<double> host((size_t)count * width);
    const int frc = fetch_strided(h, host.data(), rows, (size_t)width * sizeof(double), width, count);
    if (frc != EICOS_OK) return frc;
    HIP_TRY(hipStreamSynchronize(h->stream));
    double *dst[4] = {x, y, z, s};
    const int bit[4] = {GATHER_X, GATHER_Y, GATHER_Z, GATHER_S}, w[4] = {D.n, D.p, D.m, D.m};
    for (int q = 0; q < count; q++) {
        const double *row = host.data() + (size_t)q * width;
        for (int g = 0; g < 4; g++)
            if (want & bit[g]) { std::memcpy(dst[g] + (size_t)q * w[g], row, (size_t)w[g] * sizeof(double)); row += w[g]; }
        if (want & GATHER_INFO) {
            DevInfo d;
            std::memcpy(&d, row, sizeof d);
            if (info) info_from(d, info[q]);
            if (codes) codes[q] = d.exitcode;
        }
    }
    return EICOS_OK;
}
// the selection kernel over the whole batch behind everything on the handle's stream: ids into subset_ids(h), their number into *count
// (and, if asked, the ids into idx_out): the one host synchronisation of eicos_batch_select / _solve_where
static int select_ids(eicos_batch *h, unsigned mask, int *idx_out, int *count) {
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream));
    HIP_TRY(launch_select(h->pslot, h->inst(), h->batch, mask, subset_ids(h), h->queue() + 1, h->stream));
    HIP_TRY(hipMemcpyAsync(count, h->queue() + 1, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (*count < 0 || *count > h->batch) return fail(EICOS_E_HIP, "internal: the selection kernel returned a count outside the batch");
    if (idx_out && *count > 0) {
        HIP_TRY(hipMemcpyAsync(idx_out, subset_ids(h), (size_t)*count * sizeof(int), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
    }
    return EICOS_OK;
}

int eicos_batch_select(eicos_batch *h, unsigned mask, int *idx_out, int *count_out) {
    int rc = take_class_mask(h, mask, "eicos_batch_select"), count = 0;
    if (rc == EICOS_OK) rc = select_ids(h, mask, idx_out, &count);
    if (rc == EICOS_OK && count_out) *count_out = count;
    return rc;
}

int eicos_batch_solve_subset_async(eicos_batch *h, const int *idx, int count) {
    int rc = take_index_list(h, idx, count, "eicos_batch_solve_subset");
    if (rc != EICOS_OK || count == 0) return rc; // (an empty subset: no launch, nothing recorded)
    HIP_TRY(hipSetDevice(h->device));
    rc = upload_ids(h, idx, count, subset_ids(h));
    return rc != EICOS_OK ? rc : enqueue_solve(h, nullptr, count);
}

int eicos_batch_solve_subset(eicos_batch *h, const int *idx, int count, int *exitcodes) {
    int rc = eicos_batch_solve_subset_async(h, idx, count);
    if (rc != EICOS_OK || count == 0) return rc;
    rc = eicos_batch_sync(h);
    return rc != EICOS_OK ? rc : gather_rows(h, subset_ids(h), count, nullptr, nullptr, nullptr, nullptr, nullptr, exitcodes);
}

int eicos_batch_solve_where(eicos_batch *h, unsigned mask, int *idx_out, int *count_out, int *exitcodes) {
    int rc = take_class_mask(h, mask, "eicos_batch_solve_where"), count = 0;
    if (rc == EICOS_OK) rc = select_ids(h, mask, idx_out, &count);
    if (rc != EICOS_OK) return rc;
    if (count_out) *count_out = count;
    if (count == 0) return EICOS_OK; // (nobody is in the class: no launch, nothing recorded)
    rc = enqueue_solve(h, nullptr, count); // (the ids are used where the selection kernel left them)
    if (rc == EICOS_OK) rc = eicos_batch_sync(h);
    return rc != EICOS_OK ? rc : gather_rows(h, subset_ids(h), count, nullptr, nullptr, nullptr, nullptr, nullptr, exitcodes);
}

int eicos_batch_gather(eicos_batch *h, const int *idx, int count, double *x, double *y, double *z, double *s, eicos_info *info) {
    int rc = take_index_list(h, idx, count, "eicos_batch_gather");
    if (rc != EICOS_OK || count == 0) return rc;
    if (!x && !y && !z && !s && !info) return EICOS_OK;
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream));
    // (the buffer for the widest row a call can ask for, so that the ids at its head stay where they are)
    rc = grow_gather(h, count, gather_width(GATHER_X | GATHER_Y | GATHER_Z | GATHER_S | GATHER_INFO, h->dp.n, h->dp.p, h->dp.m));
    if (rc == EICOS_OK) rc = upload_ids(h, idx, count, h->d_gather.as<int>());
    return rc != EICOS_OK ? rc : gather_rows(h, nullptr, count, x, y, z, s, info, nullptr);
}

// ---- steps fused into the solve launch: the helpers of update_solve and the rollout ----
static FitShape fit_shape(const eicos_batch *h) { return {h->dp.n, h->dp.p, h->dp.m, h->dp.Npad, h->nlds, h->threads}; }
// a step that runs inside the solve launch: its witness (5, or 6 with staged arrays) and an empty updateData interval in the timing ring
static int fused_step_begins(eicos_batch *h, int path) {
    h->last_update_path = path;
    return end_update_timing(h, begin_update_timing(h));
}
// the pinned staging buffer (`doubles`), the ready flags (`nchunks`) and the time-out word of a staged fused update
static int grow_staging(eicos_batch *h, size_t doubles, int nchunks) {
    bool new_flags = false;
    HIP_TRY_AS("hipHostMalloc", h->stage_pin.reserve(doubles * sizeof(double), h->stream));
    HIP_TRY_AS("hipHostMalloc", h->stage_flags.reserve((size_t)nchunks * sizeof(unsigned), h->stream, &new_flags));
    if (new_flags) { std::memset(h->stage_flags.p, 0, h->stage_flags.bytes); h->stage_seq = 0; } // (fresh flags: the sequence starts over)
    if (!h->d_err) { HIP_TRY_AS("hipMalloc", h->d_err.alloc(sizeof(int))); HIP_TRY(hipMemset(h->d_err.p, 0, sizeof(int))); }
    return EICOS_OK;
}
// The maps of a fused parametric step or rollout, as device copies of the handle's descriptors.  matrix: the step may carry the matrix
// map (where one is installed).  fb: the caller's own condition for the fallback record -- it travels only where the kernel writes u.
static void step_maps(const eicos_batch *h, UpdArgs &step, bool matrix, bool fb) {
    step.pmap = h->d_param.as<const ParamMapDev>(); step.omap = h->d_out.as<const OutMapDev>();
    if (matrix && h->mat.k) step.mmap = h->d_mat.as<const MatrixMapDev>();
    if (fb) step.fb = h->d_fb.as<const FallbackDev>();
}
// x_out [batch][n], u_out [batch][r] (NULL: not asked for) behind a finished solve, by kind of memory unless the kernel wrote it; complete on return
// fb_theta (outputs_to): the step's theta rows when a fallback map applies to u rows the kernel did not write
static int deliver_results(eicos_batch *h, double *x_out, MemKind x_kind, bool x_written, double *u_out, MemKind u_kind, bool u_written,
                           const double *fb_theta = nullptr) {
    const DevPat &D = h->dp;
    if (x_out && !x_written) {
        if (x_kind == MEM_DEVICE) { // a result array in device memory: one strided copy on the device
            const size_t wb = (size_t)D.n * sizeof(double);
            HIP_TRY(hipMemcpy2DAsync(x_out, wb, h->inst() + D.i_x, D.inst_stride * sizeof(double), wb, (size_t)h->batch, hipMemcpyDeviceToDevice, h->stream));
            HIP_TRY(hipStreamSynchronize(h->stream));
        } else { const int rc = fetch_rows(h, x_out, D.i_x, D.n); if (rc != EICOS_OK) return rc; }
    }
    if (u_out && !u_written) {
        const int rc = outputs_to(h, 0, h->batch, u_out, u_kind, nullptr, fb_theta);
        if (rc != EICOS_OK) return rc;
        if (u_kind == MEM_DEVICE) HIP_TRY(hipStreamSynchronize(h->stream)); // (the range kernel writes device memory asynchronously)
    }
    return EICOS_OK;
}

// updateData + solve in ONE call: the reference's updateData(double *...) followed by solve() (include/eicos.hpp:155-158) for the whole batch.
// When every given array is memory the GPU addresses directly (pinned / registered host memory, or device memory) the updateData of an
// instance is run by the solve kernel's own workgroup right before it solves that instance (kernels.hip: update_instance): the transfer over
// PCIe is the workgroups' loads, spread over the launch and hidden behind the other workgroups' compute -- a separate updateData kernel can
// only run BEFORE the solve (the registers and the LDS of a CU are fully owned by its resident solve workgroups), so its transfer time adds to
// every step.  x_out (optional, [batch][n]): pinned host / device memory is written by the kernel as each instance finishes; pageable memory
// is filled by eicos_batch_solution afterwards (device memory, where the update is not fused, by a copy on the device).  Anything else (pageable inputs -- unless staging is switched on, below --, a handle without an
// LDS vector, vectors beyond the in-register scaling accumulators) takes eicos_batch_update + eicos_batch_solve: same results, bit for bit, on
// every path.
// Synchronous; exitcodes optional.  rhs = true: the right-hand-side-only update (G, A NULL; h and b read on their own; no accumulator limit:
// the fused form divides by the stored scalings, kernels.hip: rhs_instance), eicos_batch_update_rhs_solve.
// kind = STEP_PARAM: the parametric update (theta [batch][k] through the installed map, the five arrays NULL; fused while a theta row fits
// the LDS vector the workgroup stages it in, kernels.hip: param_instance; pageable theta is never staged), eicos_batch_update_param_solve.
// With a matrix map installed the step is a full updateData from theta (kernels.hip: matrix_param_instance): fused under the conditions of
// both, a theta row that fits and the accumulator limit of the full update.
// u_out (optional, [batch][r]; any kind, needs an output map): the output map applied to every instance's x, delivered like x_out -- written
// by the kernel where it can be, by the range kernel and a copy otherwise.
enum StepKind { STEP_FULL = 0, STEP_RHS = 1, STEP_PARAM = 2 };
static int update_solve(eicos_batch *h, const double *G, const double *A, const double *c, const double *hh, const double *b,
                        const double *theta, double *u_out, double *x_out, int *exitcodes, StepKind kind) {
    // ---- classify the inputs and the outputs
    UpdateInputs in;
    const bool rhs = kind == STEP_RHS, param = kind == STEP_PARAM;
    int rc = param ? take_theta(in, h, 0, h ? h->batch : 0, theta, true) : take_inputs(in, h, 0, h ? h->batch : 0, G, A, c, hh, b, rhs, true);
    if (rc != EICOS_OK) return rc;
    if (u_out && h->out.r == 0) return fail(EICOS_E_INVALID, "no output map (eicos_batch_set_output_map installs one)");
    if (param && (rc = fallback_fits(h)) != EICOS_OK) return rc;
    // the fallback map (eicos_batch_set_fallback_map) applies to the u rows of a parametric step: formed by the kernel that writes them, or
    // by the range kernel behind the output kernel (deliver_results)
    const bool fb_on = param && u_out && h->fb.mask != 0;
    const DevPat &D = h->dp;
    // arrays the GPU cannot address (pageable memory) are STAGED: copied into the handle's pinned staging buffer while the kernel runs
    const bool any_staged = in.any(MEM_PAGEABLE);
    if (D.n == 0) x_out = nullptr;
    const MemKind x_kind = memory_kind(x_out, (size_t)h->batch * D.n * sizeof(double));
    const MemKind u_kind = memory_kind(u_out, (size_t)h->batch * h->out.r * sizeof(double));
    // ---- choose the path
    const FitShape fs = fit_shape(h);
    const bool fits = param ? fused_param_fits(fs, h->param.k, h->mat.k != 0) : (rhs ? fused_rhs_fits(fs) : fused_full_fits(fs));
    const bool fused = fits && env_knob("EICOS_FUSED_UPDATE", 1, 0, 1);
    // (staging pageable arrays while the kernel runs is OFF by default: measured on five boxes against the bounce pipeline + solve it is
    // +5.7 ... -6.2 % -- the host's copy is the pace either way, and on a box with slow host cores the kernel's own PCIe pulls and flag polls
    // slow that copy further; EICOS_FUSED_STAGED=1 under EICOS_EXPERIMENT=1 turns it on: docs/HISTORY.md A.11 item 9)
    if (!fused || (any_staged && (param || !env_knob("EICOS_FUSED_STAGED", 0, 0, 1)))) {
        // ---- separate launches (device arrays on a handle without the fused path: the device-pointer updateData)
        const double *fb_theta = nullptr;
        rc = fb_on ? fallback_theta(h, in.src[2], in.kind[2], h->batch, fb_theta) : EICOS_OK;
        if (rc == EICOS_OK) rc = in.all(MEM_DEVICE) ? update_in_place(in, 0) : staged_update(in, -1);
        if (rc == EICOS_OK) rc = enqueue_solve(h, nullptr);
        if (rc == EICOS_OK) rc = eicos_batch_sync(h);
        if (rc == EICOS_OK) rc = deliver_results(h, x_out, x_kind, false, u_out, u_kind, false, fb_theta);
        return rc != EICOS_OK ? rc : exit_codes(h, exitcodes);
    }
    // ---- one launch: the kernel reads the arrays and writes the outputs it can address
    const double *ptr[5] = {in.src[0], in.src[1], in.src[2], in.src[3], in.src[4]};
    bool staged[5];
    size_t per = 0;
    for (int k = 0; k < 5; k++) {
        staged[k] = in.holds_data(k) && in.kind[k] == MEM_PAGEABLE;
        if (staged[k]) per += in.w[k];
    }
    // the staged arrays of the whole batch are ONE packed chunk in the staging buffer, filled in copy chunks of ~12 MB (chunk_plan.hpp)
    const PackedChunk pk = pack_chunk(in.w, staged, (size_t)h->batch, ChunkPad::Gap8);
    const int chunk = any_staged ? fused_stage_chunk(per, h->batch) : h->batch;
    const int nchunks = chunk_count(h->batch, chunk);
    if (any_staged) {
        rc = grow_staging(h, pk.total, nchunks);
        if (rc != EICOS_OK) return rc;
        for (int k = 0; k < 5; k++) if (staged[k]) ptr[k] = h->stage_pin.as<double>() + pk.off[k];
        h->stage_seq++;
        if (h->stage_seq == 0) { std::memset(h->stage_flags.p, 0, h->stage_flags.bytes); h->stage_seq = 1; } // (wrapped)
    }
    rc = fused_step_begins(h, any_staged ? 6 : 5);
    if (rc != EICOS_OK) return rc;
    const bool x_written = x_kind != MEM_PAGEABLE, u_written = u_kind != MEM_PAGEABLE;
    UpdArgs step;
    step.on = param ? UPD_PARAM : (rhs ? UPD_RHS : UPD_FULL);
    step.G = ptr[0]; step.A = ptr[1]; (param ? step.theta : step.c) = ptr[2]; step.h = ptr[3]; step.b = ptr[4];
    step.x = x_written ? x_out : nullptr; step.u = u_written ? u_out : nullptr;
    step.flags = any_staged ? h->stage_flags.as<unsigned>() : nullptr; step.chunk = chunk; step.seq = h->stage_seq; step.err = h->d_err.as<int>();
    step_maps(h, step, param, fb_on && u_written);
    rc = enqueue_solve(h, &step);
    if (rc != EICOS_OK) return rc; // (nothing was launched: no workgroup waits for a flag)
    if (any_staged) { // the kernel is running: copy chunk by chunk and release each chunk's flag behind its rows
        CopyPool &pool = CopyPool::get();
        for (int q = 0; q < nchunks; q++) {
            const size_t r0 = (size_t)q * chunk, rows = std::min<size_t>((size_t)chunk, (size_t)h->batch - r0);
            for (int k = 0; k < 5; k++) if (staged[k]) pool.copy(const_cast<double *>(ptr[k]) + r0 * in.w[k], in.src[k] + r0 * in.w[k], rows * in.w[k] * sizeof(double));
            __atomic_store_n(&h->stage_flags.as<unsigned>()[q], h->stage_seq, __ATOMIC_RELEASE); // (stream_copy ends with an sfence: the rows are visible before the flag)
        }
    }
    rc = eicos_batch_sync(h);
    if (rc != EICOS_OK) return rc;
    if (any_staged) {
        int err = 0;
        HIP_TRY(hipMemcpy(&err, h->d_err.p, sizeof(int), hipMemcpyDeviceToHost));
        if (err) { HIP_TRY(hipMemset(h->d_err.p, 0, sizeof(int))); return fail(EICOS_E_HIP, "fused updateData: a workgroup timed out waiting for its staged rows"); }
    }
    // (a fused parametric step never stages theta: the range kernel reads the rows the launch read)
    rc = deliver_results(h, x_out, x_kind, x_written, u_out, u_kind, u_written, fb_on && !u_written ? ptr[2] : nullptr);
    return rc != EICOS_OK ? rc : exit_codes(h, exitcodes);
}

int eicos_batch_update_solve(eicos_batch *h, const double *G, const double *A, const double *c, const double *hh, const double *b,
                             double *x_out, int *exitcodes) {
    return update_solve(h, G, A, c, hh, b, nullptr, nullptr, x_out, exitcodes, STEP_FULL);
}
int eicos_batch_update_rhs_solve(eicos_batch *h, const double *c, const double *hh, const double *b, double *x_out, int *exitcodes) {
    return update_solve(h, nullptr, nullptr, c, hh, b, nullptr, nullptr, x_out, exitcodes, STEP_RHS);
}
int eicos_batch_update_param_solve(eicos_batch *h, const double *theta, double *u_out, double *x_out, int *exitcodes) {
    return update_solve(h, nullptr, nullptr, nullptr, nullptr, nullptr, theta, u_out, x_out, exitcodes, STEP_PARAM);
}

// ---- index-list forms: update, read and step a chosen subset (include/eicos_amd.h) ----
// An indexed update is its range namesake with one more field in the descriptor (UpdateInputs::ids): the list is checked like a subset
// solve's (take_index_list: a refused list changes no state), the arrays by the namesake's own take_* over `count` rows, the ids go to
// device memory through the pinned list buffer (upload_ids, into d_upd_ids) and the rows travel over the namesake's paths.
// An empty list: EICOS_OK, nothing enqueued, nothing recorded.
static int ids_to_device(UpdateInputs &in, const int *idx) {
    eicos_batch *h = in.h;
    HIP_TRY_AS("hipMalloc", h->d_upd_ids.reserve((size_t)h->batch * sizeof(int), h->stream)); // (once: every list fits)
    const int rc = upload_ids(h, idx, in.count, h->d_upd_ids.as<int>());
    in.ids = h->d_upd_ids.as<const int>();
    return rc;
}
// host: the arrays are host memory (pageable: bounce pipeline; pinned: in place, synchronous); else device memory, one asynchronous launch
static int indexed_update(UpdateInputs &in, const int *idx, bool host) {
    const int rc = ids_to_device(in, idx);
    if (rc != EICOS_OK) return rc;
    return host ? staged_update(in, -1) : update_in_place(in, 0);
}
static int update_indexed(eicos_batch *h, const int *idx, int count, const double *G, const double *A, const double *c, const double *hh,
                          const double *b, bool rhs, bool host, const char *who) {
    int rc = take_index_list(h, idx, count, who);
    if (rc != EICOS_OK || count == 0) return rc;
    UpdateInputs in;
    rc = take_inputs(in, h, 0, count, G, A, c, hh, b, rhs, host);
    return rc != EICOS_OK ? rc : indexed_update(in, idx, host);
}
static int update_param_indexed(eicos_batch *h, const int *idx, int count, const double *theta, bool host, const char *who) {
    int rc = take_index_list(h, idx, count, who);
    if (rc != EICOS_OK || count == 0) return rc;
    UpdateInputs in;
    rc = take_theta(in, h, 0, count, theta, host);
    return rc != EICOS_OK ? rc : indexed_update(in, idx, host);
}
static int set_iterate_indexed(eicos_batch *h, const int *idx, int count, const double *x, const double *y, const double *z, const double *s,
                               bool host, const char *who) {
    int rc = take_index_list(h, idx, count, who);
    if (rc != EICOS_OK || count == 0) return rc;
    UpdateInputs in;
    rc = take_iterate(in, h, 0, count, x, y, z, s, host);
    return rc != EICOS_OK ? rc : indexed_update(in, idx, host);
}

int eicos_batch_update_indexed(eicos_batch *h, const int *idx, int count, const double *G, const double *A, const double *c, const double *hh,
                               const double *b) {
    return update_indexed(h, idx, count, G, A, c, hh, b, false, true, "eicos_batch_update_indexed");
}
int eicos_batch_update_indexed_device(eicos_batch *h, const int *idx, int count, const double *dG, const double *dA, const double *dc,
                                      const double *dh, const double *db) {
    return update_indexed(h, idx, count, dG, dA, dc, dh, db, false, false, "eicos_batch_update_indexed_device");
}
int eicos_batch_update_rhs_indexed(eicos_batch *h, const int *idx, int count, const double *c, const double *hh, const double *b) {
    return update_indexed(h, idx, count, nullptr, nullptr, c, hh, b, true, true, "eicos_batch_update_rhs_indexed");
}
int eicos_batch_update_rhs_indexed_device(eicos_batch *h, const int *idx, int count, const double *dc, const double *dh, const double *db) {
    return update_indexed(h, idx, count, nullptr, nullptr, dc, dh, db, true, false, "eicos_batch_update_rhs_indexed_device");
}
int eicos_batch_update_param_indexed(eicos_batch *h, const int *idx, int count, const double *theta) {
    return update_param_indexed(h, idx, count, theta, true, "eicos_batch_update_param_indexed");
}
int eicos_batch_update_param_indexed_device(eicos_batch *h, const int *idx, int count, const double *dtheta) {
    return update_param_indexed(h, idx, count, dtheta, false, "eicos_batch_update_param_indexed_device");
}
int eicos_batch_set_iterate_indexed(eicos_batch *h, const int *idx, int count, const double *x, const double *y, const double *z, const double *s) {
    return set_iterate_indexed(h, idx, count, x, y, z, s, true, "eicos_batch_set_iterate_indexed");
}
int eicos_batch_set_iterate_indexed_device(eicos_batch *h, const int *idx, int count, const double *dx, const double *dy, const double *dz,
                                           const double *ds) {
    return set_iterate_indexed(h, idx, count, dx, dy, dz, ds, false, "eicos_batch_set_iterate_indexed_device");
}

// the output rows of the listed instances, row q = instance idx[q]: eicos_batch_outputs* with the range kernel reading the slab list[q]
static int outputs_indexed(eicos_batch *h, const int *idx, int count, double *u, bool host, const char *who) {
    int rc = take_index_list(h, idx, count, who);
    if (rc != EICOS_OK || count == 0) return rc;
    rc = take_output_range(h, 0, count, u);
    if (rc != EICOS_OK) return rc;
    if (host) {
        if (memory_kind(u, 1) == MEM_DEVICE) return fail(EICOS_E_INVALID, std::string(who) + " takes a host pointer: u lives in device memory (use eicos_batch_outputs_indexed_device)");
        HIP_TRY(hipStreamSynchronize(h->stream));
    }
    HIP_TRY_AS("hipMalloc", h->d_upd_ids.reserve((size_t)h->batch * sizeof(int), h->stream));
    rc = upload_ids(h, idx, count, h->d_upd_ids.as<int>());
    return rc != EICOS_OK ? rc : outputs_to(h, 0, count, u, host ? MEM_PAGEABLE : MEM_DEVICE, h->d_upd_ids.as<const int>());
}
int eicos_batch_outputs_indexed(eicos_batch *h, const int *idx, int count, double *u) {
    return outputs_indexed(h, idx, count, u, true, "eicos_batch_outputs_indexed");
}
int eicos_batch_outputs_indexed_device(eicos_batch *h, const int *idx, int count, double *du) {
    return outputs_indexed(h, idx, count, du, false, "eicos_batch_outputs_indexed_device");
}

// ---- adjoint sensitivities (include/eicos_amd.h): eicos_batch_adjoint, _adjoint_data, _output_jacobian, _param_jacobian, _param_gradient ----
// One launch of the handle's adjoint kernel (launch.hpp: AdjointLaunch) behind everything on the handle's stream, under the handle's settings
// and dynamic regularisation.  Every check stands in front of the first enqueue: a refused call changes nothing.
namespace {
struct AdjointCall {
    const char *who;
    const int *idx; int count, nrhs; // nrhs: right-hand sides per instance (the Jacobian form: r)
    const double *g; double *grad_c, *grad_h, *grad_b, *res, *J; // arrays of the gradient form; J / res of the contracted form; NULL: not of the form, or not wanted
    bool jac, device; // the contracted form (launch.hpp: AdjointDev::J); its J, res and g live in device memory (asynchronous)
    double *grad_G = nullptr, *grad_A = nullptr; // the gradient form: the matrix gradients (optional)
    bool mmap = false, grows = false; // the contracted form: the matrix map joins when one is installed; the right-hand sides are nrhs rows of g
    const RecordRows *rec = nullptr; // the contracted device form of a recording rollout: where the step's rows go (device memory)
    const char *out_name = "J"; // what the C header calls J
};
static_assert(sizeof(AdjointDev) <= MAP_HEADER, "the adjoint record larger than its header");
}
// ---- what the sensitivity and rollout calls share: their arrays (call_arrays.hpp), the timing bracket, the held trajectory ----
static int kind_check(const Arrays &a, const char *who, bool paired = true) {
    const std::string msg = a.kind_fault(who, paired);
    return msg.empty() ? EICOS_OK : fail(EICOS_E_INVALID, msg);
}
// The arrays into `buf`.  The host form waits for the stream, grows the buffer and enqueues the copies of its inputs; the device form
// only grows the buffer for the parts both forms have.
static int stage(eicos_batch *h, DevBuf &buf, Arrays &a) {
    if (!a.device) HIP_TRY(hipStreamSynchronize(h->stream));
    HIP_TRY_AS("hipMalloc", buf.reserve(a.bytes(), h->stream));
    a.place(buf.p);
    HIP_TRY_AS("hipMemcpyAsync", a.copy_in(h->stream));
    return EICOS_OK;
}
// ... and back: the host form enqueues the copies of its outputs and waits; the device form has only enqueued
static int unstage(eicos_batch *h, const Arrays &a) {
    if (a.device) return EICOS_OK;
    HIP_TRY_AS("hipMemcpyAsync", a.copy_out(h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return EICOS_OK;
}
// A launch between the handle's adjoint events (eicos_batch_last_adjoint_ms: it counts as the handle's most recent adjoint launch)
static int timed_adjoint_launch(eicos_batch *h, const char *what, const std::function<hipError_t()> &launch) {
    if (!h->ev_a0) { HIP_TRY(hipEventCreate(&h->ev_a0)); HIP_TRY(hipEventCreate(&h->ev_a1)); }
    HIP_TRY(hipEventRecord(h->ev_a0, h->stream));
    HIP_TRY_AS(what, launch());
    HIP_TRY(hipEventRecord(h->ev_a1, h->stream));
    h->adjoint_timed = true;
    return EICOS_OK;
}
// The trajectory a backward sweep or a read of the record needs on the handle.  current: it must belong to the maps now installed.
static int held_trajectory_fault(const eicos_batch *h, const char *who, bool need_records, bool current = true) {
    if (!h) return fail(EICOS_E_INVALID, "NULL handle");
    const std::string msg = h->held.fault(who, h->map_gen, need_records, current);
    return msg.empty() ? EICOS_OK : fail(EICOS_E_INVALID, msg);
}
static int adjoint_list_fault(const eicos_batch *h, const int *idx, int count, const char *who) {
    if (!h) return fail(EICOS_E_INVALID, "NULL handle");
    if (idx) return take_index_list(h, idx, count, who);
    if (count < 0 || count > h->batch) return fail(EICOS_E_INVALID, std::string(who) + ": count must lie in [0, batch] when idx is NULL (instances 0 .. count-1)");
    return EICOS_OK;
}
// What every adjoint record carries, whatever its form: the handle's cone scaling
static AdjointDev adjoint_record(const eicos_batch *h) {
    AdjointDev rec{};
    rec.centred = h->adjoint_scaling == EICOS_ADJOINT_CENTRED;
    return rec;
}
// The record of the contracted form (launch.hpp: AdjointDev::J), filled in ONE place for adjoint_run and the fused rollout: the gradients
// contracted with the parameter map and -- matrix -- with the matrix map, where one is installed, k columns each; right-hand sides the
// rows of the output map, or -- nrhs > 0 -- nrhs rows of the caller's g (which the caller sets); rows != NULL: a recording rollout's rows.
static AdjointDev contracted_record(const eicos_batch *h, bool matrix, int nrhs, int k, double *J, double *res, const RecordRows *rows) {
    AdjointDev rec = adjoint_record(h);
    rec.pmap = h->param.k ? h->d_param.as<const ParamMapDev>() : nullptr;
    rec.mmap = matrix && h->mat.k ? h->d_mat.as<const MatrixMapDev>() : nullptr;
    rec.k = k;
    if (nrhs > 0) rec.nrhs = nrhs;
    else rec.omap = h->d_out.as<const OutMapDev>();
    rec.J = J; rec.res = res;
    if (rows) { rec.grad_c = rows->Wc; rec.grad_h = rows->Wh; rec.grad_b = rows->Wb; rec.x_rec = rows->x; rec.y_rec = rows->y; rec.z_rec = rows->z; }
    return rec;
}
static int adjoint_run(eicos_batch *h, const AdjointCall &c) {
    if (c.count == 0) return EICOS_OK;
    const DevPat &D = h->dp;
    const size_t rows = (size_t)c.count * c.nrhs, k = c.jac ? (size_t)std::max(h->param.k, c.mmap ? h->mat.k : 0) : 0;
    // The arrays, declared once -- in the order their kind is checked --, behind the launch's record and its index list.  Which of them
    // a form has is in the call: the gradient forms (no device form) take g and give a row per data group, the contracted forms give
    // J and take g only as nrhs rows (grows); every other pointer of the call is NULL.
    Arrays a(c.device);
    const int i_rec = a.fixed(MAP_HEADER), i_ids = a.fixed((size_t)h->batch * sizeof(int));
    const int i_J = a.out(c.out_name, c.J, rows * k), i_g = a.in("g", c.g, rows * D.n);
    const int i_c = a.out("grad_c", c.grad_c, rows * D.n), i_h = a.out("grad_h", c.grad_h, rows * D.m), i_b = a.out("grad_b", c.grad_b, rows * D.p);
    const int i_G = a.out("grad_G", c.grad_G, rows * D.nnzG), i_A = a.out("grad_A", c.grad_A, rows * D.nnzA), i_res = a.out("res", c.res, rows);
    int rc = kind_check(a, c.who, c.jac);
    if (rc != EICOS_OK) return rc;
    HIP_TRY(hipSetDevice(h->device));
    if ((rc = stage(h, h->d_adj, a)) != EICOS_OK) return rc;
    int *d_ids = nullptr;
    if (c.idx) {
        d_ids = static_cast<int *>(a.at(i_ids));
        if ((rc = upload_ids(h, c.idx, c.count, d_ids)) != EICOS_OK) return rc;
    }
    AdjointDev &rec = h->adj;
    if (c.jac) rec = contracted_record(h, c.mmap, c.grows ? c.nrhs : 0, (int)k, a.dbl(i_J), a.dbl(i_res), c.rec);
    else {
        rec = adjoint_record(h);
        rec.nrhs = c.nrhs; rec.res = a.dbl(i_res);
        rec.grad_c = a.dbl(i_c); rec.grad_h = a.dbl(i_h); rec.grad_b = a.dbl(i_b); rec.grad_G = a.dbl(i_G); rec.grad_A = a.dbl(i_A);
    }
    rec.g = a.dbl(i_g);
    HIP_TRY(hipMemcpyAsync(a.at(i_rec), &rec, sizeof rec, hipMemcpyHostToDevice, h->stream));
    // (the slabs, the launch shape and the settings of the handle's solves: solve_launch)
    const SolveLaunch S = solve_launch(h, -1);
    const AdjointLaunch L{S.ps, S.inst, S.work, c.count, d_ids, S.batch, S.grid, S.threads, S.nlds, S.idx16, S.dyn_delta, S.dyn_eps, S.cfg, S.dyn_lds,
                          static_cast<const AdjointDev *>(a.at(i_rec))};
    rc = timed_adjoint_launch(h, "adjoint launch", [&] { return solve_build(h->threads, h->ldsres, h->w2, h->ubl).adjoint(L, h->stream); });
    return rc != EICOS_OK ? rc : unstage(h, a);
}

// eicos_batch_adjoint and, with the matrix gradients, eicos_batch_adjoint_data
static int adjoint_gradients(eicos_batch *h, const char *who, const int *idx, int count, int nrhs, const double *g, double *grad_c, double *grad_h,
                             double *grad_b, double *grad_G, double *grad_A, double *res) {
    const int rc = adjoint_list_fault(h, idx, count, who);
    if (rc != EICOS_OK) return rc;
    if (nrhs < 1 || nrhs > EICOS_ADJOINT_MAX_RHS) return fail(EICOS_E_INVALID, std::string(who) + ": nrhs must lie in [1, " + std::to_string(EICOS_ADJOINT_MAX_RHS) + "], got " + std::to_string(nrhs));
    if (!g && count > 0 && h->dp.n > 0) return fail(EICOS_E_INVALID, std::string(who) + ": g is NULL");
    AdjointCall c{who, idx, count, nrhs, g, grad_c, grad_h, grad_b, res, nullptr, false, false};
    c.grad_G = grad_G; c.grad_A = grad_A;
    return adjoint_run(h, c);
}
int eicos_batch_adjoint(eicos_batch *h, const int *idx, int count, int nrhs, const double *g, double *grad_c, double *grad_h, double *grad_b,
                        double *res) {
    return adjoint_gradients(h, "eicos_batch_adjoint", idx, count, nrhs, g, grad_c, grad_h, grad_b, nullptr, nullptr, res);
}
int eicos_batch_adjoint_data(eicos_batch *h, const int *idx, int count, int nrhs, const double *g, double *grad_c, double *grad_h, double *grad_b,
                             double *grad_G, double *grad_A, double *res) {
    return adjoint_gradients(h, "eicos_batch_adjoint_data", idx, count, nrhs, g, grad_c, grad_h, grad_b, grad_G, grad_A, res);
}

// The contracted forms through whichever of the parameter map and the matrix map are installed (eicos_batch_param_jacobian: the rows of
// the output map; eicos_batch_param_gradient: nrhs rows of g per instance).  out = J or grad_theta.
static int param_contracted(eicos_batch *h, const int *idx, int count, int nrhs, const double *g, bool grows, double *out, const char *out_name,
                            double *res, bool device, const char *who, const RecordRows *rows = nullptr) {
    const int rc = adjoint_list_fault(h, idx, count, who);
    if (rc != EICOS_OK) return rc;
    const std::string w(who);
    if (grows && (nrhs < 1 || nrhs > EICOS_ADJOINT_MAX_RHS)) return fail(EICOS_E_INVALID, w + ": nrhs must lie in [1, " + std::to_string(EICOS_ADJOINT_MAX_RHS) + "], got " + std::to_string(nrhs));
    if (!grows && h->out.r == 0) return fail(EICOS_E_INVALID, w + ": needs an output map (eicos_batch_set_output_map): J = d u / d theta");
    if (h->param.k == 0 && h->mat.k == 0)
        return fail(EICOS_E_INVALID, w + ": needs a parameter map or a matrix map (eicos_batch_set_param_map, eicos_batch_set_matrix_map): neither is installed");
    if (h->param.k != 0 && h->mat.k != 0 && h->param.k != h->mat.k)
        return fail(EICOS_E_INVALID, w + ": the matrix map was installed for k = " + std::to_string(h->mat.k) + ", the parameter map now installed has k = " +
                                         std::to_string(h->param.k) + ": install it again");
    if (grows && !g && count > 0 && h->dp.n > 0) return fail(EICOS_E_INVALID, w + ": g is NULL");
    if (!out && count > 0) return fail(EICOS_E_INVALID, w + ": " + out_name + " is NULL");
    AdjointCall c{who, idx, count, grows ? nrhs : h->out.r, grows ? g : nullptr, nullptr, nullptr, nullptr, res, out, true, device};
    c.mmap = true; c.grows = grows; c.rec = rows; c.out_name = out_name;
    return adjoint_run(h, c);
}
int eicos_batch_param_jacobian(eicos_batch *h, const int *idx, int count, double *J, double *res) {
    return param_contracted(h, idx, count, 0, nullptr, false, J, "J", res, false, "eicos_batch_param_jacobian");
}
int eicos_batch_param_jacobian_device(eicos_batch *h, const int *idx, int count, double *dJ, double *dres) {
    return param_contracted(h, idx, count, 0, nullptr, false, dJ, "J", dres, true, "eicos_batch_param_jacobian_device");
}
int eicos_batch_param_gradient(eicos_batch *h, const int *idx, int count, int nrhs, const double *g, double *grad_theta, double *res) {
    return param_contracted(h, idx, count, nrhs, g, true, grad_theta, "grad_theta", res, false, "eicos_batch_param_gradient");
}
int eicos_batch_param_gradient_device(eicos_batch *h, const int *idx, int count, int nrhs, const double *dg, double *dgrad_theta, double *dres) {
    return param_contracted(h, idx, count, nrhs, dg, true, dgrad_theta, "grad_theta", dres, true, "eicos_batch_param_gradient_device");
}

static int output_jacobian(eicos_batch *h, const int *idx, int count, double *J, double *res, bool device, const char *who) {
    const int rc = adjoint_list_fault(h, idx, count, who);
    if (rc != EICOS_OK) return rc;
    if (h->param.k == 0 || h->out.r == 0)
        return fail(EICOS_E_INVALID, std::string(who) + ": needs a parameter map and an output map (eicos_batch_set_param_map, eicos_batch_set_output_map): J = d u / d theta");
    if (h->mat.k != 0)
        return fail(EICOS_E_INVALID, std::string(who) + ": a matrix map is installed -- the derivative then has dG and dA terms, which this call does not form (right-hand-side data only; eicos_batch_param_jacobian forms them)");
    if (!J && count > 0) return fail(EICOS_E_INVALID, std::string(who) + ": J is NULL");
    return adjoint_run(h, AdjointCall{who, idx, count, h->out.r, nullptr, nullptr, nullptr, nullptr, res, J, true, device});
}
int eicos_batch_output_jacobian(eicos_batch *h, const int *idx, int count, double *J, double *res) {
    return output_jacobian(h, idx, count, J, res, false, "eicos_batch_output_jacobian");
}
int eicos_batch_output_jacobian_device(eicos_batch *h, const int *idx, int count, double *dJ, double *dres) {
    return output_jacobian(h, idx, count, dJ, dres, true, "eicos_batch_output_jacobian_device");
}

// The closed-loop step over a chosen subset: eicos_batch_update_param_indexed + eicos_batch_solve_subset + eicos_batch_outputs_indexed (+ the
// x rows), every array in list order.  Fused under the conditions of eicos_batch_update_param_solve (update_solve, above: an LDS vector,
// a theta row that fits, theta the GPU addresses, EICOS_FUSED_UPDATE not 0; witness 5): ONE subset launch whose selection kernel also
// leaves the row map (launch.hpp: UpdArgs::rows_at), so that the workgroup that solves instance idx[q] expands row q of theta first and writes row q of
// u_out / x_out (pinned or device memory) when it is done.  Otherwise the three calls run; rows the kernel did not write come through the
// indexed output kernel and the row gather.  Same bits on either path.  Synchronous; u_out, x_out, exitcodes optional.
int eicos_batch_update_param_solve_subset(eicos_batch *h, const int *idx, int count, const double *theta, double *u_out, double *x_out,
                                          int *exitcodes) {
    int rc = take_index_list(h, idx, count, "eicos_batch_update_param_solve_subset");
    if (rc != EICOS_OK || count == 0) return rc; // (an empty subset: no launch, nothing recorded)
    UpdateInputs in;
    rc = take_theta(in, h, 0, count, theta, true);
    if (rc != EICOS_OK) return rc;
    if (u_out && h->out.r == 0) return fail(EICOS_E_INVALID, "no output map (eicos_batch_set_output_map installs one)");
    const DevPat &D = h->dp;
    if (D.n == 0) x_out = nullptr;
    const MemKind x_kind = memory_kind(x_out, (size_t)count * D.n * sizeof(double));
    const MemKind u_kind = memory_kind(u_out, (size_t)count * h->out.r * sizeof(double));
    const bool fused = fused_param_fits(fit_shape(h), h->param.k, h->mat.k != 0) && env_knob("EICOS_FUSED_UPDATE", 1, 0, 1) && !in.any(MEM_PAGEABLE);
    if ((rc = fallback_fits(h)) != EICOS_OK) return rc;
    const bool fb_on = u_out && h->fb.mask != 0; // (eicos_batch_set_fallback_map: the rows of theta and u are in list order alike)
    const double *fb_theta = nullptr;
    bool x_written = false, u_written = false;
    if (!fused) { // the update on its own, then the subset launch
        if (fb_on && (rc = fallback_theta(h, in.src[2], in.kind[2], count, fb_theta)) != EICOS_OK) return rc;
        rc = ids_to_device(in, idx);
        if (rc == EICOS_OK) rc = in.all(MEM_DEVICE) ? update_in_place(in, 0) : staged_update(in, -1);
        if (rc == EICOS_OK) rc = upload_ids(h, idx, count, subset_ids(h));
        if (rc == EICOS_OK) rc = enqueue_solve(h, nullptr, count);
    } else {
        rc = upload_ids(h, idx, count, subset_ids(h));
        if (rc == EICOS_OK) rc = fused_step_begins(h, 5);
        if (rc != EICOS_OK) return rc;
        x_written = x_out && x_kind != MEM_PAGEABLE; u_written = u_out && u_kind != MEM_PAGEABLE;
        UpdArgs step;
        step.on = UPD_PARAM; step.rows_at = subset_rows_at(h); step.theta = in.src[2];
        step.x = x_written ? x_out : nullptr; step.u = u_written ? u_out : nullptr;
        step_maps(h, step, true, fb_on && u_written);
        if (fb_on && !u_written) fb_theta = in.src[2]; // (memory the GPU addresses: the launch reads it too)
        rc = enqueue_solve(h, &step, count);
    }
    if (rc == EICOS_OK) rc = eicos_batch_sync(h);
    if (rc != EICOS_OK) return rc;
    // ---- the rows the kernel did not write, and the exit codes (deliver_results for a subset)
    if (u_out && !u_written) {
        rc = outputs_to(h, 0, count, u_out, u_kind, subset_ids(h), fb_theta);
        if (rc != EICOS_OK) return rc;
        if (u_kind == MEM_DEVICE) HIP_TRY(hipStreamSynchronize(h->stream));
    }
    if (x_out && !x_written && x_kind == MEM_DEVICE) { // the gather kernel straight into the caller's device rows
        HIP_TRY(launch_gather_rows(h->pslot, h->inst(), subset_ids(h), count, GATHER_X, x_out, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
        x_written = true;
    }
    return gather_rows(h, subset_ids(h), count, x_written ? nullptr : x_out, nullptr, nullptr, nullptr, nullptr, exitcodes);
}

// ---- plant map and rollout: theta+ = f0 + F [theta | u] (+ w), and `steps` closed-loop steps in one call ----
// The map reaches the kernels inside the rollout's record (RolloutDev), by value in the range kernel and through a pointer in the fused
// launch; k, r = the parameter and output counts installed NOW, which it is validated for.
int eicos_batch_set_plant_map(eicos_batch *h, const eicos_affine_map *f) {
    if (!h) return fail(EICOS_E_INVALID, "NULL handle");
    const int k = h->param.k, r = h->out.r;
    const AffineGroup g = {f, k, k + r, "plant map: ", "[0, k + r)"};
    std::string msg;
    if (f) {
        if (k == 0) return fail(EICOS_E_INVALID, g.who + "no parameter map (eicos_batch_set_param_map installs one)");
        if (r == 0) return fail(EICOS_E_INVALID, g.who + "no output map (eicos_batch_set_output_map installs one)");
        if (affine_fault(g, msg)) return fail(EICOS_E_INVALID, msg);
    }
    PlantMapDev M{};
    M.k = k; M.r = r; M.nnz = f ? f->rowptr[k] : 0;
    // the per-instance values go with the map they were given for (the pattern may change); install_map waits for the stream first
    // and clears the descriptor that points at them
    const int rc = install_map(h, h->d_plant, h->plant, "plant", &g, 1, 0, f ? &M : nullptr, &M.a);
    h->d_plant_f0.reset(); h->d_plant_val.reset();
    h->plant.ibase = h->plant.ival = nullptr;
    return rc;
}

// ---- per-instance plant values: rows of base / val of the plant map that belong to one instance each (launch.hpp: PlantMapDev) ----
// The descriptor travels by value inside the rollout's record, so the next rollout picks the pointers up; every check stands in front of
// the first enqueue.  The host form copies on the handle's stream and waits, the device form only enqueues.
static int plant_values_range(const eicos_batch *h, int first, int count, const std::string &w) {
    if (h->plant.k == 0) return fail(EICOS_E_INVALID, w + ": no plant map (eicos_batch_set_plant_map installs one)");
    if (first < 0 || count < 0 || first > h->batch - count) return fail(EICOS_E_INVALID, w + ": instance range out of bounds");
    return EICOS_OK;
}
static int set_plant_values(eicos_batch *h, int first, int count, const double *f0, const double *val, bool device, const char *who) {
    if (!h) return fail(EICOS_E_INVALID, "NULL handle");
    const std::string w(who);
    { const int rc = plant_values_range(h, first, count, w); if (rc != EICOS_OK) return rc; }
    if (!f0 && !val) return fail(EICOS_E_INVALID, w + ": f0 and val are both NULL");
    Arrays a(device); // (for their kind alone: the rows go straight into the handle's own)
    a.in("f0", f0, (size_t)count * h->plant.k); a.in("val", val, (size_t)count * h->plant.nnz);
    { const int rc = kind_check(a, who); if (rc != EICOS_OK) return rc; }
    HIP_TRY(hipSetDevice(h->device));
    struct Group { const double *src, *shared; size_t width; DevBuf &buf; const double *&at; };
    Group grp[2] = {{f0, h->plant.a.base, (size_t)h->plant.k, h->d_plant_f0, h->plant.ibase}, {val, h->plant.a.val, (size_t)h->plant.nnz, h->d_plant_val, h->plant.ival}};
    for (Group &g : grp) {
        if (!g.src || g.width == 0) continue; // (a map without stored entries has no val rows to give)
        if (!g.buf) {
            HIP_TRY_AS("hipMalloc", g.buf.alloc((size_t)h->batch * g.width * sizeof(double)));
            HIP_TRY(launch_fill_rows(g.shared, (int)g.width, h->batch, g.buf.as<double>(), h->stream));
            g.at = g.buf.as<double>();
        }
        if (count > 0)
            HIP_TRY(hipMemcpyAsync(g.buf.as<double>() + (size_t)first * g.width, g.src, (size_t)count * g.width * sizeof(double),
                                   device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, h->stream));
    }
    h->map_gen++; // (eicos_batch_rollout_gradient: a recorded rollout belongs to the plant values it ran under)
    if (!device) HIP_TRY(hipStreamSynchronize(h->stream));
    return EICOS_OK;
}
int eicos_batch_set_plant_values(eicos_batch *h, int first, int count, const double *f0, const double *val) {
    return set_plant_values(h, first, count, f0, val, false, "eicos_batch_set_plant_values");
}
int eicos_batch_set_plant_values_device(eicos_batch *h, int first, int count, const double *df0, const double *dval) {
    return set_plant_values(h, first, count, df0, dval, true, "eicos_batch_set_plant_values_device");
}
int eicos_batch_plant_values(eicos_batch *h, int first, int count, double *f0_out, double *val_out) {
    if (!h) return fail(EICOS_E_INVALID, "NULL handle");
    const std::string w("eicos_batch_plant_values");
    { const int rc = plant_values_range(h, first, count, w); if (rc != EICOS_OK) return rc; }
    if (!f0_out && !val_out) return fail(EICOS_E_INVALID, w + ": f0_out and val_out are both NULL");
    Arrays a(false); // (for their kind alone: the rows come straight from the handle's own)
    a.out("f0_out", f0_out, (size_t)count * h->plant.k); a.out("val_out", val_out, (size_t)count * h->plant.nnz);
    const std::string fault = a.kind_fault(w.c_str(), false);
    if (!fault.empty()) return fail(EICOS_E_INVALID, fault + " (the outputs are host arrays)");
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream));
    const struct { double *dst; const double *rows, *shared; size_t width; } grp[2] = {
        {f0_out, h->plant.ibase, h->plant.a.base, (size_t)h->plant.k}, {val_out, h->plant.ival, h->plant.a.val, (size_t)h->plant.nnz}};
    for (const auto &g : grp) {
        if (!g.dst || g.width == 0 || count == 0) continue;
        if (g.rows) { HIP_TRY(hipMemcpy(g.dst, g.rows + (size_t)first * g.width, (size_t)count * g.width * sizeof(double), hipMemcpyDeviceToHost)); continue; }
        HIP_TRY(hipMemcpy(g.dst, g.shared, g.width * sizeof(double), hipMemcpyDeviceToHost));
        for (int q = 1; q < count; q++) std::memcpy(g.dst + (size_t)q * g.width, g.dst, g.width * sizeof(double));
    }
    return EICOS_OK;
}
int eicos_batch_has_plant_values(eicos_batch *h) {
    return h ? ((h->plant.ibase ? 1 : 0) | (h->plant.ival ? 2 : 0)) : fail(EICOS_E_INVALID, "NULL handle");
}
int eicos_batch_clear_plant_values(eicos_batch *h) {
    if (!h) return fail(EICOS_E_INVALID, "NULL handle");
    if (!h->d_plant_f0 && !h->d_plant_val) { h->map_gen++; return EICOS_OK; }
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream)); // (a sweep in flight may still read the rows that go away)
    h->d_plant_f0.reset(); h->d_plant_val.reset();
    h->plant.ibase = h->plant.ival = nullptr;
    h->map_gen++;
    return EICOS_OK;
}

// ---- fallback map: the backup output law u = v0 + V theta of steps whose solve ends in a class of the mask (launch.hpp: FallbackDev) ----
// The sixth map of install_map.  The counters sit in the gap between the descriptor and the arrays, so a map that is installed again
// starts them at zero.  Range kernels take the descriptor by value, the fused launches through a pointer (UpdArgs::fb).
static size_t fallback_counts_bytes(const eicos_batch *h) { return ((size_t)h->batch * sizeof(int) + 63) & ~(size_t)63; }
int eicos_batch_set_fallback_map(eicos_batch *h, unsigned mask, const eicos_affine_map *v) {
    if (!h) return fail(EICOS_E_INVALID, "NULL handle");
    const int k = h->param.k, r = h->out.r;
    const AffineGroup g = {v, r, k, "fallback map: ", "[0, k)"};
    const bool remove = !v || mask == 0;
    std::string msg;
    if (!remove) {
        if (mask & ~(unsigned)EICOS_SEL_ALL) return fail(EICOS_E_INVALID, g.who + "mask has bits above bit 11 (EICOS_SEL_UNSOLVED)");
        // (beside other classes the bit is idle and accepted, as in a retry policy: EICOS_SEL_NOT_OPTIMAL holds it)
        if (mask == EICOS_SEL_UNSOLVED) return fail(EICOS_E_INVALID, g.who + "mask is EICOS_SEL_UNSOLVED alone, and an attempted instance is never in that class");
        if (k == 0) return fail(EICOS_E_INVALID, g.who + "no parameter map (eicos_batch_set_param_map installs one)");
        if (r == 0) return fail(EICOS_E_INVALID, g.who + "no output map (eicos_batch_set_output_map installs one)");
        if (affine_fault(g, msg)) return fail(EICOS_E_INVALID, msg);
    }
    FallbackDev M{};
    M.mask = mask; M.k = k; M.r = r;
    const int rc = install_map(h, h->d_fb, h->fb, "fallback", &g, 1, fallback_counts_bytes(h), remove ? nullptr : &M, &M.a);
    if (rc != EICOS_OK || remove) return rc;
    // the counters: zeroed, and their address into the descriptor on both sides
    h->fb.counts = reinterpret_cast<int *>(h->d_fb.as<char>() + MAP_HEADER);
    hipError_t e = hipMemset(h->fb.counts, 0, fallback_counts_bytes(h));
    if (e == hipSuccess) e = hipMemcpy(h->d_fb.p, &h->fb, sizeof(FallbackDev), hipMemcpyHostToDevice);
    if (e != hipSuccess) { h->d_fb.reset(); h->fb = FallbackDev{}; return fail(EICOS_E_HIP, std::string("fallback map: ") + hipGetErrorString(e)); }
    return EICOS_OK;
}
int eicos_batch_fallback_mask(eicos_batch *h) { return h ? (int)h->fb.mask : fail(EICOS_E_INVALID, "NULL handle"); }
int eicos_batch_fallback_counts(eicos_batch *h, int first, int count, int *fired, int reset) {
    if (!h) return fail(EICOS_E_INVALID, "NULL handle");
    if (first < 0 || count < 0 || first > h->batch - count) return fail(EICOS_E_INVALID, "fallback counts: instance range out of bounds");
    if (count > 0 && !fired) return fail(EICOS_E_INVALID, "fallback counts: fired is NULL");
    if (count == 0) return EICOS_OK;
    if (!h->d_fb) { std::fill(fired, fired + count, 0); return EICOS_OK; } // (no map: nothing has fired since it was installed)
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream));
    HIP_TRY(hipMemcpy(fired, h->fb.counts + first, (size_t)count * sizeof(int), hipMemcpyDeviceToHost));
    if (reset) {
        HIP_TRY(hipMemsetAsync(h->fb.counts + first, 0, (size_t)count * sizeof(int), h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
    }
    return EICOS_OK;
}

// ---- matrix map: the stored values of G and A affine in theta ----
// The range path takes the groups by value, the fused step reads the descriptor through a pointer (UpdArgs::mmap).
int eicos_batch_set_matrix_map(eicos_batch *h, const eicos_affine_map *G, const eicos_affine_map *A) {
    if (!h) return fail(EICOS_E_INVALID, "NULL handle");
    const DevPat &D = h->dp;
    const int k = h->param.k;
    const AffineGroup g[2] = {{G, D.nnzG, k, "matrix map of G: ", "[0, k)"}, {A, D.nnzA, k, "matrix map of A: ", "[0, k)"}};
    const bool remove = !G && !A;
    std::string msg;
    for (int q = 0; q < 2; q++) {
        if (!g[q].map) continue;
        if (k == 0) return fail(EICOS_E_INVALID, g[q].who + "no parameter map (eicos_batch_set_param_map installs one)");
        if (g[q].rows == 0) return fail(EICOS_E_INVALID, g[q].who + "the pattern has no such matrix (it stores no entries)");
        if (affine_fault(g[q], msg)) return fail(EICOS_E_INVALID, msg);
    }
    // (against the parameter map as it is now; every call that consumes theta checks again: matrix_map_fits)
    if (G && D.m > 0 && !h->param.g[1].base) return fail(EICOS_E_INVALID, "matrix map of G: the parameter map has no h group (updateData reads h with Gpr)");
    if (A && D.p > 0 && !h->param.g[2].base) return fail(EICOS_E_INVALID, "matrix map of A: the parameter map has no b group (updateData reads b with Apr)");
    MatrixMapDev M{};
    M.k = k;
    return install_map(h, h->d_mat, h->mat, "matrix", g, 2, 0, remove ? nullptr : &M, M.g);
}

int eicos_batch_matrix_map_count(eicos_batch *h) { return h ? h->mat.k : fail(EICOS_E_INVALID, "NULL handle"); }
int eicos_batch_has_matrix_map(eicos_batch *h) {
    return h ? ((h->mat.g[0].base ? 1 : 0) | (h->mat.g[1].base ? 2 : 0)) : fail(EICOS_E_INVALID, "NULL handle");
}

// ---- shift map: the warm-start vectors x, y, z, s through a square affine map each ----
// Every solve launch of the handle carries the address of the descriptor (enqueue_solve).
int eicos_batch_set_shift_map(eicos_batch *h, const eicos_affine_map *x, const eicos_affine_map *y, const eicos_affine_map *z, const eicos_affine_map *sl) {
    if (!h) return fail(EICOS_E_INVALID, "NULL handle");
    const DevPat &D = h->dp;
    const AffineGroup g[4] = {{x, D.n, D.n, "shift map of x: ", "[0, rows)"}, {y, D.p, D.p, "shift map of y: ", "[0, rows)"},
                              {z, D.m, D.m, "shift map of z: ", "[0, rows)"}, {sl, D.m, D.m, "shift map of s: ", "[0, rows)"}};
    const bool remove = !x && !y && !z && !sl;
    std::string msg;
    for (int q = 0; q < 4; q++) {
        if (!g[q].map) continue;
        if (g[q].rows == 0) return fail(EICOS_E_INVALID, g[q].who + "the pattern has no such vector (it has no rows)");
        if (affine_fault(g[q], msg)) return fail(EICOS_E_INVALID, msg);
    }
    ShiftMapDev M{};
    return install_map(h, h->d_shift, h->shift, "shift", g, 4, 0, remove ? nullptr : &M, M.g);
}

int eicos_batch_has_shift_map(eicos_batch *h) {
    if (!h) return fail(EICOS_E_INVALID, "NULL handle");
    int bits = 0;
    for (int q = 0; q < 4; q++) if (h->shift.g[q].base) bits |= 1 << q;
    return bits;
}

int eicos_batch_has_plant_map(eicos_batch *h) { return h ? (h->plant.k > 0 ? 1 : 0) : fail(EICOS_E_INVALID, "NULL handle"); }
int eicos_batch_last_rollout_launches(eicos_batch *h) { return h ? h->rollout_launches : fail(EICOS_E_INVALID, "NULL handle"); }

// Fused: ONE solve launch whose workgroups run the steps of their instances themselves (kernels.hip: k_solve, plant_instance); the
// trajectories live in the handle's device buffer and the caller's arrays -- of any kind of memory -- are copied in before and out after.
// Not fused: the same buffer, and per step four launches on the stream, the step's theta rows in two contiguous [batch][k] buffers that
// take turns (the range kernels read and write rows k / r doubles apart; k_plant_range moves them into the trajectories).
// sens (eicos_batch_rollout_jacobian): every step also leaves J_t = d u_t / d theta_t and its refinement residuals in the handle's J and res
// trajectories (eicos_batch::d_rollJ) -- fused: k_roll_sens in the place of k_solve, still one launch; not fused: one adjoint launch in
// its contracted device form (what eicos_batch_param_jacobian_device enqueues) between the step's output and plant kernels, its rows
// moved into the trajectories on the stream.  No host synchronisation between the steps on either path.
// In pieces: the checks, the layout and the reserves (rollout_layout.hpp), rollout_fused or rollout_stepwise, the copies out.
// every check of a rollout that needs no layout, in front of the first allocation
static int rollout_checks(const eicos_batch *h, int steps, const double *theta0, const double *u_traj, bool sens, const double *J_traj) {
    if (!h) return fail(EICOS_E_INVALID, "NULL handle");
    if (steps < 1) return fail(EICOS_E_INVALID, "rollout: steps must be at least 1");
    if (h->param.k == 0) return fail(EICOS_E_INVALID, "no parameter map (eicos_batch_set_param_map installs one)");
    if (h->out.r == 0) return fail(EICOS_E_INVALID, "no output map (eicos_batch_set_output_map installs one)");
    if (h->plant.k == 0) return fail(EICOS_E_INVALID, "no plant map (eicos_batch_set_plant_map installs one)");
    const int k = h->param.k, r = h->out.r;
    if (h->plant.k != k || h->plant.r != r)
        return fail(EICOS_E_INVALID, "rollout: the plant map was installed for (k, r) = (" + std::to_string(h->plant.k) + ", " + std::to_string(h->plant.r) +
                                         "), the maps now installed have (" + std::to_string(k) + ", " + std::to_string(r) + "): install it again");
    { const int rc = matrix_map_fits(h); if (rc != EICOS_OK) return rc; }
    { const int rc = fallback_fits(h); if (rc != EICOS_OK) return rc; }
    if (!theta0) return fail(EICOS_E_INVALID, "rollout: theta0 is NULL");
    if (!u_traj) return fail(EICOS_E_INVALID, "rollout: u_traj is NULL");
    if (sens && !J_traj) return fail(EICOS_E_INVALID, "rollout_jacobian: J_traj is NULL");
    return EICOS_OK;
}
// the three buffers grown to the layout's totals, and every pointer of the call out of the layout
static int rollout_reserve(eicos_batch *h, const RolloutShape &s, const RolloutLayout &L, RolloutArrays &a) {
    if (s.sens) {
        h->held.invalidate();
        HIP_TRY_AS("hipMalloc", h->d_rollJ.reserve(L.rollJ_bytes, h->stream));
    }
    if (s.recording) {
        if (h->d_rollW.reserve(L.rollW_bytes, h->stream) != hipSuccess) {
            (void)hipGetLastError();
            return fail(EICOS_E_HIP, "rollout_jacobian: the record of a recording rollout (batch * steps * (r + 1) * (n + m + p) * 8, and one step more where the rollout is not fused: " + std::to_string(L.rollW_bytes) +
                                         " bytes) could not be allocated: record fewer steps or a smaller batch, or switch recording off");
        }
    }
    HIP_TRY_AS("hipMalloc", h->d_roll.reserve(L.roll_bytes, h->stream));
    a = L.in(h->d_roll.p, h->d_rollJ.p, h->d_rollW.p);
    return EICOS_OK;
}
// ONE solve launch whose workgroups run the steps of their instances; sens: k_roll_sens, with the contracted record in front of d_rollJ
static int rollout_fused(eicos_batch *h, const RolloutShape &s, const RolloutArrays &a) {
    const int rc = fused_step_begins(h, 5);
    if (rc != EICOS_OK) return rc;
    UpdArgs step;
    step.on = UPD_ROLL; step.roll = static_cast<const RolloutDev *>(a.roll_rec);
    step_maps(h, step, true, h->fb.mask != 0); // (the fallback record: every step's u row, and with sens its J and res rows: kernels.hip, rollout_record)
    if (s.sens) {
        const AdjointDev rec = contracted_record(h, true, 0, (int)s.k, a.J, a.res, s.recording ? &a.W : nullptr);
        HIP_TRY(hipMemcpyAsync(a.adj_rec, &rec, sizeof rec, hipMemcpyHostToDevice, h->stream));
    }
    return enqueue_solve(h, &step, -1, static_cast<const AdjointDev *>(a.adj_rec));
}
// one step's rows [batch][width] into row t of the trajectory [batch][steps][width], on the handle's stream
static int step_into_trajectory(eicos_batch *h, double *traj, const double *rows, size_t width, size_t t, size_t steps) {
    const size_t wb = width * sizeof(double);
    if (wb) HIP_TRY(hipMemcpy2DAsync(traj + t * width, steps * wb, rows, wb, wb, (size_t)h->batch, hipMemcpyDeviceToDevice, h->stream));
    return EICOS_OK;
}
// Per step four launches on the stream (five with sens), the step's theta rows in the two buffers of `cur` that take turns
static int rollout_stepwise(eicos_batch *h, const RolloutShape &s, const RolloutArrays &a) {
    const size_t row_b = s.k * sizeof(double);
    HIP_TRY(hipMemcpy2DAsync(a.cur, row_b, a.theta, (s.T + 1) * row_b, row_b, s.B, hipMemcpyDeviceToDevice, h->stream));
    for (size_t t = 0; t < s.T; t++) {
        const double *cur = a.cur + (t & 1) * s.B * s.k;
        double *next = a.cur + ((t + 1) & 1) * s.B * s.k;
        int rc = begin_update_timing(h);
        if (rc == EICOS_OK) rc = param_range(h, 0, h->batch, cur, nullptr);
        rc = end_update_timing(h, rc);
        if (rc == EICOS_OK) rc = enqueue_solve(h, nullptr);
        if (rc != EICOS_OK) return rc;
        HIP_TRY(launch_outputs(h->pslot, h->inst(), 0, h->batch, h->out, h->d_u, h->stream));
        if (h->fb.mask) HIP_TRY(launch_fallback(h->pslot, h->inst(), 0, h->batch, h->fb, cur, h->d_u, h->stream));
        if (s.sens) {
            rc = param_contracted(h, nullptr, h->batch, 0, nullptr, false, a.J1, "J", a.res1, true, "eicos_batch_rollout_jacobian", s.recording ? &a.W1 : nullptr);
            if (rc != EICOS_OK) return rc;
            if (h->fb.mask) HIP_TRY(launch_fallback_jacobian(h->pslot, h->inst(), 0, h->batch, h->fb, a.J1, a.res1, h->stream));
            if (s.recording) { // the step's rows into the record, as J is moved
                if (h->fb.mask) HIP_TRY(launch_fallback_records(h->pslot, h->inst(), 0, h->batch, h->fb, a.W1.Wc, a.W1.Wh, a.W1.Wb, h->stream));
                for (int q = 0; q < 6; q++)
                    if ((rc = step_into_trajectory(h, a.W.part(q), a.W1.part(q), a.W.width[q], t, s.T)) != EICOS_OK) return rc;
            }
            if ((rc = step_into_trajectory(h, a.J, a.J1, s.r * s.k, t, s.T)) != EICOS_OK) return rc;
            if ((rc = step_into_trajectory(h, a.res, a.res1, s.r, t, s.T)) != EICOS_OK) return rc;
        }
        HIP_TRY(launch_plant(h->pslot, h->inst(), 0, h->batch, h->roll, (int)t, cur, h->d_u, next, h->stream));
    }
    return EICOS_OK;
}
static int rollout_run(eicos_batch *h, int steps, const double *theta0, const double *w, double *u_traj, double *theta_traj,
                       int *exitcodes, int *iters, bool sens, double *J_traj, double *res_traj) {
    int rc = rollout_checks(h, steps, theta0, u_traj, sens, J_traj);
    if (rc != EICOS_OK) return rc;
    const int k = h->param.k, r = h->out.r;
    const bool fused = fused_rollout_fits(fit_shape(h), k, r, h->mat.k != 0) && env_knob("EICOS_FUSED_UPDATE", 1, 0, 1);
    const RolloutShape s{(size_t)h->batch, (size_t)steps, (size_t)k, (size_t)r, (size_t)h->dp.n, (size_t)h->dp.m, (size_t)h->dp.p,
                         w != nullptr, sens, sens && h->roll_recording, fused};
    const std::string fault = rollout_shape_fault(s);
    if (!fault.empty()) return fail(EICOS_E_INVALID, fault);
    HIP_TRY(hipSetDevice(h->device));
    const RolloutLayout L(s);
    RolloutArrays a;
    if ((rc = rollout_reserve(h, s, L, a)) != EICOS_OK) return rc;
    h->roll = RolloutDev{steps, h->plant, a.theta, a.u, a.w, a.codes, a.iters};
    const size_t row_b = s.k * sizeof(double);
    HIP_TRY(hipMemcpyAsync(a.roll_rec, &h->roll, sizeof(RolloutDev), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpy2DAsync(a.theta, (s.T + 1) * row_b, theta0, row_b, row_b, s.B, hipMemcpyDefault, h->stream)); // row 0 of every trajectory
    if (w) HIP_TRY(hipMemcpyAsync(a.w, w, L.w.bytes, hipMemcpyDefault, h->stream));
    if ((rc = fused ? rollout_fused(h, s, a) : rollout_stepwise(h, s, a)) != EICOS_OK) return rc;
    h->rollout_launches = fused ? 1 : steps;
    HIP_TRY(hipMemcpyAsync(u_traj, a.u, L.u.bytes, hipMemcpyDefault, h->stream));
    if (theta_traj) HIP_TRY(hipMemcpyAsync(theta_traj, a.theta, L.theta.bytes, hipMemcpyDefault, h->stream));
    if (exitcodes) HIP_TRY(hipMemcpyAsync(exitcodes, a.codes, L.codes.bytes, hipMemcpyDefault, h->stream));
    if (iters) HIP_TRY(hipMemcpyAsync(iters, a.iters, L.iters.bytes, hipMemcpyDefault, h->stream));
    if (sens) {
        HIP_TRY(hipMemcpyAsync(J_traj, a.J, L.J.bytes, hipMemcpyDefault, h->stream));
        if (res_traj) HIP_TRY(hipMemcpyAsync(res_traj, a.res, L.res.bytes, hipMemcpyDefault, h->stream));
        h->held.hold(s.B, steps, k, r, h->plant, h->map_gen, a.J, a.res, s.recording ? &a.W : nullptr);
    }
    HIP_TRY(hipStreamSynchronize(h->stream));
    return EICOS_OK;
}
int eicos_batch_rollout(eicos_batch *h, int steps, const double *theta0, const double *w, double *u_traj, double *theta_traj,
                        int *exitcodes, int *iters) {
    return rollout_run(h, steps, theta0, w, u_traj, theta_traj, exitcodes, iters, false, nullptr, nullptr);
}
int eicos_batch_rollout_jacobian(eicos_batch *h, int steps, const double *theta0, const double *w, double *u_traj, double *theta_traj,
                                 int *exitcodes, int *iters, double *J_traj, double *res_traj) {
    return rollout_run(h, steps, theta0, w, u_traj, theta_traj, exitcodes, iters, true, J_traj, res_traj);
}

// The backward sweep over the most recent eicos_batch_rollout_jacobian of the handle (launch.hpp: launch_rollout_backprop), behind
// everything on the handle's stream.  Every check stands in front of the first enqueue.  The host form stages its arrays in d_rollG
// and waits; the device form only enqueues.
// pv != NULL (eicos_batch_rollout_plant_gradient): the sweep also forms the gradient with respect to the plant's own entries from the
// caller's u and theta trajectories; grad_theta0 is optional then, one of the four outputs is not.
struct PlantGradArgs { const double *u_traj, *theta_traj; double *grad_f0, *grad_val; };
static int rollout_gradient(eicos_batch *h, const double *gu, const double *gtheta, double *grad_theta0, double *grad_w, bool device, const char *who,
                            const PlantGradArgs *pv = nullptr) {
    int rc = held_trajectory_fault(h, who, false);
    if (rc != EICOS_OK) return rc;
    const std::string w(who);
    if (!gu && !gtheta) return fail(EICOS_E_INVALID, w + ": gu and gtheta are both NULL");
    if (!pv && !grad_theta0) return fail(EICOS_E_INVALID, w + ": grad_theta0 is NULL");
    if (pv && !pv->u_traj) return fail(EICOS_E_INVALID, w + ": u_traj is NULL");
    if (pv && !pv->theta_traj) return fail(EICOS_E_INVALID, w + ": theta_traj is NULL");
    if (pv && !grad_theta0 && !grad_w && !pv->grad_f0 && !pv->grad_val) return fail(EICOS_E_INVALID, w + ": grad_theta0, grad_w, grad_f0 and grad_val are all NULL");
    const auto &held = h->held;
    const size_t B = (size_t)h->batch, T = (size_t)held.steps, k = (size_t)held.k, r = (size_t)held.r, nnz = (size_t)held.plant.nnz;
    const size_t n_gu = B * T * r, n_gt = B * (T + 1) * k, n_g0 = B * k, n_gw = B * T * k, n_gv = B * nnz;
    Arrays a(device); // (the plant-gradient form's four are NULL in the other)
    const int i_gu = a.in("gu", gu, n_gu), i_gt = a.in("gtheta", gtheta, n_gt), i_g0 = a.out("grad_theta0", grad_theta0, n_g0), i_gw = a.out("grad_w", grad_w, n_gw);
    const int i_u = a.in("u_traj", pv ? pv->u_traj : nullptr, n_gu), i_th = a.in("theta_traj", pv ? pv->theta_traj : nullptr, n_gt);
    const int i_gf = a.out("grad_f0", pv ? pv->grad_f0 : nullptr, n_g0), i_gv = a.out("grad_val", pv ? pv->grad_val : nullptr, n_gv);
    if ((rc = kind_check(a, who)) != EICOS_OK) return rc;
    const bool want_val = pv && pv->grad_val && nnz > 0;
    if (pv && !grad_theta0 && !grad_w && !pv->grad_f0 && !want_val) return EICOS_OK; // (grad_val alone of a map without stored entries: no row to form)
    if (rollout_backprop_lds((int)k, (int)r, want_val) > 48 * 1024)
        return fail(EICOS_E_INVALID, w + (want_val ? ": 4 k + 3 r doubles must fit 48 KB of LDS" : ": 3 k + 2 r doubles must fit 48 KB of LDS"));
    HIP_TRY(hipSetDevice(h->device));
    if ((rc = stage(h, h->d_rollG, a)) != EICOS_OK) return rc;
    rc = timed_adjoint_launch(h, "launch_rollout_backprop", [&] {
        return launch_rollout_backprop(held.plant, (int)T, h->batch, held.J(), a.dbl(i_gu), a.dbl(i_gt), a.dbl(i_g0), a.dbl(i_gw), h->stream,
                                       a.dbl(i_u), a.dbl(i_th), a.dbl(i_gf), a.dbl(i_gv));
    });
    return rc != EICOS_OK ? rc : unstage(h, a);
}
int eicos_batch_rollout_jacobian_steps(eicos_batch *h) { return h ? h->held.steps : fail(EICOS_E_INVALID, "NULL handle"); }
int eicos_batch_rollout_gradient(eicos_batch *h, const double *gu, const double *gtheta, double *grad_theta0, double *grad_w) {
    return rollout_gradient(h, gu, gtheta, grad_theta0, grad_w, false, "eicos_batch_rollout_gradient");
}
int eicos_batch_rollout_gradient_device(eicos_batch *h, const double *dgu, const double *dgtheta, double *dgrad_theta0, double *dgrad_w) {
    return rollout_gradient(h, dgu, dgtheta, dgrad_theta0, dgrad_w, true, "eicos_batch_rollout_gradient_device");
}
int eicos_batch_rollout_plant_gradient(eicos_batch *h, const double *gu, const double *gtheta, const double *u_traj, const double *theta_traj,
                                       double *grad_theta0, double *grad_w, double *grad_f0, double *grad_val) {
    const PlantGradArgs pv{u_traj, theta_traj, grad_f0, grad_val};
    return rollout_gradient(h, gu, gtheta, grad_theta0, grad_w, false, "eicos_batch_rollout_plant_gradient", &pv);
}
int eicos_batch_rollout_plant_gradient_device(eicos_batch *h, const double *dgu, const double *dgtheta, const double *du_traj, const double *dtheta_traj,
                                              double *dgrad_theta0, double *dgrad_w, double *dgrad_f0, double *dgrad_val) {
    const PlantGradArgs pv{du_traj, dtheta_traj, dgrad_f0, dgrad_val};
    return rollout_gradient(h, dgu, dgtheta, dgrad_theta0, dgrad_w, true, "eicos_batch_rollout_plant_gradient_device", &pv);
}

// ---- the cone scaling of the adjoint (include/eicos_amd.h: EICOS_ADJOINT_NT / _CENTRED): host state only, read by the next adjoint launch ----
int eicos_batch_set_adjoint_scaling(eicos_batch *h, int mode) {
    if (!h) return fail(EICOS_E_INVALID, "NULL handle");
    if (mode != EICOS_ADJOINT_NT && mode != EICOS_ADJOINT_CENTRED)
        return fail(EICOS_E_INVALID, "set_adjoint_scaling: mode must be EICOS_ADJOINT_NT (0) or EICOS_ADJOINT_CENTRED (1), got " + std::to_string(mode));
    h->adjoint_scaling = mode;
    return EICOS_OK;
}
int eicos_batch_adjoint_scaling(eicos_batch *h) { return h ? h->adjoint_scaling : fail(EICOS_E_INVALID, "NULL handle"); }

// ---- a recording rollout and the gradient with respect to the controller's own data (include/eicos_amd.h) ----
size_t eicos_data_gradient_size(void) { return sizeof(eicos_data_gradient); }
int eicos_batch_set_rollout_recording(eicos_batch *h, int on) {
    if (!h) return fail(EICOS_E_INVALID, "NULL handle");
    h->roll_recording = on != 0;
    if (!on && (h->d_rollW || h->d_rollD)) { // the record goes with the switch: up to gigabytes (a sweep in flight may still read it)
        HIP_TRY(hipSetDevice(h->device));
        HIP_TRY(hipStreamSynchronize(h->stream));
        h->d_rollW.reset(); h->d_rollD.reset();
        h->held.drop_rows();
    }
    return EICOS_OK;
}
int eicos_batch_rollout_recording(eicos_batch *h) { return h ? (h->roll_recording ? 1 : 0) : fail(EICOS_E_INVALID, "NULL handle"); }
int eicos_batch_rollout_records(eicos_batch *h, double *Wc, double *Wh, double *Wb, double *x_rec, double *y_rec, double *z_rec) {
    const char *who = "eicos_batch_rollout_records";
    int rc = held_trajectory_fault(h, who, true, false); // (the record is what the rollout left, whatever has been installed since)
    if (rc != EICOS_OK) return rc;
    const RecordRows &R = h->held.records();
    const size_t rows = h->held.rows;
    double *const dst[6] = {Wc, Wh, Wb, x_rec, y_rec, z_rec};
    const char *const name[6] = {"Wc", "Wh", "Wb", "x_rec", "y_rec", "z_rec"};
    Arrays a(false); // (for their kind alone: the rows come straight from the record)
    for (int q = 0; q < 6; q++) a.out(name[q], dst[q], rows * R.width[q]);
    if ((rc = kind_check(a, who, false)) != EICOS_OK) return rc;
    HIP_TRY(hipSetDevice(h->device));
    for (int q = 0; q < 6; q++)
        if (dst[q] && R.width[q]) HIP_TRY(hipMemcpyAsync(dst[q], R.part(q), rows * R.width[q] * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return EICOS_OK;
}
// The second backward sweep (launch.hpp: launch_rollout_data_backprop), behind everything on the handle's stream.  Every check stands in
// front of the first enqueue.  The host form stages its arrays in d_rollD and waits; the device form only enqueues.
static int rollout_data_gradient(eicos_batch *h, const double *gu, const double *gtheta, const double *theta_traj, const eicos_data_gradient *out,
                                 bool device, const char *who) {
    int rc = held_trajectory_fault(h, who, true);
    if (rc != EICOS_OK) return rc;
    const std::string w(who);
    if (!gu && !gtheta) return fail(EICOS_E_INVALID, w + ": gu and gtheta are both NULL");
    if (!theta_traj) return fail(EICOS_E_INVALID, w + ": theta_traj is NULL");
    if (!out) return fail(EICOS_E_INVALID, w + ": out is NULL");
    const DevPat &P = h->dp;
    const auto &held = h->held;
    const size_t B = (size_t)h->batch, T = (size_t)held.steps, k = (size_t)held.k, r = (size_t)held.r;
    const size_t n = (size_t)P.n, m = (size_t)P.m, p = (size_t)P.p;
    // (held.gen == map_gen: the maps on the handle are the ones the rollout ran under)
    const size_t nnzC = (size_t)h->param_nnz[0], nnzH = (size_t)h->param_nnz[1], nnzB = (size_t)h->param_nnz[2], nnzU = (size_t)h->out_nnz;
    const char *slope[3] = {"grad_Cval", "grad_Hval", "grad_Bval"};
    double *const sl[3] = {out->grad_Cval, out->grad_Hval, out->grad_Bval};
    for (int q = 0; q < 3; q++)
        if (sl[q] && !h->param.g[q].base) return fail(EICOS_E_INVALID, w + ": " + slope[q] + " asked, but the parameter map has no " + "chb"[q] + " group");
    // The arrays: the sweep's own rows (launch.hpp: DataGradDev::stage), the three inputs, and the outputs in the order of the struct
    // -- a group the pattern or the map does not have has no width: no row to form
    const struct { double *host; size_t width; const char *name; } o[10] = {
        {out->grad_c, n, "grad_c"}, {out->grad_h, m, "grad_h"}, {out->grad_b, p, "grad_b"}, {out->grad_G, (size_t)P.nnzG, "grad_G"}, {out->grad_A, (size_t)P.nnzA, "grad_A"},
        {out->grad_Cval, nnzC, "grad_Cval"}, {out->grad_Hval, nnzH, "grad_Hval"}, {out->grad_Bval, nnzB, "grad_Bval"}, {out->grad_u0, r, "grad_u0"}, {out->grad_Uval, nnzU, "grad_Uval"}};
    bool any = false;
    for (const auto &q : o) any = any || q.host;
    if (!any) return fail(EICOS_E_INVALID, w + ": every output of out is NULL");
    const size_t n_gu = B * T * r, n_gt = B * (T + 1) * k;
    Arrays a(device);
    const int i_stage = a.fixed((size_t)rollout_data_backprop_grid(h->batch) * (n + m + p) * sizeof(double));
    const int i_gu = a.in("gu", gu, n_gu), i_gt = a.in("gtheta", gtheta, n_gt), i_th = a.in("theta_traj", theta_traj, n_gt);
    int i_o[10];
    for (int q = 0; q < 10; q++) i_o[q] = a.out(o[q].name, o[q].host, B * o[q].width);
    if ((rc = kind_check(a, who)) != EICOS_OK) return rc;
    if (rollout_backprop_lds((int)k, (int)r) > 48 * 1024) return fail(EICOS_E_INVALID, w + ": 3 k + 2 r doubles must fit 48 KB of LDS");
    HIP_TRY(hipSetDevice(h->device));
    if ((rc = stage(h, h->d_rollD, a)) != EICOS_OK) return rc;
    DataGradDev D{};
    D.stage = a.dbl(i_stage);
    D.gu = a.dbl(i_gu); D.gth = a.dbl(i_gt); D.theta = a.dbl(i_th);
    const RecordRows &R = held.records();
    D.J = held.J();
    D.Wc = R.Wc; D.Wh = R.Wh; D.Wb = R.Wb; D.x = R.x; D.y = R.y; D.z = R.z;
    D.pmap = h->param; D.omap = h->out;
    D.grad_c = a.dbl(i_o[0]); D.grad_h = a.dbl(i_o[1]); D.grad_b = a.dbl(i_o[2]); D.grad_G = a.dbl(i_o[3]); D.grad_A = a.dbl(i_o[4]);
    D.grad_val[0] = a.dbl(i_o[5]); D.grad_val[1] = a.dbl(i_o[6]); D.grad_val[2] = a.dbl(i_o[7]); D.grad_u0 = a.dbl(i_o[8]); D.grad_Uval = a.dbl(i_o[9]);
    rc = timed_adjoint_launch(h, "launch_rollout_data_backprop", [&] { return launch_rollout_data_backprop(h->pslot, held.plant, (int)T, h->batch, D, h->stream); });
    return rc != EICOS_OK ? rc : unstage(h, a);
}
int eicos_batch_rollout_data_gradient(eicos_batch *h, const double *gu, const double *gtheta, const double *theta_traj, const eicos_data_gradient *out) {
    return rollout_data_gradient(h, gu, gtheta, theta_traj, out, false, "eicos_batch_rollout_data_gradient");
}
int eicos_batch_rollout_data_gradient_device(eicos_batch *h, const double *dgu, const double *dgtheta, const double *dtheta_traj, const eicos_data_gradient *dout) {
    return rollout_data_gradient(h, dgu, dgtheta, dtheta_traj, dout, true, "eicos_batch_rollout_data_gradient_device");
}

int eicos_batch_solution(eicos_batch *h, double *x) {
    if (!h || !x) return fail(EICOS_E_INVALID, "NULL argument");
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return fetch_rows(h, x, h->dp.i_x, h->dp.n);
}

int eicos_batch_duals(eicos_batch *h, double *y, double *z, double *s) {
    if (!h) return fail(EICOS_E_INVALID, "NULL handle");
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream));
    int rc = fetch_rows(h, y, h->dp.i_y, h->dp.p);
    if (rc == EICOS_OK) rc = fetch_rows(h, z, h->dp.i_z, h->dp.m);
    if (rc == EICOS_OK) rc = fetch_rows(h, s, h->dp.i_s, h->dp.m);
    return rc;
}

int eicos_batch_solution_device(eicos_batch *h, const double **dx, size_t *stride) {
    if (!h || !dx || !stride) return fail(EICOS_E_INVALID, "NULL argument");
    *dx = h->inst() + h->dp.i_x; *stride = h->dp.inst_stride;
    return EICOS_OK;
}

int eicos_batch_shared_values(eicos_batch *h) {
    if (!h) return fail(EICOS_E_INVALID, "NULL handle");
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream));
    int v = -1;
    HIP_TRY(hipMemcpy(&v, h->d_shared.p, sizeof(int), hipMemcpyDeviceToHost));
    return (h->shared_on && v >= 0) ? 1 : 0;
}

int eicos_batch_kernel_build(eicos_batch *h) {
    if (!h) return fail(EICOS_E_INVALID, "NULL handle");
    return h->ldsres ? 1 : (h->w2 ? 2 : (h->ubl ? 3 : 0));
}

int eicos_internal_device(const eicos_batch *h) { return h ? h->device : -1; }
int eicos_internal_plant_dims(const eicos_batch *h, int *k, int *nnz) {
    if (!h || !k || !nnz) return EICOS_E_INVALID;
    *k = h->plant.k; *nnz = h->plant.nnz;
    return EICOS_OK;
}
int eicos_internal_map_nnz(const eicos_batch *h, int *nnz_chb, int *nnz_u) {
    if (!h || !nnz_chb || !nnz_u) return EICOS_E_INVALID;
    for (int q = 0; q < 3; q++) nnz_chb[q] = h->param_nnz[q];
    *nnz_u = h->out_nnz;
    return EICOS_OK;
}
// ms from the start of `from`'s most recent solve to the end of `to`'s (two handles on ONE device: the span of a device that holds
// several shards of an eicos_multi); both solves must have completed
int eicos_internal_solve_span_ms(eicos_batch *from, eicos_batch *to, float *ms) {
    if (!from || !to || !ms || from->device != to->device || !from->solve_timed || !to->solve_timed) return fail(EICOS_E_INVALID, "bad argument");
    HIP_TRY(hipSetDevice(from->device));
    HIP_TRY(hipEventSynchronize(from->ev_s1));
    HIP_TRY(hipEventSynchronize(to->ev_s1));
    HIP_TRY(hipEventElapsedTime(ms, from->ev_s0, to->ev_s1));
    return EICOS_OK;
}

int eicos_batch_dims(eicos_batch *h, eicos_dims *o) {
    if (!h || !o) return fail(EICOS_E_INVALID, "NULL argument");
    const Symbolic &S = h->sym;
    o->n = S.n; o->m = S.m; o->p = S.p; o->l = S.l; o->ncones = S.nc; o->dim_K = S.N; o->nnzA = S.nnzA; o->nnzG = S.nnzG;
    o->nnzK = S.nnzK; o->nnzL = S.nnzL; o->nlevels = S.nlev; o->order_mode = S.order_mode; o->batch = h->batch; o->device = h->device;
    o->factor_pairs = S.npairs;
    o->inst_bytes = h->dp.inst_stride * sizeof(double); o->work_bytes = h->dp.work_stride * sizeof(double);
    o->pattern_bytes = h->pattern_ints * sizeof(int);
    o->threads_per_block = h->threads; o->resident_blocks = h->grid; o->lds_bytes = (int)h->dyn_lds; o->instances_per_block = 1;
    o->lds_resident = h->ldsres; o->factor_path = h->sym.tile; o->cone_order = h->sym.cone_order; o->dual_rhs = h->dp.dual;
    o->arithmetic_profile = h->arith_profile; o->apex_nodes = h->dp.apex_na; o->solo_slices = h->dp.nfs_solo + h->dp.nbs_solo;
    o->shared_operands = h->d_shop ? 1 : 0;
    o->iterate_park = h->dp.xpark;
    return EICOS_OK;
}

static int elapsed(eicos_batch *h, bool ok, hipEvent_t a, hipEvent_t b, float *ms) {
    if (!h || !ms) return fail(EICOS_E_INVALID, "NULL argument");
    if (!ok) return fail(EICOS_E_INVALID, "nothing timed yet");
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipEventSynchronize(b));
    HIP_TRY(hipEventElapsedTime(ms, a, b));
    return EICOS_OK;
}
int eicos_batch_last_solve_ms(eicos_batch *h, float *ms) { return elapsed(h, h && h->solve_timed, h ? h->ev_s0 : nullptr, h ? h->ev_s1 : nullptr, ms); }
int eicos_batch_last_adjoint_ms(eicos_batch *h, float *ms) { return elapsed(h, h && h->adjoint_timed, h ? h->ev_a0 : nullptr, h ? h->ev_a1 : nullptr, ms); }
int eicos_batch_last_update_ms(eicos_batch *h, float *ms) { return elapsed(h, h && h->update_timed, h ? h->ev_u0 : nullptr, h ? h->ev_u1 : nullptr, ms); }
// Durations (ms, HIP events on the handle's stream) of the most recent launches, oldest first: which = 0 the solve launches, 1 the
// updateData calls, 2 the span from the start of the updateData call that preceded a solve launch to the end of that solve (one "step").  Returns how many were written (<= cap, <= 64: the ring's depth); waits for the most recent one to finish.
int eicos_batch_ms_history(eicos_batch *h, int which, float *ms, int cap) {
    if (!h || !ms || cap < 0 || which < 0 || which > 2) return fail(EICOS_E_INVALID, "bad argument");
    hipEvent_t (*ring)[2] = which != 1 ? h->ring_s : h->ring_u;
    const long total = which != 1 ? h->n_solve_rec : h->n_update_rec;
    if (which != 1 ? !h->solve_timed : !h->update_timed) return 0;
    const int cnt = (int)std::min<long>(std::min<long>(cap, eicos_batch::EV_RING), total);
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipEventSynchronize(which != 1 ? h->ev_s1 : h->ev_u1));
    for (int i = 0; i < cnt; i++) {
        const long at = (total - cnt + i) % eicos_batch::EV_RING;
        hipEvent_t *slot = ring[at];
        // (which = 2: the step's span.  The update ring turns as fast as the solve ring when updateData and solve alternate -- the caller's step --
        // so the start event a solve slot remembers is still that step's; with several updates per solve the span is NaN or too short: documented)
        if (hipEventElapsedTime(&ms[i], which == 2 ? h->ring_step0[at] : slot[0], slot[1]) != hipSuccess) { (void)hipGetLastError(); ms[i] = NAN; } // (a call that failed half way)
    }
    return cnt;
}

int eicos_debug_factor(eicos_batch *h, int inst, double *Dout, double *Uout) {
    if (!h || inst < 0 || inst >= h->batch) return fail(EICOS_E_INVALID, "bad argument");
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream));
    HIP_TRY(launch_debug_factor(h->pslot, h->inst(), h->work(), inst, h->threads, h->sym.tile ? h->dyn_lds : 0, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    const DevPat &P = h->dp;
    if (h->sym.tile) { // tiles -> the scalar view (D per elimination position, U = L D per CSC entry of L)
        const Symbolic &S = h->sym;
        const TilePlan &TP = h->tiles;
        std::vector<double> Dv((size_t)TP.N16), LR((size_t)TP.nt * 256 + 1);
        HIP_TRY(hipMemcpy(Dv.data(), h->work() + P.w_D, Dv.size() * sizeof(double), hipMemcpyDeviceToHost));
        if (TP.nt) HIP_TRY(hipMemcpy(LR.data(), h->work() + P.w_LR, (size_t)TP.nt * 256 * sizeof(double), hipMemcpyDeviceToHost));
        if (Dout) for (int j = 0; j < S.N; j++) Dout[j] = Dv[TP.slot[j]];
        if (Uout) {
            // the diagonal tiles themselves (strictly lower part, row-major) as the factorisation's triangular solves read them
            std::vector<double> Ld((size_t)TP.nb * 256, 0.0);
            HIP_TRY(hipMemcpy(Ld.data(), h->work() + P.w_DL, Ld.size() * sizeof(double), hipMemcpyDeviceToHost));
            std::vector<int> colj(S.nnzL);
            for (int j = 0; j < S.N; j++) for (int e = S.Lp[j]; e < S.Lp[j + 1]; e++) colj[e] = j;
            std::vector<double> ub;
            if (S.tile == 2) { // hybrid: the columns below the top block are in the scalar backward slots
                ub.resize((size_t)P.nUB + 1);
                HIP_TRY(hipMemcpy(ub.data(), h->work() + P.w_UB, (size_t)P.nUB * sizeof(double), hipMemcpyDeviceToHost));
            }
            for (int e = 0; e < S.nnzL; e++) {
                if (S.tile == 2 && colj[e] < S.n0) { Uout[e] = ub[h->posB[e]]; continue; }
                const int rr = TP.Le_rc[e] >> 4, cc = TP.Le_rc[e] & 15;
                const double lv = TP.Le_tile[e] >= 0 ? LR[(size_t)TP.Le_tile[e] * 256 + tile_res(rr, cc)] : Ld[(size_t)(-1 - TP.Le_tile[e]) * 256 + rr * 16 + cc];
                Uout[e] = lv * Dv[TP.slot[colj[e]]];
            }
        }
        return EICOS_OK;
    }
    if (Dout) HIP_TRY(hipMemcpy(Dout, h->work() + h->dp.w_D, (size_t)h->sym.N * sizeof(double), hipMemcpyDeviceToHost));
    if (Uout) {
        std::vector<double> ub((size_t)h->ub_len + 1);
        HIP_TRY(hipMemcpy(ub.data(), h->work() + h->dp.w_UB, (size_t)h->ub_len * sizeof(double), hipMemcpyDeviceToHost));
        for (int e = 0; e < h->dp.nnzL; e++) Uout[e] = ub[h->posB[e]];
    }
    return EICOS_OK;
}

int eicos_debug_kkt(eicos_batch *h, int inst, int *rows, int *cols, double *vals) {
    if (!h || inst < 0 || inst >= h->batch) return fail(EICOS_E_INVALID, "bad argument");
    const Symbolic &S = h->sym;
    const DevPat &D = h->dp;
    if (rows) std::copy(S.K_row.begin(), S.K_row.end(), rows);
    if (cols) std::copy(S.K_col.begin(), S.K_col.end(), cols);
    if (vals) {
        HIP_TRY(hipSetDevice(h->device));
        HIP_TRY(hipStreamSynchronize(h->stream));
        std::vector<double> slab(D.inst_stride);
        HIP_TRY(hipMemcpy(slab.data(), h->inst() + (size_t)inst * D.inst_stride, D.inst_stride * sizeof(double), hipMemcpyDeviceToHost));
        for (int e = 0; e < S.nnzK; e++) {
            int off;
            switch (S.K_kind[e]) { // same sources as the factor's value stream (srcoff in plan_step.cpp)
            case SRC_A: off = D.i_Av + S.K_src[e]; break;
            case SRC_G: off = D.i_Gv + S.K_src[e]; break;
            case SRC_V: off = D.i_Vv + S.K_src[e]; break;
            case SRC_POSDELTA: off = D.i_cst + 0; break;
            case SRC_NEGDELTA: off = D.i_cst + 1; break;
            default: off = D.i_cst + 2; break;
            }
            vals[e] = slab[off];
        }
    }
    return EICOS_OK;
}

int eicos_debug_scalings(eicos_batch *h, int inst, const double *s, const double *z, double *V, int *ran) {
    if (!h || inst < 0 || inst >= h->batch || !s || !z) return fail(EICOS_E_INVALID, "bad argument");
    const DevPat &D = h->dp;
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (!h->d_flag) HIP_TRY_AS("hipMalloc", h->d_flag.alloc(16 * sizeof(int)));
    double *I = h->inst() + (size_t)inst * D.inst_stride;
    if (D.m > 0) {
        HIP_TRY(hipMemcpy(I + D.i_s, s, (size_t)D.m * sizeof(double), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(I + D.i_z, z, (size_t)D.m * sizeof(double), hipMemcpyHostToDevice));
    }
    HIP_TRY(launch_debug_scalings(h->pslot, h->inst(), h->work(), inst, h->d_flag.as<int>(), h->threads, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    int ok = 0;
    HIP_TRY(hipMemcpy(&ok, h->d_flag.p, sizeof(int), hipMemcpyDeviceToHost));
    if (ran) *ran = ok;
    if (V && D.nV > 0) HIP_TRY(hipMemcpy(V, I + D.i_Vv, (size_t)D.nV * sizeof(double), hipMemcpyDeviceToHost));
    return EICOS_OK;
}

int eicos_debug_trace(eicos_batch *h, int inst, double *out) {
    if (!h || !out || inst < 0 || inst >= h->batch) return fail(EICOS_E_INVALID, "bad argument");
    // (a subset launch: its own count decides, and only its instances have a slot)
    const int launched = h->last_subset ? h->last_count : h->batch;
    if (launched > h->grid) return fail(EICOS_E_INVALID, h->last_subset ? "trace is per workspace slot: needs the subset's count <= resident instances"
                                                                         : "trace is per workspace slot: needs batch <= resident instances");
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream));
    int slot = inst;
    if (h->last_ordered) { // the launch took the instances through the order array: slot q holds instance order[q], q < launched
        std::vector<int> ord(launched);
        HIP_TRY(hipMemcpy(ord.data(), h->queue() + 16, (size_t)launched * sizeof(int), hipMemcpyDeviceToHost));
        slot = (int)(std::find(ord.begin(), ord.end(), inst) - ord.begin());
        if (slot >= launched) return fail(EICOS_E_INVALID, h->last_subset ? "instance not in the last launch" : "instance not found in the launch order");
    }
    HIP_TRY(hipMemcpy(out, h->work() + (size_t)slot * h->dp.work_stride + h->dp.w_trace,
                      (size_t)TRACE_ROWS * TRACE_COLS * sizeof(double), hipMemcpyDeviceToHost));
    return EICOS_OK;
}

int eicos_debug_pattern(eicos_batch *h, int *perm, int *Lp, int *Li) {
    if (!h) return fail(EICOS_E_INVALID, "NULL handle");
    const Symbolic &S = h->sym;
    if (perm) std::copy(S.perm.begin(), S.perm.end(), perm);
    if (Lp) std::copy(S.Lp.begin(), S.Lp.end(), Lp);
    if (Li) std::copy(S.Li.begin(), S.Li.end(), Li);
    return EICOS_OK;
}


} // extern "C"
