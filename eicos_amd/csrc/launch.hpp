// Host-callable launchers of the kernels in kernels.hip.
#pragma once
#include <hip/hip_runtime_api.h>
#include "device_types.hpp"

namespace eicos {
// Fused updateData (eicos_batch_update_solve): when `on`, every workgroup of the solve kernel first runs updateData for the instance it is
// about to solve, reading row `instance` of these [batch][...] arrays (NULL = keep the group; device or pinned host memory), and -- x != NULL
// -- writes the instance's solution to row `instance` of x [batch][n] when it is done.
// STAGED host arrays (pageable memory): the arrays are the handle's pinned staging buffer, which the host fills chunk by chunk WHILE the
// kernel runs -- flags[instance / chunk] == seq once the chunk holding an instance has been copied (pinned, host-written); the workgroup polls
// it before it touches the instance's rows (bounded: after ~5 s it gives up and raises *err).
// on = UPD_FULL: updateData (G, A, c, h, b); on = UPD_RHS: the right-hand-side-only update (c, h, b scaled by the stored scalings; G, A
// unused); on = UPD_PARAM: the parametric update (eicos_batch_update_param_solve) -- row `instance` of theta [batch][pmap->k] expanded
// through *pmap, the five arrays unused; 0: off.
// rows_at != 0 with on = UPD_PARAM (eicos_batch_update_param_solve_subset: a SUBSET launch): theta, x and u are [count][...] arrays in the
// order of the caller's list -- the row of instance `id` is rows[id], the ROW MAP the selection kernel of this launch has written
// (SolveLaunch::rows).  The map lives in the handle's queue allocation, `batch` ints starting at int rows_at of it.  k_solve parks
// rows_at in its LDS state once and passes `id` on as it always does; the per-instance functions that read or write a caller's row
// (kernels.hip: list_row) translate it.  Slab addresses always come from id.
// u != NULL (any mode, 0 included): row `instance` of u [batch][omap->r] = the output map applied to the instance's x, written like x.
// The two maps stay in device memory and travel as pointers: a launch that uses neither pays four words of kernel arguments for them.
// on = UPD_ROLL with roll != NULL (eicos_batch_rollout; theta and u unused): the workgroup takes its instance through roll->steps closed-loop
// steps before it pulls the next one -- per step the parametric update from row t of the instance's theta trajectory, the solve, the
// output row into the u trajectory, the exit code and iteration count into their records, and the plant map, which forms row t + 1 of the
// theta trajectory (RolloutDev, below).  Every other mode leaves roll NULL and pays one more word of kernel arguments for it.
enum { UPD_FULL = 1, UPD_RHS = 2, UPD_PARAM = 3, UPD_ROLL = 4 };
struct AffineDev { const double *base; const int *rowptr, *col; const double *val; };
struct ParamMapDev { int k; AffineDev g[3]; };
// Output map (eicos_batch_set_output_map): u = base + U x, r rows, CSR with n columns, in device memory, shared by every instance
struct OutMapDev { int r; AffineDev a; };
// Plant map (eicos_batch_set_plant_map): theta+ = base + F z, k rows, CSR with k + r columns over z = [theta (k) | u (r)], in device
// memory, shared by every instance; k, r = the parameter and output counts it was validated for.
// Per-instance plant values (eicos_batch_set_plant_values): ibase [batch][k] / ival [batch][nnz] in device memory, nnz = rowptr[k] --
// instance i reads row i of them in the place of a.base / a.val, the pattern stays the shared one; NULL: that group is the shared one.
struct PlantMapDev { int k, r; AffineDev a; const double *ibase, *ival; int nnz; };
// the map as instance `id` reads it (uniform id: the two rows stay scalar addresses)
#if defined(__HIPCC__)
__host__ __device__
#endif
inline AffineDev plant_of(const PlantMapDev &M, size_t id) {
    AffineDev A = M.a;
    if (M.ibase) A.base = M.ibase + id * (size_t)M.k;
    if (M.ival) A.val = M.ival + id * (size_t)M.nnz;
    return A;
}
// One rollout, in device memory: theta [batch][steps + 1][k] (row 0 given, the others written by the plant map), u [batch][steps][r],
// w [batch][steps][k] (NULL: no disturbance), codes / iters [batch][steps]
struct RolloutDev { int steps; PlantMapDev plant; double *theta, *u; const double *w; int *codes, *iters; };
// Matrix map (eicos_batch_set_matrix_map): the stored values of G and A affine in theta -- g[0] with nnzG rows, g[1] with nnzA rows, in the
// CSC order of Gpr / Apr, CSR with k columns, in device memory, shared by every instance; base == NULL: that matrix is not mapped; k = the
// parameter count it was validated for
struct MatrixMapDev { int k; AffineDev g[2]; };
// Shift map (eicos_batch_set_shift_map): the warm-start vectors x, y, z, s of an instance through one square affine map each -- g[0..3] with
// n, p, m, m rows and as many columns, CSR, in device memory, shared by every instance; base == NULL: that vector is not shifted
struct ShiftMapDev { AffineDev g[4]; };
struct RetryDev; // (below, behind SolveCfg)
// Fallback map (eicos_batch_set_fallback_map): the backup output law u = base + V theta, r rows, CSR with k columns, in device memory,
// shared by every instance; mask = the exit classes (exit_class.hpp) of a step's FINAL record whose u row comes from this law instead of
// from the output map; k, r = the parameter and output counts it was validated for; counts [batch] = steps per instance whose u row the
// law has formed since the last reset, bumped by the workgroup (fused) or the one thread (range kernel) that owns the instance.
struct FallbackDev { unsigned mask; int k, r; AffineDev a; int *counts; };
struct UpdArgs { // UpdArgs{} = the neutral launch: no fused step, no maps; every builder assigns fields by name
    // inputs: rows of the five updateData arrays, [batch][...]
    const double *G = nullptr, *A = nullptr, *c = nullptr, *h = nullptr, *b = nullptr;
    // outputs: x [batch][n], and the mode (UPD_*, 0: no fused step)
    double *x = nullptr; int on = 0;
    int rows_at = 0; // a parametric step over a chosen subset: where in the queue allocation (in ints) its row map starts; 0: row = instance (above)
    // staging: ready flags of the chunks (NULL: nothing is staged), instances per chunk, the flag value of this launch, the time-out word
    const unsigned *flags = nullptr; int chunk = 1; unsigned seq = 0; int *err = nullptr;
    // maps (device copies of the handle's descriptors) with the input theta and the output u of the parametric step
    const ParamMapDev *pmap = nullptr; const OutMapDev *omap = nullptr; const double *theta = nullptr; double *u = nullptr;
    const RolloutDev *roll = nullptr;
    const MatrixMapDev *mmap = nullptr; // UPD_PARAM / UPD_ROLL with a matrix map: the step is a full updateData from theta (kernels.hip: matrix_param_instance)
    // every-launch fields, mode 0 included.  smap: a solve that warm-starts an instance first takes its x, y, z, s through this map
    // (kernels.hip: shift_instance); NULL: no shift map.  One more word of kernel arguments, and one pointer test per instance.
    const ShiftMapDev *smap = nullptr;
    // retry: the handle's retry policy (eicos_batch_set_retry), a record in device memory; NULL: none.  An instance whose solve ends in a
    // class of the policy's mask is solved once more by the same workgroup, under the policy's settings, before anything reads its result
    // (kernels.hip: retry_between).  One more word of kernel arguments, and one pointer test per instance.
    const RetryDev *retry = nullptr;
    // fb: the handle's fallback map (eicos_batch_set_fallback_map), a record in device memory; NULL: none.  Only launches that hold theta
    // carry it (on = UPD_PARAM with u, UPD_ROLL): an instance whose final record -- after the second attempt, when the retry policy took
    // one -- is in a class of the map's mask gets its u row from the law (kernels.hip: fallback_instance).  One more word of kernel
    // arguments, and one pointer test per instance.
    const FallbackDev *fb = nullptr;
    // shared: the handle's shared-values word (eicos_batch_shared_values), read by thread 0 once per instance before the
    // instance's solve.  -1: every instance streams the product values (the sliced-ELL copies of [A' G'], A, G and the G tiles) of its own
    // slab; r >= 0: every instance of the batch holds the bits of instance r there, and all of them stream instance r's.  NULL counts as -1.
    const int *shared = nullptr;
};
// the fused step writes matrix values of its instances: full updateData; a parametric step or a rollout under a matrix map (the host then
// drops the handle's shared values in front of the launch: api.cpp, shared_clear)
inline bool writes_matrix_values(const UpdArgs &a) { return a.on == UPD_FULL || ((a.on == UPD_PARAM || a.on == UPD_ROLL) && a.mmap); }
// Runtime solver settings (eicos_batch_set_settings; eicos_settings of include/eicos_amd.h, same fields and defaults): one by-value argument
// of k_solve, copied into LDS by thread 0 (kernels.hip: Sh::cfg) before the workgroup's first instance, where the stage functions read
// it -- the exit test and the two infeasibility-residual comparisons (tolerances), the iteration cap, and kkt_solve's refinement stop test
// (linsysacc, irerrfact, nitref).  Every other constant of the reference's Settings stays compile-time (kernels.hip).
struct SolveCfg { double feastol, abstol, reltol, feastol_inacc, abstol_inacc, reltol_inacc, linsysacc, irerrfact; int iter_max, nitref; };
constexpr SolveCfg solve_cfg_default() { return {1e-8, 1e-8, 1e-8, 1e-4, 5e-5, 5e-5, 1e-14, 6., 100, 9}; }
// Retry policy (eicos_batch_set_retry; eicos_retry of include/eicos_amd.h), in device memory, one per handle: mask = the exit classes
// (exit_class.hpp) of a first attempt that trigger the second; warm, dyn_delta, dyn_eps, cfg = what the second attempt runs under in
// place of the launch's own values; counts [batch] = second attempts per instance since the last reset, bumped by the workgroup that
// owns the instance.  The host rewrites the record on the handle's stream, so a launch in flight keeps the policy it was enqueued with.
struct RetryDev { unsigned mask; double warm, dyn_delta, dyn_eps; SolveCfg cfg; int *counts; };
// One k_solve launch of a handle, as the host describes it: the pattern slot, the slabs and the queue, the launch shape, and what travels
// to the kernel by value.  order = the longest-first order array (used when B > order_min); cfg is copied into the kernel arguments, so
// a launch in flight keeps the settings it was enqueued with.
// A SUBSET launch (eicos_batch_solve_subset / _solve_where) is the same launch with list != NULL: B ids of distinct instances in device
// memory.  The selection kernel arranges them in `order` (never NULL then: list order up to order_min ids, longest first beyond), B =
// their number and grid = min(the handle's grid, B); batch = the handle's batch (the ids lie in [0, batch)).
struct SolveLaunch {
    int ps; double *inst, *work; int B; int *queue, *order;
    int grid, threads, nlds, idx16, order_min;
    double warm, dyn_delta, dyn_eps; SolveCfg cfg; size_t dyn_lds;
    const int *list; int batch, full_grid; // subset launches: the chosen ids, the handle's batch and its whole-batch grid
    int *rows; // subset launches with a step in list order (UpdArgs::rows_at): the selection kernel leaves rows[list[q]] = q here; NULL: not asked for
};
// Adjoint sensitivities (eicos_batch_adjoint, _output_jacobian), one record per launch in device memory.  Row q of every
// array belongs to the q-th instance of the launch.
// J == NULL, the gradient form: g [count][nrhs][n] in, grad_c [count][nrhs][n], grad_h [count][nrhs][m], grad_b [count][nrhs][p] and
// res [count][nrhs] out, any of the four NULL = not wanted.
// grad_G [count][nrhs][nnzG] and grad_A [count][nrhs][nnzA] (eicos_batch_adjoint_data; NULL = not wanted): the gradient with respect to
// the stored values of G and A, in the CSC order of Gpr / Apr.
// J != NULL, the contracted form: every gradient is contracted on the spot with the rows of the parameter map (pmap, NULL = none) and of
// the matrix map (mmap, NULL = none or not wanted), both with k columns: J [count][rows][k], res [count][rows]; grad_* are unused.  Its
// right-hand sides are the omap->r rows of the output map (g == NULL: the Jacobian, nrhs unused) or nrhs rows of the caller's g per
// instance (g != NULL: the gradient with respect to theta, omap unused).
// A recording rollout (eicos_batch_set_rollout_recording) runs the contracted form with grad_c / grad_h / grad_b non-NULL: the rows
// [count][rows][n], [count][rows][m], [count][rows][p] are then stored as well, with the expressions of the gradient form, in front of
// the contraction; x_rec [count][n], y_rec [count][p], z_rec [count][m] (NULL = not recorded) take the instance's un-equilibrated result
// rows, whatever the exit code.  The gradient form leaves the three NULL.
// centred != 0 (eicos_batch_set_adjoint_scaling, EICOS_ADJOINT_CENTRED; in the padding behind nrhs: the record keeps its size): the
// scaling block is formed from the re-centred pair of every second-order cone (kernels.hip: centre_cones) instead of the result rows'.
struct AdjointDev {
    int nrhs, centred; const double *g; double *grad_c, *grad_h, *grad_b, *res;
    const ParamMapDev *pmap; const OutMapDev *omap; double *J;
    double *grad_G, *grad_A; const MatrixMapDev *mmap; int k;
    double *x_rec, *y_rec, *z_rec;
};
// One k_adjoint launch of a handle: the pattern slot, the slabs and the launch shape of its solves, the settings its kkt_solve and its
// factorisation run under (by value), `count` instances -- list != NULL: those ids (device memory, distinct, inside [0, batch)), else
// 0 .. count-1 -- and the record.  The grid is min(grid, count): every workgroup owns the workspace slab of its index.
struct AdjointLaunch {
    int ps; const double *inst; double *work; int count; const int *list; int batch;
    int grid, threads, nlds, idx16; double dyn_delta, dyn_eps; SolveCfg cfg; size_t dyn_lds;
    const AdjointDev *adj;
};
// One k_solve build = these five entry points.  launch always receives an UpdArgs: UpdArgs{} when no step is fused into it.
struct SolveBuild {
    // adj == NULL: one launch of k_solve.  adj != NULL, the rollout that also records its Jacobians (eicos_batch_rollout_jacobian;
    // kernels.hip: k_roll_sens): the same launch with upd.on = UPD_ROLL over the whole batch, every step followed by the contracted adjoint
    // of *adj (device memory: J [batch][steps][r][k], res [batch][steps][r] or NULL, g == NULL) while the step's iterate is in place.
    // Kernels with an LDS vector only (L.nlds >= 1), as every fused step.
    hipError_t (*launch)(const SolveLaunch &L, hipStream_t st, const UpdArgs &upd, const AdjointDev *adj);
    hipError_t (*occupancy)(int threads, int nlds, int idx16, size_t dyn_lds, int *blocks_per_cu);
    hipError_t (*set_max_lds)(int threads, int nlds, int idx16, size_t dyn_lds); // (the build's k_solve, k_adjoint and k_roll_sens alike)
    hipError_t (*upload)(int ps, const DevPat &P);
    hipError_t (*adjoint)(const AdjointLaunch &L, hipStream_t st);
    bool operator==(const SolveBuild &o) const { return launch == o.launch; }
};
// The range launchers below (updateData in its four kinds and the output map) take an optional `list`: `count` ids of distinct instances
// in device memory.  Row q of the input or output arrays then belongs to the slab of instance list[q] instead of first + q (`first` is
// unused); NULL: the range.  The arithmetic per instance is the same either way.
// shared != NULL (only the launch that covers the whole batch, first = 0, with every matrix the pattern has given): the handle's shared-values
// word, which the host has set to 0 on `st` in front of this launch -- a workgroup whose rows of Gpr / Apr differ from row 0 in any bit
// stores -1 (kernels.hip: update_instance)
hipError_t launch_update(int ps, double *inst, int first, int count, const double *Gpr, const double *Apr,
                         const double *c, const double *h, const double *b, double *scratch, int grid, size_t lds_bytes, int vals_in_lds, hipStream_t st,
                         int *shared = nullptr, const int *list = nullptr);
// The shared factor operands of a handle (DevPat::kt0 / ub0), behind the launch_update that was given `shared`: kt0[t] = the K entry of target
// t as instance 0's slab holds it (DevPat::fac_src), and every level-0 off-diagonal target that lands in a backward slot >= ub0_off also
// into ub0 (ub0 == NULL: the handle shares the K stream only).  Plain copies: the bits instance_begin and the factorisation would produce.
hipError_t launch_shared_operands(int ps, const double *inst, double *kt0, double *ub0, hipStream_t st);
// right-hand-side-only updateData of instances [first, first + count): rows of c [count][n], h [count][m], b [count][p] (NULL = keep)
// divided by each instance's stored scalings; `width` = the summed widths of the given groups (sizes the grid)
hipError_t launch_update_rhs(int ps, double *inst, int first, int count, const double *c, const double *h, const double *b, int width, hipStream_t st,
                             const int *list = nullptr);
// Parametric right-hand sides (eicos_batch_set_param_map): per group c, h, b a base vector and a CSR matrix with k columns, in device
// memory, shared by every instance of the handle; base == NULL: the group has no map and is kept (AffineDev, ParamMapDev: above).  Passed
// to the range kernel by value.
// instances [first, first + count) from rows of theta [count][k]: entry = (base[r] + sum val * theta[col], every product and sum
// rounded on its own, in stored order) divided by the instance's stored scaling -- the bits launch_update_rhs leaves for the same vectors
hipError_t launch_update_param(int ps, double *inst, int first, int count, const ParamMapDev &map, const double *theta, int width, hipStream_t st,
                               const int *list = nullptr);
// One affine group over rows of theta [count][k] into dst [count][rows], unscaled: dst[q][r] = base[r] + sum val * theta[q][col], in stored
// order, every product and sum rounded on its own.  With a matrix map installed the parametric update expands [Gpr | Apr | c | h | b] this
// way into a device staging buffer and hands it to launch_update.
hipError_t launch_expand_affine(const AffineDev &map, int rows, int k, const double *theta, int count, double *dst, hipStream_t st);
// A caller-supplied starting point (eicos_batch_set_iterate*): rows of x [count][n], y [count][p], z [count][m], s [count][m] (NULL = keep)
// into the slabs of instances [first, first + count) as they are, and every instance marked warm-startable (exit code OPTIMAL unless it is
// OPTIMAL or close to it already, n_factor 1 if it was 0); `width` = the summed widths of the given groups (sizes the grid)
hipError_t launch_set_iterate(int ps, double *inst, int first, int count, const double *x, const double *y, const double *z, const double *s,
                              int width, hipStream_t st, const int *list = nullptr);
// rows [first, first + count) of u [count][map.r] = the output map applied to the current x of those instances: acc = base[row], then
// acc = acc + (val * x[col]) in stored order, every product and sum rounded on its own
hipError_t launch_outputs(int ps, const double *inst, int first, int count, const OutMapDev &map, double *u, hipStream_t st, const int *list = nullptr);
// The fallback map over rows [first, first + count) (or the `count` ids of `list`), behind launch_outputs on the same u rows: the rows of
// every instance whose record is in a class of fb.mask are overwritten by base + V theta-row -- acc = base[row], then acc = acc +
// (val * theta[col]) in stored order, every product and sum rounded on its own -- and its counter is bumped by one.  theta [count][fb.k]
// and u [count][fb.r] in memory the GPU addresses, row q of both belonging to instance first + q (list[q]); the map by value.
hipError_t launch_fallback(int ps, const double *inst, int first, int count, const FallbackDev &fb, const double *theta, double *u, hipStream_t st,
                           const int *list = nullptr);
// Its companion on the rollout-Jacobian path that is not fused, behind the step's adjoint launch: rows [first, first + count) of
// J [count][fb.r][fb.k] and res [count][fb.r] (NULL: not kept) of the same instances become V as a dense block -- the row zero-filled, then
// J[row][col] = J[row][col] + val in stored order -- and 0.0.  Counts nothing.
hipError_t launch_fallback_jacobian(int ps, const double *inst, int first, int count, const FallbackDev &fb, double *J, double *res, hipStream_t st);
// The same for the recorded gradient rows of a recording rollout that is not fused: rows [first, first + count) of Wc [count][fb.r][n],
// Wh [count][fb.r][m] and Wb [count][fb.r][p] of every instance whose fallback fired become 0.0 (its u row does not depend on the
// controller's data); the x, y, z records stay.
hipError_t launch_fallback_records(int ps, const double *inst, int first, int count, const FallbackDev &fb, double *Wc, double *Wh, double *Wb, hipStream_t st);
// One step of a rollout that is not fused into the solve launch, for instances [first, first + count), behind that step's solve and
// output kernels: z = [row of theta_cur [count][k] | row of u_cur [count][r]] goes through the plant map -- acc = base[row], then
// acc = acc + (val * z[col]) in stored order, then + w when given, every product and sum rounded on its own -- into theta_next [count][k]
// and into row t + 1 of the instance's theta trajectory; the u row is copied to row t of the u trajectory and the instance's exit code
// and iteration count to its records (roll: the trajectories of the whole batch, host copy of the launch's RolloutDev)
hipError_t launch_plant(int ps, const double *inst, int first, int count, const RolloutDev &roll, int t, const double *theta_cur,
                        const double *u_cur, double *theta_next, hipStream_t st);
// The backward sweep over a recorded rollout (eicos_batch_rollout_gradient; kernels.hip: k_rollout_backprop): J [batch][steps][r][k] as the
// rollout left it, gu [batch][steps][r] and gtheta [batch][steps + 1][k] (either NULL = 0.0) in, grad_theta0 [batch][k] and grad_w
// [batch][steps][k] (NULL = not wanted) out, all in device memory; the map by value.  One 64-thread workgroup per instance with
// rollout_backprop_lds bytes of LDS (at most 48 KB: the caller checks).
// The plant's own entries (eicos_batch_rollout_plant_gradient): with u_traj [batch][steps][r] and theta_traj [batch][steps + 1][k] of that
// rollout also grad_f0 [batch][k] and grad_val [batch][plant.nnz] (either NULL = not wanted; grad_theta0 is optional then) -- z_t =
// [theta_t | u_t] is staged in LDS behind mu (values = true: k + r more doubles).  Instance b sweeps with row b of the per-instance
// values where the map holds them.  Without the four new arguments: the bits of the sweep as it was.
inline size_t rollout_backprop_lds(int k, int r, bool values = false) { return ((size_t)(values ? 4 : 3) * k + (values ? 3 : 2) * (size_t)r) * sizeof(double); }
hipError_t launch_rollout_backprop(const PlantMapDev &plant, int steps, int batch, const double *J, const double *gu, const double *gtheta,
                                   double *grad_theta0, double *grad_w, hipStream_t st, const double *u_traj = nullptr,
                                   const double *theta_traj = nullptr, double *grad_f0 = nullptr, double *grad_val = nullptr);
// The backward sweep with respect to the controller's own data (eicos_batch_rollout_data_gradient; kernels.hip: k_rollout_data_backprop),
// over a rollout that recorded its Jacobians AND its gradient rows: J as above, Wc [batch][steps][r][n], Wh [..][m], Wb [..][p] and the
// x [batch][steps][n], y [..][p], z [..][m] records, gu / gtheta as above, theta_traj [batch][steps + 1][k]; pmap / omap = the handle's
// maps (host copies: device pointers, by value).  Outputs, each NULL = not wanted, one row per instance: grad_c [batch][n], grad_h
// [batch][m], grad_b [batch][p], grad_G [batch][nnzG], grad_A [batch][nnzA], grad_val[0..2] [batch][nnz of the c, h, b group of pmap],
// grad_u0 [batch][r], grad_Uval [batch][nnzU].  stage = (n + m + p) doubles per workgroup of the grid (rollout_data_backprop_grid) in
// device memory: the step's contracted rows between two barriers.  One 256-thread workgroup per instance, rollout_backprop_lds(k, r)
// bytes of LDS for the lambda / mu recursion, which is k_rollout_backprop's, bit for bit.
struct DataGradDev {
    const double *J, *Wc, *Wh, *Wb, *x, *y, *z, *gu, *gth, *theta;
    ParamMapDev pmap; OutMapDev omap;
    double *grad_c, *grad_h, *grad_b, *grad_G, *grad_A, *grad_val[3], *grad_u0, *grad_Uval, *stage;
};
inline int rollout_data_backprop_grid(int batch) { return batch < 4096 ? batch : 4096; }
hipError_t launch_rollout_data_backprop(int ps, const PlantMapDev &plant, int steps, int batch, const DataGradDev &D, hipStream_t st);
// rows [0, rows) of dst [rows][width] = src [width] (device memory): what the first eicos_batch_set_plant_values of a group starts from
hipError_t launch_fill_rows(const double *src, int width, int rows, double *dst, hipStream_t st);
// Selection (eicos_batch_select, _solve_where): the instances of 0 .. batch-1 whose exit class (exit_class.hpp) is in `mask`, compacted
// in ascending order into cand [batch], their number into *count (both device memory).  The kernel is the one that orders a subset launch
// (kernels.hip: k_select_order), run without an order array.
hipError_t launch_select(int ps, const double *inst, int batch, unsigned mask, int *cand, int *count, hipStream_t st);
// Row gather (eicos_batch_gather, the exit codes of the subset solves): for q < count the wanted groups (GATHER_* bits) of instance
// list[q] -- x, y, z, s as they stand in the slab (what eicos_batch_solution / _duals return) and the info record -- back to back into
// row q of dst [count][gather_width]; list and dst in device memory
enum { GATHER_X = 1, GATHER_Y = 2, GATHER_Z = 4, GATHER_S = 8, GATHER_INFO = 16 };
constexpr int GATHER_INFO_DOUBLES = (int)(sizeof(DevInfo) / sizeof(double));
static_assert(sizeof(DevInfo) % sizeof(double) == 0, "the info record is gathered as doubles");
inline int gather_width(int want, int n, int p, int m) {
    return (want & GATHER_X ? n : 0) + (want & GATHER_Y ? p : 0) + (want & GATHER_Z ? m : 0) + (want & GATHER_S ? m : 0) + (want & GATHER_INFO ? GATHER_INFO_DOUBLES : 0);
}
hipError_t launch_gather_rows(int ps, const double *inst, const int *list, int count, int want, double *dst, hipStream_t st);
hipError_t update_set_max_lds();
hipError_t launch_debug_factor(int ps, double *inst, double *work, int i, int threads, size_t dyn_lds, hipStream_t st);
hipError_t launch_debug_scalings(int ps, double *inst, double *work, int i, int *ok, int threads, hipStream_t st);
int max_patterns();
// The seven compilations of kernels.hip (the note at its top) export their build through one function each: the default namespace (256
// threads; updateData and the debug kernels live here too), the LDS-resident k_solve (128), the 256-thread k_solve at two waves per SIMD, the
// 128- / 512-thread k_solve of the default build, the 256- / 512-thread k_solve with U in LDS (one workgroup per CU whose U fits the idle LDS).
SolveBuild solve_entries();
namespace ldsres { SolveBuild solve_entries(); }
namespace w2 { SolveBuild solve_entries(); }
namespace t128 { SolveBuild solve_entries(); }
namespace t512 { SolveBuild solve_entries(); }
namespace ubl256 { SolveBuild solve_entries(); }
namespace ubl512 { SolveBuild solve_entries(); }
// the build a handle's solves run: U in LDS (one workgroup per CU, 256 / 512 threads), LDS-resident (128 threads), two-waves-per-SIMD (256 threads),
// or the default one of its workgroup size
inline SolveBuild solve_build(int threads, bool ldsres, bool w2, bool ubl = false) {
    if (ubl && threads == 256) return ubl256::solve_entries();
    if (ubl && threads == 512) return ubl512::solve_entries();
    if (ldsres) return ldsres::solve_entries();
    if (w2) return w2::solve_entries();
    if (threads == 128) return t128::solve_entries();
    if (threads == 512) return t512::solve_entries();
    return solve_entries();
}
} // namespace eicos
