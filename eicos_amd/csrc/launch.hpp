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
// memory, shared by every instance; k, r = the parameter and output counts it was validated for
struct PlantMapDev { int k, r; AffineDev a; };
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
struct UpdArgs {
    const double *G, *A, *c, *h, *b; double *x; int on; const unsigned *flags; int chunk; unsigned seq; int *err;
    const ParamMapDev *pmap; const OutMapDev *omap; const double *theta; double *u; // (device copies of the handle's maps)
    const RolloutDev *roll;
    const MatrixMapDev *mmap; // UPD_PARAM / UPD_ROLL with a matrix map: the step is a full updateData from theta (kernels.hip: matrix_param_instance)
    // Every mode, 0 included: a solve that warm-starts an instance first takes its x, y, z, s through this map (kernels.hip: shift_instance);
    // NULL: no shift map.  One more word of kernel arguments, and one pointer test per instance.
    const ShiftMapDev *smap;
    // Every mode, 0 included: the handle's shared-values word (eicos_batch_shared_values), read by thread 0 once per instance before the
    // instance's solve.  -1: every instance streams the product values (the sliced-ELL copies of [A' G'], A, G and the G tiles) of its own
    // slab; r >= 0: every instance of the batch holds the bits of instance r there, and all of them stream instance r's.  NULL counts as -1.
    const int *shared;
};
// Runtime solver settings (eicos_batch_set_settings; eicos_settings of include/eicos_amd.h, same fields and defaults): one by-value argument
// of k_solve, copied into LDS by thread 0 (kernels.hip: Sh::cfg) before the workgroup's first instance, where the stage functions read
// it -- the exit test and the two infeasibility-residual comparisons (tolerances), the iteration cap, and kkt_solve's refinement stop test
// (linsysacc, irerrfact, nitref).  Every other constant of the reference's Settings stays compile-time (kernels.hip).
struct SolveCfg { double feastol, abstol, reltol, feastol_inacc, abstol_inacc, reltol_inacc, linsysacc, irerrfact; int iter_max, nitref; };
constexpr SolveCfg solve_cfg_default() { return {1e-8, 1e-8, 1e-8, 1e-4, 5e-5, 5e-5, 1e-14, 6., 100, 9}; }
hipError_t launch_solve(int ps, double *inst, double *work, int B, int *queue, int *order, int grid, int threads, int nlds, int idx16,
                        int order_min, double warm, double dyn_delta, double dyn_eps, const SolveCfg &cfg, size_t dyn_lds, hipStream_t st, const UpdArgs *upd = nullptr);
// shared != NULL (only the launch that covers the whole batch, first = 0, with every matrix the pattern has given): the handle's shared-values
// word, which the host has set to 0 on `st` in front of this launch -- a workgroup whose rows of Gpr / Apr differ from row 0 in any bit
// stores -1 (kernels.hip: update_instance)
hipError_t launch_update(int ps, double *inst, int first, int count, const double *Gpr, const double *Apr,
                         const double *c, const double *h, const double *b, double *scratch, int grid, size_t lds_bytes, int vals_in_lds, hipStream_t st,
                         int *shared = nullptr);
// right-hand-side-only updateData of instances [first, first + count): rows of c [count][n], h [count][m], b [count][p] (NULL = keep)
// divided by each instance's stored scalings; `width` = the summed widths of the given groups (sizes the grid)
hipError_t launch_update_rhs(int ps, double *inst, int first, int count, const double *c, const double *h, const double *b, int width, hipStream_t st);
// Parametric right-hand sides (eicos_batch_set_param_map): per group c, h, b a base vector and a CSR matrix with k columns, in device
// memory, shared by every instance of the handle; base == NULL: the group has no map and is kept (AffineDev, ParamMapDev: above).  Passed
// to the range kernel by value.
// instances [first, first + count) from rows of theta [count][k]: entry = (base[r] + sum val * theta[col], every product and sum
// rounded on its own, in stored order) divided by the instance's stored scaling -- the bits launch_update_rhs leaves for the same vectors
hipError_t launch_update_param(int ps, double *inst, int first, int count, const ParamMapDev &map, const double *theta, int width, hipStream_t st);
// One affine group over rows of theta [count][k] into dst [count][rows], unscaled: dst[q][r] = base[r] + sum val * theta[q][col], in stored
// order, every product and sum rounded on its own.  With a matrix map installed the parametric update expands [Gpr | Apr | c | h | b] this
// way into a device staging buffer and hands it to launch_update.
hipError_t launch_expand_affine(const AffineDev &map, int rows, int k, const double *theta, int count, double *dst, hipStream_t st);
// A caller-supplied starting point (eicos_batch_set_iterate*): rows of x [count][n], y [count][p], z [count][m], s [count][m] (NULL = keep)
// into the slabs of instances [first, first + count) as they are, and every instance marked warm-startable (exit code OPTIMAL unless it is
// OPTIMAL or close to it already, n_factor 1 if it was 0); `width` = the summed widths of the given groups (sizes the grid)
hipError_t launch_set_iterate(int ps, double *inst, int first, int count, const double *x, const double *y, const double *z, const double *s,
                              int width, hipStream_t st);
// rows [first, first + count) of u [count][map.r] = the output map applied to the current x of those instances: acc = base[row], then
// acc = acc + (val * x[col]) in stored order, every product and sum rounded on its own
hipError_t launch_outputs(int ps, const double *inst, int first, int count, const OutMapDev &map, double *u, hipStream_t st);
// One step of a rollout that is not fused into the solve launch, for instances [first, first + count), behind that step's solve and
// output kernels: z = [row of theta_cur [count][k] | row of u_cur [count][r]] goes through the plant map -- acc = base[row], then
// acc = acc + (val * z[col]) in stored order, then + w when given, every product and sum rounded on its own -- into theta_next [count][k]
// and into row t + 1 of the instance's theta trajectory; the u row is copied to row t of the u trajectory and the instance's exit code
// and iteration count to its records (roll: the trajectories of the whole batch, host copy of the launch's RolloutDev)
hipError_t launch_plant(int ps, const double *inst, int first, int count, const RolloutDev &roll, int t, const double *theta_cur,
                        const double *u_cur, double *theta_next, hipStream_t st);
hipError_t update_set_max_lds();
hipError_t launch_debug_factor(int ps, double *inst, double *work, int i, int threads, size_t dyn_lds, hipStream_t st);
hipError_t launch_debug_scalings(int ps, double *inst, double *work, int i, int *ok, int threads, hipStream_t st);
hipError_t solve_occupancy(int threads, int nlds, int idx16, size_t dyn_lds, int *blocks_per_cu);
hipError_t solve_set_max_lds(int threads, int nlds, int idx16, size_t dyn_lds);
hipError_t upload_pattern(int ps, const DevPat &P);
int max_patterns();
// LDS-resident variant of k_solve (kernels_ldsres.hip = kernels.hip compiled with EICOS_LDSRES): same arguments
namespace ldsres {
hipError_t launch_solve(int ps, double *inst, double *work, int B, int *queue, int *order, int grid, int threads, int nlds, int idx16,
                        int order_min, double warm, double dyn_delta, double dyn_eps, const SolveCfg &cfg, size_t dyn_lds, hipStream_t st, const UpdArgs *upd = nullptr);
hipError_t solve_occupancy(int threads, int nlds, int idx16, size_t dyn_lds, int *blocks_per_cu);
hipError_t solve_set_max_lds(int threads, int nlds, int idx16, size_t dyn_lds);
hipError_t upload_pattern(int ps, const DevPat &P);
} // namespace ldsres
// 256-thread k_solve with the register budget of two waves per SIMD (kernels_w2.hip = kernels.hip compiled with EICOS_W2)
namespace w2 {
hipError_t launch_solve(int ps, double *inst, double *work, int B, int *queue, int *order, int grid, int threads, int nlds, int idx16,
                        int order_min, double warm, double dyn_delta, double dyn_eps, const SolveCfg &cfg, size_t dyn_lds, hipStream_t st, const UpdArgs *upd = nullptr);
hipError_t solve_occupancy(int threads, int nlds, int idx16, size_t dyn_lds, int *blocks_per_cu);
hipError_t solve_set_max_lds(int threads, int nlds, int idx16, size_t dyn_lds);
hipError_t upload_pattern(int ps, const DevPat &P);
} // namespace w2
// the 128- and 512-thread k_solve of the default build, in their own translation units (kernels_t128.hip / kernels_t512.hip = kernels.hip
// compiled with EICOS_TSPLIT): the default namespace keeps the 256-thread one
namespace t128 {
hipError_t launch_solve(int ps, double *inst, double *work, int B, int *queue, int *order, int grid, int threads, int nlds, int idx16,
                        int order_min, double warm, double dyn_delta, double dyn_eps, const SolveCfg &cfg, size_t dyn_lds, hipStream_t st, const UpdArgs *upd = nullptr);
hipError_t solve_occupancy(int threads, int nlds, int idx16, size_t dyn_lds, int *blocks_per_cu);
hipError_t solve_set_max_lds(int threads, int nlds, int idx16, size_t dyn_lds);
hipError_t upload_pattern(int ps, const DevPat &P);
} // namespace t128
namespace t512 {
hipError_t launch_solve(int ps, double *inst, double *work, int B, int *queue, int *order, int grid, int threads, int nlds, int idx16,
                        int order_min, double warm, double dyn_delta, double dyn_eps, const SolveCfg &cfg, size_t dyn_lds, hipStream_t st, const UpdArgs *upd = nullptr);
hipError_t solve_occupancy(int threads, int nlds, int idx16, size_t dyn_lds, int *blocks_per_cu);
hipError_t solve_set_max_lds(int threads, int nlds, int idx16, size_t dyn_lds);
hipError_t upload_pattern(int ps, const DevPat &P);
} // namespace t512
// the 256- / 512-thread k_solve with the factor operand array U resident in LDS (kernels_ubl256.hip / kernels_ubl512.hip = kernels.hip compiled
// with EICOS_UBL): launches of one workgroup per CU whose U fits the idle LDS
namespace ubl256 {
hipError_t launch_solve(int ps, double *inst, double *work, int B, int *queue, int *order, int grid, int threads, int nlds, int idx16,
                        int order_min, double warm, double dyn_delta, double dyn_eps, const SolveCfg &cfg, size_t dyn_lds, hipStream_t st, const UpdArgs *upd = nullptr);
hipError_t solve_occupancy(int threads, int nlds, int idx16, size_t dyn_lds, int *blocks_per_cu);
hipError_t solve_set_max_lds(int threads, int nlds, int idx16, size_t dyn_lds);
hipError_t upload_pattern(int ps, const DevPat &P);
} // namespace ubl256
namespace ubl512 {
hipError_t launch_solve(int ps, double *inst, double *work, int B, int *queue, int *order, int grid, int threads, int nlds, int idx16,
                        int order_min, double warm, double dyn_delta, double dyn_eps, const SolveCfg &cfg, size_t dyn_lds, hipStream_t st, const UpdArgs *upd = nullptr);
hipError_t solve_occupancy(int threads, int nlds, int idx16, size_t dyn_lds, int *blocks_per_cu);
hipError_t solve_set_max_lds(int threads, int nlds, int idx16, size_t dyn_lds);
hipError_t upload_pattern(int ps, const DevPat &P);
} // namespace ubl512
// one k_solve build = these four entry points
struct SolveBuild {
    decltype(&launch_solve) launch;
    decltype(&solve_occupancy) occupancy;
    decltype(&solve_set_max_lds) set_max_lds;
    decltype(&upload_pattern) upload;
};
// the build a handle's solves run: U in LDS (one workgroup per CU, 256 / 512 threads), LDS-resident (128 threads), two-waves-per-SIMD (256 threads),
// or the default one of its workgroup size
inline SolveBuild solve_build(int threads, bool ldsres, bool w2, bool ubl = false) {
    if (ubl && threads == 256) return {ubl256::launch_solve, ubl256::solve_occupancy, ubl256::solve_set_max_lds, ubl256::upload_pattern};
    if (ubl && threads == 512) return {ubl512::launch_solve, ubl512::solve_occupancy, ubl512::solve_set_max_lds, ubl512::upload_pattern};
    if (ldsres) return {ldsres::launch_solve, ldsres::solve_occupancy, ldsres::solve_set_max_lds, ldsres::upload_pattern};
    if (w2) return {w2::launch_solve, w2::solve_occupancy, w2::solve_set_max_lds, w2::upload_pattern};
    if (threads == 128) return {t128::launch_solve, t128::solve_occupancy, t128::solve_set_max_lds, t128::upload_pattern};
    if (threads == 512) return {t512::launch_solve, t512::solve_occupancy, t512::solve_set_max_lds, t512::upload_pattern};
    return {launch_solve, solve_occupancy, solve_set_max_lds, upload_pattern};
}
} // namespace eicos
