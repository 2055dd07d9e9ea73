/*
 * include/eicos_amd.h -- C ABI of the MI355X batched SOCP interior-point solver.
 *
 * This is the drop-in boundary for the EiCOS hot path.  The reference has no FFI of its own;
 * its public surface is class EiCOS::Solver (reference include/eicos.hpp:137-163) and the
 * closest thing to a C ABI is the ECOS shim of reference test/ecos.h:11-34
 * (ECOS_setup / ECOS_solve / ECOS_updateData / ECOS_cleanup).  Each entry point below names
 * the reference interface it replaces.  include/eicos.hpp (this repo) re-creates
 * class EiCOS::Solver on top of this ABI with batch = 1; INTEGRATION.md shows the bindings.
 *
 * Conventions: plain pointers and sizes only; the caller owns every buffer it passes; all
 * functions return 0 on success or a negative EICOS_E_* code (never throw across the ABI);
 * eicos_last_error() returns a thread-local message for the last failure.
 * All arithmetic is fp64, indices are 32-bit int (Eigen's default StorageIndex).
 *
 * One handle = one sparsity pattern (G: m x n CSC, A: p x n CSC, cone sizes q) analysed once
 * on the host + `batch` numeric instances resident in HBM on one GPU.  Instances are
 * independent: several GPUs of one node are driven from ONE process through eicos_multi_* (below: contiguous shards, one handle
 * and stream per device), or from one process per GPU with one handle each (bench.py --gpus N under torch.distributed).
 */
#ifndef EICOS_AMD_H
#define EICOS_AMD_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct eicos_batch eicos_batch; /* opaque */

enum {
    EICOS_OK = 0,
    EICOS_E_INVALID = -1,   /* bad argument / inconsistent dimensions          */
    EICOS_E_NOGPU = -2,     /* no usable HIP device (there is NO CPU fallback) */
    EICOS_E_HIP = -3,       /* a HIP runtime call failed                       */
    EICOS_E_UNSUPPORTED = -4 /* pattern too dense for the current factor path  */
};

/* exit codes per instance: values of enum class EiCOS::exitcode (reference include/eicos.hpp:8-21) */
enum {
    EICOS_OPTIMAL = 0, EICOS_PINF = 1, EICOS_DINF = 2, EICOS_MAXIT = -1, EICOS_NUMERICS = -2,
    EICOS_OUTCONE = -3, EICOS_FATAL = -7, EICOS_INACC_OFFSET = 10
};

/* Mirror of struct EiCOS::Information (reference include/eicos.hpp:49-73); the three
 * std::optional<double> members are flattened into value + has_* flag.  tau/kap/exitcode and
 * the n_* counters are additions (the counters feed the roofline byte model of bench.py). */
typedef struct eicos_info {
    double pcost, dcost, pres, dres, gap, relgap, sigma, mu, step, step_aff, kapovert;
    double pinfres, dinfres, tau, kap;
    int has_relgap, has_pinfres, has_dinfres, pinf, dinf;
    int iter, nitref1, nitref2, nitref3, exitcode;
    int n_factor;   /* numeric LDL' factorisations in the last solve (1 + completed passes) */
    int n_ldlsolve; /* LDL' solves in the last solve (incl. refinement solves)             */
    int n_sweep;    /* passes over the factor L in the last solve: = n_ldlsolve, except that a solve of two right-hand
                     * sides at once (eicos_dims.dual_rhs) counts one pass for both                  */
    int reserved_;
    double solve_us; /* device wall time of this instance's last solve (its workgroup, microseconds): max / p95 over the batch
                      * against eicos_batch_last_solve_ms shows how much of a launch is its slowest instances */
} eicos_info;

/* Pattern / size report of a handle (for byte accounting and tests). */
typedef struct eicos_dims {
    int n, m, p, l, ncones, dim_K, nnzA, nnzG, nnzK, nnzL, nlevels, order_mode, batch, device;
    long long factor_pairs;      /* multiply-subtract pairs of one numeric factorisation */
    size_t inst_bytes, work_bytes, pattern_bytes;
    int threads_per_block;
    int resident_blocks; /* instances resident on the GPU at a time = resident workgroups */
    int lds_bytes; /* dynamic LDS per workgroup (solve vector staged in LDS), 0 if in HBM */
    int instances_per_block; /* always 1 (field kept for ABI stability: the lock-step pairs of round 2 were measured slower and removed) */
    int lds_resident; /* 1: small pattern, the solve works on LDS copies of the instance's slabs (lds_bytes includes them) */
    int factor_path;  /* 0 scalar level-scheduled program, 1 dense 16x16 tiles (MFMA), 2 hybrid: tiles for the top of the tree */
    int cone_order;   /* 1: the two expansion columns of every second-order cone are eliminated after the cone's own rows (the
                       * numerically preferable order, csrc/symbolic.cpp); 0: unconstrained minimum degree (or no cones) */
    int dual_rhs;     /* 1: the two independent KKT systems of the initialisation and of every pass are solved in one sweep */
    /* the arithmetic path of this handle (what decides the rounding of a result besides the data): the profile it was created under
     * (eicos_set_arithmetic_profile), the nodes of the dense apex (0 = none: level schedule to the root) and the slices of the
     * single-wavefront part of the two sweep plans (0 = no split); two handles on one pattern with equal threads_per_block, factor_path,
     * apex_nodes and solo_slices give bit-identical results for equal data */
    int arithmetic_profile, apex_nodes, solo_slices;
    int shared_operands; /* 1: the handle keeps one copy of the factor operands that are plain entries of A, G or constants (the K entries of
                          * the numeric factorisation outside the scaling block, the level-0 columns of the backward sweep), filled when
                          * eicos_batch_shared_values turns 1 and read by every instance while it stays 1; 0: every instance reads its own
                          * (builds that keep the factor in LDS, the tile paths, EICOS_SHARED_VALUES=0).  Results are bit-identical. */
    int iterate_park; /* where a refinement step of the KKT solve keeps the iterate while the LDS vector serves the sweeps: 1 = registers of
                       * the owning threads (two-waves-per-SIMD build, dim_K <= 26 * threads_per_block), 0 = the workspace slab (or the
                       * iterate has an LDS vector of its own); the results are bit-identical */
} eicos_dims;

/* Process-wide choice of how a handle's PLANS are shaped, read by eicos_batch_create / eicos_multi_create (no reference counterpart: the
 * reference has one code path).  0 (default): by the launch -- workgroup size, dense apex and the single-wavefront tree top follow the
 * batch size, so the last bits of an instance's result can depend on the batch (or shard) it is solved in.  1: by the pattern alone, as
 * for a batch beyond one workgroup per CU -- an instance gives the same bits in a batch of 1, of 4096 and in any shard of an eicos_multi
 * (at the price of the small-batch plan choices: a few percent below profile 0 there).  Returns EICOS_OK or EICOS_E_INVALID. */
int eicos_set_arithmetic_profile(int profile);
int eicos_get_arithmetic_profile(void);

/* ---- construction: replaces Solver::Solver(n,m,p,l,ncones,q,Gpr,Gjc,Gir,Apr,Ajc,Air,c,h,b)
 * (reference include/eicos.hpp:151-154, src/eicos.cpp:91-120) + build() (:132-187), for a
 * whole batch.  Pattern only; values arrive through eicos_batch_update*.  The reference ignores `l`
 * and derives it as m - sum(q) (src/eicos.cpp:91,155): pass l < 0 for exactly that; l >= 0 is checked
 * (l + sum(q) must equal m, else EICOS_E_INVALID).  The arrays are trusted to hold n+1 column pointers,
 * jc[n] row indices and ncones cone sizes.  NULL Gjc/Gir (or Ajc/Air) mean "no G" ("no A").
 * device < 0 selects the current HIP device. */
int eicos_batch_create(int n, int m, int p, int l, int ncones, const int *q,
                       const int *Gjc, const int *Gir, const int *Ajc, const int *Air,
                       int batch, int device, eicos_batch **out);

/* ---- updateData: replaces Solver::updateData(double*Gpr,double*Apr,double*c,double*h,double*b)
 * (reference include/eicos.hpp:155-156, src/eicos.cpp:2053-2082) for instances
 * [first, first+count).  Arrays are [count][nnzG], [count][nnzA], [count][n], [count][m],
 * [count][p], row-major, HOST pointers; NULL = keep that group (h is read only with Gpr, b only
 * with Apr, as in the reference).  Runs un-equilibrate -> copy-in -> setEquilibration (:302-374)
 * -> transposes -> KKT value refresh on the GPU. */
int eicos_batch_update(eicos_batch *hd, int first, int count,
                       const double *Gpr, const double *Apr,
                       const double *c, const double *h, const double *b);
/* How the host arrays travel (csrc/api.cpp: eicos_internal_update_staged).  PAGEABLE arrays (plain malloc / std::vector / numpy) go through
 * two pinned bounce buffers in chunks of ~16 MB: the host copies chunk k + 1 in while the updateData kernel of chunk k reads its inputs
 * straight out of the other buffer over PCIe; the call returns once the last chunk has been copied (the arrays are the caller's again),
 * with the kernels still in flight on the handle's stream.  PINNED arrays (eicos_host_alloc below, hipHostMalloc, hipHostRegister) are
 * read in place by ONE kernel launch; the call waits for it, so the arrays may be overwritten on return -- as with the reference's
 * synchronous updateData.  eicos_batch_last_update_path tells which path the most recent call took (1 bounce, 2 pinned in place,
 * 3 peer GPU in place, 4 staged peer copies). */
void *eicos_host_alloc(size_t bytes); /* pinned host memory the GPU addresses directly; NULL on failure */
int eicos_host_free(void *p);
/* ... or pin arrays the caller already owns IN PLACE (hipHostRegister): they then take the pinned path as well.  Registering costs about
 * as much as a few bounce copies of the same bytes -- worth it for arrays reused across calls; unregister before freeing them.  An array is
 * read or written in place only when its WHOLE extent is pinned (first byte, last byte and a probe every 2 MB are checked per call; anything
 * else takes the bounce path -- never a GPU page fault).  Registering a base pointer that is already registered returns EICOS_OK when the
 * existing registration covers [p, p + bytes) and EICOS_E_INVALID when it is smaller (the runtime would map nothing new); a registration
 * belongs to whoever made it: eicos_host_unregister(p) ends it for every user of that memory.  paths 5 / 6: eicos_batch_update_solve below. */
int eicos_host_register(void *p, size_t bytes);
int eicos_host_unregister(void *p);
int eicos_batch_last_update_path(eicos_batch *hd);
/* updateData + solve in ONE synchronous call for the whole batch: replaces Solver::updateData(double *...) followed by Solver::solve()
 * (reference include/eicos.hpp:155-158, src/eicos.cpp:2053-2082 + :848).  Same array conventions as eicos_batch_update (NULL = keep the group).
 * When every given array is memory the GPU addresses directly -- eicos_host_alloc / eicos_host_register memory, or device memory -- each
 * workgroup of the solve kernel runs updateData for the instance it is about to solve: the PCIe transfer is spread over the launch behind
 * the other workgroups' compute instead of preceding it (path 5 of eicos_batch_last_update_path).  PAGEABLE arrays take the bounce
 * pipeline of eicos_batch_update, then the solve (an experiment switch stages them instead -- the kernel is launched at once and the host
 * copies the arrays chunk by chunk into a pinned staging buffer WHILE it runs, one flag per chunk, path 6: faster on some hosts, slower on
 * others, off by default).  x_out: optional [batch][n] result array
 * (pinned host / device memory is written by the kernel as instances finish).  Handles without an LDS vector (patterns too large for LDS)
 * run eicos_batch_update + eicos_batch_solve (+ eicos_batch_solution).  A device x_out is honoured on every branch: where the kernel does
 * not write it, it is filled by one strided copy on the device.  Results are bit-identical on every path.  exitcodes: optional [batch]. */
int eicos_batch_update_solve(eicos_batch *hd, const double *Gpr, const double *Apr, const double *c, const double *h, const double *b,
                             double *x_out, int *exitcodes);
/* Same, DEVICE pointers (inputs already resident in HBM; no PCIe traffic). */
int eicos_batch_update_device(eicos_batch *hd, int first, int count,
                              const double *dGpr, const double *dApr,
                              const double *dc, const double *dh, const double *db);

/* ---- right-hand-side-only updateData (no reference counterpart: the reference's updateData reads h only with Gpr and b only with Apr,
 * src/eicos.cpp:2053-2074, so changing a vector there means re-sending the matrices).  Instances [first, first+count); arrays [count][n],
 * [count][m], [count][p], row-major; NULL = keep that group, and h and b are read on their own.  A, G and the equilibration are not touched:
 * the new vectors are divided by the scalings the instance's last updateData stored -- the very division updateData ends with, so the
 * result equals, bit for bit, an eicos_batch_update that re-sends unchanged Gpr and Apr with the same vectors.  An instance that has had
 * no updateData yet has no scalings: its vectors are stored as given (scalings of 1), and a later eicos_batch_update that keeps them
 * equilibrates them exactly as if they had been given to it.  Host arrays take the paths of eicos_batch_update (pageable: the bounce
 * pipeline, path 1; pinned / registered: read in place, path 2; synchronous in the same way). */
int eicos_batch_update_rhs(eicos_batch *hd, int first, int count, const double *c, const double *h, const double *b);
/* Same, DEVICE pointers; asynchronous like eicos_batch_update_device. */
int eicos_batch_update_rhs_device(eicos_batch *hd, int first, int count, const double *dc, const double *dh, const double *db);
/* right-hand-side-only updateData + solve of the whole batch in one synchronous call: eicos_batch_update_solve's paths and conventions
 * (x_out [batch][n] and exitcodes [batch] optional).  When every given array is GPU-addressable (pinned / registered host memory or device
 * memory) each workgroup of the solve kernel scales its instance's vectors right before it solves it (path 5); otherwise, and on handles
 * without an LDS vector, eicos_batch_update_rhs + eicos_batch_solve.  Bit-identical on every path. */
int eicos_batch_update_rhs_solve(eicos_batch *hd, const double *c, const double *h, const double *b, double *x_out, int *exitcodes);

/* ---- parametric right-hand sides (no reference counterpart).  In a closed loop c, h and b are usually affine in a few numbers -- the
 * measured state, a reference, some bounds: c = c0 + C theta, h = h0 + H theta, b = b0 + B theta with theta of length k.  A handle holds
 * one such map for all its instances; per step only theta travels ([count][k] doubles, 8 k bytes per instance) and the GPU expands it.
 * eicos_affine_map: base[rows] and a CSR matrix rows x k (rowptr[rows + 1], col / val[rowptr[rows]]), rows = n, m, p for c, h, b.
 * eicos_batch_set_param_map COPIES the host arrays; a NULL group is not parametric and is kept by the update, exactly as a NULL group of
 * eicos_batch_update_rhs; a later call replaces the map, all groups NULL (or k = 0) removes it.  EICOS_E_INVALID, with a message naming the
 * fault, for rowptr[0] != 0, decreasing row pointers, a column outside [0, k) and a map for a group the pattern does not have (values are
 * not checked for finiteness, as elsewhere).  eicos_batch_param_count: k, 0 = no map installed.
 * eicos_batch_update_param for instance i, row r of a mapped group:
 *     acc = base[r];  for t in rowptr[r] .. rowptr[r+1]-1, in stored order:  acc = acc + (val[t] * theta[i][col[t]])
 * with the product and the sum EACH rounded to fp64 (no fused multiply-add), then the division by the stored scaling with which
 * eicos_batch_update_rhs ends.  The state it leaves therefore equals, bit for bit, that of eicos_batch_update_rhs on vectors evaluated
 * on the host in that order; A, G, the scalings and the solve state are not touched.  theta takes the paths of eicos_batch_update
 * (pageable: bounce pipeline, path 1; pinned / registered: read in place, path 2); the host form is synchronous in the same way, the
 * _device form asynchronous like eicos_batch_update_rhs_device.  EICOS_E_INVALID without a map ("no parameter map"). */
typedef struct eicos_affine_map { const double *base; const int *rowptr; const int *col; const double *val; } eicos_affine_map;
int eicos_batch_set_param_map(eicos_batch *hd, int k, const eicos_affine_map *c, const eicos_affine_map *h, const eicos_affine_map *b);
int eicos_batch_param_count(eicos_batch *hd);
int eicos_batch_update_param(eicos_batch *hd, int first, int count, const double *theta /* host [count][k] */);
int eicos_batch_update_param_device(eicos_batch *hd, int first, int count, const double *dtheta);

/* ---- output map and the closed-loop step (no reference counterpart).  A controller applies a few numbers of x -- the first move,
 * usually after an affine un-scaling: u = u0 + U x with u of length r.  A handle holds one such map for all its instances, mirroring the
 * parameter map: eicos_affine_map with base[r] and a CSR matrix r x n (rowptr[r + 1], col / val[rowptr[r]]; columns index x).
 * eicos_batch_set_output_map COPIES the host arrays into one device allocation; a later call replaces the map, r = 0 or u = NULL removes
 * it.  EICOS_E_INVALID, with a message naming the fault, for rowptr[0] != 0, decreasing row pointers, a column outside [0, n), r < 0 and a
 * pattern with n = 0.  eicos_batch_output_count: r, 0 = no map installed.
 * Row `row` of instance i:
 *     acc = base[row];  for t in rowptr[row] .. rowptr[row+1]-1, in stored order:  acc = acc + (val[t] * x[i][col[t]])
 * with the product and the sum EACH rounded to fp64 (no fused multiply-add) and x the solution as eicos_batch_solution returns it: u is,
 * bit for bit, what a host restatement in that order computes from eicos_batch_solution.  It is computed from whatever x the instance
 * ended with, whatever its exit code (as x_out is) -- unless the call is a step that holds theta and the handle has a fallback map
 * (eicos_batch_set_fallback_map, below) whose mask holds the class the instance ended in.
 * eicos_batch_outputs: synchronous -- waits for the handle's stream, evaluates the map on the current x of instances [first, first+count)
 * and fetches the rows (a pinned destination gets one copy, a pageable one goes through the bounce buffers like eicos_batch_solution).
 * eicos_batch_outputs_device: the same into caller-owned device memory, asynchronous on the handle's stream.  Both: EICOS_E_INVALID
 * without a map ("no output map").
 * eicos_batch_update_param_solve: eicos_batch_update_param + eicos_batch_solve + eicos_batch_outputs of the whole batch in ONE synchronous
 * call, with the conventions of eicos_batch_update_rhs_solve (u_out [batch][r], x_out [batch][n], exitcodes [batch]: each optional).  When
 * theta is memory the GPU addresses directly (pinned / registered host memory or device memory), the handle has an LDS vector and a theta
 * row fits it, each workgroup of the solve kernel expands the theta row of the instance it is about to solve and, when it is done, writes
 * that instance's u row (and x row, if asked) straight to the caller's pinned or device array (path 5): 8 k bytes in, 8 r bytes out per
 * instance, one launch.  Otherwise (pageable theta, EICOS_FUSED_UPDATE=0, no LDS vector, k beyond the LDS vector) it runs the three calls;
 * a device or pageable u_out the kernel did not write is filled by the range kernel and a copy, as x_out is.  Bit-identical on every path.
 * EICOS_E_INVALID for u_out != NULL without an output map ("no output map") and without a parameter map ("no parameter map"). */
int eicos_batch_set_output_map(eicos_batch *hd, int r, const eicos_affine_map *u);
int eicos_batch_output_count(eicos_batch *hd);
int eicos_batch_outputs(eicos_batch *hd, int first, int count, double *u /* host [count][r] */);
int eicos_batch_outputs_device(eicos_batch *hd, int first, int count, double *du);
int eicos_batch_update_param_solve(eicos_batch *hd, const double *theta /* [batch][k] */, double *u_out /* [batch][r], optional */,
                                   double *x_out /* [batch][n], optional */, int *exitcodes /* optional */);

/* ---- plant map and the closed-loop rollout (no reference counterpart).  In a simulated closed loop the next parameter row is itself
 * affine in the current one and in the move just computed: theta+ = f0 + F [theta | u] (+ w).  A handle holds one such map beside the
 * other two: eicos_affine_map with base[k] and a CSR matrix k x (k + r) (rowptr[k + 1], col / val[rowptr[k]]; columns index
 * z = [theta (k) | u (r)], i.e. lie in [0, k + r)).  eicos_batch_set_plant_map COPIES the host arrays into one device allocation; a later
 * call replaces the map, f = NULL removes it (either way the per-instance values of eicos_batch_set_plant_values are dropped).  It needs a parameter map (k > 0) and an output map (r > 0) and remembers the (k, r) it was
 * validated for.  EICOS_E_INVALID, with a message naming the fault, for rowptr[0] != 0, decreasing row pointers, a column outside
 * [0, k + r), "no parameter map" and "no output map".  eicos_batch_has_plant_map: 1 / 0.
 * eicos_batch_rollout takes every instance through `steps` closed-loop steps in ONE synchronous call.  For instance i:
 *     theta_traj[i][0] = theta0[i], copied verbatim;
 *     for t = 0 .. steps-1: exactly what eicos_batch_update_param_solve does for the row theta_traj[i][t] -- the update, the solve (with the
 *     warm start and dynamic regularisation set on the handle) and the output row: u_traj[i][t] = that row, exitcodes[i][t] / iters[i][t]
 *     = that solve's exit code / iteration count -- and then row j of theta_traj[i][t+1]:
 *         acc = base[j];  for s in rowptr[j] .. rowptr[j+1]-1, in stored order:  acc = acc + (val[s] * z[col[s]])
 *         with z = [theta_traj[i][t] | u_traj[i][t]];  then, if w != NULL:  acc = acc + w[i][t][j]
 *     with every product and every sum rounded to fp64 on its own (no fused multiply-add).
 * A step whose solve does not end OPTIMAL still produces its u row and the loop goes on (as u_out does); the per-step codes are the
 * caller's record.  The rollout leaves the handle (instance slabs, eicos_batch_info / _solution / _duals, the KKT values of eicos_debug_kkt)
 * and the returned arrays equal, bit for bit, to `steps` calls of eicos_batch_update_param_solve whose theta rows a host loop advances in
 * the order above, on every build of the solve kernel and on both paths below; afterwards eicos_batch_info / _solution describe the last step.
 * FUSED (eicos_batch_last_rollout_launches = 1): one launch of the solve kernel, in which a workgroup takes an instance through all its
 * steps before it pulls the next one -- no launch, no transfer and no barrier across the batch between steps.  Taken when the handle has
 * an LDS vector, k + r <= the length of that vector (the padded KKT dimension: the plant map stages [theta | u] there) and
 * EICOS_FUSED_UPDATE is not 0.  Otherwise (= steps) the call enqueues, per step, the parametric range kernel, the solve launch, the output
 * range kernel and the plant range kernel on the handle's stream, without host synchronisation in between.
 * Every array may be pageable, pinned / registered or device memory: the handle keeps device copies of the trajectories (grown on
 * demand), copies theta0 and w in before the launch and the results out after it.  theta_traj, exitcodes and iters are optional.
 * EICOS_E_INVALID for steps < 1, u_traj == NULL, theta0 == NULL, a missing map of any of the three kinds, and a plant map installed for
 * another (k, r) than the maps now installed (the message names both pairs). */
int eicos_batch_set_plant_map(eicos_batch *hd, const eicos_affine_map *f);
int eicos_batch_has_plant_map(eicos_batch *hd);
int eicos_batch_rollout(eicos_batch *hd, int steps, const double *theta0 /* [batch][k] */, const double *w /* [batch][steps][k], optional */,
                        double *u_traj /* [batch][steps][r] */, double *theta_traj /* [batch][steps + 1][k], optional */,
                        int *exitcodes /* [batch][steps], optional */, int *iters /* [batch][steps], optional */);
int eicos_batch_last_rollout_launches(eicos_batch *hd); /* solve-kernel launches of the most recent rollout: 1 = fused */

/* ---- fallback map: a backup output law for steps whose solve does not end well (no reference counterpart).  A step that stops at the
 * iteration cap or ends NUMERICS / PINF would hand the plant a u row formed from a meaningless iterate.  A handle may hold one affine
 * law u = v0 + V theta for all its instances -- eicos_affine_map with base[r] and a CSR matrix r x k (rowptr[r + 1], col / val[rowptr[r]];
 * columns index theta) -- and a mask of exit classes (EICOS_SEL_*).
 * The rule: in a step call that has theta in hand -- eicos_batch_update_param_solve, eicos_batch_update_param_solve_subset,
 * eicos_batch_rollout, eicos_batch_rollout_jacobian and their eicos_multi_* forms --, an instance whose FINAL record (after the second
 * attempt, when a retry policy took one) falls in a class of the mask gets its u row from the law instead of from the output map,
 * wherever that row is read: the caller's u_out, the rollout's u trajectory, the plant map, and the recorded Jacobian.  Row j of instance i:
 *     acc = v0[j];  for t in rowptr[j] .. rowptr[j+1]-1, in stored order:  acc = acc + (val[t] * theta[i][col[t]])
 * with the product and the sum EACH rounded to fp64, like every other map.  In a step over a subset theta[i] is the row at the
 * instance's position in the list.  On every path (fused or not; theta and u_out pageable, pinned or device memory; every kernel build)
 * the bits are the same.  A step that is asked for no u row (u_out == NULL) forms none and counts nothing.
 * The fallback leaves x, y, z, s, the info records, the retry counts, x_out, the exit codes a call returns and the codes / iters of a
 * rollout bit for bit what they are without the map: that the law fired for a step is eicos_exit_class(code, 1) & mask, and per instance
 * the cumulative counter eicos_batch_fallback_counts reads (fired[i] = steps of instance first + i whose u row the law formed since the
 * counter was last zeroed; reset != 0 zeroes the counters read; it waits for the handle's stream).
 * In eicos_batch_rollout_jacobian a step whose fallback fired records J_t = V as a dense r x k block -- every row zero-filled, then
 * J[j][col[t]] = J[j][col[t]] + val[t] in stored order -- and res_t = 0.0, and runs no adjoint; eicos_batch_rollout_gradient then sees
 * finite rows for it.
 * The calls that hold no theta -- eicos_batch_outputs*, eicos_batch_param_jacobian*, eicos_batch_output_jacobian*, eicos_batch_adjoint* --
 * stay the plain map of x (and NaN rows for instances that did not end OPTIMAL / OPTIMAL_INACC), with or without a fallback map.
 * eicos_batch_set_fallback_map COPIES the host arrays into one device allocation and starts the counters at zero; a later call
 * replaces the map, v == NULL or mask == 0 removes it.  It needs a parameter map (k > 0) and an output map (r > 0) and remembers the (k, r)
 * it was validated for: a step under maps with another (k, r) is refused ("install it again").  Installing or removing it counts as a
 * map install for eicos_batch_rollout_gradient, which refuses a Jacobian trajectory recorded before it.  EICOS_E_INVALID, with a message
 * naming the fault and nothing changed, for rowptr[0] != 0, decreasing row pointers, a column outside [0, k), mask bits outside
 * EICOS_SEL_ALL, a mask that is EICOS_SEL_UNSOLVED alone (an attempted instance is never in that class), "no parameter map" and "no
 * output map".  A mask that holds EICOS_SEL_OPTIMAL is accepted: every step then takes the law.
 * eicos_batch_fallback_mask: the installed mask, 0 = no fallback map. */
int eicos_batch_set_fallback_map(eicos_batch *hd, unsigned mask, const eicos_affine_map *v);
int eicos_batch_fallback_mask(eicos_batch *hd);
int eicos_batch_fallback_counts(eicos_batch *hd, int first, int count, int *fired /* host [count] */, int reset);

/* ---- matrix map: G and A affine in theta (no reference counterpart).  When a model is linearised around the measured state, a gain is
 * scheduled or a cone constraint depends on the state, the VALUES of G and A move with theta as well: Gpr = G0 + Gm theta,
 * Apr = A0 + Am theta.  A handle holds one such map beside the parameter map: per matrix an eicos_affine_map with rows = nnzG (resp. nnzA),
 * one row per stored value in the CSC order of Gpr / Apr -- base[rows] and a CSR matrix rows x k (rowptr[rows + 1], col / val[rowptr[rows]];
 * columns lie in [0, k), k = the installed parameter map's theta length).  Most rows of a realistic map are empty: that value is base[e].
 * eicos_batch_set_matrix_map COPIES the host arrays into one device allocation of its own; a NULL matrix is not mapped; a later call
 * replaces the map, both NULL removes it.  It needs a parameter map (k > 0) and remembers the k it was validated for.
 * eicos_batch_has_matrix_map: bit 0 = G mapped, bit 1 = A mapped, 0 = none.  eicos_batch_matrix_map_count: that k, 0 = no matrix map.
 * Entry e of instance i:
 *     acc = base[e];  for t in rowptr[e] .. rowptr[e+1]-1, in stored order:  acc = acc + (val[t] * theta[i][col[t]])
 * with the product and the sum EACH rounded to fp64 (no fused multiply-add).
 * There are no new update entry points: with a matrix map installed, every call that consumes theta -- eicos_batch_update_param,
 * _update_param_device, _update_param_solve, eicos_batch_rollout and their eicos_multi_* forms -- becomes a FULL updateData
 * (re-equilibration included) whose inputs the GPU forms from theta.  The state such a call leaves for an instance (instance slabs, the
 * KKT values of eicos_debug_kkt, every later solve / solution / duals / info) equals, bit for bit, this host sequence on arrays
 * evaluated on the host in the order above (and c, h, b in the order of eicos_batch_update_param):
 *     1. eicos_batch_update(first, count, G(theta) or NULL, A(theta) or NULL, c(theta) or NULL, h(theta), b(theta)) with h(theta) passed
 *        only if G is mapped and b(theta) only if A is mapped; an unmapped group is NULL: kept and re-equilibrated, as updateData does;
 *     2. then eicos_batch_update_rhs(NULL, h(theta) if h is mapped and G is not, b(theta) if b is mapped and A is not), when not empty.
 * Without a matrix map nothing changes for any call.
 * Range path (eicos_batch_update_param / _device, peer theta, and the step / rollout when they are not fused): a row-parallel kernel expands
 * [Gpr | Apr | c | h | b] of a chunk of instances into a device staging buffer of the handle (grown on demand and capped: a large batch
 * goes in several chunks, stream-ordered) and the unchanged updateData kernel runs on it; then the right-hand-side kernel for step 2.
 * Fused path (eicos_batch_update_param_solve: path 5; eicos_batch_rollout: one launch): each workgroup of the solve kernel evaluates its
 * instance's entries from the theta row and runs updateData's equilibration right before it solves.  Taken when the conditions of the
 * fused eicos_batch_update_solve hold (an LDS vector; n, p <= 8 and m <= 16 entries per thread of the workgroup) AND those of
 * eicos_batch_update_param_solve / _rollout (GPU-addressable theta, k resp. k + r <= the LDS vector, EICOS_FUSED_UPDATE not 0); otherwise
 * the calls run per step through the range path.  Bit-identical on every path.
 * EICOS_E_INVALID, with a message naming the fault, for rowptr[0] != 0, decreasing row pointers, a column outside [0, k), a map for a
 * matrix the pattern stores no entries of, "no parameter map", and a G map while the parameter map has no h group and m > 0 / an A map
 * while it has no b group and p > 0 (updateData reads h only with Gpr and b only with Apr).  The last two are checked again by every call
 * that consumes theta, because the parameter map can be replaced afterwards; such a call also refuses a matrix map installed for another k
 * than the one now installed (the message names both). */
int eicos_batch_set_matrix_map(eicos_batch *hd, const eicos_affine_map *G, const eicos_affine_map *A);
int eicos_batch_has_matrix_map(eicos_batch *hd);
int eicos_batch_matrix_map_count(eicos_batch *hd);

/* ---- solve: replaces exitcode Solver::solve(bool) (reference include/eicos.hpp:158,
 * src/eicos.cpp:848-1262) for every instance of the batch.  exitcodes (host, [batch]) may be
 * NULL.  Synchronous: returns after the GPU work has completed. */
int eicos_batch_solve(eicos_batch *hd, int *exitcodes);
/* Asynchronous half: enqueue on the handle's stream and return; eicos_batch_sync waits. */
int eicos_batch_solve_async(eicos_batch *hd);
int eicos_batch_sync(eicos_batch *hd);

/* ---- solve a chosen subset of the batch: by index list or by exit class (no reference counterpart).  The update calls work on ranges
 * of instances; these are the matching solve calls, for "retry the three instances that stopped at the iteration cap under other
 * settings", "only the controllers whose sample time fired", "only the scenarios still alive".
 * Exit classes: every instance is in exactly ONE class, by the exit code and n_factor of its info record.  eicos_exit_class returns that
 * bit; it needs no handle and no GPU, and the selection kernel on the GPU evaluates the very same function.
 *   EICOS_SEL_OPTIMAL (0)  _PINF (1)  _DINF (2)  _OPTIMAL_INACC (10)  _PINF_INACC (11)  _DINF_INACC (12)
 *   EICOS_SEL_MAXIT (-1)  _NUMERICS (-2)  _OUTCONE (-3)  _FATAL (-7)  EICOS_SEL_OTHER (any other code)
 *   EICOS_SEL_UNSOLVED: n_factor == 0 -- never solved and never given a starting point; it takes precedence over the code, which is 0
 *   in a fresh record. */
enum {
    EICOS_SEL_OPTIMAL = 1 << 0, EICOS_SEL_PINF = 1 << 1, EICOS_SEL_DINF = 1 << 2,
    EICOS_SEL_OPTIMAL_INACC = 1 << 3, EICOS_SEL_PINF_INACC = 1 << 4, EICOS_SEL_DINF_INACC = 1 << 5,
    EICOS_SEL_MAXIT = 1 << 6, EICOS_SEL_NUMERICS = 1 << 7, EICOS_SEL_OUTCONE = 1 << 8, EICOS_SEL_FATAL = 1 << 9,
    EICOS_SEL_OTHER = 1 << 10, EICOS_SEL_UNSOLVED = 1 << 11,
    EICOS_SEL_FAILED = EICOS_SEL_MAXIT | EICOS_SEL_NUMERICS | EICOS_SEL_OUTCONE | EICOS_SEL_FATAL,
    EICOS_SEL_ALL = (1 << 12) - 1,
    EICOS_SEL_NOT_OPTIMAL = EICOS_SEL_ALL & ~EICOS_SEL_OPTIMAL
};
int eicos_exit_class(int exitcode, int n_factor);
/* eicos_batch_select: the instances whose class is in `mask`, ascending, into idx_out ([batch], optional) and their number into
 * *count_out (optional).  Waits for the handle's stream, runs the selection kernel over the info records in HBM and copies the count
 * (and the ids, if asked) back: no info record travels.
 * eicos_batch_solve_subset_async / _solve_subset: an ORDINARY solve launch over the instances idx[0 .. count) (host array) instead of
 * the whole batch -- the same kernel with the launch order = the chosen ids and the batch = their number, min(resident workgroups,
 * count) workgroups, and everything else as for eicos_batch_solve: warm start, shift map, a caller-supplied iterate, shared matrix
 * values, settings and dynamic regularisation by value, the timing ring.  Up to one instance per CU the ids are taken in list order;
 * beyond that longest first, as a whole-batch launch orders its instances.  The synchronous form returns the exit codes of the chosen
 * instances in list order (exitcodes [count], optional), gathered on the GPU: no info record of another instance travels.
 * eicos_batch_solve_where = select + subset solve, with the id list used in place on the GPU: it waits for the handle's stream, runs
 * the selection kernel, reads the count (and the ids, if asked) -- the one host synchronisation; a retry follows a finished solve anyway
 * -- and launches; it returns when the solve has finished, like eicos_batch_solve.  idx_out ([batch], optional, ascending), *count_out (optional), exitcodes ([*count_out], order of idx_out, optional).
 * Contract, for every instance IN the subset: take a twin handle on which eicos_batch_solve ran at the same point of the same call
 * sequence; the instance ends in the same state as on the twin, bit for bit -- slab, eicos_batch_solution, _duals, _info except solve_us,
 * eicos_debug_kkt -- cold, warm, under a shift map, from a caller-supplied iterate and with shared matrix values.
 * Contract, for every instance OUTSIDE the subset: nothing the host can read changes, its info record and solve_us included (the
 * LDS-resident build writes back only the slabs it solved; shared matrix values are kept).
 * An empty subset (count == 0, or a mask nobody is in) is EICOS_OK with no launch and nothing recorded: eicos_batch_last_solve_ms and the
 * timing ring keep their last entry.
 * eicos_batch_gather: rows of the chosen instances -- x [count][n], y [count][p], z, s [count][m] exactly as eicos_batch_solution /
 * _duals return them, info [count] -- in list order; any destination may be NULL.  A row-gather kernel packs them into a compact device
 * buffer of the handle (grown on demand) and ONE copy takes that buffer to the host, over the paths of eicos_batch_solution.
 * eicos_debug_trace after a subset launch: workspace slot q holds instance order[q], q < count; it needs count <= resident workgroups
 * (instead of batch <=), and an instance that was not in the last launch is EICOS_E_INVALID ("instance not in the last launch").
 * EICOS_E_INVALID, with a message naming the fault and NO state changed (checked on the host before anything is enqueued): a NULL handle;
 * count < 0 or count > batch; NULL idx with count > 0; an index outside [0, batch) (the message names index and position); a DUPLICATE
 * index (named: two workgroups would solve one slab at once; eicos_batch_gather refuses it like the solve calls); mask == 0 or bits above
 * bit 11.
 * Feeding a subset: the index-list forms of the update calls and the closed-loop step over a subset, below.
 * Out of scope: rollouts over a subset, fused FULL and right-hand-side steps over a subset (eicos_batch_update_solve / _update_rhs_solve
 * take the whole batch), and id lists that live on the GPU (a "step where"). */
int eicos_batch_select(eicos_batch *hd, unsigned mask, int *idx_out /* [batch], ascending, optional */, int *count_out);
int eicos_batch_solve_subset_async(eicos_batch *hd, const int *idx /* host [count] */, int count);
int eicos_batch_solve_subset(eicos_batch *hd, const int *idx, int count, int *exitcodes /* [count], list order, optional */);
int eicos_batch_solve_where(eicos_batch *hd, unsigned mask, int *idx_out /* [batch], optional, ascending */, int *count_out,
                            int *exitcodes /* [*count_out], order of idx_out, optional */);
int eicos_batch_gather(eicos_batch *hd, const int *idx, int count, double *x, double *y, double *z, double *s, eicos_info *info);

/* ---- update, read and step a chosen subset (no reference counterpart): the index-list forms of the update calls.
 * idx is always a HOST array of `count` distinct ids in [0, batch); row q of every data array ([count][...], row-major) belongs to
 * instance idx[q] -- the list-order convention of eicos_batch_solve_subset and _gather.  Everything else is the range namesake's
 * (eicos_batch_update / _update_rhs / _update_param / _set_iterate and their _device forms): NULL groups, h read only with Gpr and b only
 * with Apr in the full form, the memory kinds and transfer paths (pageable host arrays through the bounce pipeline in chunks, pinned or
 * registered arrays read in place, device arrays read in place by one asynchronous launch), synchrony, eicos_batch_last_update_path, the
 * timing ring, a matrix map turning update_param_indexed into a full updateData (expanded on the GPU, chunked), and the namesake's
 * refusals.  The list is checked as for the subset solves (NULL handle, count outside [0, batch], NULL idx, an id out of range, a
 * DUPLICATE -- two workgroups would write one slab): EICOS_E_INVALID with a message naming the fault and no state changed.  An empty list
 * is EICOS_OK: nothing enqueued, nothing recorded.
 * Contract: the state the call leaves (slabs, solution, duals, info, eicos_debug_kkt, every later solve) equals, bit for bit, that of the
 * loop  for q: range_form(first = idx[q], count = 1, row q)  on a twin handle; instances outside the list keep everything the host can
 * read.  Shared matrix values (eicos_batch_shared_values) are kept by the rhs, param (without a matrix map) and iterate forms and dropped
 * by eicos_batch_update_indexed and by the param form under a matrix map, as a sub-range call drops them; an indexed call never detects.
 * The ids travel through the handle's pinned list buffer into a device area of their own: a queued subset launch keeps its ids. */
int eicos_batch_update_indexed(eicos_batch *hd, const int *idx /* host [count] */, int count, const double *Gpr, const double *Apr,
                               const double *c, const double *h, const double *b);
int eicos_batch_update_rhs_indexed(eicos_batch *hd, const int *idx, int count, const double *c, const double *h, const double *b);
int eicos_batch_update_param_indexed(eicos_batch *hd, const int *idx, int count, const double *theta /* [count][k] */);
int eicos_batch_set_iterate_indexed(eicos_batch *hd, const int *idx, int count, const double *x, const double *y, const double *z, const double *s);
/* ... data arrays in device memory (idx stays a host array), asynchronous on the handle's stream like their range namesakes */
int eicos_batch_update_indexed_device(eicos_batch *hd, const int *idx, int count, const double *dGpr, const double *dApr, const double *dc,
                                      const double *dh, const double *db);
int eicos_batch_update_rhs_indexed_device(eicos_batch *hd, const int *idx, int count, const double *dc, const double *dh, const double *db);
int eicos_batch_update_param_indexed_device(eicos_batch *hd, const int *idx, int count, const double *dtheta);
int eicos_batch_set_iterate_indexed_device(eicos_batch *hd, const int *idx, int count, const double *dx, const double *dy, const double *dz,
                                           const double *ds);
/* eicos_batch_outputs_indexed / _device: row q of u [count][r] = the output map on the current x of instance idx[q], bit-identical to row
 * idx[q] of eicos_batch_outputs (the same range kernel, reading the slab of idx[q]).  Refusals: those of eicos_batch_outputs (no output
 * map, NULL u, a device pointer handed to the host form) and of the list check. */
int eicos_batch_outputs_indexed(eicos_batch *hd, const int *idx, int count, double *u /* host [count][r] */);
int eicos_batch_outputs_indexed_device(eicos_batch *hd, const int *idx, int count, double *du);
/* ---- Adjoint sensitivities: gradients through a solve, and the Jacobian of the output map ----
 * Definition.  For an instance whose last solve ended OPTIMAL or OPTIMAL_INACC (codes 0 and 10), with the returned (x, y, z, s) and the
 * caller's un-equilibrated A, G:
 *
 *     K = [ 0  A'  G' ]      W^2 = the NT scaling of (s, z): s_i / z_i on an LP row, eta^2 * Wbar^2 per second-order cone
 *         [ A  0   0  ]            (what every pass of the solve puts into its KKT matrix)
 *         [ G  0  -W^2]
 *     K [w_x; w_y; w_z] = [g; 0; 0],      grad_c = -w_x,   grad_b = w_y,   grad_h = w_z
 *
 * (grad_c, grad_h, grad_b) is the gradient of l = g'x with respect to (c, h, b).  It is exact for the central-path point at the
 * iterate's mu, where ds = -W^2 dz holds exactly, and therefore the derivative of the solution map wherever that derivative exists: a
 * unique solution and strict complementarity.  ELSEWHERE -- a degenerate or non-unique optimum -- IT IS A SMOOTHED VALUE, not a
 * derivative: K is then close to singular and the result depends on where on the central path the solve stopped.
 * With a parameter map c = c0 + C theta, h = h0 + H theta, b = b0 + B theta and an output map u = u0 + U x, row i of the Jacobian
 * du / dtheta is J[i, :] = grad_c(U_i)' C + grad_h(U_i)' H + grad_b(U_i)' B: r adjoint solves instead of k forward solves.
 * Invariances: W does not change under the common 1 / tau scaling of the embedding; equilibration enters as K = D^-1 K~ D^-1 with
 * D = diag(1 / xe, 1 / ae, 1 / ge), so w = D K~^-1 D rhs; the static regularisation of the factor is removed by the iterative refinement
 * of the KKT solve against the unregularised system, as in a solve.
 * Cost: one factorisation and nrhs refined KKT solves per instance, in one launch over the chosen instances, under the handle's
 * linsysacc, irerrfact, nitref and dynamic regularisation (the refinement takes one step beyond the linsysacc threshold: the small
 * components of w, grad_c at a vertex, converge later than the error norm shows).
 *
 * eicos_batch_adjoint: idx = a host list of `count` distinct ids, or NULL = instances 0 .. count-1; g [count][nrhs][n], 1 <= nrhs <=
 * EICOS_ADJOINT_MAX_RHS; outputs (host, each optional) grad_c [count][nrhs][n], grad_h [count][nrhs][m], grad_b [count][nrhs][p] and
 * res [count][nrhs] = the error norm at which the refinement of that KKT solve stopped, divided by 1 + |rhs|_inf, in the equilibrated
 * space in which it is measured.  An instance whose last solve did not end OPTIMAL / OPTIMAL_INACC, or whose recomputed scalings or
 * factorisation fail, gets NaN in every row and in res; the call still returns EICOS_OK.  Synchronous.
 * eicos_batch_output_jacobian / _device: J [count][r][k] and res [count][r] (optional) from the installed parameter and output maps; the
 * right-hand sides are the rows of U and the gradients are contracted on the GPU without being stored.  The device form takes J and res in
 * device memory and is asynchronous on the handle's stream; both forms return the same bits.
 * Refusals (EICOS_E_INVALID with a message, nothing changed): a duplicate or out-of-range id, nrhs outside its range, NULL g or J,
 * output_jacobian without a parameter map and an output map, or with a matrix map installed (its derivative has dG and dA terms:
 * eicos_batch_param_jacobian, below, forms them).
 * An adjoint call changes nothing a later call reads: x, y, z, s, every info field, the retry counts and what a warm start takes from the
 * previous solve stay as they are (eicos_debug_kkt afterwards shows the scaling block at the returned iterate). */
#define EICOS_ADJOINT_MAX_RHS 64
int eicos_batch_adjoint(eicos_batch *hd, const int *idx, int count, int nrhs, const double *g, double *grad_c, double *grad_h,
                        double *grad_b, double *res);
int eicos_batch_output_jacobian(eicos_batch *hd, const int *idx, int count, double *J, double *res);
int eicos_batch_output_jacobian_device(eicos_batch *hd, const int *idx, int count, double *dJ, double *dres);
/* Matrix data.  Linearising the optimality conditions with dA, dG present (A'dy + G'dz = -dc - dA'y - dG'z, A dx = db - dA x,
 * G dx - W^2 dz = dh - dG x) gives the gradient of l = g'x with respect to the stored value e = (row i, column j) of G and of A:
 *
 *     grad_G[e] = grad_c[j] z[i] - grad_h[i] x[j],      grad_A[e] = grad_c[j] y[i] - grad_b[i] x[j]
 *
 * with the returned, un-equilibrated x, y, z: a sampled outer product on the sparsity pattern, which costs no further factorisation and
 * no further KKT solve.  Each is formed as written (two products, one difference, each rounded on its own) from the stored values of
 * grad_c, grad_h, grad_b.  The caveat of the definition above applies unchanged.
 * eicos_batch_adjoint_data: eicos_batch_adjoint with two more optional outputs, grad_G [count][nrhs][nnzG] and grad_A [count][nrhs][nnzA]
 * in the CSC order of Gpr / Apr.  grad_c, grad_h, grad_b and res are those of eicos_batch_adjoint bit for bit; an ineligible instance
 * gets NaN rows.  Host arrays, synchronous.
 * With a matrix map Gpr = G0 + M_G theta, Apr = A0 + M_A theta the derivative with respect to theta gains grad_G' M_G + grad_A' M_A:
 * eicos_batch_param_jacobian / _device: J [count][r][k] = du / dtheta through the output map and WHICHEVER of the parameter map and the
 * matrix map are installed (at least one; installed for the same k).  Without a matrix map: the bits of eicos_batch_output_jacobian.
 * eicos_batch_param_gradient / _device: grad_theta [count][nrhs][k] = the gradient of g'x with respect to theta through the same maps,
 * g [count][nrhs][n] from the caller; no output map is needed.  With g = the rows of U: the bits of eicos_batch_param_jacobian.
 * Contraction order (fixed): per chunk of eight columns every thread sums, over the rows it owns (row e of a group: thread e mod T), the
 * c, h, b groups in ascending row order, then its stored values of G, then of A, each ascending; one workgroup reduction per chunk.  No
 * gradient row is stored.  The device forms take g, J / grad_theta and res in device memory and are asynchronous on the handle's stream
 * (what a training loop on the GPU calls); the host forms are synchronous; both return the same bits.
 * Refusals (EICOS_E_INVALID with a message, nothing changed): those of eicos_batch_adjoint (a duplicate or out-of-range id, nrhs outside
 * its range, NULL g / J / grad_theta); param_jacobian without an output map; param_jacobian and param_gradient with neither a parameter
 * map nor a matrix map, or with a matrix map installed for another k than the parameter map; a host pointer handed to a device form or
 * a device pointer handed to a host form. */
int eicos_batch_adjoint_data(eicos_batch *hd, const int *idx, int count, int nrhs, const double *g, double *grad_c, double *grad_h,
                             double *grad_b, double *grad_G, double *grad_A, double *res);
int eicos_batch_param_jacobian(eicos_batch *hd, const int *idx, int count, double *J, double *res);
int eicos_batch_param_jacobian_device(eicos_batch *hd, const int *idx, int count, double *dJ, double *dres);
int eicos_batch_param_gradient(eicos_batch *hd, const int *idx, int count, int nrhs, const double *g, double *grad_theta, double *res);
int eicos_batch_param_gradient_device(eicos_batch *hd, const int *idx, int count, int nrhs, const double *dg, double *dgrad_theta,
                                      double *dres);
/* The cone scaling of the adjoint's K, per handle.  EICOS_ADJOINT_NT (the default): W^2 = the NT scaling of the returned (s, z), as
 * defined above.  On an LP row that is s_i / z_i, which needs no centrality.  On an ACTIVE, strictly complementary second-order cone --
 * s = (l1 c1 + l2 c2) / 2, z = (w1 c1 + w2 c2) / 2 in a common Jordan frame c1,2 = (1, +-u), l1 and w2 of order one, l2 and w1 close to
 * zero -- W^2 has the eigenvalues l1 / w1 and l2 / w2 on the frame and eta^2 = (l1 / w2) sqrt(l2 w2 / (l1 w1)) on the d - 2 directions
 * perpendicular to u, along which the optimum slides on the cone's surface.  The tangent of the complementarity manifold there is
 * ds = -(l1 / w2) dz, so eta^2 is right only up to the ratio of the two complementary products: whatever centrality error the last
 * step of the solve left, a factor of order one.  Where the cone's curvature fixes the optimum, the NT-mode gradients are wrong by
 * that factor.
 * EICOS_ADJOINT_CENTRED: the same K with W^2 = the NT scaling of the RE-CENTRED pair, formed per second-order cone (rows o .. o+d-1,
 * head o, tail 1:) from the un-equilibrated result rows; LP rows are untouched:
 *
 *     v = s[1:] / s[0] - z[1:] / z[0];  nv = |v|_2;  nv == 0 (which covers d == 1): the cone stays as it is
 *     u = v / nv
 *     l1 = s[0] + s[1:]'u;  l2 = s[0] - s[1:]'u;  w1 = z[0] + z[1:]'u;  w2 = z[0] - z[1:]'u
 *     min(l1, l2, w1, w2) <= 0: the cone stays as it is
 *     mu = sqrt(l1 w1 l2 w2)
 *     l1 >= w1: w1 = mu / l1, else l1 = mu / w1;      l2 >= w2: w2 = mu / l2, else l2 = mu / w2
 *     s = ((l1 + l2) / 2, (l1 - l2) / 2 u);   z = ((w1 + w2) / 2, (w1 - w2) / 2 u)
 *
 * -- the large eigenvalue of each complementary pair is kept, the small one replaced so that l1 w1 = l2 w2.  Everything else of the
 * definition is unchanged (the factor path, the refinement against the unregularised system, the NaN rules, the gradient and contraction
 * formulas), and a cone the rule leaves alone behaves exactly as under EICOS_ADJOINT_NT.  Use it on any pattern with cones; on a pattern
 * without cones both modes give the same bits.
 * eicos_batch_set_adjoint_scaling: the mode holds from the next adjoint launch, for every path: eicos_batch_adjoint, _adjoint_data,
 * _output_jacobian, _param_jacobian, _param_gradient and their device forms, and the adjoints of eicos_batch_rollout_jacobian (fused or
 * not) -- through its J and its recorded rows, the three rollout gradients.  A J trajectory already on the handle stays as it was
 * recorded; setting the mode is no map install.  eicos_debug_kkt after an adjoint call then shows the CENTRED scaling block.  A solve
 * never sees the mode.  An unknown mode is EICOS_E_INVALID with a message naming the value, and nothing changes.
 * eicos_batch_adjoint_scaling: the handle's mode (negative: an error code). */
#define EICOS_ADJOINT_NT 0
#define EICOS_ADJOINT_CENTRED 1
int eicos_batch_set_adjoint_scaling(eicos_batch *hd, int mode);
int eicos_batch_adjoint_scaling(eicos_batch *hd);
/* ---- rollout sensitivities: the Jacobian of every step of a rollout, and the gradient of a closed-loop cost (no reference counterpart).
 * eicos_batch_rollout_jacobian: eicos_batch_rollout -- the first eight arguments with exactly its meaning, arrays in pageable, pinned or
 * device memory -- that also records J_traj [batch][steps][r][k] (required) and res_traj [batch][steps][r] (optional): J_traj[i][t] and
 * res_traj[i][t] are what eicos_batch_param_jacobian returns for instance i when it is called right after step t's solve -- under the
 * handle's linsysacc, irerrfact, nitref and dynamic regularisation, through whichever of the parameter map and the matrix map are
 * installed, at the iterate the step ended with (after the second attempt, if a retry policy took one).  The rows of a step that did not
 * end OPTIMAL / OPTIMAL_INACC are NaN, and the loop goes on.
 * Defined by its HOST TWIN, bit for bit:  for t = 0 .. steps-1:  eicos_batch_update_param_solve(theta_t);  eicos_batch_param_jacobian;
 * the plant map on the host.  Every returned array equals the twin's, and so does the handle afterwards: slabs, solution, duals, info,
 * retry counts, eicos_debug_kkt.  u_traj, theta_traj, exitcodes, iters and x, y, z, s, info also equal those of plain
 * eicos_batch_rollout; only the scaling block eicos_debug_kkt shows follows the adjoint, as documented for eicos_batch_adjoint.
 * FUSED under the conditions of the fused rollout (eicos_batch_last_rollout_launches = 1): one launch of the rollout twin of the solve
 * kernel, whose workgroups run the adjoint of a step while its iterate is still in place, between the step's records and its plant map.
 * Otherwise the per-step enqueue of eicos_batch_rollout with one adjoint launch (the contracted device form) between the output and the
 * plant kernels, no host synchronisation between steps; eicos_batch_last_rollout_launches = steps.  Same bits on either path.
 * The handle keeps the device copy of the J trajectory of its most recent rollout_jacobian for:
 * eicos_batch_rollout_gradient / _device: the gradient of  L = sum_t gu_t' u_t + sum_t gtheta_t' theta_t  over that rollout (T = its step
 * count) with respect to theta_0 and, optionally, to the disturbances.  gu [batch][T][r] = dL/du_t and gtheta [batch][T+1][k] = dL/dtheta_t:
 * each optional, at least one given; grad_theta0 [batch][k]; grad_w [batch][T][k], optional.  One small workgroup per instance sweeps
 * backward through  dtheta_{t+1}/dtheta_t = F_theta + F_u J_t  (F = [F_theta | F_u] the plant map).  The order is fixed, every product
 * and sum is rounded on its own (no FMA), a missing cotangent array counts as 0.0 and is still added:
 *
 *     lambda = gtheta[T]
 *     for t = T-1 .. 0:
 *         grad_w[t] = lambda
 *         v[c] = 0.0;  for i = 0..k-1, s in rowptr[i]..rowptr[i+1]-1 (stored order), col[s] == c:  v[c] = v[c] + (val[s] * lambda[i])     (c in [0, k + r))
 *         mu[j] = gu[t][j] + v[k + j]
 *         lambda'[c] = gtheta[t][c] + v[c];  for j = 0..r-1:  lambda'[c] = lambda'[c] + (J[t][j][c] * mu[j])
 *         lambda = lambda'
 *     grad_theta0 = lambda
 *
 * A NaN Jacobian row (a step that did not end OPTIMAL / OPTIMAL_INACC) makes that instance's gradient NaN.  The host form is synchronous;
 * the device form takes all four arrays in device memory, is asynchronous on the handle's stream and returns the same bits.
 * Caveats, beside the one of the definition above (a degenerate optimum gives a smoothed value): with a warm start or a shift map the
 * point step t + 1 returns depends on step t's iterate within the exit tolerance -- the gradient treats each step's solution as a
 * function of theta_t alone; gradients with respect to the plant map's own entries come from eicos_batch_rollout_plant_gradient (below),
 * those with respect to the entries of the parameter, matrix, output and fallback maps are out of scope.
 * Refusals (EICOS_E_INVALID with a message, nothing changed): rollout_jacobian -- everything eicos_batch_rollout refuses, a NULL J_traj,
 * a matrix map that does not fit the parameter map; rollout_gradient -- no J trajectory on the handle, a parameter, matrix, output or
 * plant map installed since that rollout, both cotangents NULL, a NULL grad_theta0, host and device pointers mixed (as
 * eicos_batch_param_gradient refuses them). */
int eicos_batch_rollout_jacobian(eicos_batch *hd, int steps, const double *theta0, const double *w, double *u_traj, double *theta_traj,
                                 int *exitcodes, int *iters, double *J_traj, double *res_traj);
int eicos_batch_rollout_jacobian_steps(eicos_batch *hd); /* T of the J trajectory the handle holds; 0: none */
int eicos_batch_rollout_gradient(eicos_batch *hd, const double *gu, const double *gtheta, double *grad_theta0, double *grad_w);
int eicos_batch_rollout_gradient_device(eicos_batch *hd, const double *dgu, const double *dgtheta, double *dgrad_theta0, double *dgrad_w);

/* ---- per-instance plant values, and the gradient with respect to the plant's entries (no reference counterpart).  A robustness study
 * runs ONE controller against MANY plants: every instance of the batch simulated against its own true system.  That cannot go through
 * theta (F(phi) [theta | u] is bilinear), so a handle with a plant map may also hold, per instance, values of its own for the map:
 * f0_i [batch][k] in the place of base and / or val_i [batch][nnzF] in the place of val, nnzF = rowptr[k] of the installed map, in its
 * stored CSR order.  The pattern (rowptr, col) stays the shared one.  In every rollout form -- eicos_batch_rollout, _rollout_jacobian,
 * fused or not, _rollout_gradient, and the eicos_multi_* forms -- the plant row of instance i is then formed with exactly the arithmetic
 * stated at eicos_batch_rollout, reading f0_i[i] / val_i[i]:  acc = f0_i[i][j];  acc = acc + (val_i[i][s] * z[col[s]]) in stored order;
 * then + w.  A group that was never given stays the shared one.  The contract is the usual one, bit for bit: the rollout equals the host
 * loop of eicos_batch_update_param_solve with the plant evaluated per instance on the host, rollout_jacobian equals its host twin with
 * the same plant, and rollout_gradient sweeps with val_i of each instance.  A handle without per-instance values takes exactly the code
 * paths and returns exactly the bits it did before.
 * eicos_batch_set_plant_values: rows of instances [first, first + count) from host arrays f0 [count][k] and / or val [count][nnzF]
 * (either NULL = keep that group; synchronous).  The FIRST call of a group allocates its [batch][...] array and fills EVERY instance
 * with the shared values, then overwrites the given range: instances outside every range given so far behave exactly as under the
 * shared map.  _device: the same from device arrays, asynchronous on the handle's stream.  eicos_batch_plant_values reads rows back
 * into host arrays (either NULL = not wanted): the installed rows, and the shared values where none are installed.
 * eicos_batch_has_plant_values: bit 0 f0, bit 1 val.  eicos_batch_clear_plant_values drops both groups (it waits for the handle's
 * stream).  eicos_batch_set_plant_map, whether it installs or removes a map, drops them too: the pattern may have changed.  Setting and
 * clearing values count as a map install for eicos_batch_rollout_gradient, which refuses a Jacobian trajectory recorded before them.
 * eicos_batch_rollout_plant_gradient / _device: eicos_batch_rollout_gradient over the handle's recorded J trajectory -- the same
 * grad_theta0 / grad_w bits, each optional here -- that also returns the gradient of L with respect to the plant's own entries, per
 * instance: grad_f0 [batch][k] and grad_val [batch][nnzF] (each optional; at least one of the four outputs).  u_traj [batch][T][r] and
 * theta_traj [batch][T+1][k] are the arrays that rollout_jacobian returned -- the fallback law's rows included where it fired, because
 * that is what the plant read.  For instance b, every product and sum rounded on its own:
 *
 *     gf0[i] = 0.0, gval[s] = 0.0;  lambda = gtheta[T]
 *     for t = T-1 .. 0:
 *         gf0[i]  = gf0[i]  + lambda[i]                                 (i in [0, k))
 *         gval[s] = gval[s] + (lambda[row(s)] * z_t[col[s]])            (s in stored order; z_t = [theta_traj[b][t] | u_traj[b][t]])
 *         ... the recursion of eicos_batch_rollout_gradient for grad_w[t], v, mu, lambda' ...   (with val_i of instance b where installed)
 *     grad_theta0 = lambda
 *     gf0[i] = gf0[i] + (0.0 * lambda[i]);  gval[s] = gval[s] + (0.0 * lambda[row(s)])
 *
 * A NaN Jacobian row makes all of that instance's rows NaN: one of a step t >= 1 through lambda, one of step 0 -- which the sums never
 * meet -- through the last line, which leaves finite rows as they are.  The call also works with the shared plant; the gradient of a
 * shared entry is the sum of its rows over the batch, which the caller forms.  One thread owns f0 row i and the stored values of row i
 * and accumulates them over t in the stated order, so the bits do not depend on the launch.
 * Refusals (EICOS_E_INVALID with the cause named, nothing changed): no plant map; an instance range out of bounds; both groups NULL; host
 * and device pointers mixed or handed to the wrong form (as eicos_batch_param_gradient refuses them); for the gradient call everything
 * eicos_batch_rollout_gradient refuses except a NULL grad_theta0, a NULL u_traj or theta_traj, and all four outputs NULL.
 * Out of scope: per-instance patterns, an indexed form, per-instance parameter / output / fallback maps. */
int eicos_batch_set_plant_values(eicos_batch *hd, int first, int count, const double *f0 /* [count][k], optional */,
                                 const double *val /* [count][nnzF], optional */);
int eicos_batch_set_plant_values_device(eicos_batch *hd, int first, int count, const double *df0, const double *dval);
int eicos_batch_plant_values(eicos_batch *hd, int first, int count, double *f0_out, double *val_out);
int eicos_batch_has_plant_values(eicos_batch *hd); /* bit 0: f0, bit 1: val */
int eicos_batch_clear_plant_values(eicos_batch *hd);
int eicos_batch_rollout_plant_gradient(eicos_batch *hd, const double *gu, const double *gtheta, const double *u_traj /* [batch][T][r] */,
                                       const double *theta_traj /* [batch][T+1][k] */, double *grad_theta0 /* optional */,
                                       double *grad_w /* optional */, double *grad_f0 /* [batch][k], optional */,
                                       double *grad_val /* [batch][nnzF], optional */);
int eicos_batch_rollout_plant_gradient_device(eicos_batch *hd, const double *dgu, const double *dgtheta, const double *du_traj,
                                              const double *dtheta_traj, double *dgrad_theta0, double *dgrad_w, double *dgrad_f0,
                                              double *dgrad_val);
/* The gradient of a closed-loop cost with respect to the CONTROLLER's own data: the data vectors c, h, b, the stored
 * values of G and A, the slopes of the parameter map and the output map.
 *
 * Recording (off by default).  eicos_batch_set_rollout_recording(hd, 1): from then on eicos_batch_rollout_jacobian also leaves, in
 * device memory owned by the handle, for every instance and step
 *     Wc [batch][T][r][n], Wh [batch][T][r][m], Wb [batch][T][r][p]   the rows grad_c, grad_h, grad_b of u_a = (row a of U)' x: the bits
 *         eicos_batch_adjoint returns at that step for g = the dense rows of the output map (entries of a column summed in stored order);
 *     x_rec [batch][T][n], y_rec [batch][T][p], z_rec [batch][T][m]    the un-equilibrated result the step's u row was formed from (the
 *         final attempt under a retry policy).
 * A step whose fallback law fired records 0.0 in its W rows (its u does not depend on the controller's data) and still records x, y, z;
 * a step that did not end OPTIMAL / OPTIMAL_INACC records NaN W rows, as J does.  u, theta, codes, iters, J, res and the handle's state
 * afterwards are bit-identical with recording on and off; with recording off every call keeps its code path and its allocations.  The
 * record takes batch * T * (r + 1) * (n + m + p) * 8 bytes (MPC02 at batch 1024, r = 4, T = 20: about 4.9 GB), and one step more of
 * it (T + 1 in the place of T) where the rollout is not fused; an allocation that fails is refused with EICOS_E_HIP and a message
 * naming the size, and the handle is left without a trajectory.  The handle keeps the record until recording is switched off:
 * eicos_batch_set_rollout_recording(hd, 0) waits for the handle's stream and frees it (and the staging of the data-gradient call); the J
 * trajectory stays, eicos_batch_rollout_records and eicos_batch_rollout_data_gradient then refuse ("no recorded rows").
 * eicos_batch_rollout_recording: 1 / 0.  eicos_batch_rollout_records copies whichever arrays are wanted to the host (any NULL).
 *
 * eicos_batch_rollout_data_gradient / _device: a second backward sweep over the recorded rollout, for the cost of
 * eicos_batch_rollout_gradient, L = sum_t gu_t' u_t + sum_t gtheta_t' theta_t; theta_traj [batch][T+1][k] is the array rollout_jacobian
 * returned.  Outputs: the non-NULL members of *out, one row per instance (for data shared by the batch the caller sums the rows):
 *     grad_c [batch][n], grad_h [batch][m], grad_b [batch][p]   a perturbation of the data vector applied at every step (= the base
 *                                                              vectors of the parameter map)
 *     grad_G [batch][nnzG], grad_A [batch][nnzA]                the same for the stored values, CSC order of Gpr / Apr (= the base values
 *                                                              under a matrix map)
 *     grad_Cval, grad_Hval, grad_Bval [batch][nnz of the group] the slopes of the parameter map, stored CSR order
 *     grad_u0 [batch][r], grad_Uval [batch][nnzU]               the output map
 * For instance b, with mu_t of eicos_batch_rollout_gradient's recursion (the same bits; per-instance plant values where installed) and
 * every product and sum rounded on its own, for t = T-1 .. 0:
 *     d_c[i] = 0.0, then d_c[i] + (mu_t[a] * Wc_t[a][i]) for a ascending; likewise d_h, d_b
 *     grad_c[i] = grad_c[i] + d_c[i]; likewise h, b
 *     grad_Cval[s] = grad_Cval[s] + (d_c[i] * theta_t[col[s]])          (s over row i in stored order; likewise Hval, Bval)
 *     grad_G[e] = grad_G[e] + ((d_c[j] * z_t[i]) - (d_h[i] * x_t[j]))   (e = (i, j)); grad_A with y_t, d_b in the place of z_t, d_h
 *     grad_u0[a] = grad_u0[a] + mu_t[a];  grad_Uval[s] = grad_Uval[s] + (mu_t[row(s)] * x_t[col[s]])
 * One thread owns every output entry, so the bits do not depend on the launch.  A step with NaN rows makes grad_c, grad_h, grad_b, grad_G,
 * grad_A and the slopes of that instance NaN and leaves other instances as they are.  The output-map gradients count every step,
 * also one whose fallback fired.
 * Refusals (EICOS_E_INVALID with a message, nothing changed): everything eicos_batch_rollout_gradient refuses; no recorded rows on the
 * handle (recording was off for the rollout it holds); a NULL theta_traj or out; a slope output of a group without a map; all outputs
 * NULL; host and device pointers mixed or handed to the wrong form.
 * Out of scope: the matrix map's slopes, the fallback law's V, the shift map, subset rollouts, a reduction over the batch on the GPU. */
typedef struct eicos_data_gradient {
    double *grad_c, *grad_h, *grad_b;
    double *grad_G, *grad_A;
    double *grad_Cval, *grad_Hval, *grad_Bval;
    double *grad_u0, *grad_Uval;
} eicos_data_gradient;
size_t eicos_data_gradient_size(void); /* sizeof(eicos_data_gradient), for bindings that mirror the struct */
int eicos_batch_set_rollout_recording(eicos_batch *hd, int on);
int eicos_batch_rollout_recording(eicos_batch *hd);
int eicos_batch_rollout_records(eicos_batch *hd, double *Wc, double *Wh, double *Wb, double *x_rec, double *y_rec, double *z_rec);
int eicos_batch_rollout_data_gradient(eicos_batch *hd, const double *gu, const double *gtheta, const double *theta_traj,
                                      const eicos_data_gradient *out);
int eicos_batch_rollout_data_gradient_device(eicos_batch *hd, const double *dgu, const double *dgtheta, const double *dtheta_traj,
                                             const eicos_data_gradient *dout);
/* eicos_batch_update_param_solve_subset: the closed-loop step over a subset = eicos_batch_update_param_indexed + eicos_batch_solve_subset
 * + eicos_batch_outputs_indexed (+ the x rows), every array in list order; synchronous.
 * Fused under exactly the conditions of eicos_batch_update_param_solve (an LDS vector, a theta row that fits it, GPU-addressable theta,
 * EICOS_FUSED_UPDATE not 0; witness: eicos_batch_last_update_path == 5): ONE subset launch in which each workgroup expands row q of
 * theta for the instance idx[q] it is about to solve (a full updateData from theta under a matrix map) and writes row q of u_out / x_out
 * when it is done, if that array is pinned or device memory -- 8 k bytes in and 8 r bytes out per CHOSEN instance.  The selection kernel
 * in front of the launch leaves a row map (id -> position in the list) next to the launch order; slab addresses still come from the id.
 * Otherwise the three calls run; a pageable or unwritten u_out / x_out is filled through the indexed output kernel and the row gather.
 * Contract: for every instance in the list, the state and the returned rows equal, bit for bit, those of a twin that ran the three
 * calls -- cold, warm, under a shift map, under a matrix map, with shared matrix values (kept without a matrix map, dropped with one).
 * Every instance outside the list keeps everything the host can read, info and solve_us included.  With idx = 0 .. batch-1 the call
 * equals eicos_batch_update_param_solve.  An empty list is EICOS_OK with no launch.  Refusals: the list check, those of
 * eicos_batch_update_param (no parameter map, NULL theta, a matrix map that no longer fits), u_out without an output map. */
int eicos_batch_update_param_solve_subset(eicos_batch *hd, const int *idx, int count, const double *theta /* [count][k] */,
                                          double *u_out /* [count][r], optional */, double *x_out /* [count][n], optional */,
                                          int *exitcodes /* [count], optional */);

/* ---- results: replaces solution() (reference include/eicos.hpp:160) / getInfo() (:163).
 * x: [batch][n] host.  y,z,s are extras the reference keeps private; any may be NULL.  A pinned destination receives one strided
 * device-to-host copy; a pageable one is filled through the pinned bounce buffers (copy of chunk k + 1 in flight while chunk k is copied out). */
int eicos_batch_solution(eicos_batch *hd, double *x);
int eicos_batch_duals(eicos_batch *hd, double *y, double *z, double *s);
int eicos_batch_info(eicos_batch *hd, eicos_info *info /* [batch] */);
/* Device-resident results (no copy): pointer to instance 0's x and the stride in doubles. */
int eicos_batch_solution_device(eicos_batch *hd, const double **dx, size_t *stride_doubles);

/* ---- warm start (N3 of SURVEY.md 8f; NOT in the reference, whose solve() always cold-starts, src/eicos.cpp:855-984).
 * shift > 0: a solve of an instance whose previous solve ended OPTIMAL skips the two initialisation solves and starts
 * from that solution -- re-equilibrated, with s and z pushed into the cone (LP rows floored at shift * mean|.|, cone
 * heads at ||tail|| + the same margin), tau = kap = 1.  shift = 0 (default) restores the reference behaviour.
 * 0.1 is a good value for MPC re-solves (1 % data perturbation: 13-15 -> 8-10 iterations). */
int eicos_batch_set_warm_start(eicos_batch *hd, double shift);

/* ---- a caller-supplied starting point (no reference counterpart).  The warm start above can only reuse what the previous solve of the
 * same instance left in its slab; eicos_batch_set_iterate writes a starting point there instead -- from another handle, a coarser model, a
 * neighbouring instance, a run saved to disk.  Rows of x [count][n], y [count][p], z [count][m], s [count][m], row-major, for instances
 * [first, first + count), in the units of eicos_batch_solution / eicos_batch_duals (backscaled); NULL keeps a group as it is, all four NULL
 * is EICOS_E_INVALID.  The rows are stored in the instances' slabs as they are, and every instance of the range is marked warm-startable
 * by the rule the solve kernel reads: its info record gets exitcode = EICOS_OPTIMAL unless it is EICOS_OPTIMAL or EICOS_OPTIMAL +
 * EICOS_INACC_OFFSET already, and n_factor = 1 if it was 0; nothing else of the record changes.  eicos_batch_solution, _duals and _info
 * return exactly that afterwards.
 * With warm start shift > 0 the next solve of such an instance starts from the supplied point through the unchanged warm path
 * (re-equilibrated, s and z pushed into the cone: they need not lie in it).  With shift == 0 the point is ignored: the next solve runs
 * cold and overwrites it.  Values are not checked for finiteness, as elsewhere.
 * Host form: the paths of eicos_batch_update_rhs -- pageable arrays through the pinned bounce buffers, pinned / registered arrays read in
 * place -- synchronous in the same way, eicos_batch_last_update_path reports the path.  Device form: one launch on the handle's stream,
 * asynchronous.  Both run one row-parallel kernel with plain stores.
 * EICOS_E_INVALID, with a message naming the fault: NULL handle, a range outside the batch, y with p = 0, z or s with m = 0. */
int eicos_batch_set_iterate(eicos_batch *hd, int first, int count, const double *x /* [count][n] */, const double *y /* [count][p] */,
                            const double *z /* [count][m] */, const double *s /* [count][m] */);
int eicos_batch_set_iterate_device(eicos_batch *hd, int first, int count, const double *dx, const double *dy, const double *dz, const double *ds);

/* ---- shift map: the warm start moved by an affine map, inside the solve kernel (no reference counterpart).  The standard warm start of
 * a receding-horizon controller is the previous solution moved one stage forward: stage t + 1 becomes stage t, the last stage is
 * repeated.  A handle holds one such map: per vector x, y, z, s an eicos_affine_map with rows = n, p, m, m -- base[rows] and a SQUARE CSR
 * matrix rows x rows (rowptr[rows + 1], col / val[rowptr[rows]]; columns lie in [0, rows)).  A NULL group is not shifted.
 * eicos_batch_set_shift_map COPIES the host arrays into one device allocation of its own; a later call replaces the map, all four NULL
 * removes it.  eicos_batch_has_shift_map: bit 0 = x, 1 = y, 2 = z, 3 = s mapped; 0 = none.
 * When a solve of the handle WARM-STARTS an instance (warm start shift > 0, and the instance's last exit code is EICOS_OPTIMAL or
 * EICOS_OPTIMAL + EICOS_INACC_OFFSET), the workgroup first replaces that instance's vectors -- for every mapped group v and row j
 *     new[j] = base[j];  for t in rowptr[j] .. rowptr[j+1]-1, in stored order:  new[j] = new[j] + (val[t] * old[col[t]])
 * with the product and the sum EACH rounded to fp64 (no fused multiply-add), old = the group's vector before the shift (the backscaled
 * values eicos_batch_solution / _duals return) -- and the warm start's re-equilibration and cone push follow: a shifted s or z that leaves
 * the cone is pushed back by construction.  A solve that does not warm-start an instance (shift == 0, or a previous exit that is neither
 * OPTIMAL nor close to it) leaves its vectors alone and runs cold, as without a map.
 * There is no new update call: the shift is part of the per-instance prologue of the solve kernel, so eicos_batch_solve, _solve_async,
 * _update_solve, _update_rhs_solve, _update_param_solve and every step of eicos_batch_rollout (fused or per step) pick it up, on every
 * build of the solve kernel and on handles without an LDS vector.  Without a shift map a launch pays one pointer test per instance and
 * every result stays bit-identical.
 * Contract: on a handle with a shift map and warm start shift > 0, any solve leaves the same state -- instance slabs, solution, duals,
 * info, the KKT values of eicos_debug_kkt -- bit for bit, as a twin WITHOUT the map on which the host runs, before the same solve:
 *     1. eicos_batch_solution / _duals / _info, for every instance whose last solve ended with exit code 0 or 10;
 *     2. the map evaluated on those vectors in the order above;
 *     3. eicos_batch_set_iterate with the result.
 * For eicos_batch_rollout the twin is the host loop of eicos_batch_update_param_solve calls with the plant evaluated on the host, and
 * steps 1-3 before each of them.
 * EICOS_E_INVALID, with a message naming the fault, for rowptr[0] != 0, decreasing row pointers, a column outside [0, rows) and a map for
 * a vector the pattern does not have (y with p = 0, z or s with m = 0). */
int eicos_batch_set_shift_map(eicos_batch *hd, const eicos_affine_map *x, const eicos_affine_map *y, const eicos_affine_map *z,
                              const eicos_affine_map *s);
int eicos_batch_has_shift_map(eicos_batch *hd); /* bit 0 x, 1 y, 2 z, 3 s; 0 = none */

/* ---- dynamic regularisation (N4 of SURVEY.md 8f; NOT in the reference, whose Settings::delta / ::eps are dead,
 * include/eicos.hpp:26,28).  delta > 0: during the numeric LDL' a pivot whose sign disagrees with the quasi-definite
 * sign pattern of the KKT matrix, or whose magnitude is below eps, is replaced by sign * delta (ECOS: delta = 2e-7,
 * eps = 1e-13).  delta = 0 (default): static regularisation only, an exactly zero pivot ends the solve with
 * EICOS_FATAL as in the reference (src/eicos.cpp:1166-1170). */
int eicos_batch_set_dynamic_regularization(eicos_batch *hd, double delta, double eps);

/* ---- runtime solver settings: the fields of struct EiCOS::Settings (reference include/eicos.hpp:23-47) a caller tunes per application --
 * the exit tolerances and their relaxed ("inaccurate") counterparts, the iteration cap, and the iterative refinement of the KKT solves.
 * Defaults = the reference's values (right column).  Where the solve kernel reads them (reference src/eicos.cpp):
 *   feastol, abstol, reltol (+ _inacc)  checkExitConditions (:533-546); reltol also decides whether the infeasibility residuals pinfres /
 *                                       dinfres exist (:720, :724)
 *   iter_max                            the pass at which the main loop gives up (:990): EICOS_MAXIT, or EICOS_OPTIMAL / _PINF / _DINF +
 *                                       EICOS_INACC_OFFSET when the relaxed test passes there
 *   linsysacc, irerrfact, nitref        the stop test of the iterative refinement of every KKT solve (:1479, :1495, :1588-1590):
 *                                       nitref = 0 means no refinement step at all
 * Ranges: the eight doubles finite and > 0; iter_max in [1, 100] (the per-pass trace rows -- eicos_debug_trace's out[102][12] -- are sized
 * for 100 passes, and only pass 0 creates the best iterate that the iteration-cap exit may restore); nitref in [0, 100] (nothing in the
 * KKT solve is sized by it; 100 merely bounds the loop).
 * Scope: exactly these ten.  gamma, deltastat, stepmin / stepmax, sigmamin / sigmamax, safeguard and equil_iters stay compile-time
 * constants of the kernel: they shape the arithmetic of every pass, and delta / eps have eicos_batch_set_dynamic_regularization.
 * A handle starts with the defaults.  eicos_batch_set_settings stores a COPY and takes effect from the next solve launch the handle
 * enqueues -- eicos_batch_solve, _solve_async, _update_solve, _update_rhs_solve, _update_param_solve and every step of eicos_batch_rollout,
 * fused or per step, on every build of the solve kernel and on handles without an LDS vector.  A launch already in flight keeps the values
 * it was enqueued with: they travel as kernel arguments by value.  Settings are per handle, not per instance.
 * A handle on which eicos_batch_set_settings was never called, or was called with eicos_settings_default's values, gives bit-identical
 * results on every path.
 * EICOS_E_INVALID, with a message naming the field, and the handle's settings UNCHANGED, for a NULL handle or struct, a non-finite or
 * non-positive tolerance / linsysacc / irerrfact, iter_max outside [1, 100] and nitref outside [0, 100]. */
typedef struct eicos_settings {
    double feastol, abstol, reltol;                    /* 1e-8, 1e-8, 1e-8  */
    double feastol_inacc, abstol_inacc, reltol_inacc;  /* 1e-4, 5e-5, 5e-5  */
    double linsysacc, irerrfact;                       /* 1e-14, 6          */
    int iter_max, nitref;                              /* 100, 9            */
} eicos_settings;
void   eicos_settings_default(eicos_settings *out);   /* no handle, no GPU needed */
size_t eicos_settings_size(void);                     /* sizeof(eicos_settings), for bindings that mirror the struct */
int eicos_batch_set_settings(eicos_batch *hd, const eicos_settings *s);
int eicos_batch_get_settings(eicos_batch *hd, eicos_settings *out);

/* ---- retry policy: a second attempt INSIDE the solve launch (no reference counterpart).  The solve kernel is a persistent workgroup per
 * instance; with a policy installed, a workgroup whose instance ends in an exit class of `mask` (EICOS_SEL_*, above) solves the same
 * instance once more, under the policy's own settings, before anything reads the result: the x row and the output row of a fused step,
 * the records and the plant map of a rollout step, the pull of the workgroup's next instance.  At most ONE extra attempt; no second
 * launch, no selection kernel, no barrier across the batch -- and it works between the steps of a one-launch eicos_batch_rollout, where
 * no host retry can.  It applies to every solve launch of the handle: eicos_batch_solve(_async), _solve_subset, _solve_where,
 * _update_solve, _update_rhs_solve, _update_param_solve and its subset form, and every step of eicos_batch_rollout, fused or per step,
 * on every build of the solve kernel and on handles without an LDS vector.
 * Contract: let a launch cover the instance set S (the batch, or a list).  Every instance ends bit-identical -- x, y, z, s, every info
 * field except solve_us, eicos_debug_kkt, the u rows, the rollout records -- to this host sequence: (1) the same launch without the policy;
 * (2) ids = the instances of S whose class is in mask; (3) eicos_batch_set_settings(settings), _set_warm_start(warm),
 * _set_dynamic_regularization(dyn_delta, dyn_eps); (4) eicos_batch_solve_subset(ids); (5) the three settings restored -- with the outputs,
 * the x rows and the plant map of a fused step taken after (5): per rollout step update from theta -> solve -> retry -> outputs -> plant.
 * The fused update of an instance runs once, before the first attempt.  An instance outside the mask is untouched by the policy, and a
 * handle without one behaves exactly as before.  Exit codes, the codes / iters of a rollout, eicos_batch_gather and _select see the
 * final attempt.
 * The second attempt is an ordinary solve of the instance: COLD by default (warm = 0).  With warm > 0 it warm-starts only if the record
 * the first attempt left allows it (EICOS_OPTIMAL or EICOS_OPTIMAL + EICOS_INACC_OFFSET; a MAXIT or NUMERICS record starts cold whatever
 * warm says), and a shift map (eicos_batch_set_shift_map) is then applied AGAIN, to the first attempt's result.
 * eicos_batch_set_retry stores a copy; NULL or mask 0 removes the policy.  The record lives in device memory and is rewritten on the
 * handle's stream, so a launch already enqueued keeps the policy it was enqueued with.  eicos_batch_retry_counts: retries[i] = second
 * attempts instance first + i has run since its counter was last reset (cumulative: after a rollout, its retried steps); reset != 0
 * zeroes the counters of the range after reading them.  Waits for the handle's stream.
 * EICOS_E_INVALID, with a message naming the cause, and the policy UNCHANGED: a NULL handle (before any GPU call); mask bits above bit
 * 11; a mask that is EICOS_SEL_UNSOLVED alone (an attempted instance is never in that class, so the policy could never act; beside
 * other classes the bit is idle and accepted -- EICOS_SEL_NOT_OPTIMAL holds it); warm, dyn_delta or dyn_eps negative or NaN; any
 * settings value eicos_batch_set_settings refuses (same check, the field named); a range outside [0, batch) or NULL retries. */
typedef struct eicos_retry {
    unsigned mask;             /* OR of EICOS_SEL_*: classes of the first attempt that trigger the second; 0 = no policy */
    double warm;               /* warm-start shift of the second attempt (0 = cold, the default) */
    double dyn_delta, dyn_eps; /* dynamic regularisation of the second attempt (0, 0 = off) */
    eicos_settings settings;   /* runtime settings of the second attempt */
} eicos_retry;
void   eicos_retry_default(eicos_retry *out);   /* mask 0, warm 0, dyn 0 / 0, default settings; no handle, no GPU needed */
size_t eicos_retry_size(void);                  /* sizeof(eicos_retry), for bindings that mirror the struct */
int eicos_batch_set_retry(eicos_batch *hd, const eicos_retry *r);
int eicos_batch_get_retry(eicos_batch *hd, eicos_retry *out);
int eicos_batch_retry_counts(eicos_batch *hd, int first, int count, int *retries /* host [count] */, int reset);

/* ---- plumbing */
int eicos_batch_dims(eicos_batch *hd, eicos_dims *out);
/* Which compilation of the solve kernel this handle launches (chosen at creation from pattern size and batch; no reference
 * counterpart): 0 = default build, 1 = LDS-resident build for small patterns (eicos_dims.lds_resident), 2 = the 256-thread kernel
 * compiled for two waves per SIMD (launches of at most two workgroups per CU), 3 = the 256- / 512-thread kernel with the factor operand
 * array resident in LDS (launches of one workgroup per CU whose factor fits the idle LDS).  Negative: error code. */
int eicos_batch_kernel_build(eicos_batch *hd);
/* Shared matrix values (no reference counterpart; transparent: results are bit-identical with it on and off).  Many batches are one plant
 * with many states or scenarios: every instance gets the same Gpr and Apr and only c, h, b differ.  Equilibration reads A and G only, so
 * every instance then holds the same bits in the value copies its matrix-vector products stream, and the solve kernel reads ONE copy --
 * instance 0's, resident in L2 -- instead of one per instance from HBM.  The handle finds this out by itself:
 *   sets it    eicos_batch_update_device over the whole batch (first = 0, count = batch) with Gpr and Apr both given (a pattern without A: Gpr):
 *              its kernel compares every row with row 0 bit for bit (-0.0 differs from +0.0, a NaN equals only the same NaN) and the
 *              values are shared when no row differs;
 *   keeps it   everything that leaves matrix values alone: eicos_batch_update_rhs*, _update_param* without a matrix map, _update_rhs_solve,
 *              _update_param_solve and eicos_batch_rollout without a matrix map, warm start, starting points, settings, solves;
 *   drops it   every other updateData: host-pointer and other-GPU forms, sub-ranges, calls that keep Gpr or Apr, eicos_batch_update_solve,
 *              and the parametric forms and rollouts under a matrix map.
 * eicos_batch_shared_values: 1 when the next solve will read shared values, else 0; waits for the handle's stream.  Always 0 on the
 * LDS-resident build (eicos_batch_kernel_build = 1), whose values are in LDS anyway.  Negative: error code. */
int eicos_batch_shared_values(eicos_batch *hd);
/* Use a caller-owned HIP stream (hipStream_t passed as void*); NULL restores the own stream. */
int eicos_batch_set_stream(eicos_batch *hd, void *hip_stream);
/* HIP-event timing of the most recent solve / update kernels on the handle's stream (ms). */
int eicos_batch_last_solve_ms(eicos_batch *hd, float *ms);
int eicos_batch_last_update_ms(eicos_batch *hd, float *ms);
/* ... and of the kernel of the most recent eicos_batch_adjoint / _adjoint_data / _output_jacobian / _param_jacobian / _param_gradient call (ms) */
int eicos_batch_last_adjoint_ms(eicos_batch *hd, float *ms);
/* The durations (ms) of the most recent launches, oldest first: which = 0 the solve launches, 1 the updateData calls, 2 the span of a
 * whole step (start of the updateData call that preceded a solve launch -> end of that solve; meaningful when the two alternate).  The handle keeps a
 * ring of 64 event pairs, so a caller that enqueues K steps back to back (update + solve_async, no host synchronisation in between) can
 * read every launch's duration afterwards.  Returns the number written (<= cap, <= 64) or a negative error; waits for the most recent
 * launch to finish.  No reference counterpart (measurement only). */
int eicos_batch_ms_history(eicos_batch *hd, int which, float *ms, int cap);
/* replaces the Solver destructor / ECOS_cleanup (reference test/ecos.h:31-34) */
int eicos_batch_destroy(eicos_batch *hd);

/* ---- single-instance surface: the same entry points for one problem, i.e. exactly what
 * class EiCOS::Solver needs.  A handle made by eicos_create is a batch of one; every eicos_batch_* call works on it.
 *   eicos_create   <-> Solver::Solver(n,m,p,l,ncones,q,Gpr,Gjc,Gir,Apr,Ajc,Air,c,h,b)  include/eicos.hpp:151-154
 *                      / ECOS_setup (reference test/ecos.h:11-24); values are copied, NULL groups allowed
 *   eicos_update   <-> Solver::updateData(Gpr,Apr,c,h,b)  include/eicos.hpp:155-156 / ECOS_updateData test/ecos.h:28-29
 *   eicos_solve    <-> exitcode Solver::solve()  include/eicos.hpp:158 / ECOS_solve test/ecos.h:26; returns the
 *                      exit code through *exitcode (the function's own return value is the EICOS_E_* status)
 *   eicos_solution <-> Solver::solution()  include/eicos.hpp:160 (x[n], host)
 *   eicos_info_get <-> Solver::getInfo()   include/eicos.hpp:163
 *   eicos_destroy  <-> ~Solver / ECOS_cleanup test/ecos.h:31-34 */
int eicos_create(int n, int m, int p, int l, int ncones, const int *q,
                 const double *Gpr, const int *Gjc, const int *Gir,
                 const double *Apr, const int *Ajc, const int *Air,
                 const double *c, const double *h, const double *b, int device, eicos_batch **out);
int eicos_update(eicos_batch *hd, const double *Gpr, const double *Apr, const double *c, const double *h, const double *b);
int eicos_solve(eicos_batch *hd, int *exitcode);
int eicos_solution(eicos_batch *hd, double *x);
int eicos_info_get(eicos_batch *hd, eicos_info *info);
int eicos_destroy(eicos_batch *hd);

/* ---- multi-GPU (SURVEY.md 8b "eicos_batch_create(pattern, B, device_ids...)", 8e): ONE pattern, `batch` instances in contiguous
 * shards over the listed devices -- shard s = instances [s*base + min(s, rem), ...) with base = batch / ndev, rem = batch % ndev, the
 * first `rem` shards one instance longer.  Host C++ above the single-GPU entry points: one eicos_batch handle and one HIP stream per
 * list entry, no collective on the data path (instances are independent), no torch / RCCL dependency.  The reference has no
 * counterpart (EiCOS::Solver solves one problem on one core, include/eicos.hpp:137-163); every call mirrors its eicos_batch_*
 * namesake over the whole batch, arrays [batch][...] row-major in GLOBAL instance order.  A device may be listed several times: its
 * shards then run concurrently on separate streams of that GPU.  Errors: eicos_multi_last_error() (names the failing shard). */
typedef struct eicos_multi eicos_multi; /* opaque */
int eicos_multi_create(int n, int m, int p, int l, int ncones, const int *q,
                       const int *Gjc, const int *Gir, const int *Ajc, const int *Air,
                       int batch, const int *device_ids, int ndev, eicos_multi **out);
/* updateData from HOST arrays: every shard moves its rows over its own GPU's PCIe link (eicos_batch_update's pinned bounce pipeline), all
 * shards in parallel -- one persistent host thread per shard, started by eicos_multi_create */
int eicos_multi_update(eicos_multi *mh, int first, int count, const double *Gpr, const double *Apr,
                       const double *c, const double *h, const double *b);
/* updateData + solve in one synchronous call (eicos_batch_update_solve on every shard, concurrently; whole batch; x_out / exitcodes optional) */
int eicos_multi_update_solve(eicos_multi *mh, const double *Gpr, const double *Apr, const double *c, const double *h, const double *b,
                             double *x_out, int *exitcodes);
/* updateData from arrays resident in the HBM of ONE GPU (src_device): shards on that GPU read them in place; the others read their rows
 * in place as well, over xGMI (peer access is enabled between the listed devices at creation), or -- without peer access -- pull them with
 * staged hipMemcpyPeerAsync copies on their own streams: the "batch scatter" of north_star without a collective.
 * ASYNCHRONOUS, like eicos_batch_update_device: the call returns with the updateData kernels enqueued on the shards' streams, and those
 * kernels read the source buffers IN PLACE (on src_device itself and, with peer access, from the other GPUs).  The source buffers must stay
 * valid and unmodified until eicos_multi_sync (or a solve / result call, which synchronise) has returned; work that PRODUCES them on
 * src_device must have completed before the call (the shards' streams are not ordered against the producer's stream). */
int eicos_multi_update_device(eicos_multi *mh, int src_device, int first, int count, const double *dGpr, const double *dApr,
                              const double *dc, const double *dh, const double *db);
/* right-hand-side-only updateData (eicos_batch_update_rhs / _device / _solve on every shard, in global instance order): from host arrays,
 * from arrays in the HBM of ONE GPU (src_device; asynchronous, with the source-buffer rules of eicos_multi_update_device), and fused with
 * the solve of the whole batch (x_out / exitcodes optional) */
int eicos_multi_update_rhs(eicos_multi *mh, int first, int count, const double *c, const double *h, const double *b);
int eicos_multi_update_rhs_device(eicos_multi *mh, int src_device, int first, int count, const double *dc, const double *dh, const double *db);
int eicos_multi_update_rhs_solve(eicos_multi *mh, const double *c, const double *h, const double *b, double *x_out, int *exitcodes);
/* parametric right-hand sides (eicos_batch_set_param_map / _update_param / _update_param_device on every shard): the map is installed on
 * every shard, theta rows [count][k] are in global instance order; src_device as for eicos_multi_update_rhs_device */
int eicos_multi_set_param_map(eicos_multi *mh, int k, const eicos_affine_map *c, const eicos_affine_map *h, const eicos_affine_map *b);
int eicos_multi_param_count(eicos_multi *mh);
int eicos_multi_update_param(eicos_multi *mh, int first, int count, const double *theta);
int eicos_multi_update_param_device(eicos_multi *mh, int src_device, int first, int count, const double *dtheta);
/* output map and the closed-loop step (eicos_batch_set_output_map / _output_count / _outputs / _update_param_solve on every shard): the map
 * is installed on every shard; theta, u, u_out and x_out are in global instance order, every shard takes its rows, the shards of
 * eicos_multi_update_param_solve run concurrently */
int eicos_multi_set_output_map(eicos_multi *mh, int r, const eicos_affine_map *u);
int eicos_multi_output_count(eicos_multi *mh);
int eicos_multi_outputs(eicos_multi *mh, int first, int count, double *u);
int eicos_multi_update_param_solve(eicos_multi *mh, const double *theta, double *u_out, double *x_out, int *exitcodes);
/* plant map and rollout (eicos_batch_set_plant_map / _has_plant_map / _rollout on every shard): the map is installed on every shard; the
 * arrays are in global instance order ([batch][steps][...]: every shard's rows are contiguous), the shards run concurrently */
int eicos_multi_set_plant_map(eicos_multi *mh, const eicos_affine_map *f);
int eicos_multi_has_plant_map(eicos_multi *mh);
int eicos_multi_rollout(eicos_multi *mh, int steps, const double *theta0, const double *w, double *u_traj, double *theta_traj,
                        int *exitcodes, int *iters);
/* eicos_batch_rollout_jacobian / _gradient per shard on its rows, the shards concurrently (T of the gradient = the step count of the
 * rollout_jacobian every shard ran last) */
int eicos_multi_rollout_jacobian(eicos_multi *mh, int steps, const double *theta0, const double *w, double *u_traj, double *theta_traj,
                                 int *exitcodes, int *iters, double *J_traj, double *res_traj);
int eicos_multi_rollout_gradient(eicos_multi *mh, const double *gu, const double *gtheta, double *grad_theta0, double *grad_w);
/* per-instance plant values (eicos_batch_set_plant_values / _plant_values / _has_plant_values / _clear_plant_values): rows by global
 * instance id, every shard takes the part of the range it owns; eicos_multi_rollout_plant_gradient: rows by shard, as
 * eicos_multi_rollout_gradient's */
int eicos_multi_set_plant_values(eicos_multi *mh, int first, int count, const double *f0, const double *val);
int eicos_multi_plant_values(eicos_multi *mh, int first, int count, double *f0_out, double *val_out);
int eicos_multi_has_plant_values(eicos_multi *mh);
int eicos_multi_clear_plant_values(eicos_multi *mh);
int eicos_multi_rollout_plant_gradient(eicos_multi *mh, const double *gu, const double *gtheta, const double *u_traj, const double *theta_traj,
                                       double *grad_theta0, double *grad_w, double *grad_f0, double *grad_val);
/* recording and the data gradient (eicos_batch_set_rollout_recording / _rollout_recording / _rollout_records / _rollout_data_gradient):
 * recording is switched on every shard; records and gradients are rows by shard, as eicos_multi_rollout_plant_gradient's */
int eicos_multi_set_rollout_recording(eicos_multi *mh, int on);
int eicos_multi_rollout_recording(eicos_multi *mh);
int eicos_multi_rollout_records(eicos_multi *mh, double *Wc, double *Wh, double *Wb, double *x_rec, double *y_rec, double *z_rec);
int eicos_multi_rollout_data_gradient(eicos_multi *mh, const double *gu, const double *gtheta, const double *theta_traj,
                                      const eicos_data_gradient *out);
/* matrix map (eicos_batch_set_matrix_map / _has_matrix_map on every shard): installed on every shard; the theta-consuming calls above pick
 * it up shard by shard */
int eicos_multi_set_matrix_map(eicos_multi *mh, const eicos_affine_map *G, const eicos_affine_map *A);
int eicos_multi_has_matrix_map(eicos_multi *mh);
int eicos_multi_matrix_map_count(eicos_multi *mh);
/* starting point and shift map (eicos_batch_set_iterate / _set_shift_map / _has_shift_map): the rows of set_iterate are in global
 * instance order and every shard takes its own; the shift map is installed on every shard */
int eicos_multi_set_iterate(eicos_multi *mh, int first, int count, const double *x, const double *y, const double *z, const double *s);
int eicos_multi_set_shift_map(eicos_multi *mh, const eicos_affine_map *x, const eicos_affine_map *y, const eicos_affine_map *z,
                              const eicos_affine_map *s);
int eicos_multi_has_shift_map(eicos_multi *mh);
/* solve: async = enqueue every shard's kernels on its stream and return; sync waits for all; eicos_multi_solve = both (+ exit codes, may be NULL) */
int eicos_multi_solve_async(eicos_multi *mh);
int eicos_multi_sync(eicos_multi *mh);
int eicos_multi_solve(eicos_multi *mh, int *exitcodes);
/* subset solves (eicos_batch_select / _solve_subset(_async) / _solve_where / _gather): indices are GLOBAL instance ids.  A list is checked
 * as a whole first -- a refused list changes no shard --, then split by shard, every id reduced by the shard's first instance; shards with
 * an empty share are skipped, the others run concurrently.  Ids, exit codes and rows come back in global order (select, solve_where:
 * ascending) or in list order (solve_subset, gather). */
int eicos_multi_select(eicos_multi *mh, unsigned mask, int *idx_out, int *count_out);
int eicos_multi_solve_subset_async(eicos_multi *mh, const int *idx, int count);
int eicos_multi_solve_subset(eicos_multi *mh, const int *idx, int count, int *exitcodes);
int eicos_multi_solve_where(eicos_multi *mh, unsigned mask, int *idx_out, int *count_out, int *exitcodes);
int eicos_multi_gather(eicos_multi *mh, const int *idx, int count, double *x, double *y, double *z, double *s, eicos_info *info);
/* index-list updates, output rows and the closed-loop step over a subset (eicos_batch_*_indexed, _outputs_indexed,
 * _update_param_solve_subset) with GLOBAL ids and host arrays in list order: the list is checked as a whole first -- a refused list
 * changes no shard --, every shard's rows are packed on the host and handed to its handle with shard-local ids, results are scattered back
 * to list order; the shards of eicos_multi_update_param_solve_subset run concurrently.  The _indexed_device forms have no multi form. */
int eicos_multi_update_indexed(eicos_multi *mh, const int *idx, int count, const double *Gpr, const double *Apr, const double *c,
                               const double *h, const double *b);
int eicos_multi_update_rhs_indexed(eicos_multi *mh, const int *idx, int count, const double *c, const double *h, const double *b);
int eicos_multi_update_param_indexed(eicos_multi *mh, const int *idx, int count, const double *theta);
int eicos_multi_set_iterate_indexed(eicos_multi *mh, const int *idx, int count, const double *x, const double *y, const double *z, const double *s);
int eicos_multi_outputs_indexed(eicos_multi *mh, const int *idx, int count, double *u);
/* adjoint sensitivities (eicos_batch_adjoint, _output_jacobian) with GLOBAL ids and host arrays in list order; idx NULL = 0 .. count-1 */
int eicos_multi_adjoint(eicos_multi *mh, const int *idx, int count, int nrhs, const double *g, double *grad_c, double *grad_h,
                        double *grad_b, double *res);
int eicos_multi_output_jacobian(eicos_multi *mh, const int *idx, int count, double *J, double *res);
/* ... and eicos_batch_adjoint_data, _param_jacobian, _param_gradient likewise */
int eicos_multi_adjoint_data(eicos_multi *mh, const int *idx, int count, int nrhs, const double *g, double *grad_c, double *grad_h,
                             double *grad_b, double *grad_G, double *grad_A, double *res);
int eicos_multi_param_jacobian(eicos_multi *mh, const int *idx, int count, double *J, double *res);
int eicos_multi_param_gradient(eicos_multi *mh, const int *idx, int count, int nrhs, const double *g, double *grad_theta, double *res);
/* the cone scaling of the adjoint (eicos_batch_set_adjoint_scaling on every shard; a refused mode changes no shard); get: the first shard's */
int eicos_multi_set_adjoint_scaling(eicos_multi *mh, int mode);
int eicos_multi_adjoint_scaling(eicos_multi *mh);
int eicos_multi_update_param_solve_subset(eicos_multi *mh, const int *idx, int count, const double *theta, double *u_out, double *x_out,
                                          int *exitcodes);
/* results gathered into the caller's host arrays in global instance order (the "gather" of north_star: per-device copies) */
int eicos_multi_solution(eicos_multi *mh, double *x);
int eicos_multi_duals(eicos_multi *mh, double *y, double *z, double *s);
int eicos_multi_info(eicos_multi *mh, eicos_info *info /* [batch] */);
int eicos_multi_set_warm_start(eicos_multi *mh, double shift);
int eicos_multi_set_dynamic_regularization(eicos_multi *mh, double delta, double eps);
/* runtime settings (eicos_batch_set_settings on every shard; a refused struct changes no shard); get: the first shard's */
int eicos_multi_set_settings(eicos_multi *mh, const eicos_settings *s);
int eicos_multi_get_settings(eicos_multi *mh, eicos_settings *out);
/* retry policy (eicos_batch_set_retry on every shard; a refused policy changes no shard); get: the first shard's; counts: global ids */
int eicos_multi_set_retry(eicos_multi *mh, const eicos_retry *r);
int eicos_multi_get_retry(eicos_multi *mh, eicos_retry *out);
int eicos_multi_retry_counts(eicos_multi *mh, int first, int count, int *retries /* host [count] */, int reset);
/* fallback map (eicos_batch_set_fallback_map on every shard; a refused map changes no shard); mask: the first shard's; counts: global ids */
int eicos_multi_set_fallback_map(eicos_multi *mh, unsigned mask, const eicos_affine_map *v);
int eicos_multi_fallback_mask(eicos_multi *mh);
int eicos_multi_fallback_counts(eicos_multi *mh, int first, int count, int *fired /* host [count] */, int reset);
/* the shards: their number, and shard s's single-GPU handle (every eicos_batch_* call works on it), instance range and device */
int eicos_multi_num_shards(eicos_multi *mh);
int eicos_multi_shard(eicos_multi *mh, int s, eicos_batch **handle, int *first, int *count, int *device);
/* HIP-event duration of the most recent solve (ms): per_shard ([num_shards], optional) = every shard's own launch; ms_max = the slowest
 * DEVICE -- for a device that holds several shards, from the start of its first launch to the end of its last one */
int eicos_multi_last_solve_ms(eicos_multi *mh, float *ms_max, float *per_shard);
int eicos_multi_destroy(eicos_multi *mh);
const char *eicos_multi_last_error(void);

const char *eicos_last_error(void);
/* number of visible HIP devices (0 when there is no GPU); never initialises a context */
int eicos_device_count(void);

/* Debug/parity hooks (tests only): numeric LDL' of instance `inst` with the KKT values as they
 * stand. Host buffers. There is no hook for a single LDL' solve: the triangular sweeps are checked
 * through the solve kernel itself, run with eicos_settings.nitref = 0 so that no refinement step
 * follows them, against the CPU oracle under the same setting (tests/test_unrefined_solves.py). */
int eicos_debug_factor(eicos_batch *hd, int inst, double *D /*[dim_K], permuted*/, double *U /*[nnzL] CSC, permuted*/);
/* per-iteration history of instance `inst` in the last solve: out[102][12] = {pcost,dcost,gap,pres,dres,
 * kap/tau,mu,step,sigma,tau,kap,nitref3} per IPM pass (valid while batch <= resident workgroups; after a subset launch: while its
 * count <= resident workgroups, for the instances of that launch). */
int eicos_debug_trace(eicos_batch *hd, int inst, double *out);
int eicos_debug_pattern(eicos_batch *hd, int *perm /*[dim_K]*/, int *Lp /*[dim_K+1]*/, int *Li /*[nnzL]*/);
/* upper triangle of instance `inst`'s KKT matrix as the numeric factorisation reads it (equilibrated A/G values,
 * scaling block, +-delta), coordinate form in the reference's column layout (src/eicos.cpp:1734-1890); each [nnzK] */
int eicos_debug_kkt(eicos_batch *hd, int inst, int *rows, int *cols, double *vals);
/* the solver's own updateScalings + updateKKTScalings stage (reference src/eicos.cpp:1160-1162) for a given (s, z):
 * V[l + sum(3 q_i + 1)] = scaling block of K in the slot order of reference cacheIndices (:1944-1987); *ran = 1 if
 * the stage reached the scalings.  The cone state persists between calls, as it does between iterations. */
int eicos_debug_scalings(eicos_batch *hd, int inst, const double *s, const double *z, double *V, int *ran);

/* Host-only self check of the symbolic analysis + factor/solve programs (no GPU needed):
 * returns ||K x - b||_inf / ||b||_inf for random quasi-definite values, < 0 on error. */
double eicos_debug_host_check(int n, int m, int p, int ncones, const int *q, const int *Gjc, const int *Gir,
                              const int *Ajc, const int *Air, unsigned seed, int order_mode, int *stats);

/* the same for the tile (dense-front) path: block factorisation over 16 x 16 tiles + tile sweeps emulated on the host
 * with the device's index structures; stats = {dim_K, nnzK, nnzL, block levels, tile pairs, order_mode, blocks, tiles} */
double eicos_debug_host_check_tiles(int n, int m, int p, int ncones, const int *q, const int *Gjc, const int *Gir,
                                    const int *Ajc, const int *Air, unsigned seed, int order_mode, int *stats);

/* host-only: elimination order (perm[dim_K]: new -> KKT index), block partition (blk_ptr[blocks + 1]) and L pattern of the tile path; returns the
 * number of blocks; stats = {dim_K, nnzL, blocks, off-diagonal tiles, block levels, tile pairs, order_mode, cone_order} */
int eicos_debug_host_tile_order(int n, int m, int p, int ncones, const int *q, const int *Gjc, const int *Gir,
                                const int *Ajc, const int *Air, int order_mode, int *perm, int *blk_ptr, int *stats,
                                int *Lp /* [dim_K + 1] or NULL */, int *Li /* [nnzL] or NULL: the pattern of L in that order, CSC */);

/* the same for the hybrid path (scalar programs below the cut, tiles on the top block of the tree); returns -10 when the
 * pattern's schedule has no tail worth handing to the tile path */
double eicos_debug_host_check_hybrid(int n, int m, int p, int ncones, const int *q, const int *Gjc, const int *Gir,
                                     const int *Ajc, const int *Air, unsigned seed, int order_mode, int *stats);

#ifdef __cplusplus
}
#endif
#endif
