// May this step run inside the solve launch?  The one rule, as pure functions of integers (the knob EICOS_FUSED_UPDATE stays with the
// callers in api.cpp).  Host only: no HIP, so that the check under tests/host compiles it on its own.
#pragma once

namespace eicos {
// What the rule reads of a handle: the pattern's n, p, m and padded KKT dimension, the LDS vectors and the workgroup size of its k_solve.
struct FitShape { int n, p, m, Npad, nlds, threads; };
// The in-register scaling accumulators of updateData at T threads (kernels.hip: update_instance): 8 entries of c and b and 16 of h a thread.
constexpr bool accumulators_fit(int n, int p, int m, int T) { return n <= 8 * T && p <= 8 * T && m <= 16 * T; }
constexpr bool accumulators_fit(const FitShape &s) { return accumulators_fit(s.n, s.p, s.m, s.threads); }
// the entry-parallel updateData kernels (512 threads; their LDS-size tests stay in launch_shape)
constexpr bool update_vectors_fit(int n, int p, int m) { return accumulators_fit(n, p, m, 512); }

// Every fused step keeps its maxima or its theta row in the LDS sweep vector: the NLDS >= 1 kernels.
constexpr bool fused_full_fits(const FitShape &s) { return s.nlds >= 1 && accumulators_fit(s); }
// (no accumulator limit: the fused right-hand-side step divides by the stored scalings)
constexpr bool fused_rhs_fits(const FitShape &s) { return s.nlds >= 1; }
// `rows` doubles staged in the LDS vector -- the k of a parametric step, the k + r of a rollout's [theta | u]; under a matrix map the step
// is a full updateData from theta and needs the accumulators too
constexpr bool fused_theta_fits(const FitShape &s, int rows, bool matrix_map) { return s.nlds >= 1 && rows <= s.Npad && (!matrix_map || accumulators_fit(s)); }
constexpr bool fused_param_fits(const FitShape &s, int k, bool matrix_map) { return fused_theta_fits(s, k, matrix_map); }
constexpr bool fused_rollout_fits(const FitShape &s, int k, int r, bool matrix_map) { return fused_theta_fits(s, k + r, matrix_map); }
} // namespace eicos
