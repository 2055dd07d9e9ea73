// include/eicos.hpp -- drop-in re-creation of the reference's public C++ surface
// (reference include/eicos.hpp:8-73,137-163) on top of the MI355X C ABI (eicos_amd.h).
//
//   EiCOS::Solver(n,m,p,l,ncones,q,Gpr,Gjc,Gir,Apr,Ajc,Air,c,h,b)   raw ctor     (ref :151-154)
//   updateData(Gpr,Apr,c,h,b)                                        raw update   (ref :155-156)
//   solve(verbose) / solution() / getInfo() / getSettings()                       (ref :158-163)
//   + the Eigen-typed ctor/updateData (ref :138-148) when <Eigen/Sparse> is available.
//
// One Solver = one pattern + ONE instance on the GPU (batch = 1 of the batched engine);
// EiCOS::BatchSolver below exposes the batched updateData path the hardware is built for.
// Header-only; link with libeicos_amd.so.  Errors of the C ABI surface as exitcode::fatal
// from solve() (the reference has no exceptions by design) or std::runtime_error from ctors.
#pragma once

#include <cstddef>
#include <cstdio>
#include <optional>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "eicos_amd.h"

#if __has_include(<Eigen/Sparse>)
#include <Eigen/Sparse>
#define EICOS_HAVE_EIGEN 1
#endif

namespace EiCOS
{

    enum class exitcode // values of reference include/eicos.hpp:8-21
    {
        optimal = 0,
        primal_infeasible = 1,
        dual_infeasible = 2,
        maxit = -1,
        numerics = -2,
        outcone = -3,
        fatal = -7,
        close_to_optimal = 10,
        close_to_primal_infeasible = 11,
        close_to_dual_infeasible = 12,
        not_converged_yet = -87
    };

    // Extension: the exit classes of BatchSolver::select / solveWhere (EICOS_SEL_* of eicos_amd.h): every instance is in exactly one, by
    // the exit code and n_factor of its info record; a mask is an OR of these
    enum sel : unsigned
    {
        sel_optimal = EICOS_SEL_OPTIMAL, sel_pinf = EICOS_SEL_PINF, sel_dinf = EICOS_SEL_DINF,
        sel_optimal_inacc = EICOS_SEL_OPTIMAL_INACC, sel_pinf_inacc = EICOS_SEL_PINF_INACC, sel_dinf_inacc = EICOS_SEL_DINF_INACC,
        sel_maxit = EICOS_SEL_MAXIT, sel_numerics = EICOS_SEL_NUMERICS, sel_outcone = EICOS_SEL_OUTCONE, sel_fatal = EICOS_SEL_FATAL,
        sel_other = EICOS_SEL_OTHER, sel_unsolved = EICOS_SEL_UNSOLVED,
        sel_failed = EICOS_SEL_FAILED, sel_not_optimal = EICOS_SEL_NOT_OPTIMAL, sel_all = EICOS_SEL_ALL
    };

    // reference include/eicos.hpp:23-47.  The ten members without `const` are the runtime settings of the GPU kernels (eicos_settings of
    // eicos_amd.h: ranges and semantics there): Solver::solve() and BatchSolver::setSettings hand them to the handle.  `maxit` is the
    // reference's second name for the iteration cap: `iter_max` is the one that is read.  The const members are compile-time constants of
    // the kernels (eicos_amd/csrc/kernels.hip).
    struct Settings
    {
        const double gamma = 0.99;
        const double delta = 2e-7;
        const double deltastat = 7e-8;
        const double eps = 1e13;
        double feastol = 1e-8;
        double abstol = 1e-8;
        double reltol = 1e-8;
        double feastol_inacc = 1e-4;
        double abstol_inacc = 5e-5;
        double reltol_inacc = 5e-5;
        size_t nitref = 9;
        const size_t maxit = 100;
        bool verbose = false;
        double linsysacc = 1e-14;
        double irerrfact = 6;
        const double stepmin = 1e-6;
        const double stepmax = 0.999;
        const double sigmamin = 1e-4;
        const double sigmamax = 1.;
        const size_t equil_iters = 3;
        size_t iter_max = 100;
        const size_t safeguard = 500;

        // the ten runtime members as the C ABI takes them (a count beyond the int range becomes one the library refuses)
        eicos_settings to_c() const
        {
            const size_t big = 1u << 20;
            return eicos_settings{feastol, abstol, reltol, feastol_inacc, abstol_inacc, reltol_inacc, linsysacc, irerrfact,
                                  (int)(iter_max < big ? iter_max : big), (int)(nitref < big ? nitref : big)};
        }
        static Settings from(const eicos_settings &c)
        {
            Settings s;
            s.feastol = c.feastol; s.abstol = c.abstol; s.reltol = c.reltol;
            s.feastol_inacc = c.feastol_inacc; s.abstol_inacc = c.abstol_inacc; s.reltol_inacc = c.reltol_inacc;
            s.linsysacc = c.linsysacc; s.irerrfact = c.irerrfact; s.iter_max = (size_t)c.iter_max; s.nitref = (size_t)c.nitref;
            return s;
        }
    };

    // Extension: the retry policy of a handle (eicos_retry of eicos_amd.h: contract and refusals there).  An instance whose solve ends in
    // an exit class of `mask` (an OR of EiCOS::sel values) is solved once more INSIDE the same launch, under `settings`, `warm` (0 = cold,
    // the default) and the dynamic regularisation given here, before anything reads its result.  mask 0 = no policy.
    struct Retry
    {
        unsigned mask = 0;
        double warm = 0., dyn_delta = 0., dyn_eps = 0.;
        Settings settings;

        eicos_retry to_c() const { return eicos_retry{mask, warm, dyn_delta, dyn_eps, settings.to_c()}; }
        static Retry from(const eicos_retry &c)
        {
            Retry r;
            r.mask = c.mask; r.warm = c.warm; r.dyn_delta = c.dyn_delta; r.dyn_eps = c.dyn_eps;
            r.settings.feastol = c.settings.feastol; r.settings.abstol = c.settings.abstol; r.settings.reltol = c.settings.reltol;
            r.settings.feastol_inacc = c.settings.feastol_inacc; r.settings.abstol_inacc = c.settings.abstol_inacc;
            r.settings.reltol_inacc = c.settings.reltol_inacc; r.settings.linsysacc = c.settings.linsysacc;
            r.settings.irerrfact = c.settings.irerrfact; r.settings.iter_max = (size_t)c.settings.iter_max;
            r.settings.nitref = (size_t)c.settings.nitref;
            return r;
        }
    };

    struct Information // reference include/eicos.hpp:49-73
    {
        double pcost = 0, dcost = 0, pres = 0, dres = 0;
        bool pinf = false, dinf = false;
        std::optional<double> pinfres, dinfres;
        double gap = 0;
        std::optional<double> relgap;
        double sigma = 0, mu = 0, step = 0, step_aff = 0, kapovert = 0;
        size_t iter = 0, iter_max = 100, nitref1 = 0, nitref2 = 0, nitref3 = 0;

        static Information from(const eicos_info &i)
        {
            Information o;
            o.pcost = i.pcost; o.dcost = i.dcost; o.pres = i.pres; o.dres = i.dres;
            o.pinf = i.pinf != 0; o.dinf = i.dinf != 0;
            if (i.has_pinfres) o.pinfres = i.pinfres;
            if (i.has_dinfres) o.dinfres = i.dinfres;
            o.gap = i.gap;
            if (i.has_relgap) o.relgap = i.relgap;
            o.sigma = i.sigma; o.mu = i.mu; o.step = i.step; o.step_aff = i.step_aff; o.kapovert = i.kapovert;
            o.iter = (size_t)i.iter; o.nitref1 = (size_t)i.nitref1; o.nitref2 = (size_t)i.nitref2; o.nitref3 = (size_t)i.nitref3;
            return o;
        }
    };

    namespace detail
    {
        inline void check(int rc, const char *what)
        {
            if (rc != EICOS_OK) throw std::runtime_error(std::string(what) + ": " + eicos_last_error());
        }
    }

    // Extension: the matrix map of BatchSolver::setMatrixMap -- the stored values of G and / or A affine in the parameter row theta, one
    // eicos_affine_map row per stored value in the CSC order of Gpr / Apr (nullptr: that matrix is not mapped).  The arrays are the
    // caller's and are copied at installation.
    struct MatrixMap
    {
        const eicos_affine_map *G = nullptr;
        const eicos_affine_map *A = nullptr;
    };

    // Extension: the shift map of BatchSolver::setShiftMap -- the warm-start vectors x, y, z, s through a square eicos_affine_map each
    // (rows = n, p, m, m; nullptr: that vector is not shifted).  The arrays are the caller's and are copied at installation.
    struct ShiftMap
    {
        const eicos_affine_map *x = nullptr;
        const eicos_affine_map *y = nullptr;
        const eicos_affine_map *z = nullptr;
        const eicos_affine_map *s = nullptr;
    };

    // Extension: the fallback map of BatchSolver::setFallbackMap -- the backup output law u = v0 + V theta (eicos_affine_map: base[r] +
    // CSR matrix r x k) that a step whose final record falls in an exit class of `mask` (an OR of EICOS_SEL_*) takes its u row from.
    // The arrays are the caller's and are copied at installation; map == nullptr or mask == 0 removes the installed one.
    struct FallbackMap
    {
        unsigned mask = 0;
        const eicos_affine_map *map = nullptr;
    };

    // Batched engine: one pattern, `batch` instances.  Arrays are [batch][...] row-major in global instance order.
    // One GPU (device, -1 = current) or several: with a list of device ids the batch is cut into contiguous shards, one per
    // list entry, solved concurrently (eicos_multi_* of eicos_amd.h; a device may be listed more than once).
    class BatchSolver
    {
    public:
        BatchSolver(int n, int m, int p, int ncones, const int *q,
                    const int *Gjc, const int *Gir, const int *Ajc, const int *Air, int batch, int device = -1)
            : BatchSolver(n, m, p, ncones, q, Gjc, Gir, Ajc, Air, batch, std::vector<int>{device}) {}
        BatchSolver(int n, int m, int p, int ncones, const int *q,
                    const int *Gjc, const int *Gir, const int *Ajc, const int *Air, int batch, const std::vector<int> &device_ids)
            : n_(n), m_(m), p_(p), batch_(batch)
        {
            mcheck(eicos_multi_create(n, m, p, -1, ncones, q, Gjc, Gir, Ajc, Air, batch, device_ids.data(), (int)device_ids.size(), &h_), "eicos_multi_create");
            eicos_dims d; eicos_batch_dims(handle(), &d);
            n_ = d.n; m_ = d.m; p_ = d.p;
        }
        BatchSolver(const BatchSolver &) = delete;
        BatchSolver &operator=(const BatchSolver &) = delete;
        ~BatchSolver() { eicos_multi_destroy(h_); }

        void updateData(const double *Gpr, const double *Apr, const double *c, const double *h, const double *b,
                        int first = 0, int count = -1)
        {
            mcheck(eicos_multi_update(h_, first, count < 0 ? batch_ : count, Gpr, Apr, c, h, b), "eicos_multi_update");
        }
        // inputs already resident in the HBM of GPU `src_device`: no PCIe traffic; shards on other GPUs pull their rows over xGMI
        void updateDataDevice(int src_device, const double *dGpr, const double *dApr, const double *dc, const double *dh, const double *db,
                              int first = 0, int count = -1)
        {
            mcheck(eicos_multi_update_device(h_, src_device, first, count < 0 ? batch_ : count, dGpr, dApr, dc, dh, db), "eicos_multi_update_device");
        }
        // Extension (not in the reference, whose updateData reads h only with Gpr and b only with Apr): new c, h, b (nullptr keeps a group)
        // with G, A and their equilibration kept -- the vectors are divided by the stored scalings, bit for bit what updateData with the
        // unchanged matrices gives (eicos_batch_update_rhs of eicos_amd.h)
        void updateRHS(const double *c, const double *h, const double *b, int first = 0, int count = -1)
        {
            mcheck(eicos_multi_update_rhs(h_, first, count < 0 ? batch_ : count, c, h, b), "eicos_multi_update_rhs");
        }
        void updateRHSDevice(int src_device, const double *dc, const double *dh, const double *db, int first = 0, int count = -1)
        {
            mcheck(eicos_multi_update_rhs_device(h_, src_device, first, count < 0 ? batch_ : count, dc, dh, db), "eicos_multi_update_rhs_device");
        }
        // Extension: right-hand sides that are affine in a short parameter row, c = c0 + C theta, h = h0 + H theta, b = b0 + B theta
        // (eicos_affine_map: base vector + CSR matrix with k columns; nullptr = that group is not parametric and is kept).  The map is
        // copied to every shard once; updateParam then sends [count][k] doubles and the GPU expands them -- bit for bit what updateRHS of
        // the host-evaluated vectors leaves (rounding order: eicos_batch_update_param of eicos_amd.h).  All groups nullptr removes the map.
        void setParamMap(int k, const eicos_affine_map *c, const eicos_affine_map *h, const eicos_affine_map *b)
        {
            mcheck(eicos_multi_set_param_map(h_, k, c, h, b), "eicos_multi_set_param_map");
        }
        void updateParam(const double *theta, int first = 0, int count = -1)
        {
            mcheck(eicos_multi_update_param(h_, first, count < 0 ? batch_ : count, theta), "eicos_multi_update_param");
        }
        void updateParamDevice(int src_device, const double *dtheta, int first = 0, int count = -1)
        {
            mcheck(eicos_multi_update_param_device(h_, src_device, first, count < 0 ? batch_ : count, dtheta), "eicos_multi_update_param_device");
        }
        // Extension: the few numbers of x a controller applies, u = u0 + U x (eicos_affine_map: base[r] + CSR matrix r x n), one map for
        // all instances, copied to every shard; r = 0 or nullptr removes it.  outputs() evaluates it on the current x of instances
        // [first, first + count) -- bit for bit the map applied to solution() in the rounding order of eicos_amd.h.
        void setOutputMap(int r, const eicos_affine_map *u) { mcheck(eicos_multi_set_output_map(h_, r, u), "eicos_multi_set_output_map"); }
        void outputs(double *u, int first = 0, int count = -1)
        {
            mcheck(eicos_multi_outputs(h_, first, count < 0 ? batch_ : count, u), "eicos_multi_outputs");
        }
        // The closed-loop step in ONE call: updateParam(theta) + solve() + outputs(u_out) (+ solution(x_out)).  With theta from hostAlloc /
        // hostRegister the solve kernel's workgroups expand every instance's theta row themselves and write its u row (and x row) into
        // pinned u_out / x_out as instances finish: 8 k bytes in and 8 r bytes out per instance, one launch.  Same results on every path.
        std::vector<exitcode> stepParam(const double *theta, double *u_out, double *x_out = nullptr)
        {
            std::vector<int> codes(batch_);
            mcheck(eicos_multi_update_param_solve(h_, theta, u_out, x_out, codes.data()), "eicos_multi_update_param_solve");
            return exitcodes(codes);
        }
        // Extension: the simulated plant of a closed loop, theta+ = f0 + F [theta | u] (+ w) (eicos_affine_map: base[k] + CSR matrix
        // k x (k + r)), installed behind the parameter and the output map; nullptr removes it.  rollout() then runs `steps` closed-loop
        // steps of every instance in ONE call -- stepParam on the current theta row, then the plant map -- from theta0 [batch][k] and the
        // optional disturbance w [batch][steps][k] into u_traj [batch][steps][r] and, optionally, theta_traj [batch][steps + 1][k] and
        // iters [batch][steps]: bit for bit what the loop over stepParam gives, with an LDS vector on the handle in one launch per shard.
        // Returns the exit codes, [batch][steps].
        void setPlantMap(const eicos_affine_map *f) { mcheck(eicos_multi_set_plant_map(h_, f), "eicos_multi_set_plant_map"); }
        std::vector<exitcode> rollout(int steps, const double *theta0, double *u_traj, const double *w = nullptr, double *theta_traj = nullptr,
                                      int *iters = nullptr)
        {
            std::vector<int> codes((size_t)batch_ * (steps > 0 ? steps : 0));
            mcheck(eicos_multi_rollout(h_, steps, theta0, w, u_traj, theta_traj, codes.data(), iters), "eicos_multi_rollout");
            return exitcodes(codes);
        }
        // Extension: the stored values of G and A affine in theta (MatrixMap: per matrix an eicos_affine_map with one row per stored
        // value, CSC order, k columns), installed behind the parameter map; both nullptr removes it.  updateParam, stepParam and rollout
        // then run a full updateData whose inputs the GPU forms from theta -- bit for bit update() of the host-evaluated arrays
        // (contract and rounding order: eicos_batch_set_matrix_map of eicos_amd.h).
        void setMatrixMap(const MatrixMap &m) { mcheck(eicos_multi_set_matrix_map(h_, m.G, m.A), "eicos_multi_set_matrix_map"); }
        // Extension: the warm start moved by an affine map inside the solve kernel (ShiftMap; the receding-horizon shift: stage t + 1
        // becomes stage t).  Every solve that warm-starts an instance -- solve, stepParam, every step of rollout -- first replaces its
        // x, y, z, s by the shifted ones: bit for bit setIterate of the host-evaluated vectors before the same solve (contract and
        // rounding order: eicos_batch_set_shift_map of eicos_amd.h).  All four nullptr removes it.
        void setShiftMap(const ShiftMap &m) { mcheck(eicos_multi_set_shift_map(h_, m.x, m.y, m.z, m.s), "eicos_multi_set_shift_map"); }
        // Extension: a caller-supplied starting point for instances [first, first + count): rows of x [count][n], y [count][p],
        // z, s [count][m] in the units of solution() (nullptr keeps a group).  With setWarmStart(> 0) the next solve starts from it;
        // with warm start 0 it is ignored (eicos_batch_set_iterate of eicos_amd.h).
        void setIterate(const double *x, const double *y, const double *z, const double *s, int first = 0, int count = -1)
        {
            mcheck(eicos_multi_set_iterate(h_, first, count < 0 ? batch_ : count, x, y, z, s), "eicos_multi_set_iterate");
        }
        // Extension (not in the reference): re-solves start from the previous solution, see eicos_amd.h
        void setWarmStart(double shift) { mcheck(eicos_multi_set_warm_start(h_, shift), "eicos_multi_set_warm_start"); }
        // Extension: ECOS-style dynamic regularisation (the reference's Settings::delta / ::eps are never read)
        void setDynamicRegularization(double delta, double eps)
        {
            mcheck(eicos_multi_set_dynamic_regularization(h_, delta, eps), "eicos_multi_set_dynamic_regularization");
        }
        // Runtime settings (the ten non-const members of Settings; eicos_settings of eicos_amd.h), on every shard: in effect from the next
        // solve, stepParam or rollout.  A refused value throws and changes nothing.
        void setSettings(const Settings &s)
        {
            const eicos_settings c = s.to_c();
            mcheck(eicos_multi_set_settings(h_, &c), "eicos_multi_set_settings");
        }
        Settings settings() const
        {
            eicos_settings c;
            mcheck(eicos_multi_get_settings(h_, &c), "eicos_multi_get_settings");
            return Settings::from(c);
        }
        // Retry policy (Retry, above), on every shard: in effect from the next solve, solveSubset, stepParam or rollout -- also between the
        // steps of a one-launch rollout.  Retry{} (mask 0) removes it.  A refused value throws and changes nothing.
        // retryCounts: per instance the second attempts since the counters were last reset (cumulative over launches and rollout steps).
        void setRetry(const Retry &r)
        {
            const eicos_retry c = r.to_c();
            mcheck(eicos_multi_set_retry(h_, &c), "eicos_multi_set_retry");
        }
        Retry retry() const
        {
            eicos_retry c;
            mcheck(eicos_multi_get_retry(h_, &c), "eicos_multi_get_retry");
            return Retry::from(c);
        }
        std::vector<int> retryCounts(bool reset = false)
        {
            std::vector<int> out(batch_);
            mcheck(eicos_multi_retry_counts(h_, 0, batch_, out.data(), reset ? 1 : 0), "eicos_multi_retry_counts");
            return out;
        }
        // Extension: the backup output law (FallbackMap, above), on every shard, behind the parameter and the output map: from the next
        // stepParam, stepParamSubset, rollout or rolloutJacobian on, an instance whose final record -- after the retry, when one ran --
        // is in a class of the mask gets its u row as v0 + V theta; states, exit codes and x_out stay what they are without it
        // (eicos_batch_set_fallback_map of eicos_amd.h).  A refused map throws and changes nothing.
        // fallbackMask: 0 = none installed.  fallbackCounts: per instance the steps whose u row the law has formed since the last reset.
        void setFallbackMap(unsigned mask, const eicos_affine_map *map)
        {
            mcheck(eicos_multi_set_fallback_map(h_, mask, map), "eicos_multi_set_fallback_map");
        }
        void setFallbackMap(const FallbackMap &f) { setFallbackMap(f.mask, f.map); }
        unsigned fallbackMask() const
        {
            const int v = eicos_multi_fallback_mask(h_);
            if (v < 0) mcheck(v, "eicos_multi_fallback_mask");
            return (unsigned)v;
        }
        std::vector<int> fallbackCounts(bool reset = false)
        {
            std::vector<int> out(batch_);
            mcheck(eicos_multi_fallback_counts(h_, 0, batch_, out.data(), reset ? 1 : 0), "eicos_multi_fallback_counts");
            return out;
        }
        std::vector<exitcode> solve()
        {
            std::vector<int> codes(batch_);
            mcheck(eicos_multi_solve(h_, codes.data()), "eicos_multi_solve");
            return exitcodes(codes);
        }
        // updateData(...) + solve() in ONE call (reference include/eicos.hpp:155-158 back to back): with arrays from hostAlloc / hostRegister the
        // solve kernel's workgroups pull every instance's inputs over PCIe themselves, behind each other's compute, and write x into a pinned
        // `x_out` ([batch][n], optional) as instances finish; plain arrays take updateData + solve.  Same results on every path.
        std::vector<exitcode> solve(const double *Gpr, const double *Apr, const double *c, const double *h, const double *b, double *x_out = nullptr)
        {
            std::vector<int> codes(batch_);
            mcheck(eicos_multi_update_solve(h_, Gpr, Apr, c, h, b, x_out, codes.data()), "eicos_multi_update_solve");
            return exitcodes(codes);
        }
        // updateRHS(...) + solve() in ONE call (same paths as the form above; the solve kernel scales the vectors of pinned arrays itself)
        std::vector<exitcode> solve(const double *c, const double *h, const double *b, double *x_out = nullptr)
        {
            std::vector<int> codes(batch_);
            mcheck(eicos_multi_update_rhs_solve(h_, c, h, b, x_out, codes.data()), "eicos_multi_update_rhs_solve");
            return exitcodes(codes);
        }
        // Extension: solve a chosen subset of the batch (eicos_batch_solve_subset / _solve_where of eicos_amd.h: contract and refusals
        // there).  Indices are global instance ids, each at most once.  An instance of the subset ends, bit for bit, as a solve() of the
        // whole batch would leave it; every other instance keeps its state, its info record included.  Settings, warm start and
        // regularisation are the handle's: set them for the retry, solve the subset, set them back.
        // select: the ascending ids of the instances whose exit class is in `mask` (an OR of EiCOS::sel values), found on the GPU.
        std::vector<int> select(unsigned mask) const
        {
            std::vector<int> ids(batch_);
            int count = 0;
            mcheck(eicos_multi_select(h_, mask, ids.data(), &count), "eicos_multi_select");
            ids.resize(count);
            return ids;
        }
        // solveSubset: one launch over `indices`; the exit codes in list order.  An empty list launches nothing.
        std::vector<exitcode> solveSubset(const std::vector<int> &indices)
        {
            std::vector<int> codes(indices.size());
            mcheck(eicos_multi_solve_subset(h_, indices.data(), (int)indices.size(), codes.data()), "eicos_multi_solve_subset");
            return exitcodes(codes);
        }
        // solveWhere: select(mask) + solveSubset with the id list used in place on the GPU; (ids ascending, their exit codes)
        std::pair<std::vector<int>, std::vector<exitcode>> solveWhere(unsigned mask)
        {
            std::vector<int> ids(batch_), codes(batch_);
            int count = 0;
            mcheck(eicos_multi_solve_where(h_, mask, ids.data(), &count, codes.data()), "eicos_multi_solve_where");
            ids.resize(count); codes.resize(count);
            return {ids, exitcodes(codes)};
        }
        // gather: the rows of `indices`, in list order, into x [count][n], y [count][p], z, s [count][m] and info [count] (any nullptr):
        // packed on the GPU and fetched with one copy, instead of whole-batch solution() / duals() / getInfo()
        void gather(const std::vector<int> &indices, double *x, double *y = nullptr, double *z = nullptr, double *s = nullptr,
                    eicos_info *info = nullptr) const
        {
            mcheck(eicos_multi_gather(h_, indices.data(), (int)indices.size(), x, y, z, s, info), "eicos_multi_gather");
        }
        // Extension: update, read and step a chosen SUBSET (eicos_multi_*_indexed, _update_param_solve_subset of eicos_amd.h).  `indices` are
        // distinct global instance ids; row q of every array ([indices.size()][...]) belongs to instance indices[q], nullptr keeps a group.
        // Each overload leaves, bit for bit, what the loop of count = 1 calls of its range namesake leaves; the other instances keep
        // their state.  An empty list does nothing; a refused list (out of range, duplicate) throws and changes nothing.
        void updateData(const std::vector<int> &indices, const double *Gpr, const double *Apr, const double *c, const double *h, const double *b)
        {
            mcheck(eicos_multi_update_indexed(h_, indices.data(), (int)indices.size(), Gpr, Apr, c, h, b), "eicos_multi_update_indexed");
        }
        void updateRHS(const std::vector<int> &indices, const double *c, const double *h, const double *b)
        {
            mcheck(eicos_multi_update_rhs_indexed(h_, indices.data(), (int)indices.size(), c, h, b), "eicos_multi_update_rhs_indexed");
        }
        void updateParam(const std::vector<int> &indices, const double *theta)
        {
            mcheck(eicos_multi_update_param_indexed(h_, indices.data(), (int)indices.size(), theta), "eicos_multi_update_param_indexed");
        }
        void setIterate(const std::vector<int> &indices, const double *x, const double *y, const double *z, const double *s)
        {
            mcheck(eicos_multi_set_iterate_indexed(h_, indices.data(), (int)indices.size(), x, y, z, s), "eicos_multi_set_iterate_indexed");
        }
        void outputs(const std::vector<int> &indices, double *u)
        {
            mcheck(eicos_multi_outputs_indexed(h_, indices.data(), (int)indices.size(), u), "eicos_multi_outputs_indexed");
        }
        // stepParamSubset: the closed-loop step for the instances `indices` only -- updateParam(indices, theta) + solveSubset(indices) +
        // outputs(indices, u_out) (+ the x rows) in ONE call; theta [count][k], u_out [count][r], x_out [count][n] in list order.  With
        // theta from hostAlloc / hostRegister it is one subset launch per shard whose workgroups expand their own theta row and write
        // their rows of pinned result arrays.  Returns the exit codes in list order.
        std::vector<exitcode> stepParamSubset(const std::vector<int> &indices, const double *theta, double *u_out, double *x_out = nullptr)
        {
            std::vector<int> codes(indices.size());
            mcheck(eicos_multi_update_param_solve_subset(h_, indices.data(), (int)indices.size(), theta, u_out, x_out, codes.data()),
                   "eicos_multi_update_param_solve_subset");
            return exitcodes(codes);
        }
        // Extension: adjoint sensitivities at the returned iterate (eicos_multi_adjoint / _output_jacobian; the definition and its
        // degeneracy caveat: eicos_amd.h).  adjoint: g [count][nrhs][n] in, grad_c [count][nrhs][n], grad_h [count][nrhs][m],
        // grad_b [count][nrhs][p], res [count][nrhs] out (any nullptr) -- the gradient of g'x with respect to (c, h, b); an instance whose
        // last solve did not end OPTIMAL / OPTIMAL_INACC gets NaN rows.  outputJacobian: J [count][r][k] = du / dtheta under the installed
        // parameter and output maps, res [count][r] (optional).  The whole batch, or the instances `indices` in list order.  Nothing a
        // later call reads is changed.
        void adjoint(int nrhs, const double *g, double *grad_c, double *grad_h = nullptr, double *grad_b = nullptr, double *res = nullptr)
        {
            mcheck(eicos_multi_adjoint(h_, nullptr, batch_, nrhs, g, grad_c, grad_h, grad_b, res), "eicos_multi_adjoint");
        }
        void adjoint(const std::vector<int> &indices, int nrhs, const double *g, double *grad_c, double *grad_h = nullptr, double *grad_b = nullptr,
                     double *res = nullptr)
        {
            if (indices.empty()) return;
            mcheck(eicos_multi_adjoint(h_, indices.data(), (int)indices.size(), nrhs, g, grad_c, grad_h, grad_b, res), "eicos_multi_adjoint");
        }
        void outputJacobian(double *J, double *res = nullptr) { mcheck(eicos_multi_output_jacobian(h_, nullptr, batch_, J, res), "eicos_multi_output_jacobian"); }
        void outputJacobian(const std::vector<int> &indices, double *J, double *res = nullptr)
        {
            if (indices.empty()) return;
            mcheck(eicos_multi_output_jacobian(h_, indices.data(), (int)indices.size(), J, res), "eicos_multi_output_jacobian");
        }
        // ... with respect to the matrix data (eicos_multi_adjoint_data / _param_jacobian / _param_gradient).  adjointData: adjoint with
        // grad_G [count][nrhs][nnzG] and grad_A [count][nrhs][nnzA] (CSC order of Gpr / Apr; any nullptr): grad_G[e] = grad_c[j] z[i] -
        // grad_h[i] x[j], grad_A[e] = grad_c[j] y[i] - grad_b[i] x[j] for the stored value e = (i, j).  paramJacobian: J [count][r][k] =
        // du / dtheta through the output map and whichever of the parameter map and the matrix map are installed (without a matrix map:
        // the bits of outputJacobian).  paramGradient: grad_theta [count][nrhs][k] = the gradient of g'x with respect to theta through
        // the same maps; no output map is needed.
        void adjointData(int nrhs, const double *g, double *grad_c, double *grad_h, double *grad_b, double *grad_G, double *grad_A, double *res = nullptr)
        {
            mcheck(eicos_multi_adjoint_data(h_, nullptr, batch_, nrhs, g, grad_c, grad_h, grad_b, grad_G, grad_A, res), "eicos_multi_adjoint_data");
        }
        void adjointData(const std::vector<int> &indices, int nrhs, const double *g, double *grad_c, double *grad_h, double *grad_b, double *grad_G,
                         double *grad_A, double *res = nullptr)
        {
            if (indices.empty()) return;
            mcheck(eicos_multi_adjoint_data(h_, indices.data(), (int)indices.size(), nrhs, g, grad_c, grad_h, grad_b, grad_G, grad_A, res),
                   "eicos_multi_adjoint_data");
        }
        void paramJacobian(double *J, double *res = nullptr) { mcheck(eicos_multi_param_jacobian(h_, nullptr, batch_, J, res), "eicos_multi_param_jacobian"); }
        void paramJacobian(const std::vector<int> &indices, double *J, double *res = nullptr)
        {
            if (indices.empty()) return;
            mcheck(eicos_multi_param_jacobian(h_, indices.data(), (int)indices.size(), J, res), "eicos_multi_param_jacobian");
        }
        void paramGradient(int nrhs, const double *g, double *grad_theta, double *res = nullptr)
        {
            mcheck(eicos_multi_param_gradient(h_, nullptr, batch_, nrhs, g, grad_theta, res), "eicos_multi_param_gradient");
        }
        void paramGradient(const std::vector<int> &indices, int nrhs, const double *g, double *grad_theta, double *res = nullptr)
        {
            if (indices.empty()) return;
            mcheck(eicos_multi_param_gradient(h_, indices.data(), (int)indices.size(), nrhs, g, grad_theta, res), "eicos_multi_param_gradient");
        }
        // The cone scaling of K in every call above and in rolloutJacobian (eicos_multi_set_adjoint_scaling): EICOS_ADJOINT_NT (the
        // default) or EICOS_ADJOINT_CENTRED -- the NT scaling of the re-centred pair of every second-order cone, the derivative where an
        // active cone's curvature fixes the optimum: for any pattern with cones.  Holds from the next adjoint launch on every shard.
        void setAdjointScaling(int mode) { mcheck(eicos_multi_set_adjoint_scaling(h_, mode), "eicos_multi_set_adjoint_scaling"); }
        int adjointScaling() const
        {
            const int v = eicos_multi_adjoint_scaling(h_);
            if (v < 0) mcheck(v, "eicos_multi_adjoint_scaling");
            return v;
        }
        // Extension: rollout() that also records J_traj [batch][steps][r][k] = d u_t / d theta_t of every step (and, optionally, the
        // refinement residuals res_traj [batch][steps][r]) -- what paramJacobian returns right after step t's solve, bit for bit, still
        // in one launch per shard.  rolloutGradient then gives the gradient of L = sum_t gu_t' u_t + sum_t gtheta_t' theta_t over that
        // rollout with respect to theta_0 (grad_theta0 [batch][k]) and, optionally, to the disturbances (grad_w [batch][steps][k]); gu
        // [batch][steps][r] and gtheta [batch][steps + 1][k] are each optional, one must be given.  A step that did not end optimal has
        // NaN rows, and the gradient of that instance is NaN (definition, order and caveats: eicos_batch_rollout_jacobian of eicos_amd.h).
        std::vector<exitcode> rolloutJacobian(int steps, const double *theta0, double *u_traj, double *J_traj, const double *w = nullptr,
                                              double *theta_traj = nullptr, int *iters = nullptr, double *res_traj = nullptr)
        {
            std::vector<int> codes((size_t)batch_ * (steps > 0 ? steps : 0));
            mcheck(eicos_multi_rollout_jacobian(h_, steps, theta0, w, u_traj, theta_traj, codes.data(), iters, J_traj, res_traj), "eicos_multi_rollout_jacobian");
            return exitcodes(codes);
        }
        void rolloutGradient(const double *gu, const double *gtheta, double *grad_theta0, double *grad_w = nullptr)
        {
            mcheck(eicos_multi_rollout_gradient(h_, gu, gtheta, grad_theta0, grad_w), "eicos_multi_rollout_gradient");
        }
        // Extension: per-instance plant values -- one controller against many plants.  setPlantValues gives instances [first, first +
        // count) rows of their own in the place of the plant map's base (f0 [count][k]) and / or stored values (val [count][nnzF],
        // the map's CSR order; the pattern stays shared); nullptr keeps a group, and the first call of a group starts every instance
        // from the shared values.  Every rollout form then runs instance i against its own plant, bit for bit the host loop with the
        // plant evaluated per instance.  plantValues reads rows back (the shared values where none are installed), hasPlantValues: bit
        // 0 f0, bit 1 val; clearPlantValues and setPlantMap drop them.  rolloutPlantGradient is rolloutGradient over the recorded
        // trajectory that also returns the gradient with respect to the plant's own entries per instance, grad_f0 [batch][k] and
        // grad_val [batch][nnzF], from the u_traj and theta_traj rolloutJacobian returned; each output is optional, one must be given
        // (definition and order: eicos_batch_rollout_plant_gradient of eicos_amd.h).  For the shared plant sum the rows over the batch.
        void setPlantValues(int first, int count, const double *f0, const double *val)
        {
            mcheck(eicos_multi_set_plant_values(h_, first, count, f0, val), "eicos_multi_set_plant_values");
        }
        void plantValues(int first, int count, double *f0_out, double *val_out) const
        {
            mcheck(eicos_multi_plant_values(h_, first, count, f0_out, val_out), "eicos_multi_plant_values");
        }
        int hasPlantValues() const
        {
            const int v = eicos_multi_has_plant_values(h_);
            if (v < 0) mcheck(v, "eicos_multi_has_plant_values");
            return v;
        }
        void clearPlantValues() { mcheck(eicos_multi_clear_plant_values(h_), "eicos_multi_clear_plant_values"); }
        void rolloutPlantGradient(const double *gu, const double *gtheta, const double *u_traj, const double *theta_traj, double *grad_theta0,
                                  double *grad_w, double *grad_f0, double *grad_val)
        {
            mcheck(eicos_multi_rollout_plant_gradient(h_, gu, gtheta, u_traj, theta_traj, grad_theta0, grad_w, grad_f0, grad_val),
                   "eicos_multi_rollout_plant_gradient");
        }
        // Extension: the gradient with respect to the CONTROLLER's own data.  setRolloutRecording(true): rolloutJacobian then also
        // records, on the GPU, the gradient rows of every step's output rows and the step's x, y, z (batch * steps * (r + 1) *
        // (n + m + p) * 8 bytes; everything rolloutJacobian returns keeps its bits).  rolloutRecords copies whichever of the six
        // arrays are wanted to the host.  rolloutDataGradient sweeps backwards over the recorded rollout, for rolloutGradient's cost
        // L, and fills the non-null members of `out`, one row per instance: grad_c / grad_h / grad_b, grad_G / grad_A (stored values,
        // CSC order), grad_Cval / grad_Hval / grad_Bval (the parameter map's slopes) and grad_u0 / grad_Uval (the output map);
        // theta_traj is the array rolloutJacobian returned (definition, order and what is out of scope:
        // eicos_batch_rollout_data_gradient of eicos_amd.h).  For data shared by the batch sum the rows.
        void setRolloutRecording(bool on) { mcheck(eicos_multi_set_rollout_recording(h_, on ? 1 : 0), "eicos_multi_set_rollout_recording"); }
        bool rolloutRecording() const
        {
            const int v = eicos_multi_rollout_recording(h_);
            if (v < 0) mcheck(v, "eicos_multi_rollout_recording");
            return v != 0;
        }
        void rolloutRecords(double *Wc, double *Wh, double *Wb, double *x_rec = nullptr, double *y_rec = nullptr, double *z_rec = nullptr) const
        {
            mcheck(eicos_multi_rollout_records(h_, Wc, Wh, Wb, x_rec, y_rec, z_rec), "eicos_multi_rollout_records");
        }
        void rolloutDataGradient(const double *gu, const double *gtheta, const double *theta_traj, const eicos_data_gradient &out)
        {
            mcheck(eicos_multi_rollout_data_gradient(h_, gu, gtheta, theta_traj, &out), "eicos_multi_rollout_data_gradient");
        }
        void solveAsync() { mcheck(eicos_multi_solve_async(h_), "eicos_multi_solve_async"); } // enqueue on every shard's stream
        void sync() { mcheck(eicos_multi_sync(h_), "eicos_multi_sync"); }
        std::vector<double> solution() const
        {
            std::vector<double> x((size_t)batch_ * n_);
            if (n_ > 0) mcheck(eicos_multi_solution(h_, x.data()), "eicos_multi_solution");
            return x;
        }
        // x into caller-owned storage [batch][n] (pinned memory from hostAlloc: one strided copy per shard, no bounce)
        void solution(double *x) const { if (n_ > 0) mcheck(eicos_multi_solution(h_, x), "eicos_multi_solution"); }
        // Pinned host arrays (eicos_host_alloc): updateData reads them in place over PCIe instead of through the bounce buffers -- for the
        // arrays a closed loop rewrites every sample.  Not in the reference (which computes on the host).
        static double *hostAlloc(size_t doubles)
        {
            void *ptr = eicos_host_alloc(doubles * sizeof(double));
            if (!ptr) throw std::runtime_error(std::string("eicos_host_alloc: ") + eicos_last_error());
            return static_cast<double *>(ptr);
        }
        static void hostFree(double *ptr) { eicos_host_free(ptr); }
        // ... or pin storage the caller already owns (a std::vector's data()) in place; unregister before it is freed or reallocated
        static void hostRegister(double *ptr, size_t doubles)
        {
            if (eicos_host_register(ptr, doubles * sizeof(double)) != EICOS_OK) throw std::runtime_error(std::string("eicos_host_register: ") + eicos_last_error());
        }
        static void hostUnregister(double *ptr) { eicos_host_unregister(ptr); }
        std::vector<Information> getInfo() const
        {
            std::vector<eicos_info> raw(batch_);
            mcheck(eicos_multi_info(h_, raw.data()), "eicos_multi_info");
            std::vector<Information> out;
            for (auto &r : raw) out.push_back(Information::from(r));
            return out;
        }
        int batch() const { return batch_; }
        int n_var() const { return n_; }
        int num_shards() const { return eicos_multi_num_shards(h_); }
        eicos_batch *handle(int shard = 0) const
        {
            eicos_batch *b = nullptr;
            mcheck(eicos_multi_shard(h_, shard, &b, nullptr, nullptr, nullptr), "eicos_multi_shard");
            return b;
        }
        eicos_multi *multi_handle() const { return h_; }

    private:
        static void mcheck(int rc, const char *what)
        {
            if (rc != EICOS_OK) throw std::runtime_error(std::string(what) + ": " + eicos_multi_last_error());
        }
        static std::vector<exitcode> exitcodes(const std::vector<int> &codes) // the C ABI's exit codes as the enum
        {
            std::vector<exitcode> out(codes.size());
            for (size_t i = 0; i < codes.size(); i++) out[i] = static_cast<exitcode>(codes[i]);
            return out;
        }
        eicos_multi *h_ = nullptr;
        int n_, m_, p_, batch_;
    };

    class Solver
    {
    public:
        // traditional interface (reference include/eicos.hpp:151-154); `l` is ignored as in the
        // reference (src/eicos.cpp:91); NULL groups are allowed (src/eicos.cpp:103-117)
        Solver(int n, int m, int p, int /*l*/, int ncones, int *q,
               double *Gpr, int *Gjc, int *Gir,
               double *Apr, int *Ajc, int *Air,
               double *c, double *h, double *b)
        {
            const bool haveG = Gpr && Gjc && Gir, haveA = Apr && Ajc && Air;
            if (!c) n = 0;
            detail::check(eicos_batch_create(n, haveG ? m : 0, haveA ? p : 0, -1 /* derived, ref src/eicos.cpp:91 */, haveG ? ncones : 0, q,
                                             haveG ? Gjc : nullptr, haveG ? Gir : nullptr,
                                             haveA ? Ajc : nullptr, haveA ? Air : nullptr, 1, -1, &h_),
                          "eicos_batch_create");
            eicos_dims d; eicos_batch_dims(h_, &d);
            resize_solution(d.n);
            // first data set: every group that exists must be supplied
            static double dummy = 0.0;
            detail::check(eicos_batch_update(h_, 0, 1, haveG ? Gpr : nullptr, haveA ? Apr : nullptr,
                                             d.n ? c : &dummy, haveG ? h : nullptr, haveA ? b : nullptr),
                          "eicos_batch_update");
        }
        Solver(const Solver &) = delete;
        Solver &operator=(const Solver &) = delete;
        ~Solver() { eicos_batch_destroy(h_); }

        // reference include/eicos.hpp:155-156 : NULL = keep; h is read only with Gpr, b only with Apr
        void updateData(double *Gpr, double *Apr, double *c, double *h, double *b)
        {
            detail::check(eicos_batch_update(h_, 0, 1, Gpr, Apr, c, h, b), "eicos_batch_update");
        }

#ifdef EICOS_HAVE_EIGEN
        // Eigen-typed surface (reference include/eicos.hpp:138-148).  Inputs are copied.
        Solver(const Eigen::SparseMatrix<double> &G, const Eigen::SparseMatrix<double> &A,
               const Eigen::VectorXd &c, const Eigen::VectorXd &h, const Eigen::VectorXd &b,
               const Eigen::VectorXi &soc_dims)
            : Solver(int(c.size()), int(G.rows()), int(A.rows()), 0, int(soc_dims.size()),
                     const_cast<int *>(soc_dims.data()),
                     const_cast<double *>(G.valuePtr()), const_cast<int *>(G.outerIndexPtr()), const_cast<int *>(G.innerIndexPtr()),
                     A.rows() ? const_cast<double *>(A.valuePtr()) : nullptr,
                     A.rows() ? const_cast<int *>(A.outerIndexPtr()) : nullptr,
                     A.rows() ? const_cast<int *>(A.innerIndexPtr()) : nullptr,
                     const_cast<double *>(c.data()), const_cast<double *>(h.data()), const_cast<double *>(b.data())) {}
        void updateData(const Eigen::SparseMatrix<double> &G, const Eigen::SparseMatrix<double> &A,
                        const Eigen::VectorXd &c, const Eigen::VectorXd &h, const Eigen::VectorXd &b)
        {
            updateData(const_cast<double *>(G.valuePtr()), A.rows() ? const_cast<double *>(A.valuePtr()) : nullptr,
                       const_cast<double *>(c.data()), const_cast<double *>(h.data()), const_cast<double *>(b.data()));
        }
#endif

        exitcode solve(bool verbose = false) // reference include/eicos.hpp:158
        {
            settings_.verbose = verbose;
            int code = EICOS_FATAL;
            { // getSettings() hands out a reference: whatever the caller wrote there since the last solve goes to the handle now
                const eicos_settings c = settings_.to_c();
                if (!same(c, pushed_))
                {
                    if (eicos_batch_set_settings(h_, &c) != EICOS_OK) return exitcode::fatal; // (a refused value: eicos_last_error() names it)
                    pushed_ = c;
                }
            }
            if (eicos_batch_solve(h_, &code) != EICOS_OK) return exitcode::fatal;
            eicos_info raw;
            if (eicos_batch_info(h_, &raw) != EICOS_OK) return exitcode::fatal;
            info_ = Information::from(raw);
            if (x_.size() > 0) eicos_batch_solution(h_, x_.data());
            if (verbose)
                std::printf("EiCOS(MI355X): exit %d after %d iterations, pcost %.9g dcost %.9g pres %.1e dres %.1e gap %.1e\n",
                            code, raw.iter, raw.pcost, raw.dcost, raw.pres, raw.dres, raw.gap);
            return static_cast<exitcode>(code);
        }

        // reference include/eicos.hpp:160: `const Eigen::VectorXd &solution() const` -- a reference to solver-owned
        // storage, valid until the next solve() / destruction.  Same type when Eigen is available; without Eigen
        // (raw-pointer callers only) the storage is a std::vector<double>.
#ifdef EICOS_HAVE_EIGEN
        using SolutionVector = Eigen::VectorXd;
#else
        using SolutionVector = std::vector<double>;
#endif
        const SolutionVector &solution() const { return x_; }
        Settings &getSettings() { return settings_; }
        const Information &getInfo() const { return info_; }
        // Extension (not in the reference, which cold-starts every solve): warm-start the next solves after updateData
        void setWarmStart(double shift) { eicos_batch_set_warm_start(h_, shift); }
        void setDynamicRegularization(double delta, double eps) { eicos_batch_set_dynamic_regularization(h_, delta, eps); }
        // Extension: the retry policy (Retry, above): a solve() that ends in a class of r.mask runs once more inside the same launch.
        // false: refused, eicos_last_error() names the cause
        bool setRetry(const Retry &r)
        {
            const eicos_retry c = r.to_c();
            return eicos_batch_set_retry(h_, &c) == EICOS_OK;
        }
        // Extension: the backup output law (FallbackMap, above) of the handle; it acts in the step calls of eicos_amd.h that hold
        // theta.  false: refused, eicos_last_error() names the cause
        bool setFallbackMap(unsigned mask, const eicos_affine_map *map) { return eicos_batch_set_fallback_map(h_, mask, map) == EICOS_OK; }

    private:
        eicos_batch *h_ = nullptr;
        Settings settings_;
        eicos_settings pushed_ = Settings().to_c(); // what the handle holds: it starts with the defaults
        Information info_;
        SolutionVector x_;
        static bool same(const eicos_settings &a, const eicos_settings &b)
        {
            return a.feastol == b.feastol && a.abstol == b.abstol && a.reltol == b.reltol && a.feastol_inacc == b.feastol_inacc &&
                   a.abstol_inacc == b.abstol_inacc && a.reltol_inacc == b.reltol_inacc && a.linsysacc == b.linsysacc &&
                   a.irerrfact == b.irerrfact && a.iter_max == b.iter_max && a.nitref == b.nitref;
        }
        void resize_solution(int n)
        {
#ifdef EICOS_HAVE_EIGEN
            x_.setZero(n);
#else
            x_.assign((size_t)n, 0.0);
#endif
        }
    };

} // namespace EiCOS
