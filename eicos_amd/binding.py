"""ctypes mirror of include/eicos_amd.h (the C ABI of libeicos_amd.so).

No torch types cross the boundary: host numpy arrays or raw device pointers (ints) only.
If the HIP library is missing or no GPU is visible every compute call raises -- there is no
CPU fallback anywhere in this package.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None

EXIT_NAMES = {0: "optimal", 1: "primal_infeasible", 2: "dual_infeasible", -1: "maxit", -2: "numerics",
              -3: "outcone", -7: "fatal", 10: "close_to_optimal", 11: "close_to_primal_infeasible",
              12: "close_to_dual_infeasible", -87: "not_converged_yet"}
# exit classes (EICOS_SEL_* of include/eicos_amd.h): the mask bits of select() / solve_where(); exit_class(code, n_factor) gives an
# instance's bit.  UNSOLVED (n_factor == 0: never solved, never given a starting point) takes precedence over the code.
SEL_OPTIMAL, SEL_PINF, SEL_DINF, SEL_OPTIMAL_INACC, SEL_PINF_INACC, SEL_DINF_INACC = (1 << k for k in range(6))
SEL_MAXIT, SEL_NUMERICS, SEL_OUTCONE, SEL_FATAL, SEL_OTHER, SEL_UNSOLVED = (1 << k for k in range(6, 12))
SEL_FAILED = SEL_MAXIT | SEL_NUMERICS | SEL_OUTCONE | SEL_FATAL
SEL_ALL = (1 << 12) - 1
SEL_NOT_OPTIMAL = SEL_ALL & ~SEL_OPTIMAL


class Info(C.Structure):
    """struct eicos_info (mirror of EiCOS::Information, reference include/eicos.hpp:49-73)."""
    _fields_ = [(k, C.c_double) for k in (
        "pcost", "dcost", "pres", "dres", "gap", "relgap", "sigma", "mu", "step", "step_aff",
        "kapovert", "pinfres", "dinfres", "tau", "kap")] + [(k, C.c_int) for k in (
        "has_relgap", "has_pinfres", "has_dinfres", "pinf", "dinf", "iter", "nitref1", "nitref2",
        "nitref3", "exitcode", "n_factor", "n_ldlsolve", "n_sweep", "reserved_")] + [("solve_us", C.c_double)]

    def asdict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class Dims(C.Structure):
    _fields_ = [(k, C.c_int) for k in ("n", "m", "p", "l", "ncones", "dim_K", "nnzA", "nnzG", "nnzK", "nnzL",
                                       "nlevels", "order_mode", "batch", "device")] + \
               [("factor_pairs", C.c_longlong), ("inst_bytes", C.c_size_t), ("work_bytes", C.c_size_t),
                ("pattern_bytes", C.c_size_t), ("threads_per_block", C.c_int), ("resident_blocks", C.c_int),
                ("lds_bytes", C.c_int), ("instances_per_block", C.c_int),
                ("lds_resident", C.c_int), ("factor_path", C.c_int), ("cone_order", C.c_int), ("dual_rhs", C.c_int),
                ("arithmetic_profile", C.c_int), ("apex_nodes", C.c_int), ("solo_slices", C.c_int),
                ("shared_operands", C.c_int), ("iterate_park", C.c_int)]

    def asdict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class AffineMap(C.Structure):
    """struct eicos_affine_map: base vector + CSR matrix of one group of a parameter map."""
    _fields_ = [("base", C.POINTER(C.c_double)), ("rowptr", C.POINTER(C.c_int)), ("col", C.POINTER(C.c_int)), ("val", C.POINTER(C.c_double))]


class Settings(C.Structure):
    """struct eicos_settings: the runtime solver settings of a handle (tolerances, iteration cap, refinement)."""
    _fields_ = [(k, C.c_double) for k in ("feastol", "abstol", "reltol", "feastol_inacc", "abstol_inacc", "reltol_inacc",
                                          "linsysacc", "irerrfact")] + [("iter_max", C.c_int), ("nitref", C.c_int)]

    def asdict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


SETTINGS_FIELDS = tuple(k for k, _ in Settings._fields_)


DATA_GRADIENT_KEYS = ("grad_c", "grad_h", "grad_b", "grad_G", "grad_A", "grad_Cval", "grad_Hval", "grad_Bval", "grad_u0", "grad_Uval")


class Retry(C.Structure):
    """struct eicos_retry: the retry policy of a handle (a second attempt inside the solve launch for the exit classes of `mask`)."""
    _fields_ = [("mask", C.c_uint), ("warm", C.c_double), ("dyn_delta", C.c_double), ("dyn_eps", C.c_double), ("settings", Settings)]

    def asdict(self):
        return {"mask": int(self.mask), "warm": self.warm, "dyn": (self.dyn_delta, self.dyn_eps), "settings": self.settings.asdict()}


class DataGradient(C.Structure):
    """eicos_data_gradient: the output pointers of eicos_batch_rollout_data_gradient, NULL = not wanted."""
    _fields_ = [(k, C.c_void_p) for k in DATA_GRADIENT_KEYS]


def library_path() -> str:
    # EICOS_AMD_LIB: alternative build of the same library (used by tuning sweeps only)
    return os.environ.get("EICOS_AMD_LIB") or os.path.join(_HERE, "libeicos_amd.so")


def build_library(force: bool = False) -> str:
    """Compile the HIP library in-tree for gfx950 (hipcc cross-compiles without a GPU)."""
    src = os.path.join(_HERE, "csrc")
    args = ["make", "-C", src] + (["-B"] if force else [])
    subprocess.check_call(args, stdout=subprocess.DEVNULL)
    return library_path()


def _signatures():
    """The C ABI as ctypes sees it, one entry per function of include/eicos_amd.h: (name, argument types[, return type if not int]).
    `eicos_*_name` stands for eicos_batch_name and eicos_multi_name, one argument list (the handle is a void * in both); the multi-GPU
    *_device forms take a source device in front and are entries of their own.  A new entry point is one entry here;
    tests/test_abi_and_symbolic.py holds every entry against the header.  Returns [(full name, argument types, return type)]."""
    i, u, d, size, vp, hp = C.c_int, C.c_uint, C.c_double, C.c_size_t, C.c_void_p, C.POINTER(C.c_void_p)
    dp, ip, fp, infop = C.POINTER(C.c_double), C.POINTER(C.c_int), C.POINTER(C.c_float), C.POINTER(Info)
    mp, sp, rp = C.POINTER(AffineMap), C.POINTER(Settings), C.POINTER(Retry)
    problem = [i] * 4 + [ip] * 5  # n, m, p, ncones, then q, Gjc, Gir, Ajc, Air
    host_check = problem + [u, i, ip]
    table = [
        # process-wide
        ("eicos_set_arithmetic_profile", [i]), ("eicos_get_arithmetic_profile", []), ("eicos_device_count", []), ("eicos_exit_class", [i, i]),
        ("eicos_last_error", [], C.c_char_p), ("eicos_multi_last_error", [], C.c_char_p),
        ("eicos_host_alloc", [size], vp), ("eicos_host_free", [vp]), ("eicos_host_register", [vp, size]), ("eicos_host_unregister", [vp]),
        ("eicos_settings_default", [sp], None), ("eicos_settings_size", [], size), ("eicos_retry_default", [rp], None), ("eicos_retry_size", [], size),
        # handles
        ("eicos_batch_create", [i] * 5 + [ip] * 5 + [i, i, hp]), ("eicos_multi_create", [i] * 5 + [ip] * 5 + [i, ip, i, hp]), ("eicos_*_destroy", [vp]),
        ("eicos_batch_dims", [vp, C.POINTER(Dims)]), ("eicos_batch_kernel_build", [vp]), ("eicos_batch_set_stream", [vp, vp]),
        ("eicos_multi_num_shards", [vp]), ("eicos_multi_shard", [vp, i, hp, ip, ip, ip]),
        # updateData: all five groups, the right-hand sides, theta under the installed maps
        ("eicos_*_update", [vp, i, i] + [dp] * 5), ("eicos_batch_update_device", [vp, i, i] + [vp] * 5), ("eicos_multi_update_device", [vp, i, i, i] + [vp] * 5),
        ("eicos_*_update_rhs", [vp, i, i] + [dp] * 3), ("eicos_batch_update_rhs_device", [vp, i, i] + [vp] * 3), ("eicos_multi_update_rhs_device", [vp, i, i, i] + [vp] * 3),
        ("eicos_*_update_param", [vp, i, i, dp]), ("eicos_batch_update_param_device", [vp, i, i, vp]), ("eicos_multi_update_param_device", [vp, i, i, i, vp]),
        ("eicos_*_update_solve", [vp] + [dp] * 6 + [ip]), ("eicos_*_update_rhs_solve", [vp] + [dp] * 4 + [ip]), ("eicos_*_update_param_solve", [vp, dp, dp, dp, ip]),
        ("eicos_batch_shared_values", [vp]), ("eicos_batch_last_update_path", [vp]),
        # the six maps
        ("eicos_*_set_param_map", [vp, i, mp, mp, mp]), ("eicos_*_param_count", [vp]), ("eicos_*_set_output_map", [vp, i, mp]), ("eicos_*_output_count", [vp]),
        ("eicos_*_set_plant_map", [vp, mp]), ("eicos_*_has_plant_map", [vp]), ("eicos_*_set_shift_map", [vp] + [mp] * 4), ("eicos_*_has_shift_map", [vp]),
        ("eicos_*_set_matrix_map", [vp, mp, mp]), ("eicos_*_has_matrix_map", [vp]), ("eicos_*_matrix_map_count", [vp]),
        ("eicos_*_set_fallback_map", [vp, u, mp]), ("eicos_*_fallback_mask", [vp]), ("eicos_*_fallback_counts", [vp, i, i, ip, i]),
        # starting point, outputs, rollout
        ("eicos_*_set_iterate", [vp, i, i] + [dp] * 4), ("eicos_batch_set_iterate_device", [vp, i, i] + [vp] * 4),
        ("eicos_*_outputs", [vp, i, i, dp]), ("eicos_batch_outputs_device", [vp, i, i, vp]),
        ("eicos_*_rollout", [vp, i] + [dp] * 4 + [ip, ip]), ("eicos_*_rollout_jacobian", [vp, i] + [dp] * 4 + [ip, ip, dp, dp]),
        ("eicos_*_rollout_gradient", [vp] + [dp] * 4), ("eicos_batch_rollout_gradient_device", [vp] + [vp] * 4),
        ("eicos_batch_last_rollout_launches", [vp]), ("eicos_batch_rollout_jacobian_steps", [vp]),
        # per-instance plant values and the gradient with respect to the plant's entries
        ("eicos_*_set_plant_values", [vp, i, i, dp, dp]), ("eicos_batch_set_plant_values_device", [vp, i, i, vp, vp]),
        ("eicos_*_plant_values", [vp, i, i, dp, dp]), ("eicos_*_has_plant_values", [vp]), ("eicos_*_clear_plant_values", [vp]),
        ("eicos_*_rollout_plant_gradient", [vp] + [dp] * 8), ("eicos_batch_rollout_plant_gradient_device", [vp] + [vp] * 8),
        # a recording rollout and the gradient with respect to the controller's own data (the struct of output pointers travels as void *)
        ("eicos_data_gradient_size", [], size), ("eicos_*_set_rollout_recording", [vp, i]), ("eicos_*_rollout_recording", [vp]),
        ("eicos_*_rollout_records", [vp] + [dp] * 6), ("eicos_*_rollout_data_gradient", [vp, dp, dp, dp, vp]),
        ("eicos_batch_rollout_data_gradient_device", [vp, vp, vp, vp, vp]),
        # solve, subset solves, results
        ("eicos_*_solve", [vp, ip]), ("eicos_*_solve_async", [vp]), ("eicos_*_sync", [vp]), ("eicos_*_select", [vp, u, ip, ip]),
        ("eicos_*_solve_subset_async", [vp, ip, i]), ("eicos_*_solve_subset", [vp, ip, i, ip]), ("eicos_*_solve_where", [vp, u, ip, ip, ip]),
        ("eicos_*_gather", [vp, ip, i] + [dp] * 4 + [infop]), ("eicos_*_solution", [vp, dp]), ("eicos_*_duals", [vp, dp, dp, dp]), ("eicos_*_info", [vp, infop]),
        ("eicos_batch_solution_device", [vp, hp, C.POINTER(size)]),
        # the indexed calls
        ("eicos_*_update_indexed", [vp, ip, i] + [dp] * 5), ("eicos_batch_update_indexed_device", [vp, ip, i] + [vp] * 5),
        ("eicos_*_update_rhs_indexed", [vp, ip, i] + [dp] * 3), ("eicos_batch_update_rhs_indexed_device", [vp, ip, i] + [vp] * 3),
        ("eicos_*_update_param_indexed", [vp, ip, i, dp]), ("eicos_batch_update_param_indexed_device", [vp, ip, i, vp]),
        ("eicos_*_set_iterate_indexed", [vp, ip, i] + [dp] * 4), ("eicos_batch_set_iterate_indexed_device", [vp, ip, i] + [vp] * 4),
        ("eicos_*_outputs_indexed", [vp, ip, i, dp]), ("eicos_batch_outputs_indexed_device", [vp, ip, i, vp]),
        ("eicos_*_update_param_solve_subset", [vp, ip, i, dp, dp, dp, ip]),
        # adjoint sensitivities
        ("eicos_*_adjoint", [vp, ip, i, i] + [dp] * 5), ("eicos_*_adjoint_data", [vp, ip, i, i] + [dp] * 7),
        ("eicos_*_output_jacobian", [vp, ip, i, dp, dp]), ("eicos_batch_output_jacobian_device", [vp, ip, i, vp, vp]),
        ("eicos_*_param_jacobian", [vp, ip, i, dp, dp]), ("eicos_batch_param_jacobian_device", [vp, ip, i, vp, vp]),
        ("eicos_*_param_gradient", [vp, ip, i, i, dp, dp, dp]), ("eicos_batch_param_gradient_device", [vp, ip, i, i, vp, vp, vp]),
        ("eicos_*_set_adjoint_scaling", [vp, i]), ("eicos_*_adjoint_scaling", [vp]),
        # policies and timers
        ("eicos_*_set_warm_start", [vp, d]), ("eicos_*_set_dynamic_regularization", [vp, d, d]), ("eicos_*_retry_counts", [vp, i, i, ip, i]),
        ("eicos_*_set_settings", [vp, sp]), ("eicos_*_get_settings", [vp, sp]), ("eicos_*_set_retry", [vp, rp]), ("eicos_*_get_retry", [vp, rp]),
        ("eicos_batch_last_solve_ms", [vp, fp]), ("eicos_multi_last_solve_ms", [vp, fp, fp]), ("eicos_batch_last_update_ms", [vp, fp]),
        ("eicos_batch_last_adjoint_ms", [vp, fp]), ("eicos_batch_ms_history", [vp, i, fp, i]),
        # the single-instance form (include/ecos.h sits on it; Python does not call it)
        ("eicos_create", [i] * 5 + [ip, dp, ip, ip, dp, ip, ip, dp, dp, dp, i, hp]), ("eicos_update", [vp] + [dp] * 5), ("eicos_solve", [vp, ip]),
        ("eicos_solution", [vp, dp]), ("eicos_info_get", [vp, infop]), ("eicos_destroy", [vp]),
        # debug
        ("eicos_debug_factor", [vp, i, dp, dp]), ("eicos_debug_pattern", [vp, ip, ip, ip]), ("eicos_debug_trace", [vp, i, dp]),
        ("eicos_debug_kkt", [vp, i, ip, ip, dp]), ("eicos_debug_scalings", [vp, i, dp, dp, dp, ip]), ("eicos_debug_host_tile_order", problem + [i] + [ip] * 5),
        ("eicos_debug_host_check", host_check, d), ("eicos_debug_host_check_tiles", host_check, d), ("eicos_debug_host_check_hybrid", host_check, d),
        # the HIP runtime the library is linked against, as _device_form uses it
        ("hipMalloc", [hp, size]), ("hipMemcpy", [vp, vp, size, i]), ("hipFree", [vp]),
    ]
    return [(full, args, ret[0] if ret else i) for name, args, *ret in table
            for full in ((name.replace("*", "batch"), name.replace("*", "multi")) if "*" in name else (name,))]


_SIGNATURES = _signatures()


def _lib():
    global _LIB
    if _LIB is None:
        path = library_path()
        if not os.path.exists(path):
            raise RuntimeError(f"{path} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                               "(there is no CPU fallback)")
        L = C.CDLL(path)
        found = set()
        for name, args, restype in _SIGNATURES:
            fn = getattr(L, name, None)
            if fn is not None:  # (an older library -- EICOS_AMD_LIB A/B runs, bench.py's prev_round leg -- lacks some: calling one fails at the call)
                fn.argtypes, fn.restype = args, restype
                found.add(name)
        if "eicos_settings_size" in found and L.eicos_settings_size() != C.sizeof(Settings):
            raise RuntimeError(f"{path}: struct eicos_settings has {L.eicos_settings_size()} bytes, the ctypes mirror {C.sizeof(Settings)}")
        if "eicos_retry_size" in found and L.eicos_retry_size() != C.sizeof(Retry):
            raise RuntimeError(f"{path}: struct eicos_retry has {L.eicos_retry_size()} bytes, the ctypes mirror {C.sizeof(Retry)}")
        if "eicos_data_gradient_size" in found and L.eicos_data_gradient_size() != C.sizeof(DataGradient):
            raise RuntimeError(f"{path}: struct eicos_data_gradient has {L.eicos_data_gradient_size()} bytes, the ctypes mirror {C.sizeof(DataGradient)}")
        _LIB = L
    return _LIB


def set_arithmetic_profile(profile: int) -> None:
    """0 (default): plans shaped by the launch; 1: by the pattern alone -- batch- and shard-independent bits (eicos_set_arithmetic_profile)."""
    _chk(_lib().eicos_set_arithmetic_profile(int(profile)))


def default_settings() -> dict:
    """The ten runtime settings at their defaults (eicos_settings_default: the reference's values); needs no GPU."""
    st = Settings()
    _lib().eicos_settings_default(C.byref(st))
    return st.asdict()


def default_retry() -> dict:
    """The retry policy that is no policy (eicos_retry_default: mask 0, cold, no regularisation, default settings); needs no GPU."""
    r = Retry()
    _lib().eicos_retry_default(C.byref(r))
    return r.asdict()


def exit_class(exitcode: int, n_factor: int = 1) -> int:
    """The SEL_* bit of an instance with this exit code and n_factor (eicos_exit_class: the function the selection kernel runs on the
    GPU); needs no handle and no GPU."""
    return int(_lib().eicos_exit_class(int(exitcode), int(n_factor)))


def device_count() -> int:
    return int(_lib().eicos_device_count())


def _chk(rc):
    if rc != 0:
        raise RuntimeError(f"eicos_amd error {rc}: {_lib().eicos_last_error().decode()}")


def _ip(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_int))


def _dp(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))


# How an array travels when it may be None or empty.  A pointer made by _ip / _dp keeps its array alive, dummies included.
def _dp_or_dummy(a):
    """None as NULL; an empty array as a pointer to a one-element dummy (the library gets a valid address)."""
    return _dp(a if a is None or a.size else np.zeros(1))


def _ip_or_dummy(a):
    return _ip(a if a is None or a.size else np.zeros(1, np.int32))


def _dp_or_null(a):
    """None and an empty array as NULL."""
    return _dp(a) if (a is not None and a.size) else None


def _dev(*addresses):
    """Raw device addresses (ints) as void pointers; 0 as NULL."""
    return [C.c_void_p(int(p) or None) for p in addresses]


def _nonneg(v):
    """The value of a call that returns a count or a flag, or a negative error code (raised)."""
    if v < 0:
        _chk(v)
    return v


def _info_columns(arr, count):
    """The first `count` records of an Info array as a dict of arrays, one per field in declaration order."""
    raw = np.frombuffer(arr, dtype=np.dtype([(k, "f8" if t is C.c_double else "i4") for k, t in Info._fields_]))[:count]
    return {k: raw[k].copy() for k in raw.dtype.names}


# the cone scaling of the adjoint's K (EICOS_ADJOINT_* of include/eicos_amd.h)
ADJOINT_NT, ADJOINT_CENTRED = 0, 1
ADJOINT_SCALINGS = {"nt": ADJOINT_NT, "centred": ADJOINT_CENTRED}


def centred_pair(pat, s, z):
    """The pair (s, z) [m] the centred adjoint scaling is formed from (EICOS_ADJOINT_CENTRED; include/eicos_amd.h): per second-order
    cone, in the Jordan frame (1, +-u) that s and z share, the larger eigenvalue of each complementary pair (l1, w1), (l2, w2) is kept
    and the smaller one replaced so that l1 w1 = l2 w2 = sqrt(l1 w1 l2 w2).  LP rows, cones of dimension 1, cones whose s and z are
    parallel and cones with an eigenvalue <= 0 are returned as they are.  The numpy restatement of what adjoint_instance does on the
    un-equilibrated result rows; returns new arrays."""
    s, z = np.array(s, dtype=np.float64), np.array(z, dtype=np.float64)
    o = pat.l
    for d in (int(v) for v in pat.q):
        sc, zc = s[o:o + d], z[o:o + d]
        o += d
        if d == 1:
            continue
        v = sc[1:] / sc[0] - zc[1:] / zc[0]
        nv = np.sqrt(v @ v)
        if not nv > 0.0:
            continue
        u = v / nv
        su, zu = sc[1:] @ u, zc[1:] @ u
        l1, l2, w1, w2 = sc[0] + su, sc[0] - su, zc[0] + zu, zc[0] - zu
        if not min(l1, l2, w1, w2) > 0.0:
            continue
        mu = np.sqrt(l1 * w1 * l2 * w2)
        if l1 >= w1:
            w1 = mu / l1
        else:
            l1 = mu / w1
        if l2 >= w2:
            w2 = mu / l2
        else:
            l2 = mu / w2
        sc[0], sc[1:] = 0.5 * (l1 + l2), 0.5 * (l1 - l2) * u
        zc[0], zc[1:] = 0.5 * (w1 + w2), 0.5 * (w1 - w2) * u
    return s, z


def _known_settings(who, fields):
    """TypeError for a name that is no field of eicos_settings."""
    unknown = sorted(set(fields) - set(SETTINGS_FIELDS))
    if unknown:
        raise TypeError(f"{who}: unknown field(s) {', '.join(unknown)} (the settings are {', '.join(SETTINGS_FIELDS)})")


def _assign_settings(st, fields):
    for k, v in fields.items():
        setattr(st, k, int(v) if k in ("iter_max", "nitref") else float(v))


class PinnedArray:
    """A float64 array in pinned host memory (eicos_host_alloc): `.a` is the numpy view.  updateData reads such arrays in place over PCIe
    (no bounce copy), solution() / duals() write into them with one strided copy.  Freed by close() or with the object."""

    def __init__(self, shape):
        shape = tuple(int(v) for v in (shape if hasattr(shape, "__len__") else (shape,)))
        n = int(np.prod(shape)) if shape else 1
        self._p = _lib().eicos_host_alloc(max(n, 1) * 8)
        if not self._p:
            raise RuntimeError("eicos_host_alloc failed: " + _lib().eicos_last_error().decode())
        self.a = np.ctypeslib.as_array(C.cast(self._p, C.POINTER(C.c_double)), shape=(max(n, 1),))[:n].reshape(shape)

    def close(self):
        if getattr(self, "_p", None):
            self.a = None
            _lib().eicos_host_free(self._p)
            self._p = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def host_register(a):
    """Pin a C-contiguous float64 numpy array IN PLACE (eicos_host_register): updateData then reads it over PCIe without a bounce copy.
    Keep the array alive and call host_unregister(a) before it is freed."""
    assert a.dtype == np.float64 and a.flags.c_contiguous
    _chk(_lib().eicos_host_register(C.c_void_p(a.ctypes.data), a.nbytes))
    return a


def host_unregister(a):
    _chk(_lib().eicos_host_unregister(C.c_void_p(a.ctypes.data)))


def _group_ptrs(groups, widths, count):
    """Any subset of the input groups as (keep-alive arrays, C pointers): contiguous float64 [count, width] each, sizes checked; None keeps
    a group (NULL)."""
    arrs, ptrs = [], []
    for a, w in zip(groups, widths):
        if a is not None:
            a = np.ascontiguousarray(a, dtype=np.float64)
            if a.size != count * w:
                raise ValueError(f"array has {a.size} elements, expected {count}x{w}")
        arrs.append(a)
        ptrs.append(_dp_or_dummy(a))  # (zero-width groups: NULL-safe dummies)
    return arrs, ptrs


def _rhs_ptrs(pat, count, c, h, b):
    """c, h, b as C pointers for a right-hand-side-only update of `count` instances (None keeps the group; sizes checked)."""
    return _group_ptrs((c, h, b), (pat.n, pat.m, pat.p), count)


def _as_group(g):
    """One group `(base, rowptr, col, val)` of an affine map -- base vector and CSR matrix -- as contiguous float64 / int32 / int32 /
    float64 arrays; None (no such group) passes."""
    if g is None:
        return None
    return (np.ascontiguousarray(g[0], np.float64), np.ascontiguousarray(g[1], np.int32), np.ascontiguousarray(g[2], np.int32),
            np.ascontiguousarray(g[3], np.float64))


def _affine_eval(group, v, base_i=None, val_i=None):
    """base + M v for the rows of v [B, columns]: [B, rows].  Row r: acc = base[r], then for every stored entry t of the row, in stored
    order, acc = acc + (val[t] * v[col[t]]) -- the product and the sum each rounded to float64 (numpy has no fused multiply-add).  This
    is the rounding order every map keeps on the GPU; the evaluate() of all five map classes is this function.
    base_i [B, rows] / val_i [B, stored entries] (the plant map's per-instance values): row b of them stands in for base / val in
    row b of the result, the same arithmetic."""
    base, rowptr, col, val = group
    acc = np.repeat(base[None, :], v.shape[0], axis=0) if base_i is None else base_i.copy()
    length = np.diff(rowptr)
    for j in range(int(length.max()) if length.size else 0):  # entry j of every row that has one
        rows = np.nonzero(length > j)[0]
        t = rowptr[rows] + j
        acc[:, rows] = acc[:, rows] + (val[t][None, :] if val_i is None else val_i[:, t]) * v[:, col[t]]
    return acc


def _affine_ptr(group, rows, who, what, fits=True):
    """One group as (keep-alive objects, C pointer to eicos_affine_map), (None, None) for None.  The array sizes are checked here --
    ValueError `who`base[..], rowptr[..], col[..], val[..] do not describe `what`, also when the caller's own condition `fits` fails --,
    their contents (row pointers, column range, what the pattern and the handle must have) by the library."""
    if group is None:
        return None, None
    base, rowptr, col, val = group
    if not fits or base.size != rows or rowptr.size != rows + 1 or col.size != val.size or rowptr[-1] > col.size:
        raise ValueError(f"{who}base[{base.size}], rowptr[{rowptr.size}], col[{col.size}], val[{val.size}] do not describe {what}")
    one = np.zeros(1)
    m = AffineMap(_dp(base if base.size else one), _ip(rowptr), _ip(col if col.size else np.zeros(1, np.int32)), _dp(val if val.size else one))
    return (m, one), C.pointer(m)


def _affine_ptrs(groups):
    """_affine_ptr over (group, rows, who, what) tuples: (keep-alive objects, [C pointer or None per group])."""
    pairs = [_affine_ptr(*g) for g in groups]
    return [k for k, _ in pairs], [p for _, p in pairs]


class ParamMap:
    """Right-hand sides affine in a parameter row theta of length k: c = c0 + C theta, h = h0 + H theta, b = b0 + B theta.  Per group
    `(base, rowptr, col, val)` -- base vector and CSR matrix with k columns -- or None: that group is not parametric (an update keeps it).
    evaluate() is the host restatement of what update_param computes on the GPU, in the same rounding order."""

    def __init__(self, k: int, c=None, h=None, b=None):
        self.k = int(k)
        self.c, self.h, self.b = _as_group(c), _as_group(h), _as_group(b)

    def groups(self):
        return self.c, self.h, self.b

    def evaluate(self, theta):
        """(c, h, b) for theta [B, k]: arrays [B, rows], None for a group without a map, in the order of eicos_batch_update_param
        (_affine_eval)."""
        theta = _theta_rows(theta, self.k, None)[0]
        return tuple(None if g is None else _affine_eval(g, theta) for g in self.groups())


def _param_map_ptrs(pmap, pat):
    """A ParamMap as (keep-alive structs, [c, h, b] as C pointers to eicos_affine_map or None)."""
    return _affine_ptrs((g, rows, f"parameter map of {name}: ", f"{rows} rows") for name, g, rows in zip("chb", pmap.groups(), (pat.n, pat.m, pat.p)))


class OutputMap:
    """The numbers of x a controller applies, u = u0 + U x with u of length r: `(base, rowptr, col, val)` -- base[r] and a CSR matrix with
    n columns -- shared by all instances.  evaluate() is the host restatement of what outputs() / update_param_solve compute on the GPU,
    in the same rounding order."""

    def __init__(self, n: int, u):
        self.n = int(n)
        self.base, self.rowptr, self.col, self.val = _as_group(u)
        self.r = int(self.base.size)

    def evaluate(self, x):
        """u [B, r] for x [B, n], in the order of eicos_batch_outputs (_affine_eval)."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        if x.ndim != 2 or x.shape[1] != self.n:
            raise ValueError(f"x has shape {x.shape}, expected [count, {self.n}]")
        return _affine_eval((self.base, self.rowptr, self.col, self.val), x)


def _output_map_ptr(omap, pat):
    """An OutputMap as (keep-alive objects, C pointer to eicos_affine_map)."""
    return _affine_ptr((omap.base, omap.rowptr, omap.col, omap.val), omap.r, f"output map: n = {omap.n}, ",
                       f"{omap.r} rows over {pat.n} variables", omap.n == pat.n)


def _cotangent(a, shape, name):
    """A cotangent array of a rollout (None passes through) as contiguous float64 of exactly `shape`."""
    if a is None:
        return None
    a = np.ascontiguousarray(a, dtype=np.float64)
    if a.shape != tuple(shape):
        raise ValueError(f"{name} has shape {a.shape}, expected {list(shape)}")
    return a


class PlantMap:
    """The simulated plant of a closed loop, theta+ = f0 + F [theta | u] (+ w): `(base, rowptr, col, val)` -- base[k] and a CSR matrix
    with k rows whose columns index z = [theta (k) | u (r)], i.e. lie in [0, k + r) -- shared by all instances.  evaluate() is the host
    restatement of what rollout() computes on the GPU between two steps, in the same rounding order."""

    def __init__(self, k: int, r: int, f):
        self.k, self.r = int(k), int(r)
        self.base, self.rowptr, self.col, self.val = _as_group(f)

    def nnz(self) -> int:
        """Stored entries of F the map uses: rowptr[k]."""
        return int(self.rowptr[-1])

    def _instance_values(self, B, f0, val):
        """The per-instance values of a call as contiguous float64 [B, k] / [B, nnz] (None passes); ValueError otherwise."""
        out = []
        for name, a, width in (("f0", f0, self.k), ("val", val, self.nnz())):
            if a is not None:
                a = np.ascontiguousarray(a, dtype=np.float64)
                if a.shape != (B, width):
                    raise ValueError(f"{name} has shape {a.shape}, expected [{B}, {width}] (one row per instance)")
            out.append(a)
        return out

    def evaluate(self, theta, u, w=None, f0=None, val=None):
        """theta+ [B, k] for theta [B, k], u [B, r] and, optionally, the disturbance w [B, k]: the map over z = [theta | u]
        (_affine_eval), then acc = acc + w[j], one more rounded sum -- the order of eicos_batch_rollout.  f0 [B, k] / val [B, nnz]
        (eicos_batch_set_plant_values): row b of them in the place of base / val for instance b, the same arithmetic; None: the
        shared values."""
        theta, u = _theta_rows(theta, self.k, None)[0], np.ascontiguousarray(u, dtype=np.float64)
        if u.shape != (theta.shape[0], self.r):
            raise ValueError(f"u has shape {u.shape}, expected [{theta.shape[0]}, {self.r}]")
        if w is not None:
            w = np.ascontiguousarray(w, dtype=np.float64)
            if w.shape != theta.shape:
                raise ValueError(f"w has shape {w.shape}, expected {theta.shape}")
        f0, val = self._instance_values(theta.shape[0], f0, val)
        acc = _affine_eval((self.base, self.rowptr, self.col, self.val), np.concatenate((theta, u), axis=1), f0, val)
        return acc if w is None else acc + w

    def backprop(self, J, gu=None, gtheta=None, val=None):
        """(grad_theta0 [B, k], grad_w [B, T, k]): the gradient of L = sum_t gu_t' u_t + sum_t gtheta_t' theta_t over a rollout with
        the step Jacobians J [B, T, r, k] (rollout_jacobian) -- gu [B, T, r] and gtheta [B, T + 1, k], each optional, one must be
        given.  The scalar loop of eicos_batch_rollout_gradient in its stated order, every product and sum rounded on its own; a
        missing cotangent counts as 0.0 and is still added.  A NaN row of J makes that instance's gradient NaN.  val [B, nnz]: the
        per-instance values the rollout ran under (None: the shared ones)."""
        return self._sweep(J, gu, gtheta, val, None, None)[:2]

    def backprop_values(self, J, u, theta, gu=None, gtheta=None, val=None):
        """(grad_theta0 [B, k], grad_w [B, T, k], grad_f0 [B, k], grad_val [B, nnz]): backprop() that also returns the gradient with
        respect to the plant's own entries, per instance -- u [B, T, r] and theta [B, T + 1, k] the trajectories of the rollout, which
        the plant read.  The scalar loop of eicos_batch_rollout_plant_gradient in its stated order: before the recursion of step t,
        grad_f0[i] = grad_f0[i] + lambda[i] and grad_val[s] = grad_val[s] + (lambda[row(s)] * z_t[col[s]]), z_t = [theta_t | u_t];
        after step 0, 0.0 * grad_theta0[row] is added to every entry, so that a NaN of J_0 reaches them as those of later steps do.
        For the shared plant sum the rows over the batch."""
        k, r = self.k, self.r
        J = np.ascontiguousarray(J, dtype=np.float64)
        if J.ndim != 4:
            raise ValueError(f"J has shape {J.shape}, expected [batch, steps, {r}, {k}]")
        B, T = int(J.shape[0]), int(J.shape[1])
        u, theta = _cotangent(u, (B, T, r), "u"), _cotangent(theta, (B, T + 1, k), "theta")
        if u is None or theta is None:
            raise ValueError("u and theta (the trajectories of the rollout) are both needed")
        return self._sweep(J, gu, gtheta, val, u, theta)

    def _sweep(self, J, gu, gtheta, val_i, u, theta):
        k, r = self.k, self.r
        J = np.ascontiguousarray(J, dtype=np.float64)
        if J.ndim != 4 or J.shape[2:] != (r, k):
            raise ValueError(f"J has shape {J.shape}, expected [batch, steps, {r}, {k}]")
        B, T = int(J.shape[0]), int(J.shape[1])
        if gu is None and gtheta is None:
            raise ValueError("gu and gtheta are both None")
        gu, gtheta = _cotangent(gu, (B, T, r), "gu"), _cotangent(gtheta, (B, T + 1, k), "gtheta")
        val_i = self._instance_values(B, None, val_i)[1]
        rowptr, col = self.rowptr, self.col
        nnz = self.nnz()
        g0, gw = np.zeros((B, k)), np.zeros((B, T, k))
        gf0, gval = np.zeros((B, k)), np.zeros((B, nnz))
        zero = np.float64(0.0)
        for b in range(B):
            val = self.val if val_i is None else val_i[b]
            lam = [gtheta[b, T, c] if gtheta is not None else zero for c in range(k)]
            for t in range(T - 1, -1, -1):
                if u is not None:
                    z = [theta[b, t, c] for c in range(k)] + [u[b, t, j] for j in range(r)]
                    for i in range(k):
                        gf0[b, i] = gf0[b, i] + lam[i]
                        for s in range(int(rowptr[i]), int(rowptr[i + 1])):
                            gval[b, s] = gval[b, s] + (lam[i] * z[col[s]])
                gw[b, t, :] = lam
                v = [zero] * (k + r)
                for i in range(k):
                    for s in range(int(rowptr[i]), int(rowptr[i + 1])):
                        v[col[s]] = v[col[s]] + (val[s] * lam[i])
                mu = [(gu[b, t, j] if gu is not None else zero) + v[k + j] for j in range(r)]
                new = []
                for c in range(k):
                    acc = (gtheta[b, t, c] if gtheta is not None else zero) + v[c]
                    for j in range(r):
                        acc = acc + (J[b, t, j, c] * mu[j])
                    new.append(acc)
                lam = new
            g0[b, :] = lam
            if u is not None:
                with np.errstate(invalid="ignore"):
                    for i in range(k):
                        poison = zero * lam[i]
                        gf0[b, i] = gf0[b, i] + poison
                        for s in range(int(rowptr[i]), int(rowptr[i + 1])):
                            gval[b, s] = gval[b, s] + poison
        return g0, gw, gf0, gval


def _dense_rows(omap):
    """The rows of an OutputMap as a dense [r, n] block, formed as the contracted adjoint forms its right-hand sides: zero-filled, then
    the entries of a column summed in stored order."""
    U = np.zeros((omap.r, omap.n))
    for a in range(omap.r):
        for t in range(int(omap.rowptr[a]), int(omap.rowptr[a + 1])):
            U[a, omap.col[t]] = U[a, omap.col[t]] + omap.val[t]
    return U


def rollout_data_backprop(pattern, pmap, omap, fmap, J, W, x, y, z, theta, gu=None, gtheta=None, val=None, want=DATA_GRADIENT_KEYS):
    """The host restatement of eicos_batch_rollout_data_gradient, bit for bit: the gradient of L = sum_t gu_t' u_t + sum_t gtheta_t'
    theta_t with respect to the controller's own data, per instance, as a dict over `want` (DATA_GRADIENT_KEYS).  pattern: the Pattern
    (Gjc, Gir, Ajc, Air give the (row, column) of every stored value); pmap / omap / fmap: the ParamMap, OutputMap and PlantMap of the
    rollout; J [B, T, r, k] what rollout_jacobian returned; W = (Wc [B, T, r, n], Wh [B, T, r, m], Wb [B, T, r, p]) and x [B, T, n],
    y [B, T, p], z [B, T, m] its records (rollout_records); theta [B, T + 1, k] its theta trajectory; val [B, nnzF]: the per-instance
    plant values it ran under.  mu_t is PlantMap.backprop's; behind it, for t = T-1 .. 0, every product and sum rounded on its own:
    d[i] = 0.0, then d[i] + (mu_t[a] * W_t[a][i]) for a ascending; grad_c[i] + d_c[i]; grad_Cval[s] + (d_c[i] * theta_t[col[s]]);
    grad_G[e] + ((d_c[j] * z_t[i]) - (d_h[i] * x_t[j])), grad_A with y_t and d_b; grad_u0[a] + mu_t[a]; grad_Uval[s] + (mu_t[row(s)] *
    x_t[col[s]]).  A NaN row of W makes the sums it enters NaN; other instances are untouched."""
    k, r = fmap.k, fmap.r
    J = np.ascontiguousarray(J, dtype=np.float64)
    if J.ndim != 4 or J.shape[2:] != (r, k):
        raise ValueError(f"J has shape {J.shape}, expected [batch, steps, {r}, {k}]")
    B, T = int(J.shape[0]), int(J.shape[1])
    n, m, p = int(pattern.n), int(pattern.m), int(pattern.p)
    if omap.r != r or omap.n != n or pmap.k != k:
        raise ValueError(f"the maps do not fit: output map {omap.r} x {omap.n}, parameter map k = {pmap.k}, plant map (k, r) = ({k}, {r}), n = {n}")
    if gu is None and gtheta is None:
        raise ValueError("gu and gtheta are both None")
    gu, gtheta = _cotangent(gu, (B, T, r), "gu"), _cotangent(gtheta, (B, T + 1, k), "gtheta")
    theta = _cotangent(theta, (B, T + 1, k), "theta")
    if theta is None or W is None or len(W) != 3:
        raise ValueError("theta and W = (Wc, Wh, Wb) are needed")
    W = [_cotangent(a, (B, T, r, w), name) for a, w, name in zip(W, (n, m, p), ("Wc", "Wh", "Wb"))]
    x, y, z = _cotangent(x, (B, T, n), "x"), _cotangent(y, (B, T, p), "y"), _cotangent(z, (B, T, m), "z")
    if any(a is None for a in W + [x, y, z]):
        raise ValueError("Wc, Wh, Wb, x, y and z (rollout_records) are all needed")
    unknown = [q for q in want if q not in DATA_GRADIENT_KEYS]
    if unknown or not want:
        raise ValueError(f"want must name some of {DATA_GRADIENT_KEYS}, got {tuple(want)}")
    groups = pmap.groups()
    for q, name in enumerate(("grad_Cval", "grad_Hval", "grad_Bval")):
        if name in want and groups[q] is None:
            raise ValueError(f"{name} asked, but the parameter map has no {'chb'[q]} group")
    val_i = fmap._instance_values(B, None, val)[1]
    Gcol = np.repeat(np.arange(n), np.diff(pattern.Gjc)) if pattern.nnzG else np.zeros(0, np.int64)
    Acol = np.repeat(np.arange(n), np.diff(pattern.Ajc)) if pattern.nnzA else np.zeros(0, np.int64)
    Gir, Air = np.asarray(pattern.Gir, np.int64)[:pattern.nnzG], np.asarray(pattern.Air, np.int64)[:pattern.nnzA]
    Urow = np.repeat(np.arange(r), np.diff(omap.rowptr[:r + 1]))
    nnzU = int(omap.rowptr[r])
    Ucol = np.asarray(omap.col[:nnzU], np.int64)
    rows_of = [None if g is None else np.repeat(np.arange(w), np.diff(g[1][:w + 1])) for g, w in zip(groups, (n, m, p))]
    out = {"grad_c": np.zeros((B, n)), "grad_h": np.zeros((B, m)), "grad_b": np.zeros((B, p)), "grad_G": np.zeros((B, pattern.nnzG)),
           "grad_A": np.zeros((B, pattern.nnzA)), "grad_u0": np.zeros((B, r)), "grad_Uval": np.zeros((B, nnzU))}
    for q, name in enumerate(("grad_Cval", "grad_Hval", "grad_Bval")):
        out[name] = np.zeros((B, 0 if groups[q] is None else int(groups[q][1][(n, m, p)[q]])))
    rowptr, col = fmap.rowptr, fmap.col
    zero = np.float64(0.0)
    with np.errstate(invalid="ignore"):
        for b in range(B):
            fval = fmap.val if val_i is None else val_i[b]
            lam = [gtheta[b, T, c] if gtheta is not None else zero for c in range(k)]
            for t in range(T - 1, -1, -1):
                v = [zero] * (k + r)
                for i in range(k):
                    for s in range(int(rowptr[i]), int(rowptr[i + 1])):
                        v[col[s]] = v[col[s]] + (fval[s] * lam[i])
                mu = np.array([(gu[b, t, j] if gu is not None else zero) + v[k + j] for j in range(r)])
                d = []
                for Wg, w in zip(W, (n, m, p)):
                    acc = np.zeros(w)
                    for a in range(r):
                        acc = acc + (mu[a] * Wg[b, t, a])
                    d.append(acc)
                for q, name in enumerate(("grad_c", "grad_h", "grad_b")):
                    out[name][b] = out[name][b] + d[q]
                for q, name in enumerate(("grad_Cval", "grad_Hval", "grad_Bval")):
                    if groups[q] is not None and out[name].shape[1]:
                        nz = out[name].shape[1]
                        out[name][b] = out[name][b] + (d[q][rows_of[q]] * theta[b, t, groups[q][2][:nz]])
                out["grad_G"][b] = out["grad_G"][b] + ((d[0][Gcol] * z[b, t, Gir]) - (d[1][Gir] * x[b, t, Gcol]))
                out["grad_A"][b] = out["grad_A"][b] + ((d[0][Acol] * y[b, t, Air]) - (d[2][Air] * x[b, t, Acol]))
                out["grad_u0"][b] = out["grad_u0"][b] + mu
                out["grad_Uval"][b] = out["grad_Uval"][b] + (mu[Urow] * x[b, t, Ucol])
                new = []
                for c in range(k):
                    acc = (gtheta[b, t, c] if gtheta is not None else zero) + v[c]
                    for j in range(r):
                        acc = acc + (J[b, t, j, c] * mu[j])
                    new.append(acc)
                lam = new
    return {q: out[q] for q in want}


def _plant_map_ptr(fmap, k, r):
    """A PlantMap as (keep-alive objects, C pointer to eicos_affine_map) for a handle with k parameters and r outputs."""
    return _affine_ptr((fmap.base, fmap.rowptr, fmap.col, fmap.val), k, f"plant map: k = {fmap.k}, r = {fmap.r}, ",
                       f"{k} rows over {k} parameters and {r} outputs", fmap.k == k and fmap.r == r)


class FallbackMap:
    """The backup output law of a closed loop, u = v0 + V theta: `v0` [r] and `V` = `(rowptr, col, val)`, a CSR matrix with r rows and k
    columns, shared by all instances, with `mask`, an OR of SEL_* bits -- a step whose final record falls in one of these exit classes
    takes its u row from this law instead of from the output map (eicos_batch_set_fallback_map).  evaluate() is the host restatement
    of what such a step computes on the GPU, in the same rounding order."""

    def __init__(self, v0, V, mask: int, k: int | None = None):
        self.base, self.rowptr, self.col, self.val = _as_group((v0, *V))
        self.r, self.mask = int(self.base.size), int(mask)
        self.k = int(k) if k is not None else (int(self.col.max()) + 1 if self.col.size else 0)

    def evaluate(self, theta):
        """u [B, r] for theta [B, k]: row j is acc = v0[j], then acc = acc + (val[t] * theta[col[t]]) over the row's entries in stored
        order, numpy float64 scalars throughout -- the product and the sum each rounded on their own."""
        theta = np.ascontiguousarray(theta, dtype=np.float64)
        if theta.ndim != 2 or theta.shape[1] != self.k:
            raise ValueError(f"theta has shape {theta.shape}, expected [count, {self.k}]")
        u = np.zeros((theta.shape[0], self.r))
        for b in range(theta.shape[0]):
            for j in range(self.r):
                acc = self.base[j]
                for t in range(int(self.rowptr[j]), int(self.rowptr[j + 1])):
                    acc = acc + (self.val[t] * theta[b, self.col[t]])
                u[b, j] = acc
        return u

    def dense(self, k: int | None = None):
        """V as the dense [r, k] block a fired step of rollout_jacobian records: zero-filled, then J[j, col[t]] = J[j, col[t]] + val[t]
        in stored order (duplicates of a column accumulate in that order)."""
        J = np.zeros((self.r, self.k if k is None else int(k)))
        for j in range(self.r):
            for t in range(int(self.rowptr[j]), int(self.rowptr[j + 1])):
                J[j, self.col[t]] = J[j, self.col[t]] + self.val[t]
        return J


def _fallback_map_ptr(fmap, k, r):
    """A FallbackMap as (keep-alive objects, C pointer to eicos_affine_map) for a handle with k parameters and r outputs."""
    return _affine_ptr((fmap.base, fmap.rowptr, fmap.col, fmap.val), r, f"fallback map: r = {fmap.r}, ",
                       f"{r} rows over {k} parameters", fmap.r == r)


class MatrixMap:
    """The stored values of G and A affine in the parameter row theta of length k: Gpr = G0 + Gm theta, Apr = A0 + Am theta.  Per matrix
    `(base, rowptr, col, val)` -- base[nnz] and a CSR matrix with one row per stored value (CSC order of Gpr / Apr) and k columns -- or
    None: that matrix is not mapped (an update keeps and re-equilibrates it).  evaluate() is the host restatement of what a parametric
    update forms on the GPU under the map, in the same rounding order."""

    def __init__(self, k: int, G=None, A=None):
        self.k = int(k)
        self.G, self.A = _as_group(G), _as_group(A)

    def groups(self):
        return self.G, self.A

    def evaluate(self, theta):
        """(Gpr, Apr) for theta [B, k]: arrays [B, nnz], None for a matrix without a map, in the order of eicos_batch_set_matrix_map
        (_affine_eval)."""
        theta = _theta_rows(theta, self.k, None)[0]
        return tuple(None if g is None else _affine_eval(g, theta) for g in self.groups())


def _matrix_map_ptrs(mmap, nnzG, nnzA):
    """A MatrixMap as (keep-alive structs, [G, A] as C pointers to eicos_affine_map or None)."""
    return _affine_ptrs((g, rows, f"matrix map of {name}: ", f"{rows} stored values") for name, g, rows in zip("GA", mmap.groups(), (nnzG, nnzA)))


class ShiftMap:
    """The warm start of a re-solve moved by an affine map: per vector x, y, z, s `(base, rowptr, col, val)` -- base[rows] and a SQUARE CSR
    matrix with rows = n, p, m, m -- or None: that vector is not shifted.  Installed with set_shift_map, a solve that warm-starts an
    instance first replaces its vectors by the shifted ones (the receding-horizon shift: stage t + 1 becomes stage t).  evaluate() is the
    host restatement of what the solve kernel computes, in the same rounding order."""

    def __init__(self, n: int, p: int, m: int, x=None, y=None, z=None, s=None):
        self.n, self.p, self.m = int(n), int(p), int(m)
        self.x, self.y, self.z, self.s = _as_group(x), _as_group(y), _as_group(z), _as_group(s)

    @classmethod
    def from_sources(cls, n: int, p: int, m: int, x_src=None, y_src=None, z_src=None, s_src=None):
        """The pure permutation / duplication shift: row j of a group copies entry src[j] of the same vector (base 0, one stored value
        1.0 per row); None leaves the group unshifted."""
        def group(src, rows, name):
            if src is None:
                return None
            src = np.ascontiguousarray(src, dtype=np.int32)
            if src.shape != (rows,):
                raise ValueError(f"{name}_src has shape {src.shape}, expected [{rows}]")
            return np.zeros(rows), np.arange(rows + 1, dtype=np.int32), src, np.ones(rows)
        return cls(n, p, m, group(x_src, n, "x"), group(y_src, p, "y"), group(z_src, m, "z"), group(s_src, m, "s"))

    def groups(self):
        return self.x, self.y, self.z, self.s

    def rows(self):
        return self.n, self.p, self.m, self.m

    def evaluate(self, x=None, y=None, z=None, s=None):
        """(x', y', z', s') for vectors [B, rows]: a group without a map (or not given) comes back as it was passed; a mapped one goes
        through its map as it was BEFORE the shift, in the order of eicos_batch_set_shift_map (_affine_eval)."""
        out = []
        for name, g, rows, v in zip("xyzs", self.groups(), self.rows(), (x, y, z, s)):
            if g is None or v is None:
                out.append(v)
                continue
            v = np.ascontiguousarray(v, dtype=np.float64)
            if v.ndim != 2 or v.shape[1] != rows:
                raise ValueError(f"{name} has shape {v.shape}, expected [count, {rows}]")
            out.append(_affine_eval(g, v))
        return tuple(out)


def _shift_map_ptrs(smap, pat):
    """A ShiftMap as (keep-alive structs, [x, y, z, s] as C pointers to eicos_affine_map or None)."""
    if (smap.n, smap.p, smap.m) != (pat.n, pat.p, pat.m):
        raise ValueError(f"shift map: built for (n, p, m) = ({smap.n}, {smap.p}, {smap.m}), the pattern has ({pat.n}, {pat.p}, {pat.m})")
    return _affine_ptrs((g, rows, f"shift map of {name}: ", f"{rows} rows") for name, g, rows in zip("xyzs", smap.groups(), smap.rows()))


def _disturbance(w, count, steps, k):
    """w as a contiguous float64 [count, steps, k] array (None passes); ValueError otherwise."""
    if w is None:
        return None
    w = np.ascontiguousarray(w, dtype=np.float64)
    if w.shape != (count, steps, k):
        raise ValueError(f"w has shape {w.shape}, expected [{count}, {steps}, {k}]")
    return w


def _result_rows(a, rows, width, name):
    """A caller-owned result array: C-contiguous float64 [rows, width] (None passes); ValueError otherwise."""
    if a is not None and not (isinstance(a, np.ndarray) and a.dtype == np.float64 and a.flags.c_contiguous and a.shape == (rows, width)):
        raise ValueError(f"{name} must be a C-contiguous float64 array of shape [{rows}, {width}]"
                         + (f", not {a.dtype} {a.shape}" if isinstance(a, np.ndarray) else ""))
    return a


def _theta_rows(theta, k, count):
    """theta as a contiguous float64 [count, k] array (count None: its leading dimension); ValueError otherwise."""
    theta = np.ascontiguousarray(theta, dtype=np.float64)
    if theta.ndim != 2 or theta.shape[1] != k or (count is not None and theta.shape[0] != count):
        raise ValueError(f"theta has shape {theta.shape}, expected [{'count' if count is None else count}, {k}]")
    return theta, theta.shape[0]


def _index_rows(indices):
    """The index list of an indexed call: a contiguous int32 vector and its pointer (a 1-element dummy keeps the pointer valid).  Anything
    that is not a one-dimensional list of integers is a TypeError / ValueError here; range and duplicates are the library's to check."""
    idx = np.asarray(indices)
    if idx.size and not np.issubdtype(idx.dtype, np.integer):
        raise TypeError(f"indices must be integers, not {idx.dtype}")
    if idx.ndim > 1:
        raise ValueError(f"indices must be one-dimensional, not of shape {idx.shape}")
    idx = np.ascontiguousarray(idx, dtype=np.int32).reshape(-1)
    return idx, _ip_or_dummy(idx)


def _indexed_groups(names, groups, widths, count):
    """The row arrays of an indexed call as (keep-alive arrays, C pointers): every given array is [count, width] with count =
    len(indices); ValueError otherwise.  None keeps a group."""
    for name, a, w in zip(names, groups, widths):
        if a is not None and np.shape(a) != (count, w):
            raise ValueError(f"{name} has shape {np.shape(a)}, expected [{count}, {w}] (one row per index)")
    return _group_ptrs(groups, widths, count)


def _rows(groups, default):
    """The instance count of an update: the leading dimension of the first two-dimensional array given."""
    return next((np.shape(a)[0] for a in groups if a is not None and np.ndim(a) == 2), default)


def _pattern_ptrs(pat):
    """(keep-alive int32 arrays, [q, Gjc, Gir, Ajc, Air] as C pointers) of a pattern; empty groups are NULL."""
    keep = [np.ascontiguousarray(a, dtype=np.int32) for a in (pat.q, pat.Gjc, pat.Gir, pat.Ajc, pat.Air)]
    q, Gjc, Gir, Ajc, Air = keep
    return keep, [_ip(q) if pat.ncones else None, _ip(Gjc) if pat.m > 0 else None, _ip(Gir) if pat.m > 0 else None,
                  _ip(Ajc) if pat.p > 0 else None, _ip(Air) if pat.p > 0 else None]


UPDATE_PATHS = {0: "none", 1: "pinned bounce", 2: "pinned source in place", 3: "peer GPU in place", 4: "staged peer copies", 5: "fused into the solve", 6: "fused into the solve, staged while it runs"}


class _Solver:
    """What BatchSolver (eicos_batch_*) and MultiBatchSolver (eicos_multi_*) share: the same calls on host arrays in global instance
    order, told apart by the C prefix and the error getter."""
    _prefix = _error = None

    def _call(self, name, *args):
        rc = getattr(_lib(), self._prefix + name)(self._h, *args)
        if rc != 0:
            raise RuntimeError(f"eicos_amd error {rc}: {getattr(_lib(), self._error)().decode()}")

    def _query(self, name) -> int:
        """A call that only returns a number of the handle (a count, a flag set)."""
        return int(getattr(_lib(), self._prefix + name)(self._h))

    def _widths(self):
        pat = self.pat
        return pat.nnzG, pat.nnzA, pat.n, pat.m, pat.p

    def _solve_with(self, name, ptr, x_out):
        if x_out is not None:
            assert x_out.dtype == np.float64 and x_out.flags.c_contiguous and x_out.shape == (self.batch, self.pat.n)
        codes = np.zeros(self.batch, np.int32)
        self._call(name, *ptr, _dp_or_null(x_out), _ip(codes))
        return codes

    # ---- updateData ----
    def update(self, Gpr=None, Apr=None, c=None, h=None, b=None, first: int = 0, count: int | None = None):
        """Host arrays shaped [count, ...]; None keeps the group (reference semantics)."""
        count = _rows((Gpr, Apr, c, h, b), self.batch) if count is None else count
        _keep, ptr = _group_ptrs((Gpr, Apr, c, h, b), self._widths(), count)
        self._call("update", first, count, *ptr)

    # ---- right-hand-side-only updateData (G, A and the equilibration kept; include/eicos_amd.h: eicos_batch_update_rhs) ----
    def update_rhs(self, c=None, h=None, b=None, first: int = 0, count: int | None = None):
        """New c, h, b (host arrays [count, ...]; None keeps the group) for instances [first, first + count), divided by the stored
        scalings: bit for bit what update() with the unchanged Gpr, Apr and these vectors gives."""
        count = _rows((c, h, b), self.batch) if count is None else count
        _keep, ptr = _rhs_ptrs(self.pat, count, c, h, b)
        self._call("update_rhs", first, count, *ptr)

    def update_rhs_solve(self, c=None, h=None, b=None, x_out=None):
        """update_rhs + solve of the whole batch in one call (eicos_batch_update_rhs_solve; on every shard, concurrently): with pinned /
        registered arrays the solve kernel scales every instance's vectors itself.  Returns the exit codes."""
        _keep, ptr = _rhs_ptrs(self.pat, self.batch, c, h, b)
        return self._solve_with("update_rhs_solve", ptr, x_out)

    # ---- parametric right-hand sides (include/eicos_amd.h: eicos_batch_set_param_map / eicos_batch_update_param) ----
    def set_param_map(self, pmap: "ParamMap | None"):
        """Install (copy) a ParamMap for all instances; None, or a map without groups, removes the installed one."""
        self._param_nnz = (0, 0, 0)  # (the widths of rollout_data_gradient's slope outputs: the stored entries of the installed groups)
        if pmap is None:
            self._call("set_param_map", 0, None, None, None)
            return
        _keep, ptr = _param_map_ptrs(pmap, self.pat)
        self._call("set_param_map", pmap.k, *ptr)
        self._param_nnz = tuple(0 if g is None else int(g[1][-1]) for g in pmap.groups())

    def param_count(self) -> int:
        """k of the installed parameter map, 0 without one."""
        return self._query("param_count")

    def update_param(self, theta, first: int = 0, count: int | None = None):
        """theta [count, k] (host array) for instances [first, first + count): the GPU expands it into the mapped groups of c, h, b and
        divides by the stored scalings -- bit for bit what update_rhs(*map.evaluate(theta)) leaves."""
        k = self.param_count()
        if k > 0:
            theta, count = _theta_rows(theta, k, count)
        else:  # (the library refuses: "no parameter map")
            theta = np.ascontiguousarray(theta, dtype=np.float64)
            count = (theta.shape[0] if theta.ndim == 2 else self.batch) if count is None else count
        self._call("update_param", first, count, _dp_or_dummy(theta))

    # ---- output map and the closed-loop step (include/eicos_amd.h: eicos_batch_set_output_map / eicos_batch_update_param_solve) ----
    def set_output_map(self, omap: "OutputMap | None"):
        """Install (copy) an OutputMap for all instances; None, or a map without rows, removes the installed one."""
        self._out_nnz = 0
        if omap is None or omap.r == 0:
            self._call("set_output_map", 0, None)
            return
        _keep, ptr = _output_map_ptr(omap, self.pat)
        self._call("set_output_map", omap.r, ptr)
        self._out_nnz = int(omap.rowptr[-1])

    def output_count(self) -> int:
        """r of the installed output map, 0 without one."""
        return self._query("output_count")

    def outputs(self, first: int = 0, count: int | None = None):
        """u [count, r] of instances [first, first + count): the output map applied to their current x -- bit for bit
        OutputMap.evaluate(solution()[first:first + count])."""
        count = self.batch - first if count is None else count
        u = np.zeros((max(count, 0), self.output_count()))
        self._call("outputs", first, count, _dp_or_dummy(u))
        return u

    def update_param_solve(self, theta, u_out=None, x_out=None):
        """The closed-loop step in one call: update_param(theta) + solve() of the whole batch, u (and x) delivered into `u_out` [batch, r]
        (and `x_out` [batch, n]) -- with pinned / registered theta the solve kernel expands every instance's theta row itself and writes
        its rows into pinned result arrays.  Returns the exit codes."""
        k = self.param_count()
        if k > 0:
            theta, _ = _theta_rows(theta, k, self.batch)
        else:  # (the library refuses: "no parameter map")
            theta = np.ascontiguousarray(theta, dtype=np.float64)
        _result_rows(u_out, self.batch, self.output_count(), "u_out")
        _result_rows(x_out, self.batch, self.pat.n, "x_out")
        codes = np.zeros(self.batch, np.int32)
        self._call("update_param_solve", _dp_or_dummy(theta), _dp_or_null(u_out), _dp_or_null(x_out), _ip(codes))
        return codes

    # ---- plant map and the closed-loop rollout (include/eicos_amd.h: eicos_batch_set_plant_map / eicos_batch_rollout) ----
    def set_plant_map(self, fmap: "PlantMap | None"):
        """Install (copy) a PlantMap for all instances, behind the parameter and the output map it refers to; None removes it.  Either
        way the per-instance values of set_plant_values() are dropped (the pattern may have changed)."""
        if fmap is None:
            self._call("set_plant_map", None)
            return
        _keep, ptr = _plant_map_ptr(fmap, self.param_count(), self.output_count())
        self._call("set_plant_map", ptr)
        self._plant_shape = (fmap.k, fmap.nnz())  # (the widths of the per-instance value rows: set_plant_values)

    def has_plant_map(self) -> bool:
        return bool(self._query("has_plant_map"))

    # ---- fallback map: the backup output law of steps that do not end well (include/eicos_amd.h: eicos_batch_set_fallback_map) ----
    def set_fallback_map(self, fmap: "FallbackMap | None"):
        """Install (copy) a FallbackMap for all instances, behind the parameter and the output map it refers to; None, or a map with
        mask 0, removes it.  From then on update_param_solve, update_param_solve_subset, rollout and rollout_jacobian form the u row of
        an instance whose final record is in a class of the mask as fmap.evaluate(theta); everything else they return is unchanged."""
        if fmap is None or not fmap.mask:
            self._call("set_fallback_map", 0, None)
            return
        k, r = self.param_count(), self.output_count()
        if k > 0 and r > 0:
            _keep, ptr = _fallback_map_ptr(fmap, k, r)
        else:  # (the library refuses: "no parameter map" / "no output map")
            _keep, ptr = _fallback_map_ptr(fmap, k, fmap.r)
        self._call("set_fallback_map", fmap.mask, ptr)

    def fallback_mask(self) -> int:
        """The mask of the installed fallback map, 0 without one."""
        return _nonneg(self._query("fallback_mask"))

    def fallback_counts(self, reset: bool = False):
        """Per instance the steps whose u row the fallback law has formed since its counter was last zeroed (cumulative: after a
        rollout, its fired steps); reset=True zeroes the counters after reading them."""
        out = np.zeros(self.batch, np.int32)
        self._call("fallback_counts", 0, self.batch, _ip(out), 1 if reset else 0)
        return out

    # ---- matrix map: G and A affine in theta (include/eicos_amd.h: eicos_batch_set_matrix_map) ----
    def set_matrix_map(self, mmap: "MatrixMap | None"):
        """Install (copy) a MatrixMap for all instances, behind the parameter map it refers to; None removes it.  update_param,
        update_param_device, update_param_solve and rollout then run a full updateData whose inputs the GPU forms from theta: the state
        of update(*mmap.evaluate(theta), *pmap.evaluate(theta)) in the contract of eicos_batch_set_matrix_map, bit for bit."""
        if mmap is None:
            self._call("set_matrix_map", None, None)
            return
        _keep, ptrs = _matrix_map_ptrs(mmap, self.pat.nnzG, self.pat.nnzA)
        self._call("set_matrix_map", *ptrs)

    def has_matrix_map(self) -> int:
        """Bit 0: G is mapped, bit 1: A is mapped; 0: no matrix map."""
        return self._query("has_matrix_map")

    # ---- starting point and shift map (include/eicos_amd.h: eicos_batch_set_iterate / eicos_batch_set_shift_map) ----
    def set_iterate(self, x=None, y=None, z=None, s=None, first: int = 0, count: int | None = None):
        """A caller-supplied starting point for instances [first, first + count): host arrays x [count, n], y [count, p], z, s [count, m]
        in the units of solution() / duals(); None keeps a group.  The instances are marked warm-startable: with set_warm_start(> 0) the
        next solve starts from the point, with warm start 0 it runs cold and overwrites it."""
        pat = self.pat
        count = _rows((x, y, z, s), self.batch - first) if count is None else count
        for name, a, w in zip("xyzs", (x, y, z, s), (pat.n, pat.p, pat.m, pat.m)):
            if a is not None and np.shape(a) != (count, w):
                raise ValueError(f"{name} has shape {np.shape(a)}, expected [{count}, {w}]")
        _keep, ptr = _group_ptrs((x, y, z, s), (pat.n, pat.p, pat.m, pat.m), count)
        self._call("set_iterate", first, count, *ptr)

    def set_shift_map(self, smap: "ShiftMap | None"):
        """Install (copy) a ShiftMap for all instances; None, or a map without groups, removes the installed one.  Every solve that
        warm-starts an instance then first takes its x, y, z, s through the map: bit for bit set_iterate(*smap.evaluate(solution(),
        *duals())) on the warm-startable instances before the same solve (contract: eicos_batch_set_shift_map)."""
        if smap is None:
            self._call("set_shift_map", None, None, None, None)
            return
        _keep, ptrs = _shift_map_ptrs(smap, self.pat)
        self._call("set_shift_map", *ptrs)

    def has_shift_map(self) -> int:
        """Bit 0: x, 1: y, 2: z, 3: s is mapped; 0: no shift map."""
        return self._query("has_shift_map")

    def rollout(self, theta0, steps: int, w=None):
        """`steps` closed-loop steps of the whole batch in one call: from theta0 [batch, k], every step is update_param_solve on the
        current theta row and then the plant map, theta+ = PlantMap.evaluate(theta, u, w[:, t]) -- with an LDS vector on the handle one
        launch in which every workgroup takes its instances through all their steps.  Returns u_traj [batch, steps, r], theta_traj
        [batch, steps + 1, k], exitcodes and iters [batch, steps]: bit for bit what the host loop over update_param_solve gives."""
        return self._rollout("rollout", theta0, steps, w, False)[0]

    def _rollout(self, name, theta0, steps, w, jacobian):
        """rollout and rollout_jacobian: the checked inputs, the four trajectories and, with `jacobian`, J and res behind them.
        Returns (the result arrays in the call's order, (T, k, r))."""
        steps = int(steps)
        k, r = self.param_count(), self.output_count()
        if k > 0:
            theta0, _ = _theta_rows(theta0, k, self.batch)
            w = _disturbance(w, self.batch, steps, k)
        else:  # (the library refuses: "no parameter map")
            theta0 = np.ascontiguousarray(theta0, dtype=np.float64)
            w = None if w is None else np.ascontiguousarray(w, dtype=np.float64)
        T = max(steps, 0)
        u_traj, theta_traj = np.zeros((self.batch, T, r)), np.zeros((self.batch, T + 1, k))
        codes, iters = np.zeros((self.batch, T), np.int32), np.zeros((self.batch, T), np.int32)
        more = [np.zeros((self.batch, T, r, k)), np.zeros((self.batch, T, r))] if jacobian else []
        self._call(name, steps, _dp_or_dummy(theta0), _dp_or_dummy(w), _dp_or_dummy(u_traj), _dp_or_dummy(theta_traj), _ip(codes), _ip(iters),
                   *[_dp_or_dummy(a) for a in more])
        return (u_traj, theta_traj, codes, iters, *more), (T, k, r)

    def rollout_jacobian(self, theta0, steps: int, w=None):
        """rollout() that also records the Jacobian of every step: returns (u_traj, theta_traj, exitcodes, iters, J [batch, steps, r, k],
        res [batch, steps, r]) -- J[i, t] and res[i, t] are what param_jacobian() returns for instance i right after step t's solve, bit
        for bit, the first four what rollout() returns; still one launch with an LDS vector on the handle.  A step that did not end
        OPTIMAL / OPTIMAL_INACC has NaN rows, and the loop goes on.  The handle keeps J on the GPU for rollout_gradient()."""
        out, self._rollout_shape = self._rollout("rollout_jacobian", theta0, steps, w, True)
        return out

    def rollout_gradient(self, gu=None, gtheta=None, device=False):
        """(grad_theta0 [batch, k], grad_w [batch, T, k]): the gradient of L = sum_t gu_t' u_t + sum_t gtheta_t' theta_t over the most
        recent rollout_jacobian() of the handle, by a backward sweep on the GPU -- gu [batch, T, r], gtheta [batch, T + 1, k], each
        optional, one must be given.  Bit for bit PlantMap.backprop of the returned J.  device=True (single-GPU handles): through the
        device form, fetched here; the same bits."""
        shape = getattr(self, "_rollout_shape", None)
        if shape is None:  # (no rollout_jacobian yet: the library refuses, with its message)
            gu, gtheta = (None if a is None else np.ascontiguousarray(a, dtype=np.float64) for a in (gu, gtheta))
            self._call("rollout_gradient", _dp(gu), _dp(gtheta), _dp(np.zeros(1)), None)
            raise RuntimeError("rollout_gradient: no rollout_jacobian() on this handle")
        T, k, r = shape
        gu, gtheta = _cotangent(gu, (self.batch, T, r), "gu"), _cotangent(gtheta, (self.batch, T + 1, k), "gtheta")
        g0, gw = np.zeros((self.batch, k)), np.zeros((self.batch, T, k))
        if device:
            self._device_form("rollout_gradient_device", None, 0, (), (gu, gtheta), (g0, gw), lead=())
        else:
            self._call("rollout_gradient", *[_dp_or_dummy(a) for a in (gu, gtheta, g0, gw)])
        return g0, gw

    # ---- the cone scaling of the adjoint (include/eicos_amd.h: EICOS_ADJOINT_NT / _CENTRED) ----
    def set_adjoint_scaling(self, mode: str):
        """"nt" (the default): K of every adjoint carries the NT scaling of the returned (s, z).  "centred": of centred_pair(s, z) --
        the derivative of the solution map where an active second-order cone's curvature fixes the optimum; use it on any pattern
        with cones.  Holds from the next adjoint launch, for adjoint(), adjoint_data(), output_jacobian(), param_jacobian(),
        param_gradient() and rollout_jacobian(); a J trajectory the handle holds stays as it was recorded."""
        if mode not in ADJOINT_SCALINGS:
            raise ValueError(f"set_adjoint_scaling: mode must be one of {', '.join(map(repr, ADJOINT_SCALINGS))}, got {mode!r}")
        self._call("set_adjoint_scaling", ADJOINT_SCALINGS[mode])

    def adjoint_scaling(self) -> str:
        v = _nonneg(self._query("adjoint_scaling"))
        return {c: k for k, c in ADJOINT_SCALINGS.items()}[v]

    # ---- a recording rollout and the gradient with respect to the controller's own data (include/eicos_amd.h) ----
    def set_rollout_recording(self, on: bool):
        """From now on rollout_jacobian() also records, on the GPU, the gradient rows of every step's output rows and the step's x, y, z
        (off by default; batch * T * (r + 1) * (n + m + p) * 8 bytes): what rollout_data_gradient() sweeps over.  Everything
        rollout_jacobian() returns, and the handle's state afterwards, keep their bits."""
        self._call("set_rollout_recording", 1 if on else 0)

    def rollout_recording(self) -> bool:
        return _nonneg(self._query("rollout_recording")) != 0

    def rollout_records(self):
        """(Wc [batch, T, r, n], Wh [batch, T, r, m], Wb [batch, T, r, p], x [batch, T, n], y [batch, T, p], z [batch, T, m]) of the most
        recent rollout_jacobian() under recording: per step the rows adjoint(g = the dense rows of the output map) returns there (0.0
        where the fallback law fired, NaN where the step did not end optimal) and the result rows the step's u was formed from."""
        shape = getattr(self, "_rollout_shape", None)
        if shape is None:  # (no rollout_jacobian yet: the library refuses, with its message)
            self._call("rollout_records", *[None] * 6)
            raise RuntimeError("rollout_records: no rollout_jacobian() on this handle")
        T, k, r = shape
        B, n, m, p = self.batch, self.pat.n, self.pat.m, self.pat.p
        outs = (np.zeros((B, T, r, n)), np.zeros((B, T, r, m)), np.zeros((B, T, r, p)), np.zeros((B, T, n)), np.zeros((B, T, p)), np.zeros((B, T, m)))
        self._call("rollout_records", *[_dp_or_dummy(a) for a in outs])
        return outs

    def rollout_data_gradient(self, theta, gu=None, gtheta=None, want=DATA_GRADIENT_KEYS, device=False):
        """The gradient of L = sum_t gu_t' u_t + sum_t gtheta_t' theta_t over the most recent rollout_jacobian() under recording with
        respect to the controller's own data, per instance (sum the rows over the batch for shared data): a dict over `want`, some of
        DATA_GRADIENT_KEYS -- grad_c [batch, n], grad_h, grad_b, grad_G [batch, nnzG], grad_A, grad_Cval / _Hval / _Bval [batch, stored
        entries of the parameter map's group], grad_u0 [batch, r], grad_Uval [batch, nnzU].  theta [batch, T + 1, k]: the trajectory
        that rollout returned.  Bit for bit rollout_data_backprop() of the records.  device=True as in rollout_gradient()."""
        shape = getattr(self, "_rollout_shape", None)
        want = tuple(want)
        unknown = [q for q in want if q not in DATA_GRADIENT_KEYS]
        if unknown or not want:
            raise ValueError(f"want must name some of {DATA_GRADIENT_KEYS}, got {want}")
        if shape is None:  # (no rollout_jacobian yet: the library refuses, with its message)
            one = np.zeros(1)
            st = DataGradient(grad_c=one.ctypes.data)
            self._call("rollout_data_gradient", _dp(one), None, _dp(one), C.byref(st))
            raise RuntimeError("rollout_data_gradient: no rollout_jacobian() on this handle")
        T, k, r = shape
        B = self.batch
        if gu is None and gtheta is None:
            raise ValueError("gu and gtheta are both None")
        gu, gtheta = _cotangent(gu, (B, T, r), "gu"), _cotangent(gtheta, (B, T + 1, k), "gtheta")
        theta = _cotangent(theta, (B, T + 1, k), "theta")
        if theta is None:
            raise ValueError("theta (the trajectory of the rollout) is needed")
        nnzG, nnzA, n, m, p = self._widths()
        widths = dict(zip(DATA_GRADIENT_KEYS, (n, m, p, nnzG, nnzA) + tuple(getattr(self, "_param_nnz", (0, 0, 0))) + (r, getattr(self, "_out_nnz", 0))))
        outs = {q: np.zeros((B, widths[q])) for q in want}
        if not device:
            # (an empty array travels as a one-element dummy: the library sees that the output was asked for)
            keep = {q: (a if a.size else np.zeros(1)) for q, a in outs.items()}
            st = DataGradient(**{q: a.ctypes.data for q, a in keep.items()})
            self._call("rollout_data_gradient", _dp_or_dummy(gu), _dp_or_dummy(gtheta), _dp_or_dummy(theta), C.byref(st))
            return outs
        if self._prefix != "eicos_batch_":
            raise ValueError("rollout_data_gradient: device=True needs a single-GPU handle")
        hip = _lib()
        ins, names, bufs = (gu, gtheta, theta), list(outs), []
        try:
            for a in list(ins) + [outs[q] for q in names]:
                d = C.c_void_p()
                if a is not None and hip.hipMalloc(C.byref(d), max(a.nbytes, 8)) != 0:
                    raise RuntimeError("hipMalloc failed")
                bufs.append(d)
            for a, d in zip(ins, bufs):
                if a is not None and a.nbytes and hip.hipMemcpy(d, a.ctypes.data, a.nbytes, 1) != 0:  # hipMemcpyHostToDevice
                    raise RuntimeError("hipMemcpy failed")
            st = DataGradient(**{q: d.value for q, d in zip(names, bufs[3:])})
            self._call("rollout_data_gradient_device", *bufs[:3], C.byref(st))
            self._call("sync")
            for q, d in zip(names, bufs[3:]):
                if outs[q].nbytes and hip.hipMemcpy(outs[q].ctypes.data, d, outs[q].nbytes, 2) != 0:  # hipMemcpyDeviceToHost
                    raise RuntimeError("hipMemcpy failed")
        finally:
            for d in bufs:
                hip.hipFree(d)
        return outs

    # ---- per-instance plant values (include/eicos_amd.h: eicos_batch_set_plant_values / _rollout_plant_gradient) ----
    def _plant_widths(self):
        """(k, nnzF) of the installed plant map as set_plant_map() last saw it; (0, 0) without one."""
        return getattr(self, "_plant_shape", (0, 0)) if self.has_plant_map() else (0, 0)

    def set_plant_values(self, f0=None, val=None, first: int = 0, device=False):
        """Per-instance values of the installed plant map for instances [first, first + count), count = the rows given: f0 [count, k]
        in the place of its base, val [count, nnzF] in the place of its stored values (same pattern, stored order); None keeps a
        group.  The first call of a group fills every instance with the shared values first.  Every rollout form then runs instance i
        against PlantMap.evaluate(..., f0=, val=) with its own rows.  device=True (single-GPU handles): through the device form."""
        k, nnz = self._plant_widths()
        if f0 is None and val is None:
            raise ValueError("f0 and val are both None")
        count = _rows((f0, val), None)
        for name, a, w in (("f0", f0, k), ("val", val, nnz)):
            if a is not None and (np.ndim(a) != 2 or np.shape(a) != (count, w)):
                raise ValueError(f"{name} has shape {np.shape(a)}, expected [{count}, {w}] (one row per instance)")
        first = int(first)
        if first < 0 or count > self.batch - first:
            raise ValueError(f"instances [{first}, {first + count}) lie outside [0, {self.batch})")
        arrs, ptrs = _group_ptrs((f0, val), (k, nnz), count)
        if device:
            self._device_form("set_plant_values_device", None, 0, (), arrs, (), lead=(first, count))
        else:
            self._call("set_plant_values", first, count, *ptrs)

    def plant_values(self, first: int = 0, count: int | None = None):
        """(f0 [count, k], val [count, nnzF]) of instances [first, first + count) as the rollouts read them: the installed per-instance
        rows, and the shared values where none are installed."""
        k, nnz = self._plant_widths()
        first = int(first)
        count = self.batch - first if count is None else int(count)
        f0, val = np.zeros((max(count, 0), k)), np.zeros((max(count, 0), nnz))
        self._call("plant_values", first, count, _dp_or_dummy(f0), _dp_or_dummy(val))
        return f0, val

    def has_plant_values(self) -> int:
        """Bit 0: per-instance f0 rows are installed, bit 1: per-instance val rows; 0: every instance runs the shared plant."""
        return _nonneg(self._query("has_plant_values"))

    def clear_plant_values(self):
        """Drop the per-instance values: every instance runs the shared plant map again."""
        self._call("clear_plant_values")

    def rollout_plant_gradient(self, u, theta, gu=None, gtheta=None, device=False):
        """(grad_theta0 [batch, k], grad_w [batch, T, k], grad_f0 [batch, k], grad_val [batch, nnzF]): rollout_gradient() that also
        returns the gradient with respect to the plant's own entries, per instance -- u [batch, T, r] and theta [batch, T + 1, k] the
        trajectories the most recent rollout_jacobian() returned.  Bit for bit PlantMap.backprop_values of the returned J (with the
        per-instance val where installed).  With the shared plant, sum the rows over the batch.  device=True as in rollout_gradient()."""
        shape = getattr(self, "_rollout_shape", None)
        if shape is None:  # (no rollout_jacobian yet: the library refuses, with its message)
            one = _dp(np.zeros(1))
            self._call("rollout_plant_gradient", one, None, one, one, one, None, None, None)
            raise RuntimeError("rollout_plant_gradient: no rollout_jacobian() on this handle")
        T, k, r = shape
        nnz = self._plant_widths()[1]
        if gu is None and gtheta is None:
            raise ValueError("gu and gtheta are both None")
        gu, gtheta = _cotangent(gu, (self.batch, T, r), "gu"), _cotangent(gtheta, (self.batch, T + 1, k), "gtheta")
        u, theta = _cotangent(u, (self.batch, T, r), "u"), _cotangent(theta, (self.batch, T + 1, k), "theta")
        if u is None or theta is None:
            raise ValueError("u and theta (the trajectories of the rollout) are both needed")
        outs = (np.zeros((self.batch, k)), np.zeros((self.batch, T, k)), np.zeros((self.batch, k)), np.zeros((self.batch, nnz)))
        if device:
            self._device_form("rollout_plant_gradient_device", None, 0, (), (gu, gtheta, u, theta), outs, lead=())
        else:
            self._call("rollout_plant_gradient", *[_dp_or_dummy(a) for a in (gu, gtheta, u, theta) + outs])
        return outs

    # ---- solve ----
    def solve(self):
        codes = np.zeros(self.batch, np.int32)
        self._call("solve", _ip(codes))
        return codes

    def solve_async(self):
        self._call("solve_async")

    def sync(self):
        self._call("sync")

    # ---- subset solves: by index list or by exit class (include/eicos_amd.h: eicos_batch_solve_subset / _solve_where) ----
    @staticmethod
    def _index_list(indices):
        """indices as a contiguous int32 vector (the library checks range and duplicates); a 1-element dummy keeps the pointer valid."""
        idx = np.ascontiguousarray(indices, dtype=np.int32).reshape(-1)
        return idx, _ip_or_dummy(idx)

    def select(self, mask: int):
        """The ascending ids of the instances whose exit class is in `mask` (an OR of SEL_* bits), found by the selection kernel on the
        GPU: only the count and the ids travel."""
        ids, count = np.zeros(self.batch, np.int32), C.c_int(0)
        self._call("select", C.c_uint(int(mask)), _ip(ids), C.byref(count))
        return ids[: count.value].copy()

    def solve_subset(self, indices):
        """One solve launch over the instances `indices` (each at most once) instead of the whole batch: they end, bit for bit, as
        solve() would leave them, every other instance keeps its state and its info record.  Returns their exit codes in list order;
        an empty list launches nothing."""
        idx, ptr = self._index_list(indices)
        codes = np.zeros(idx.size, np.int32)
        self._call("solve_subset", ptr, int(idx.size), _ip(codes) if idx.size else None)
        return codes

    def solve_subset_async(self, indices):
        """solve_subset without waiting for the GPU (sync() waits)."""
        idx, ptr = self._index_list(indices)
        self._call("solve_subset_async", ptr, int(idx.size))

    def solve_where(self, mask: int):
        """select(mask) + solve_subset with the id list used in place on the GPU: (ids ascending, their exit codes).  A class nobody is
        in launches nothing and returns two empty arrays."""
        ids, codes, count = np.zeros(self.batch, np.int32), np.zeros(self.batch, np.int32), C.c_int(0)
        self._call("solve_where", C.c_uint(int(mask)), _ip(ids), C.byref(count), _ip(codes))
        return ids[: count.value].copy(), codes[: count.value].copy()

    def gather(self, indices):
        """The rows of the instances `indices`, in list order, packed on the GPU and fetched with one copy: a dict of x [count, n],
        y [count, p], z, s [count, m] -- the rows solution() / duals() return -- and info, a dict of arrays like info_arrays()."""
        idx, ptr = self._index_list(indices)
        pat, k = self.pat, int(idx.size)
        x, y, z, s = np.zeros((k, pat.n)), np.zeros((k, pat.p)), np.zeros((k, pat.m)), np.zeros((k, pat.m))
        arr = (Info * max(k, 1))()
        self._call("gather", ptr, k, *[_dp_or_null(a) for a in (x, y, z, s)], arr)
        return {"x": x, "y": y, "z": z, "s": s, "info": _info_columns(arr, k)}

    # ---- update, read and step a chosen subset (include/eicos_amd.h: eicos_batch_update_indexed ... _update_param_solve_subset) ----
    def update_indexed(self, indices, Gpr=None, Apr=None, c=None, h=None, b=None):
        """update() for the instances `indices` (each at most once): row q of every array [len(indices), ...] belongs to instance
        indices[q]; None keeps the group.  Bit for bit the loop of update(first=indices[q], count=1) calls."""
        idx, ptr = _index_rows(indices)
        _keep, rows = _indexed_groups(("Gpr", "Apr", "c", "h", "b"), (Gpr, Apr, c, h, b), self._widths(), int(idx.size))
        self._call("update_indexed", ptr, int(idx.size), *rows)

    def update_rhs_indexed(self, indices, c=None, h=None, b=None):
        """update_rhs() for the instances `indices`, rows in list order."""
        idx, ptr = _index_rows(indices)
        pat = self.pat
        _keep, rows = _indexed_groups("chb", (c, h, b), (pat.n, pat.m, pat.p), int(idx.size))
        self._call("update_rhs_indexed", ptr, int(idx.size), *rows)

    def update_param_indexed(self, indices, theta):
        """update_param() for the instances `indices`: theta [len(indices), k], row q for instance indices[q]."""
        idx, ptr = _index_rows(indices)
        theta = self._theta_for(theta, int(idx.size))
        self._call("update_param_indexed", ptr, int(idx.size), _dp_or_dummy(theta))

    def set_iterate_indexed(self, indices, x=None, y=None, z=None, s=None):
        """set_iterate() for the instances `indices`, rows in list order."""
        idx, ptr = _index_rows(indices)
        pat = self.pat
        _keep, rows = _indexed_groups("xyzs", (x, y, z, s), (pat.n, pat.p, pat.m, pat.m), int(idx.size))
        self._call("set_iterate_indexed", ptr, int(idx.size), *rows)

    def outputs_indexed(self, indices):
        """u [len(indices), r]: row q = the output map on the current x of instance indices[q] -- row indices[q] of outputs()."""
        idx, ptr = _index_rows(indices)
        u = np.zeros((int(idx.size), self.output_count()))
        self._call("outputs_indexed", ptr, int(idx.size), _dp_or_dummy(u))
        return u

    # ---- adjoint sensitivities (include/eicos_amd.h: eicos_batch_adjoint, _output_jacobian) ----
    def _adjoint_rows(self, idx):
        """(pointer or None, count) of an adjoint call: idx None = the whole batch."""
        if idx is None:
            return None, self.batch
        ids, ptr = _index_rows(idx)
        return ptr, int(ids.size)

    def adjoint(self, g, idx=None):
        """Gradients of g'x with respect to (c, h, b) at the iterate the last solve returned: g [count, nrhs, n] (or [count, n] for one
        right-hand side), count = len(idx) or the batch.  Returns (grad_c [count, nrhs, n], grad_h [count, nrhs, m], grad_b
        [count, nrhs, p], res [count, nrhs]); an instance whose last solve did not end OPTIMAL / OPTIMAL_INACC has NaN rows.  One
        factorisation and nrhs refined KKT solves per instance; nothing a later call reads is changed.  At a degenerate optimum the
        result is a smoothed value, not a derivative."""
        ptr, count = self._adjoint_rows(idx)
        pat = self.pat
        g = self._adjoint_g(g, count)
        nrhs = int(g.shape[1])
        gc, gh, gb, res = (np.zeros((count, nrhs, w)) for w in (pat.n, pat.m, pat.p, 1))
        self._call("adjoint", ptr, count, nrhs, *[_dp_or_null(a) for a in (g, gc, gh, gb, res)])
        return gc, gh, gb, res[:, :, 0]

    def output_jacobian(self, idx=None, device=False):
        """(J [count, r, k], res [count, r]): the Jacobian du / dtheta of the output map through the parameter map at the iterate the
        last solve returned -- r adjoint solves per instance, contracted with the map on the GPU.  device=True (single-GPU handles):
        the call that writes J and res into device memory, fetched here afterwards; the same bits."""
        ptr, count = self._adjoint_rows(idx)
        r, k = max(self.output_count(), 0), max(self.param_count(), 0)
        J, res = np.zeros((count, r, k)), np.zeros((count, r))
        if not device:
            self._call("output_jacobian", ptr, count, _dp_or_dummy(J), _dp_or_null(res))
        elif self._prefix != "eicos_batch_":
            raise ValueError("output_jacobian(device=True) needs a single-GPU handle")  # (this call's own wording, older than _device_form's)
        else:
            self._device_form("output_jacobian_device", ptr, count, (), (), (J, res))
        return J, res

    # ---- ... with respect to the matrix data (eicos_batch_adjoint_data, _param_jacobian, _param_gradient) ----
    def _adjoint_g(self, g, count):
        g = np.ascontiguousarray(g, dtype=np.float64)
        if g.ndim == 2:
            g = g[:, None, :]
        if g.ndim != 3 or g.shape[0] != count or g.shape[2] != self.pat.n:
            raise ValueError(f"g must have shape [{count}, nrhs, {self.pat.n}], not {g.shape}")
        return g

    def adjoint_data(self, g, idx=None):
        """adjoint() with the gradients with respect to the stored values of G and A: returns (grad_c, grad_h, grad_b, grad_G
        [count, nrhs, nnzG], grad_A [count, nrhs, nnzA], res), the matrix gradients in the CSC order of Gpr / Apr --
        grad_G[e] = grad_c[j] z[i] - grad_h[i] x[j] and grad_A[e] = grad_c[j] y[i] - grad_b[i] x[j] for the stored value e = (i, j).
        grad_c, grad_h, grad_b and res are the bits of adjoint(); no further factorisation or KKT solve."""
        ptr, count = self._adjoint_rows(idx)
        pat = self.pat
        g = self._adjoint_g(g, count)
        nrhs = int(g.shape[1])
        gc, gh, gb, gG, gA, res = (np.zeros((count, nrhs, w)) for w in (pat.n, pat.m, pat.p, pat.nnzG, pat.nnzA, 1))
        self._call("adjoint_data", ptr, count, nrhs, *[_dp_or_null(a) for a in (g, gc, gh, gb, gG, gA, res)])
        return gc, gh, gb, gG, gA, res[:, :, 0]

    def matrix_map_count(self) -> int:
        """k the installed matrix map was validated for, 0 without one."""
        return self._query("matrix_map_count")

    def _theta_width(self):
        return max(self.param_count(), 0) or max(self.matrix_map_count(), 0)

    def _device_form(self, name, ptr, count, head, ins, outs, lead=None):
        """A *_device call on host arrays: device copies of `ins`, the call, sync, `outs` fetched -- the same bits as the host form.
        An input that is None travels as a NULL pointer; lead: the arguments in front of `head` when they are not (ptr, count)."""
        if self._prefix != "eicos_batch_":
            raise ValueError(name + ": device=True needs a single-GPU handle")
        hip = _lib()  # (the HIP runtime the library is linked against: hipMalloc, hipMemcpy, hipFree of the signature table)
        bufs = []
        try:
            for a in list(ins) + list(outs):
                d = C.c_void_p()
                if a is not None and hip.hipMalloc(C.byref(d), max(a.nbytes, 8)) != 0:
                    raise RuntimeError("hipMalloc failed")
                bufs.append(d)
            for a, d in zip(ins, bufs):
                if a is not None and a.nbytes and hip.hipMemcpy(d, a.ctypes.data, a.nbytes, 1) != 0:  # hipMemcpyHostToDevice
                    raise RuntimeError("hipMemcpy failed")
            self._call(name, *((ptr, count) if lead is None else lead), *head, *bufs)
            self._call("sync")
            for a, d in zip(outs, bufs[len(ins):]):
                if a.nbytes and hip.hipMemcpy(a.ctypes.data, d, a.nbytes, 2) != 0:  # hipMemcpyDeviceToHost
                    raise RuntimeError("hipMemcpy failed")
        finally:
            for d in bufs:
                hip.hipFree(d)

    def param_jacobian(self, idx=None, device=False):
        """(J [count, r, k], res [count, r]): du / dtheta through the output map and whichever of the parameter map and the matrix map
        are installed -- the matrix terms grad_G' M_G + grad_A' M_A join the contraction on the GPU.  Without a matrix map: the bits of
        output_jacobian().  device=True (single-GPU handles): through the device form, fetched here; the same bits."""
        ptr, count = self._adjoint_rows(idx)
        r, k = max(self.output_count(), 0), self._theta_width()
        J, res = np.zeros((count, r, k)), np.zeros((count, r))
        if device:
            self._device_form("param_jacobian_device", ptr, count, (), (), (J, res))
        else:
            self._call("param_jacobian", ptr, count, _dp_or_dummy(J), _dp_or_null(res))
        return J, res

    def param_gradient(self, g, idx=None, device=False):
        """(grad_theta [count, nrhs, k], res [count, nrhs]): the gradient of g'x with respect to theta through the installed parameter
        and matrix maps, g [count, nrhs, n]; no output map is needed.  device=True as in param_jacobian()."""
        ptr, count = self._adjoint_rows(idx)
        g = self._adjoint_g(g, count)
        nrhs = int(g.shape[1])
        gt, res = np.zeros((count, nrhs, self._theta_width())), np.zeros((count, nrhs))
        if device:
            self._device_form("param_gradient_device", ptr, count, (nrhs,), (g,), (gt, res))
        else:
            self._call("param_gradient", ptr, count, nrhs, _dp_or_null(g), _dp_or_dummy(gt), _dp_or_null(res))
        return gt, res

    def update_param_solve_subset(self, indices, theta, u_out=None, x_out=None):
        """The closed-loop step over the instances `indices` in one call: update_param_indexed + solve_subset + outputs_indexed, theta
        [len(indices), k], u_out [len(indices), r] and x_out [len(indices), n] in list order -- with pinned / registered theta ONE subset
        launch whose workgroups expand their own theta row and write their rows into pinned result arrays.  Every other instance keeps
        its state.  Returns the exit codes in list order; an empty list launches nothing."""
        idx, ptr = _index_rows(indices)
        count = int(idx.size)
        theta = self._theta_for(theta, count)
        _result_rows(u_out, count, self.output_count(), "u_out")
        _result_rows(x_out, count, self.pat.n, "x_out")
        codes = np.zeros(count, np.int32)
        self._call("update_param_solve_subset", ptr, count, _dp_or_dummy(theta), _dp_or_null(u_out), _dp_or_null(x_out), _ip(codes) if count else None)
        return codes

    def _theta_for(self, theta, count):
        """theta rows of an indexed call: [count, k] when a parameter map is installed (ValueError otherwise); without one the library
        refuses ("no parameter map"), so only the leading dimension is checked."""
        k = self.param_count()
        if k > 0:
            return _theta_rows(theta, k, count)[0]
        theta = np.ascontiguousarray(theta, dtype=np.float64)
        if theta.ndim == 2 and theta.shape[0] != count:
            raise ValueError(f"theta has {theta.shape[0]} rows, expected {count} (one row per index)")
        return theta

    def set_warm_start(self, shift: float):
        """shift > 0: re-solves start from the previous solution (not in the reference; see include/eicos_amd.h)."""
        self._call("set_warm_start", float(shift))

    def set_dynamic_regularization(self, delta: float, eps: float):
        """delta > 0: ECOS-style dynamic regularisation of the LDL' pivots (not in the reference)."""
        self._call("set_dynamic_regularization", float(delta), float(eps))

    def set_settings(self, **fields):
        """Runtime solver settings of the handle (every shard of a multi-GPU one): feastol, abstol, reltol, their _inacc counterparts,
        linsysacc, irerrfact, iter_max, nitref (ranges and semantics: eicos_settings of include/eicos_amd.h).  Fields that are not
        named keep their current value; the change takes effect from the next solve launch.  An unknown name raises TypeError before
        the library is called, a refused value RuntimeError with the handle's settings unchanged."""
        _known_settings("set_settings", fields)
        st = Settings()
        self._call("get_settings", C.byref(st))
        _assign_settings(st, fields)
        self._call("set_settings", C.byref(st))

    def settings(self) -> dict:
        st = Settings()
        self._call("get_settings", C.byref(st))
        return st.asdict()

    # ---- retry policy: a second attempt inside the solve launch (include/eicos_amd.h: eicos_retry) ----
    def set_retry(self, mask=None, warm: float = 0.0, dyn=(0.0, 0.0), **settings_fields):
        """An instance whose solve ends in an exit class of `mask` (an OR of SEL_* bits) is solved once more inside the same launch --
        every launch of the handle, the steps of a one-launch rollout included -- before anything reads its result.  The second
        attempt runs cold (warm = 0) or warm-started where its record allows it, under dyn = (delta, eps) and under the DEFAULT
        settings with the named fields changed (the names of set_settings).  mask None or 0 removes the policy.  An unknown field
        raises TypeError before the library is called, a refused value RuntimeError with the policy unchanged."""
        _known_settings("set_retry", settings_fields)
        if not mask:
            self._call("set_retry", None)
            return
        r = Retry()
        _lib().eicos_retry_default(C.byref(r))
        r.mask, r.warm, r.dyn_delta, r.dyn_eps = int(mask), float(warm), float(dyn[0]), float(dyn[1])
        _assign_settings(r.settings, settings_fields)
        self._call("set_retry", C.byref(r))

    def retry(self) -> dict:
        """The installed policy: {"mask", "warm", "dyn": (delta, eps), "settings": {...}}; mask 0 = none."""
        r = Retry()
        self._call("get_retry", C.byref(r))
        return r.asdict()

    def retry_counts(self, reset: bool = False):
        """Per instance the second attempts it has run since its counter was last reset (cumulative: after a rollout, its retried
        steps); reset=True zeroes the counters after reading them."""
        out = np.zeros(self.batch, np.int32)
        self._call("retry_counts", 0, self.batch, _ip(out), 1 if reset else 0)
        return out

    # ---- results ----
    def solution(self):
        x = np.zeros((self.batch, self.pat.n))
        if self.pat.n:
            self._call("solution", _dp(x))
        return x

    def duals(self):
        pat = self.pat
        y, z, s = np.zeros((self.batch, pat.p)), np.zeros((self.batch, pat.m)), np.zeros((self.batch, pat.m))
        self._call("duals", _dp(y) if pat.p else None, _dp(z) if pat.m else None, _dp(s) if pat.m else None)
        return y, z, s

    def info_arrays(self):
        arr = (Info * self.batch)()
        self._call("info", arr)
        return _info_columns(arr, self.batch)

    def close(self):
        if getattr(self, "_h", None):
            getattr(_lib(), self._prefix + "destroy")(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class BatchSolver(_Solver):
    """One sparsity pattern, `batch` numeric instances on one GPU.

    Mirrors the reference's Solver surface (ctor / updateData / solve / solution / getInfo,
    reference include/eicos.hpp:137-163) with a leading batch dimension on every array.
    """
    _prefix, _error = "eicos_batch_", "eicos_last_error"

    def __init__(self, pat, batch: int, device: int = -1):
        self.pat, self.batch = pat, int(batch)
        self._keep, ptrs = _pattern_ptrs(pat)
        h = C.c_void_p()
        _chk(_lib().eicos_batch_create(pat.n, pat.m, pat.p, pat.l, pat.ncones, *ptrs, self.batch, device, C.byref(h)))
        self._h = h

    def update_solve(self, Gpr=None, Apr=None, c=None, h=None, b=None, x_out=None):
        """updateData + solve in one call (eicos_batch_update_solve): host arrays shaped [batch, ...] (None keeps the group).  With pinned /
        registered arrays the solve kernel pulls every instance's inputs itself (no separate updateData launch) and writes x into a pinned
        `x_out`.  Returns the exit codes."""
        _keep, ptr = _group_ptrs((Gpr, Apr, c, h, b), self._widths(), self.batch)
        return self._solve_with("update_solve", ptr, x_out)

    def update_device(self, dG=0, dA=0, dc=0, dh=0, db=0, first: int = 0, count: int | None = None):
        """Raw device pointers (ints, e.g. torch.Tensor.data_ptr()); 0 keeps the group."""
        count = self.batch if count is None else count
        self._call("update_device", first, count, *_dev(dG, dA, dc, dh, db))

    def update_rhs_device(self, dc=0, dh=0, db=0, first: int = 0, count: int | None = None):
        """update_rhs from raw device pointers (ints); 0 keeps the group.  Asynchronous, like update_device."""
        count = self.batch if count is None else count
        self._call("update_rhs_device", first, count, *_dev(dc, dh, db))

    def update_param_device(self, dtheta, first: int = 0, count: int | None = None):
        """update_param from a raw device pointer (int) to theta [count, k].  Asynchronous, like update_rhs_device."""
        count = self.batch if count is None else count
        self._call("update_param_device", first, count, *_dev(dtheta))

    def set_iterate_device(self, dx=0, dy=0, dz=0, ds=0, first: int = 0, count: int | None = None):
        """set_iterate from raw device pointers (ints) to x [count, n], y [count, p], z, s [count, m]; 0 keeps the group.  Asynchronous on
        the handle's stream."""
        count = self.batch - first if count is None else count
        self._call("set_iterate_device", first, count, *_dev(dx, dy, dz, ds))

    def outputs_device(self, du, first: int = 0, count: int | None = None):
        """outputs() into a raw device pointer (int) to u [count, r].  Asynchronous on the handle's stream."""
        count = self.batch - first if count is None else count
        self._call("outputs_device", first, count, *_dev(du))

    # ---- the indexed calls from raw device pointers (ints); `indices` stays a host list.  Asynchronous on the handle's stream ----
    def update_indexed_device(self, indices, dG=0, dA=0, dc=0, dh=0, db=0):
        idx, ptr = _index_rows(indices)
        self._call("update_indexed_device", ptr, int(idx.size), *_dev(dG, dA, dc, dh, db))

    def update_rhs_indexed_device(self, indices, dc=0, dh=0, db=0):
        idx, ptr = _index_rows(indices)
        self._call("update_rhs_indexed_device", ptr, int(idx.size), *_dev(dc, dh, db))

    def update_param_indexed_device(self, indices, dtheta):
        idx, ptr = _index_rows(indices)
        self._call("update_param_indexed_device", ptr, int(idx.size), *_dev(dtheta))

    def set_iterate_indexed_device(self, indices, dx=0, dy=0, dz=0, ds=0):
        idx, ptr = _index_rows(indices)
        self._call("set_iterate_indexed_device", ptr, int(idx.size), *_dev(dx, dy, dz, ds))

    def outputs_indexed_device(self, indices, du):
        """outputs_indexed() into a raw device pointer (int) to u [len(indices), r]."""
        idx, ptr = _index_rows(indices)
        self._call("outputs_indexed_device", ptr, int(idx.size), *_dev(du))

    def output_jacobian_device(self, dJ, dres=0, idx=None):
        """output_jacobian() into raw device pointers (int): J [count, r, k] and, optionally, res [count, r]; asynchronous (sync() waits)."""
        ptr, count = self._adjoint_rows(idx)
        self._call("output_jacobian_device", ptr, count, *_dev(dJ, dres))

    def param_jacobian_device(self, dJ, dres=0, idx=None):
        """param_jacobian() into raw device pointers (int): J [count, r, k] and, optionally, res [count, r]; asynchronous (sync() waits)."""
        ptr, count = self._adjoint_rows(idx)
        self._call("param_jacobian_device", ptr, count, *_dev(dJ, dres))

    def param_gradient_device(self, nrhs, dg, dgrad_theta, dres=0, idx=None):
        """param_gradient() on raw device pointers (int): g [count, nrhs, n] in, grad_theta [count, nrhs, k] and, optionally, res
        [count, nrhs] out; asynchronous on the handle's stream (sync() waits) -- what a training loop on the GPU calls."""
        ptr, count = self._adjoint_rows(idx)
        self._call("param_gradient_device", ptr, count, int(nrhs), *_dev(dg, dgrad_theta, dres))

    def set_stream(self, stream_ptr: int):
        self._call("set_stream", *_dev(stream_ptr))

    def info(self):
        arr = (Info * self.batch)()
        self._call("info", arr)
        return [arr[i].asdict() for i in range(self.batch)]

    def dims(self) -> dict:
        d = Dims()
        self._call("dims", C.byref(d))
        return d.asdict()

    def kernel_build(self) -> str:
        """Which compilation of the solve kernel the handle launches: 'default', 'lds-resident', 'w2' (256 VGPRs, <= 2 workgroups per CU) or
        'u-in-lds' (one workgroup per CU, the factor operand array in LDS)."""
        return ("default", "lds-resident", "w2", "u-in-lds")[_nonneg(_lib().eicos_batch_kernel_build(self._h))]

    def shared_values(self) -> bool:
        """True when the handle's last updateData found every instance's G and A bit-identical to instance 0's, so that the next solve's
        products stream one copy of the values (eicos_batch_shared_values); waits for the handle's stream."""
        return bool(_nonneg(_lib().eicos_batch_shared_values(self._h)))

    def last_solve_ms(self) -> float:
        ms = C.c_float()
        _chk(_lib().eicos_batch_last_solve_ms(self._h, C.byref(ms)))
        return float(ms.value)

    def last_update_ms(self) -> float:
        ms = C.c_float()
        _chk(_lib().eicos_batch_last_update_ms(self._h, C.byref(ms)))
        return float(ms.value)

    def ms_history(self, which="solve", cap=64):
        """HIP-event durations (ms) of the most recent solve launches / updateData calls, oldest first (the handle's ring of 64 event pairs; which = "solve" | "update" | "step" = update start -> solve end):
        lets a caller time K back-to-back steps without synchronising inside its loop.  None with a library that predates the call."""
        L = _lib()
        if not hasattr(L, "eicos_batch_ms_history"):
            return None
        buf = (C.c_float * cap)()
        n = _nonneg(L.eicos_batch_ms_history(self._h, {"solve": 0, "update": 1, "step": 2}[which], buf, cap))
        return [float(buf[i]) for i in range(n)]

    def last_rollout_launches(self) -> int:
        """Solve-kernel launches of the most recent rollout(): 1 = the steps ran inside one launch, `steps` = one launch per step."""
        return self._query("last_rollout_launches")

    def last_update_path(self) -> str:
        """How the most recent host-pointer / peer updateData moved its inputs (UPDATE_PATHS)."""
        return UPDATE_PATHS[_lib().eicos_batch_last_update_path(self._h)]

    def solution_into(self, x):
        """solution() into a caller-owned [batch, n] float64 array (e.g. a PinnedArray's `.a`: one strided device-to-host copy)."""
        assert x.dtype == np.float64 and x.flags.c_contiguous and x.shape == (self.batch, self.pat.n)
        if self.pat.n:
            _chk(_lib().eicos_batch_solution(self._h, _dp(x)))
        return x

    def debug_factor(self, inst: int = 0):
        d = self.dims()
        D, U = np.zeros(max(d["dim_K"], 1)), np.zeros(max(d["nnzL"], 1))
        _chk(_lib().eicos_debug_factor(self._h, inst, _dp(D), _dp(U)))
        return D[: d["dim_K"]], U[: d["nnzL"]]

    TRACE_COLS = ("pcost", "dcost", "gap", "pres", "dres", "kapovert", "mu", "step", "sigma", "tau", "kap", "nitref3")

    def debug_trace(self, inst: int = 0, iters: int | None = None):
        """Per-iteration history [iters+1, 12] of instance `inst` (needs batch <= resident workgroups)."""
        out = np.zeros((102, 12))
        _chk(_lib().eicos_debug_trace(self._h, inst, _dp(out)))
        return out if iters is None else out[: iters + 1]

    def debug_kkt(self, inst: int = 0):
        """Upper triangle of the instance's KKT matrix as the factorisation reads it: (rows, cols, vals)."""
        d = self.dims()
        r, c, v = np.zeros(max(d["nnzK"], 1), np.int32), np.zeros(max(d["nnzK"], 1), np.int32), np.zeros(max(d["nnzK"], 1))
        _chk(_lib().eicos_debug_kkt(self._h, inst, _ip(r), _ip(c), _dp(v)))
        return r[: d["nnzK"]], c[: d["nnzK"]], v[: d["nnzK"]]

    def debug_scalings(self, s, z, inst: int = 0):
        """The solver's updateScalings + updateKKTScalings stage for (s, z): (ran, scaling block of K)."""
        pat = self.pat
        nV = pat.l + int(sum(3 * int(q) + 1 for q in pat.q))
        s, z = np.ascontiguousarray(s, np.float64), np.ascontiguousarray(z, np.float64)
        V, ran = np.zeros(max(nV, 1)), np.zeros(1, np.int32)
        _chk(_lib().eicos_debug_scalings(self._h, inst, _dp(s), _dp(z), _dp(V), _ip(ran)))
        return bool(ran[0]), V[:nV]

    def debug_pattern(self):
        d = self.dims()
        perm, Lp, Li = np.zeros(max(d["dim_K"], 1), np.int32), np.zeros(d["dim_K"] + 1, np.int32), np.zeros(max(d["nnzL"], 1), np.int32)
        _chk(_lib().eicos_debug_pattern(self._h, _ip(perm), _ip(Lp), _ip(Li)))
        return perm[: d["dim_K"]], Lp, Li[: d["nnzL"]]


def _mchk(rc):
    if rc != 0:
        raise RuntimeError(f"eicos_amd error {rc}: {_lib().eicos_multi_last_error().decode()}")


class MultiBatchSolver(_Solver):
    """One sparsity pattern, `batch` instances in contiguous shards over `device_ids` (eicos_multi_* of include/eicos_amd.h):
    ONE process drives every listed GPU, one handle + stream per list entry, no collective.  Arrays are [batch, ...] in global
    instance order; a device may be listed more than once (its shards run concurrently on that GPU)."""
    _prefix, _error = "eicos_multi_", "eicos_multi_last_error"

    def __init__(self, pat, batch: int, device_ids):
        self.pat, self.batch = pat, int(batch)
        self._keep, ptrs = _pattern_ptrs(pat)
        dev = np.ascontiguousarray(device_ids, dtype=np.int32)
        h = C.c_void_p()
        _mchk(_lib().eicos_multi_create(pat.n, pat.m, pat.p, pat.l, pat.ncones, *ptrs, self.batch, _ip(dev), len(dev), C.byref(h)))
        self._h = h

    def update_device(self, src_device: int, dG=0, dA=0, dc=0, dh=0, db=0, first: int = 0, count: int | None = None):
        """Raw pointers into the HBM of GPU `src_device` (arrays [count, ...]); 0 keeps the group."""
        count = self.batch if count is None else count
        self._call("update_device", int(src_device), first, count, *_dev(dG, dA, dc, dh, db))

    def update_rhs_device(self, src_device: int, dc=0, dh=0, db=0, first: int = 0, count: int | None = None):
        """update_rhs from raw pointers into the HBM of GPU `src_device` (arrays [count, ...]); 0 keeps the group.  Asynchronous."""
        count = self.batch if count is None else count
        self._call("update_rhs_device", int(src_device), first, count, *_dev(dc, dh, db))

    def update_param_device(self, src_device: int, dtheta, first: int = 0, count: int | None = None):
        """update_param from a raw pointer into the HBM of GPU `src_device` (theta [count, k], global instance order).  Asynchronous."""
        count = self.batch if count is None else count
        self._call("update_param_device", int(src_device), first, count, *_dev(dtheta))

    def shards(self):
        """[(first, count, device)] of every shard."""
        out = []
        for s in range(_lib().eicos_multi_num_shards(self._h)):
            hh, f, c, d = C.c_void_p(), C.c_int(), C.c_int(), C.c_int()
            _mchk(_lib().eicos_multi_shard(self._h, s, C.byref(hh), C.byref(f), C.byref(c), C.byref(d)))
            out.append((f.value, c.value, d.value))
        return out

    def _shard_handle(self, s, count=None):
        """The eicos_batch handle of shard s (eicos_multi_shard); count: a c_int that receives the shard's instance count."""
        hh = C.c_void_p()
        _mchk(_lib().eicos_multi_shard(self._h, s, C.byref(hh), None, None if count is None else C.byref(count), None))
        return hh

    def shard_update_device(self, s: int, dG=0, dA=0, dc=0, dh=0, db=0):
        """updateData of shard s from raw pointers into the HBM of THAT shard's GPU (arrays [count of the shard, ...]): inputs resident
        on every device -- no copy at all (eicos_batch_update_device on the shard's handle)."""
        c = C.c_int()
        hh = self._shard_handle(s, c)
        _chk(_lib().eicos_batch_update_device(hh, 0, c.value, *_dev(dG, dA, dc, dh, db)))

    def shard_last_update(self, s: int):
        """(path, HIP-event ms) of shard s's most recent updateData."""
        hh = self._shard_handle(s)
        ms = C.c_float()
        _chk(_lib().eicos_batch_last_update_ms(hh, C.byref(ms)))
        return UPDATE_PATHS[_lib().eicos_batch_last_update_path(hh)], float(ms.value)

    def shard_shared_values(self, s: int) -> bool:
        """BatchSolver.shared_values of shard s: every shard compares with ITS first instance and reads its own reference."""
        return bool(_nonneg(_lib().eicos_batch_shared_values(self._shard_handle(s))))

    def shard_dims(self, s: int = 0) -> dict:
        d = Dims()
        _chk(_lib().eicos_batch_dims(self._shard_handle(s), C.byref(d)))
        return d.asdict()

    def last_solve_ms(self):
        """(max over the shards, [per shard]) of the most recent solve's HIP-event duration."""
        n = _lib().eicos_multi_num_shards(self._h)
        mx, per = C.c_float(), (C.c_float * n)()
        _mchk(_lib().eicos_multi_last_solve_ms(self._h, C.byref(mx), per))
        return float(mx.value), [float(v) for v in per]


def _host_check(fn, keys, pat, seed, order_mode):
    _keep, ptrs = _pattern_ptrs(pat)
    st = np.zeros(8, np.int32)
    r = fn(pat.n, pat.m, pat.p, pat.ncones, *ptrs, seed, order_mode, _ip(st))
    return float(r), dict(zip(keys, (int(v) for v in st)))


def host_check_tiles(pat, seed: int = 1, order_mode: int = -1, hybrid: bool = False):
    """Host-only check of the tile (dense-front) plan, or of the hybrid plan (scalar programs + tiles on the top block
    of the tree; residual -10 = the pattern does not qualify) -- no GPU: returns (relative residual, stats dict)."""
    fn = _lib().eicos_debug_host_check_hybrid if hybrid else _lib().eicos_debug_host_check_tiles
    return _host_check(fn, ("dim_K", "nnzK", "nnzL", "block_levels", "tile_pairs", "order_mode", "blocks", "tiles"), pat, seed, order_mode)


def host_check(pat, seed: int = 1, order_mode: int = -1):
    """Host-only check of the symbolic analysis (no GPU): returns (relative residual, stats dict)."""
    keys = ("dim_K", "nnzK", "nnzL", "nlevels", "factor_pairs", "order_mode", "max_row", "max_col")
    return _host_check(_lib().eicos_debug_host_check, keys, pat, seed, order_mode)
