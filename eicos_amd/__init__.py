"""eicos_amd -- MI355X-native batched SOCP interior-point solver (EiCOS-compatible hot path).

The product is the C-ABI shared library eicos_amd/libeicos_amd.so (sources in
eicos_amd/csrc, ABI in include/eicos_amd.h).  This Python package is only a thin ctypes
mirror of that ABI for tests and bench.py.  It never imports anything from oracle/.
"""
from .binding import BatchSolver, MultiBatchSolver, FallbackMap, MatrixMap, OutputMap, ParamMap, PlantMap, ShiftMap, PinnedArray, host_register, host_unregister, Info, build_library, library_path, device_count, set_arithmetic_profile, default_settings, Settings, default_retry, Retry, rollout_data_backprop, DATA_GRADIENT_KEYS, centred_pair, ADJOINT_NT, ADJOINT_CENTRED  # noqa: F401
from .binding import (exit_class, SEL_OPTIMAL, SEL_PINF, SEL_DINF, SEL_OPTIMAL_INACC, SEL_PINF_INACC, SEL_DINF_INACC, SEL_MAXIT,  # noqa: F401
                      SEL_NUMERICS, SEL_OUTCONE, SEL_FATAL, SEL_OTHER, SEL_UNSOLVED, SEL_FAILED, SEL_NOT_OPTIMAL, SEL_ALL)
from .problem_io import Pattern, Values, read_ecos_header, read_epb, read_problem, write_ecos_header, write_epb  # noqa: F401
