// Exit classes (include/eicos_amd.h: EICOS_SEL_*): ONE definition of the rule that maps an instance's info record to its class bit, for
// the host (eicos_exit_class) and for the selection kernel (kernels.hip: k_select_order).
#pragma once
#include "../../include/eicos_amd.h"

#if defined(__HIPCC__)
#define EICOS_HOST_DEVICE __host__ __device__
#else
#define EICOS_HOST_DEVICE
#endif

namespace eicos {
// n_factor == 0: the record is fresh -- never solved and never given a starting point -- whatever the code (0 in a fresh record)
EICOS_HOST_DEVICE inline unsigned exit_class(int exitcode, int n_factor) {
    if (n_factor == 0) return EICOS_SEL_UNSOLVED;
    switch (exitcode) {
    case EICOS_OPTIMAL: return EICOS_SEL_OPTIMAL;
    case EICOS_PINF: return EICOS_SEL_PINF;
    case EICOS_DINF: return EICOS_SEL_DINF;
    case EICOS_OPTIMAL + EICOS_INACC_OFFSET: return EICOS_SEL_OPTIMAL_INACC;
    case EICOS_PINF + EICOS_INACC_OFFSET: return EICOS_SEL_PINF_INACC;
    case EICOS_DINF + EICOS_INACC_OFFSET: return EICOS_SEL_DINF_INACC;
    case EICOS_MAXIT: return EICOS_SEL_MAXIT;
    case EICOS_NUMERICS: return EICOS_SEL_NUMERICS;
    case EICOS_OUTCONE: return EICOS_SEL_OUTCONE;
    case EICOS_FATAL: return EICOS_SEL_FATAL;
    default: return EICOS_SEL_OTHER;
    }
}
} // namespace eicos
