// Entry points of api.cpp that the multi-GPU layer (multi.cpp) uses and include/eicos_amd.h does not publish.
#pragma once
#include "../../include/eicos_amd.h"

extern "C" {
// updateData from buffers that are not in the handle's HBM: host memory (src_dev < 0) or the HBM of GPU `src_dev`; rhs = 1: the
// right-hand-side-only update (G, A NULL)
int eicos_internal_update_staged(eicos_batch *h, int first, int count, const double *G, const double *A,
                                 const double *c, const double *hh, const double *b, int src_dev, int rhs);
// the parametric update (eicos_batch_update_param) from such buffers: theta [count][k]
int eicos_internal_update_param_staged(eicos_batch *h, int first, int count, const double *theta, int src_dev);
int eicos_internal_device(const eicos_batch *h);
// ms from the start of `from`'s most recent solve to the end of `to`'s (two handles on one device)
int eicos_internal_solve_span_ms(eicos_batch *from, eicos_batch *to, float *ms);
}
