// Entry points of api.cpp that the multi-GPU layer (multi.cpp) uses and include/eicos_amd.h does not publish.
#pragma once
#include "../../include/eicos_amd.h"

#include <string>
#include <vector>

extern "C" {
// updateData from buffers that are not in the handle's HBM: host memory (src_dev < 0) or the HBM of GPU `src_dev`; rhs = 1: the
// right-hand-side-only update (G, A NULL)
int eicos_internal_update_staged(eicos_batch *h, int first, int count, const double *G, const double *A,
                                 const double *c, const double *hh, const double *b, int src_dev, int rhs);
// the parametric update (eicos_batch_update_param) from such buffers: theta [count][k]
int eicos_internal_update_param_staged(eicos_batch *h, int first, int count, const double *theta, int src_dev);
int eicos_internal_device(const eicos_batch *h);
// the row widths of the per-instance plant values: k the installed plant map was validated for and its stored entries rowptr[k]; 0, 0 without one
int eicos_internal_plant_dims(const eicos_batch *h, int *k, int *nnz);
// the row widths of eicos_batch_rollout_data_gradient's slope outputs: stored entries of the c, h, b groups of the installed parameter map
// (0 for a group without one) and of the output map
int eicos_internal_map_nnz(const eicos_batch *h, int *nnz_chb, int *nnz_u);
// ms from the start of `from`'s most recent solve to the end of `to`'s (two handles on one device)
int eicos_internal_solve_span_ms(eicos_batch *from, eicos_batch *to, float *ms);
}

namespace eicos {
// What is wrong with the index list of a subset call over `batch` instances (eicos_batch_solve_subset, _gather and their eicos_multi_*
// forms, which check global ids before any shard sees its share); empty: nothing.  Duplicates are found with a bitmap.
inline std::string index_list_fault(const int *idx, int count, int batch) {
    if (count < 0 || count > batch) return "count " + std::to_string(count) + " outside [0, batch = " + std::to_string(batch) + "]";
    if (count > 0 && !idx) return "idx is NULL with count " + std::to_string(count);
    std::vector<char> seen((size_t)batch, 0);
    for (int q = 0; q < count; q++) {
        const int i = idx[q];
        if (i < 0 || i >= batch) return "index " + std::to_string(i) + " at position " + std::to_string(q) + " is outside [0, " + std::to_string(batch) + ")";
        if (seen[i]) return "duplicate index " + std::to_string(i) + " at position " + std::to_string(q) + " (two workgroups would solve one slab at once)";
        seen[i] = 1;
    }
    return std::string();
}
// ... and with a class mask (EICOS_SEL_*)
inline std::string class_mask_fault(unsigned mask) {
    if (mask == 0) return "mask is 0: it selects no exit class";
    if (mask & ~(unsigned)EICOS_SEL_ALL) return "mask has bits above bit 11 (EICOS_SEL_UNSOLVED)";
    return std::string();
}
} // namespace eicos
