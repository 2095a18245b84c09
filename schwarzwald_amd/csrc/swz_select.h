// swz_select.h -- the box selection (swz_select.hip) for the callers inside the library: swz_box_select_device itself and
// swz_dataset_query (swz_query.hip), which runs it chunk by chunk.
#pragma once
#include "swz_internal.h"

namespace swz {

// swz_box_select_device as include/swz_gpu.h describes it; `who` starts the messages.  Synchronises c's stream.
int box_select(swz_ctx* c, const char* who, const double* d_xyz, uint64_t n, const swz_attribute_columns* d_in, uint32_t mask,
               const double box_min[3], const double box_max[3], uint64_t capacity, double* d_xyz_out,
               const swz_attribute_columns* d_out, uint32_t* d_row_out, uint64_t* count_out);

}  // namespace swz
