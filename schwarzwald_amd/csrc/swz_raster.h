// swz_raster.h -- the raster (swz_raster.hip) for the callers inside the library: the frame of a grid, the preset of a cell
// table and the accumulate kernel's launch.  swz_raster_frame_of, swz_raster_clear_device and swz_raster_accumulate_device
// are these three behind the C ABI; swz_dataset_rasterize (swz_qraster.hip) runs them around the chunks of a data set.
#pragma once
#include "swz_internal.h"

namespace swz {

// the refusals and the arithmetic of include/swz_gpu.h, `who` in front of the text; host only, c may be NULL (only the status
// comes back)
int raster_frame(swz_ctx* c, const char* who, const double box_min[3], const double box_max[3], const swz_raster_grid* grid,
                 swz_raster_frame* frame_out);
// an empty cell: count 0, sum 0, the codes of +inf and -inf
swz_raster_cell raster_empty_cell();
// presets the frame's nx * ny cells on c's stream; no synchronisation
int raster_clear(swz_ctx* c, const char* who, const swz_raster_frame* frame, swz_raster_cell* d_cells);
// adds n rows to the table as include/swz_gpu.h describes it; everything is checked before the launch.  Synchronises c's
// stream: the rows may be a chunk's, which the next chunk's unpack overwrites.
int raster_accumulate(swz_ctx* c, const char* who, const double* d_xyz, uint64_t n, const void* d_value, const double box_min[3],
                      const double box_max[3], const swz_raster_frame* frame, swz_raster_cell* d_cells);

}  // namespace swz
