// swz_select.h -- the selection (swz_select.hip) for the callers inside the library: the three entries
// swz_box_select_device, swz_region_select_device and swz_filter_select_device, and the data-set query (swz_query.hip),
// which runs it chunk by chunk.  All of them describe what they select in one Selection and call region_select.
#pragma once
#include <algorithm>
#include <cstring>
#include <vector>

#include "swz_internal.h"

namespace swz {

// a swz_region checked and copied (host only): what the node rule of swz_qplan.hip reads
struct RegionHost {
  int kind = SWZ_REGION_BOX;
  uint32_t count = 0;
  std::vector<double> v;  // count x (a, b, c, d) or count x (x, y)
};
// the refusals of include/swz_gpu.h, `who` in front; region == NULL is the box.  c may be NULL (only the status comes back).
int region_check(swz_ctx* c, const char* who, const swz_region* region, RegionHost* out);
// the polygon test of include/swz_gpu.h on the host, operation for operation what the kernel evaluates
bool region_polygon_inside(const RegionHost& r, double px, double py);

// what the kernels take: planes by value, a polygon's vertices in the workspace buffer "sel_poly"
struct RegionPlanes {
  double p[SWZ_REGION_MAX_PLANES][4];
  uint32_t count;
};
struct RegionDev {
  int kind = SWZ_REGION_BOX;
  RegionPlanes planes{};
  const double* d_xy = nullptr;  // polygon: count x (x, y)
  uint32_t vertices = 0;
};
// uploads a polygon's vertices (once per call; once per query); synchronises c's stream
int region_upload(swz_ctx* c, const RegionHost& r, RegionDev* out);

// swz_filter_check for the callers inside the library: `who` in front of the text, c may be NULL (only the status comes
// back).  *attrs_out: the mask of the attributes the clauses name (0 without a filter).
int filter_check(swz_ctx* c, const char* who, const swz_filter* filter, uint32_t* attrs_out);
// "SWZ_ATTR_CLASSIFICATION", for the refusals
const char* attribute_name(int attribute);

// What a call selects: the rows of the closed box that the region keeps and that pass the filter.  The region is one that
// region_check has passed: `region`, still on the host -- region_select uploads it once every other check has passed -- or
// `uploaded`, already on the device (the query: once for all chunks); neither is the box alone.  `filter`: one that
// filter_check has passed, or NULL; one without a clause selects what NULL selects.
struct Selection {
  const double *box_min, *box_max;  // [3] each; a NULL is refused
  const RegionHost* region;
  const RegionDev* uploaded;
  const swz_filter* filter;
};

// The three select entries as include/swz_gpu.h describes them; `who` starts the messages.  Synchronises c's stream.
int region_select(swz_ctx* c, const char* who, const double* d_xyz, uint64_t n, const swz_attribute_columns* d_in, uint32_t mask,
                  const Selection& sel, uint64_t capacity, double* d_xyz_out, const swz_attribute_columns* d_out, uint32_t* d_row_out,
                  uint64_t* count_out);

}  // namespace swz
