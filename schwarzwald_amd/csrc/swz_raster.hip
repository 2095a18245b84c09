// swz_raster.hip -- the raster of include/swz_gpu.h: per cell of a grid in x-y the count, the integer sum and the min / max
// codes of a value of the rows inside a closed box.  The frame of a grid (swz_raster_frame_of) and the decode of a table
// (swz_raster_finish) are host code; the preset of a table and the accumulate kernel run on the device.
//
// The accumulate kernel: one workgroup takes RAS_TILE consecutive rows, one per lane.  A lane tests its row against the box
// with the compares of the selection (swz_select.hip), finds its cell -- a subtraction, a division and a floor per axis, then
// the clamp -- and its value: z, or the element of the value's column.  Rows come in stored order, close to Morton order, so
// the lanes of a wave fall into few cells: a lane whose cell differs from the lane below it heads a run (lanes outside the box
// carry a cell number no cell has, so they break a run and form runs of their own that write nothing), the ballot of the heads
// tells every lane where its run ends, and six rounds of shuffles reduce every run onto its head: count, sum of
// q = llrint((v - v0) * scale), min and max of the order-preserving codes of swz_nodebox.h.  The head issues four relaxed
// agent-scope 64-bit atomics on its cell.  Integer add, min and max commute: the table is the same bits whatever the order of
// the workgroups, the chunking or the runs.  No LDS, no barrier.
#include <cmath>
#include <cstddef>
#include <cstring>
#include <limits>
#include <string>

#include "swz_device.h"
#include "swz_hostio.h"
#include "swz_nodebox.h"
#include "swz_raster.h"
#include "swz_select.h"

static_assert(sizeof(swz_raster_grid) == 16 && offsetof(swz_raster_grid, value) == 8 && sizeof(swz_raster_frame) == 64 &&
                offsetof(swz_raster_frame, v0) == 32 && offsetof(swz_raster_frame, nx) == 48 && offsetof(swz_raster_frame, value) == 56 &&
                sizeof(swz_raster_cell) == 32 && offsetof(swz_raster_cell, sum) == 8 && offsetof(swz_raster_cell, min_code) == 16 &&
                offsetof(swz_raster_cell, max_code) == 24,
              "the structs of the raster as include/swz_gpu.h and the bindings lay them out");

namespace swz {

constexpr uint32_t RAS_TILE = 256;  // rows per workgroup, one per lane
constexpr uint32_t RAS_NO_CELL = 0xFFFFFFFFu;  // (a table holds 2^26 cells at the most)
enum { RAS_Z = 0, RAS_U8 = 1, RAS_I8 = 2, RAS_U16 = 3 };

struct RasterBox {
  double lo[3], hi[3];
};

__global__ void raster_clear_kernel(swz_raster_cell* __restrict__ cells, uint32_t n) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  swz_raster_cell e;
  e.count = 0;
  e.sum = 0;
  e.min_code = BOX_CODE_POS_INF;
  e.max_code = BOX_CODE_NEG_INF;
  cells[i] = e;
}

// the index along one axis: floor((p - p0) / side) clamped to cells - 1; a flat axis (side 0, one cell) divides nothing.
// p0 <= p for a row of the box, so the quotient is >= 0; a quotient that is no number below cells - 1 takes the last cell.
__device__ __forceinline__ uint32_t raster_axis(double p, double p0, double side, uint32_t cells) {
  if (cells == 1u) return 0u;
  const double f = floor((p - p0) / side);
  return f < (double)(cells - 1u) ? (uint32_t)f : cells - 1u;
}

template <int KIND>
__global__ __launch_bounds__(RAS_TILE) void raster_accumulate_kernel(const double* __restrict__ xyz, uint32_t n, RasterBox box,
                                                                     swz_raster_frame f, const uint8_t* __restrict__ col,
                                                                     swz_raster_cell* __restrict__ cells) {
  const uint32_t lane = threadIdx.x % WAVE;
  const uint64_t r = (uint64_t)blockIdx.x * RAS_TILE + threadIdx.x;
  uint32_t cell = RAS_NO_CELL;
  uint32_t cnt = 0;
  long long sum = 0;
  unsigned long long lo = BOX_CODE_POS_INF, hi = BOX_CODE_NEG_INF;
  if (r < n) {
    const double x = xyz[3 * r], y = xyz[3 * r + 1], z = xyz[3 * r + 2];
    // closed on every face; a NaN compares false and is outside (select_inside of swz_select.hip)
    if (x >= box.lo[0] && x <= box.hi[0] && y >= box.lo[1] && y <= box.hi[1] && z >= box.lo[2] && z <= box.hi[2]) {
      cell = raster_axis(y, f.y0, f.ch, f.ny) * f.nx + raster_axis(x, f.x0, f.cw, f.nx);
      double v;
      if constexpr (KIND == RAS_Z) {
        v = z;
        sum = llrint((v - f.v0) * f.scale);
      } else {
        int32_t e;  // the element as a filter's RANGE clause reads it (clause_passes of swz_select.hip)
        if constexpr (KIND == RAS_U16) e = reinterpret_cast<const uint16_t*>(col)[r];
        else if constexpr (KIND == RAS_I8) e = reinterpret_cast<const int8_t*>(col)[r];
        else e = col[r];
        v = (double)e;
        sum = e;  // v0 = 0, scale = 1
      }
      cnt = 1;
      lo = hi = box_code(v);
    }
  }
  // where this lane's run ends: the next lane above it that heads a run, or the end of the wave
  const uint32_t cell_before = __shfl_up(cell, 1u, WAVE);
  const bool head = lane == 0u || cell_before != cell;
  const unsigned long long heads = __ballot(head);
  const unsigned long long above = heads & ~((2ull << lane) - 1ull);  // (lane 63: 2 << 63 is 0, the mask all ones)
  const uint32_t end = above ? (uint32_t)__ffsll((long long)above) - 1u : (uint32_t)WAVE;
#pragma unroll
  for (uint32_t i = 0; i < 6; ++i) {
    const uint32_t cnt_far = __shfl_down(cnt, 1u << i, WAVE);
    const long long sum_far = __shfl_down(sum, 1u << i, WAVE);
    const unsigned long long lo_far = __shfl_down(lo, 1u << i, WAVE);
    const unsigned long long hi_far = __shfl_down(hi, 1u << i, WAVE);
    if (lane + (1u << i) < end) {  // lane + 2^i is in this lane's run and holds the run's next 2^i lanes
      cnt += cnt_far;
      sum += sum_far;
      lo = min(lo, lo_far);
      hi = max(hi, hi_far);
    }
  }
  if (head && cell != RAS_NO_CELL) {  // cell < nx * ny: both indices are clamped
    swz_raster_cell* const out = cells + cell;
    (void)__hip_atomic_fetch_add(reinterpret_cast<unsigned long long*>(&out->count), (unsigned long long)cnt, __ATOMIC_RELAXED,
                                 __HIP_MEMORY_SCOPE_AGENT);
    (void)__hip_atomic_fetch_add(reinterpret_cast<long long*>(&out->sum), sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    (void)__hip_atomic_fetch_min(reinterpret_cast<unsigned long long*>(&out->min_code), lo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    (void)__hip_atomic_fetch_max(reinterpret_cast<unsigned long long*>(&out->max_code), hi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

static int raster_kind(int value) {
  if (value == SWZ_RASTER_VALUE_Z) return RAS_Z;
  if (ATTR_BYTES[value] == 2) return RAS_U16;
  return value == SWZ_ATTR_SCAN_ANGLE_RANK ? RAS_I8 : RAS_U8;
}

swz_raster_cell raster_empty_cell() {
  swz_raster_cell e{};
  e.min_code = BOX_CODE_POS_INF;
  e.max_code = BOX_CODE_NEG_INF;
  return e;
}

int raster_frame(swz_ctx* c, const char* who, const double box_min[3], const double box_max[3], const swz_raster_grid* grid,
                 swz_raster_frame* frame_out) {
  auto refuse = [&](const std::string& what) { return fail(c, SWZ_ERR_BAD_ARG, std::string(who) + ": " + what); };
  if (!box_min || !box_max || !grid || !frame_out) return refuse("NULL argument");
  if (grid->reserved) return refuse("the grid's reserved must be 0");
  if (grid->nx == 0 || grid->ny == 0) return refuse("nx or ny is 0");
  if ((uint64_t)grid->nx * grid->ny > SWZ_RASTER_MAX_CELLS)
    return refuse("nx * ny is more than SWZ_RASTER_MAX_CELLS (2^26): " + std::to_string(grid->nx) + " x " + std::to_string(grid->ny));
  if (!finite3(box_min) || !finite3(box_max)) return refuse("a bound of the box is not finite");
  for (int a = 0; a < 3; ++a)
    if (box_min[a] > box_max[a]) return refuse("box_min > box_max");
  if (grid->value != SWZ_RASTER_VALUE_Z) {
    if (grid->value < 0 || grid->value >= SWZ_ATTR_COUNT) return refuse("a value that is neither SWZ_RASTER_VALUE_Z nor an attribute of the table");
    if (ATTR_BYTES[grid->value] > 2 || grid->value == SWZ_ATTR_RGB)
      return refuse(std::string(attribute_name(grid->value)) + " is not a value the raster takes (z, or a scalar column of one or two bytes)");
  }
  if (box_min[0] == box_max[0] && grid->nx != 1) return refuse("the box is flat along x (box_min == box_max) and nx is not 1");
  if (box_min[1] == box_max[1] && grid->ny != 1) return refuse("the box is flat along y (box_min == box_max) and ny is not 1");
  swz_raster_frame f{};
  f.x0 = box_min[0];
  f.y0 = box_min[1];
  f.cw = (box_max[0] - box_min[0]) / (double)grid->nx;
  f.ch = (box_max[1] - box_min[1]) / (double)grid->ny;
  f.nx = grid->nx;
  f.ny = grid->ny;
  f.value = grid->value;
  f.v0 = 0.0;
  f.scale = 1.0;
  const double range = box_max[2] - box_min[2];
  if (!std::isfinite(f.cw) || !std::isfinite(f.ch) || !std::isfinite(range)) return refuse("the box is wider than a double holds");
  if (grid->value == SWZ_RASTER_VALUE_Z) {
    f.v0 = box_min[2];
    int k = 0;
    if (range != 0.0) k = std::min(900, std::max(-900, 30 - std::ilogb(range)));
    f.scale = std::ldexp(1.0, k);
  }
  *frame_out = f;
  return SWZ_OK;
}

// is `frame` what raster_frame makes of the box and the frame's own nx, ny and value?  Bit for bit.
static int raster_frame_check(swz_ctx* c, const char* who, const double box_min[3], const double box_max[3], const swz_raster_frame* frame) {
  auto refuse = [&](const std::string& what) { return fail(c, SWZ_ERR_BAD_ARG, std::string(who) + ": " + what); };
  if (!frame || !box_min || !box_max) return refuse("NULL argument");
  swz_raster_grid grid{};
  grid.nx = frame->nx;
  grid.ny = frame->ny;
  grid.value = frame->value;
  grid.reserved = frame->reserved;
  swz_raster_frame want;
  SWZ_TRY(raster_frame(c, who, box_min, box_max, &grid, &want));
  if (memcmp(&want, frame, sizeof(want)) != 0) return refuse("the frame is not the one swz_raster_frame_of derives from this box");
  return SWZ_OK;
}

int raster_clear(swz_ctx* c, const char* who, const swz_raster_frame* frame, swz_raster_cell* d_cells) {
  auto refuse = [&](const std::string& what) { return c->fail(SWZ_ERR_BAD_ARG, std::string(who) + ": " + what); };
  if (!frame || !d_cells) return refuse("NULL argument");
  const uint64_t n = (uint64_t)frame->nx * frame->ny;
  if (n == 0 || n > SWZ_RASTER_MAX_CELLS) return refuse("a frame of no cell or of more than SWZ_RASTER_MAX_CELLS");
  if ((uintptr_t)d_cells % 8u) return refuse("cells that are not aligned to their element");
  SWZ_HIP(c, hipSetDevice(c->device));
  ProfScope ps(c, "raster_clear", n * sizeof(swz_raster_cell), 1);
  hipLaunchKernelGGL(raster_clear_kernel, dim3(div_up(n, 256)), dim3(256), 0, c->stream, d_cells, (uint32_t)n);
  SWZ_LAUNCH_CHECK(c);
  return SWZ_OK;
}

int raster_accumulate(swz_ctx* c, const char* who, const double* d_xyz, uint64_t n, const void* d_value, const double box_min[3],
                      const double box_max[3], const swz_raster_frame* frame, swz_raster_cell* d_cells) {
  auto refuse = [&](const std::string& what) { return c->fail(SWZ_ERR_BAD_ARG, std::string(who) + ": " + what); };
  // ---- everything is checked on the host before anything is launched
  SWZ_TRY(raster_frame_check(c, who, box_min, box_max, frame));
  if (!d_cells) return refuse("NULL d_cells");
  if (n > BOX_MAX_POINTS) return refuse("more than 2^32-65536 rows");
  if (n && !d_xyz) return refuse("NULL d_xyz");
  if ((uintptr_t)d_xyz % 8u || (uintptr_t)d_cells % 8u) return refuse("positions or cells that are not aligned to their element");
  const int kind = raster_kind(frame->value);
  if (kind != RAS_Z) {
    if (n && !d_value) return refuse(std::string("the value is ") + attribute_name(frame->value) + ", which has no input column");
    if ((uintptr_t)d_value % ATTR_BYTES[frame->value]) return refuse(std::string("the column of ") + attribute_name(frame->value) + " is not aligned to its element");
  }
  if (n == 0) return SWZ_OK;

  SWZ_HIP(c, hipSetDevice(c->device));
  RasterBox box;
  for (int a = 0; a < 3; ++a) {
    box.lo[a] = box_min[a];
    box.hi[a] = box_max[a];
  }
  const uint8_t* col = static_cast<const uint8_t*>(d_value);
  const dim3 grid(div_up(n, RAS_TILE)), block(RAS_TILE);
  {
    ProfScope ps(c, "raster_accumulate", (24 + (kind == RAS_Z ? 0 : ATTR_BYTES[frame->value])) * n, 1);
    if (kind == RAS_Z) hipLaunchKernelGGL(raster_accumulate_kernel<RAS_Z>, grid, block, 0, c->stream, d_xyz, (uint32_t)n, box, *frame, col, d_cells);
    else if (kind == RAS_U16) hipLaunchKernelGGL(raster_accumulate_kernel<RAS_U16>, grid, block, 0, c->stream, d_xyz, (uint32_t)n, box, *frame, col, d_cells);
    else if (kind == RAS_I8) hipLaunchKernelGGL(raster_accumulate_kernel<RAS_I8>, grid, block, 0, c->stream, d_xyz, (uint32_t)n, box, *frame, col, d_cells);
    else hipLaunchKernelGGL(raster_accumulate_kernel<RAS_U8>, grid, block, 0, c->stream, d_xyz, (uint32_t)n, box, *frame, col, d_cells);
    SWZ_LAUNCH_CHECK(c);
  }
  SWZ_HIP(c, hipStreamSynchronize(c->stream));
  return SWZ_OK;
}

}  // namespace swz

using namespace swz;

extern "C" {

uint32_t swz_raster_tile(void) { return RAS_TILE; }

int swz_raster_frame_of(const double box_min[3], const double box_max[3], const swz_raster_grid* grid, swz_raster_frame* frame_out,
                        char* why_out, uint64_t why_bytes) {
  swz_ctx text;  // (only its error text is used: no device is touched)
  return why_text(raster_frame(&text, "swz_raster_frame_of", box_min, box_max, grid, frame_out), text, why_out, why_bytes);
}

int swz_raster_finish(const swz_raster_frame* frame, const swz_raster_cell* cells, uint64_t* count_out, double* min_out, double* max_out,
                      double* mean_out) {
  if (!frame || !cells) return SWZ_ERR_BAD_ARG;
  const uint64_t n = (uint64_t)frame->nx * frame->ny;
  if (n == 0 || n > SWZ_RASTER_MAX_CELLS) return SWZ_ERR_BAD_ARG;
  for (uint64_t i = 0; i < n; ++i) {
    const swz_raster_cell& e = cells[i];
    if (count_out) count_out[i] = e.count;
    if (min_out) min_out[i] = box_decode(e.min_code);
    if (max_out) max_out[i] = box_decode(e.max_code);
    if (mean_out) {
      double mean = std::numeric_limits<double>::quiet_NaN();
      if (e.count) {
        const double per_row = (double)e.sum / (double)e.count;
        const double steps = per_row / frame->scale;
        mean = frame->v0 + steps;
      }
      mean_out[i] = mean;
    }
  }
  return SWZ_OK;
}

int swz_raster_clear_device(swz_ctx* c, const swz_raster_frame* frame, swz_raster_cell* d_cells) {
  if (!c) return SWZ_ERR_BAD_ARG;
  SWZ_TRY(raster_clear(c, "swz_raster_clear_device", frame, d_cells));
  SWZ_HIP(c, hipStreamSynchronize(c->stream));
  return SWZ_OK;
}

int swz_raster_accumulate_device(swz_ctx* c, const double* d_xyz, uint64_t n, const void* d_value, const double box_min[3],
                                 const double box_max[3], const swz_raster_frame* frame, swz_raster_cell* d_cells) {
  if (!c) return SWZ_ERR_BAD_ARG;
  return raster_accumulate(c, "swz_raster_accumulate_device", d_xyz, n, d_value, box_min, box_max, frame, d_cells);
}

}  // extern "C"
