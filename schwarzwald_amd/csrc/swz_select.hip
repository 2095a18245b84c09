// swz_select.hip -- the rows of a closed box, compacted in their order (swz_box_select_device): what swz_dataset_query
// (swz_query.hip) runs on every chunk.  Two launches around the library's scan: select_count_kernel leaves the number of
// selected rows of every tile of SEL_TILE rows (wave ballot, popcount, the wave totals summed in LDS), scan_exclusive_u32
// turns the tile counts into the tiles' first output rows and the total, which the host reads before anything is written
// (the capacity refusal touches no output), and select_scatter_kernel evaluates the predicate again, ranks the selected rows
// inside the tile the same way and moves them.  No atomic decides a place: the output is the same bytes on every run.
//
// The scatter, per workgroup: the tile's positions come into LDS as consecutive doubles; every lane takes its row's three
// out of it, the selected ones go back into the SAME array at 3 x rank (rank <= lane, behind a barrier), and the compacted
// run leaves as consecutive doubles.  The source row of every output row stays in LDS: lane t then moves output row t of the
// tile column by column -- 8- and 12-byte rows as whole words, consecutive lanes consecutive addresses; the 1-, 2- and
// 3-byte rows as plain per-row stores (putting them together into dwords has not been measured).
#include <cmath>
#include <cstring>
#include <string>

#include "swz_device.h"
#include "swz_hostio.h"
#include "swz_select.h"

namespace swz {

constexpr uint32_t SEL_TILE = 256;  // rows per workgroup, one per thread
constexpr uint64_t SEL_MAX_ROWS = 0xFFFFFFFFull - 65535ull;
constexpr uint32_t SEL_WAVES = SEL_TILE / WAVE;
constexpr uint32_t SEL_BYTES[SWZ_ATTR_COUNT] = {3, 12, 2, 1, 1, 8, 1, 1, 2, 1, 1, 1};  // ATTR_BYTES (swz_hostio.h), for the compiler

struct SelectBox {
  double lo[3], hi[3];
};

struct SelectArgs {
  const double* xyz;
  uint32_t n;
  SelectBox box;
  const uint32_t* tile_first;  // scanned tile counts
  double* xyz_out;
  uint32_t* row_out;  // may be null
  const uint8_t* in[SWZ_ATTR_COUNT];
  uint8_t* out[SWZ_ATTR_COUNT];  // null: the column is not moved
};

// closed on every face; a NaN compares false and is outside
__device__ __forceinline__ bool select_inside(const SelectBox& b, double x, double y, double z) {
  return x >= b.lo[0] && x <= b.hi[0] && y >= b.lo[1] && y <= b.hi[1] && z >= b.lo[2] && z <= b.hi[2];
}

// the rank of this lane's row among the tile's selected rows, and their number; every lane of the workgroup calls it
__device__ __forceinline__ uint32_t select_rank(bool in, uint32_t* s_wave, uint32_t* total) {
  const uint32_t lane = threadIdx.x % WAVE, wave = threadIdx.x / WAVE;
  const uint64_t bal = __ballot(in);
  if (lane == 0) s_wave[wave] = (uint32_t)__popcll(bal);
  __syncthreads();
  uint32_t before = 0, all = 0;
#pragma unroll
  for (uint32_t w = 0; w < SEL_WAVES; ++w) {
    const uint32_t v = s_wave[w];
    before += w < wave ? v : 0u;
    all += v;
  }
  *total = all;
  return before + (uint32_t)__popcll(bal & ((1ull << lane) - 1ull));
}

__global__ __launch_bounds__(SEL_TILE) void select_count_kernel(const double* __restrict__ xyz, uint32_t n, SelectBox box,
                                                                uint32_t* __restrict__ tile_count) {
  __shared__ uint32_t s_wave[SEL_WAVES];
  const uint64_t r = (uint64_t)blockIdx.x * SEL_TILE + threadIdx.x;
  bool in = false;
  if (r < n) in = select_inside(box, xyz[3 * r], xyz[3 * r + 1], xyz[3 * r + 2]);
  uint32_t total;
  (void)select_rank(in, s_wave, &total);
  if (threadIdx.x == 0) tile_count[blockIdx.x] = total;
}

template <uint32_t W>
__device__ __forceinline__ void select_move(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, uint64_t src, uint64_t dst) {
  if constexpr (W == 8) {
    reinterpret_cast<uint64_t*>(out)[dst] = reinterpret_cast<const uint64_t*>(in)[src];
  } else if constexpr (W == 12) {
    const uint32_t* i4 = reinterpret_cast<const uint32_t*>(in) + 3 * src;
    uint32_t* o4 = reinterpret_cast<uint32_t*>(out) + 3 * dst;
    const uint32_t a = i4[0], b = i4[1], c = i4[2];
    o4[0] = a;
    o4[1] = b;
    o4[2] = c;
  } else if constexpr (W == 2) {
    reinterpret_cast<uint16_t*>(out)[dst] = reinterpret_cast<const uint16_t*>(in)[src];
  } else {
#pragma unroll
    for (uint32_t i = 0; i < W; ++i) out[W * dst + i] = in[W * src + i];
  }
}

__global__ __launch_bounds__(SEL_TILE) void select_scatter_kernel(SelectArgs a) {
  __shared__ double s_xyz[3 * SEL_TILE];
  __shared__ uint32_t s_src[SEL_TILE];
  __shared__ uint32_t s_wave[SEL_WAVES];
  const uint32_t t = threadIdx.x;
  const uint64_t r0 = (uint64_t)blockIdx.x * SEL_TILE;
  const uint32_t rows = (uint32_t)min((uint64_t)SEL_TILE, (uint64_t)a.n - r0);
  for (uint32_t i = t; i < 3u * rows; i += SEL_TILE) s_xyz[i] = a.xyz[3 * r0 + i];
  __syncthreads();
  double x = 0, y = 0, z = 0;
  bool in = false;
  if (t < rows) {
    x = s_xyz[3 * t];
    y = s_xyz[3 * t + 1];
    z = s_xyz[3 * t + 2];
    in = select_inside(a.box, x, y, z);
  }
  uint32_t cnt;
  const uint32_t rank = select_rank(in, s_wave, &cnt);  // (its barrier: every lane holds its row before the array is reused)
  if (cnt == 0u) return;                                // (block-uniform)
  if (in) {
    s_xyz[3 * rank] = x;
    s_xyz[3 * rank + 1] = y;
    s_xyz[3 * rank + 2] = z;
    s_src[rank] = t;
  }
  __syncthreads();
  const uint64_t base = a.tile_first[blockIdx.x];
  for (uint32_t i = t; i < 3u * cnt; i += SEL_TILE) a.xyz_out[3 * base + i] = s_xyz[i];
  if (t >= cnt) return;
  const uint64_t src = r0 + s_src[t], dst = base + t;
  if (a.row_out) a.row_out[dst] = (uint32_t)src;
#pragma unroll
  for (int k = 0; k < SWZ_ATTR_COUNT; ++k) {
    if (!a.out[k]) continue;  // (block-uniform)
    switch (k) {
      case SWZ_ATTR_RGB: select_move<3>(a.in[k], a.out[k], src, dst); break;
      case SWZ_ATTR_NORMAL: select_move<12>(a.in[k], a.out[k], src, dst); break;
      case SWZ_ATTR_INTENSITY:
      case SWZ_ATTR_POINT_SOURCE_ID: select_move<2>(a.in[k], a.out[k], src, dst); break;
      case SWZ_ATTR_GPS_TIME: select_move<8>(a.in[k], a.out[k], src, dst); break;
      default: select_move<1>(a.in[k], a.out[k], src, dst); break;
    }
  }
}

static bool overlap(const void* a, uint64_t a_bytes, const void* b, uint64_t b_bytes) {
  if (!a || !b || !a_bytes || !b_bytes) return false;
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return a0 < b0 + b_bytes && b0 < a0 + a_bytes;
}

int box_select(swz_ctx* c, const char* who, const double* d_xyz, uint64_t n, const swz_attribute_columns* d_in, uint32_t mask,
               const double box_min[3], const double box_max[3], uint64_t capacity, double* d_xyz_out,
               const swz_attribute_columns* d_out, uint32_t* d_row_out, uint64_t* count_out) {
  auto refuse = [&](const std::string& what) { return c->fail(SWZ_ERR_BAD_ARG, std::string(who) + ": " + what); };
  static_assert(SEL_BYTES[SWZ_ATTR_RGB] == 3 && SEL_BYTES[SWZ_ATTR_NORMAL] == 12 && SEL_BYTES[SWZ_ATTR_INTENSITY] == 2 &&
                  SEL_BYTES[SWZ_ATTR_POINT_SOURCE_ID] == 2 && SEL_BYTES[SWZ_ATTR_GPS_TIME] == 8,
                "the widths select_scatter_kernel moves");
  for (int k = 0; k < SWZ_ATTR_COUNT; ++k)
    if (SEL_BYTES[k] != ATTR_BYTES[k]) return c->fail(SWZ_ERR_INTERNAL, "swz_select.hip: SEL_BYTES is not ATTR_BYTES");
  // ---- everything is checked on the host before anything is launched
  if (!box_min || !box_max || !count_out) return refuse("NULL argument");
  *count_out = 0;
  const bool count_only = !d_xyz_out && capacity == 0;
  if (!d_xyz_out && !count_only) return refuse("NULL d_xyz_out with a capacity (count only: NULL and capacity 0)");
  if (n > SEL_MAX_ROWS) return refuse("more than 2^32-65536 rows");
  if (mask & ~((1u << SWZ_ATTR_COUNT) - 1u)) return refuse("the mask names an attribute that does not exist");
  if (!finite3(box_min) || !finite3(box_max)) return refuse("a bound of the box is not finite");
  for (int k = 0; k < 3; ++k)
    if (box_min[k] > box_max[k]) return refuse("box_min > box_max");
  for (int k = 0; k < SWZ_ATTR_COUNT; ++k) {
    if (!((mask >> k) & 1u)) continue;
    if (!d_in || !d_in->column[k]) return refuse("a bit of the mask without an input column");
    if (!count_only && (!d_out || !d_out->column[k])) return refuse("a bit of the mask without an output column");
    const uintptr_t align = ATTR_BYTES[k] == 8 ? 8 : ATTR_BYTES[k] == 12 ? 4 : ATTR_BYTES[k] == 2 ? 2 : 1;
    if ((uintptr_t)d_in->column[k] % align || (!count_only && (uintptr_t)d_out->column[k] % align))
      return refuse("a column that is not aligned to its element");
  }
  if (n && !d_xyz) return refuse("NULL d_xyz");
  if (((uintptr_t)d_xyz | (uintptr_t)d_xyz_out) % 8u || (uintptr_t)d_row_out % 4u) return refuse("positions or rows that are not aligned to their element");
  if (!count_only) {
    // an output that is (part of) an input: the tiles run in any order
    const void* outs[SWZ_ATTR_COUNT + 2];
    uint64_t out_bytes[SWZ_ATTR_COUNT + 2];
    outs[0] = d_xyz_out;
    out_bytes[0] = 24 * capacity;
    outs[1] = d_row_out;
    out_bytes[1] = 4 * capacity;
    for (int k = 0; k < SWZ_ATTR_COUNT; ++k) {
      outs[2 + k] = ((mask >> k) & 1u) ? d_out->column[k] : nullptr;
      out_bytes[2 + k] = (uint64_t)ATTR_BYTES[k] * capacity;
    }
    for (int o = 0; o < SWZ_ATTR_COUNT + 2; ++o) {
      bool alias = overlap(outs[o], out_bytes[o], d_xyz, 24 * n);
      for (int k = 0; k < SWZ_ATTR_COUNT; ++k)
        alias = alias || (((mask >> k) & 1u) && overlap(outs[o], out_bytes[o], d_in->column[k], (uint64_t)ATTR_BYTES[k] * n));
      if (alias) return refuse("an output aliases an input");
    }
  }
  if (n == 0) return SWZ_OK;

  SWZ_HIP(c, hipSetDevice(c->device));
  const uint32_t nb = div_up(n, SEL_TILE);
  uint32_t *d_tiles = nullptr, *d_total = nullptr;
  SWZ_TRY(c->get("sel_tiles", (size_t)nb, &d_tiles));
  SWZ_TRY(c->get("sel_total", (size_t)1, &d_total));
  SelectArgs a{};
  a.xyz = d_xyz;
  a.n = (uint32_t)n;
  for (int k = 0; k < 3; ++k) {
    a.box.lo[k] = box_min[k];
    a.box.hi[k] = box_max[k];
  }
  {
    ProfScope ps(c, "box_select_count", 24 * n, 1);
    hipLaunchKernelGGL(select_count_kernel, dim3(nb), dim3(SEL_TILE), 0, c->stream, d_xyz, a.n, a.box, d_tiles);
    SWZ_LAUNCH_CHECK(c);
  }
  SWZ_TRY(scan_exclusive_u32(c, d_tiles, d_tiles, nb, d_total, "sel"));
  uint32_t total = 0;
  SWZ_TRY(read_u32(c, d_total, &total));
  *count_out = total;
  if (count_only || total == 0) return SWZ_OK;
  if (total > capacity)
    return refuse("capacity " + std::to_string(capacity) + " is less than the " + std::to_string(total) + " rows of the box");
  a.tile_first = d_tiles;
  a.xyz_out = d_xyz_out;
  a.row_out = d_row_out;
  uint64_t row_bytes = 24 + (d_row_out ? 4 : 0);
  for (int k = 0; k < SWZ_ATTR_COUNT; ++k) {
    if (!((mask >> k) & 1u)) continue;
    a.in[k] = static_cast<const uint8_t*>(d_in->column[k]);
    a.out[k] = static_cast<uint8_t*>(d_out->column[k]);
    row_bytes += 2 * ATTR_BYTES[k];
  }
  {
    ProfScope ps(c, "box_select_scatter", 24 * n + row_bytes * total, 1);
    hipLaunchKernelGGL(select_scatter_kernel, dim3(nb), dim3(SEL_TILE), 0, c->stream, a);
    SWZ_LAUNCH_CHECK(c);
  }
  SWZ_HIP(c, hipStreamSynchronize(c->stream));
  return SWZ_OK;
}

}  // namespace swz

using namespace swz;

extern "C" {

uint32_t swz_box_select_tile(void) { return SEL_TILE; }

int swz_box_select_device(swz_ctx* c, const double* d_xyz, uint64_t n, const swz_attribute_columns* d_in, uint32_t attribute_mask,
                          const double box_min[3], const double box_max[3], uint64_t capacity, double* d_xyz_out,
                          const swz_attribute_columns* d_out, uint32_t* d_row_out, uint64_t* count_out) {
  if (!c) return SWZ_ERR_BAD_ARG;
  return box_select(c, "swz_box_select_device", d_xyz, n, d_in, attribute_mask, box_min, box_max, capacity, d_xyz_out, d_out, d_row_out,
                    count_out);
}

}  // extern "C"
