// swz_select.hip -- the selection: the rows of a closed box, cut by a region (planes, or a polygon in x-y) and filtered by
// up to eight clauses over the attribute columns (the formulas: include/swz_gpu.h), compacted in their order.  It is what
// swz_box_select_device, swz_region_select_device and swz_filter_select_device run, and what swz_dataset_query* (swz_query.hip)
// runs on every chunk: one host path, region_select, for all of them.
//
// Two launches around the library's scan.  select_count_kernel<R, FILTER> leaves the number of selected rows of every tile of
// SEL_TILE rows (wave ballot, popcount, the wave totals summed in LDS); scan_exclusive_u32 turns the tile counts into the
// tiles' first output rows and the total, which the host reads before anything is written (the capacity refusal touches no
// output); select_scatter_kernel<BALLOTS> ranks the selected rows inside the tile the same way and moves them.  No atomic
// decides a place: the output is the same bytes on every run.
//
// The count pass, per row: the box, then the region's test (R: RegionNone, RegionPlanes in the kernel arguments,
// RegionPolygon staged in LDS), then with FILTER the clauses in order, a column element loaded only for a row that is still
// in; the filter travels in the kernel arguments, and without one the instantiation has no such parameters.  Who decides a
// row in the scatter follows from it.  The box alone, <RegionNone, false>: the scatter tests the box again
// (select_scatter_kernel<false>).  Every other instantiation also stores each wave's ballot, and select_scatter_kernel<true>
// reads it back in place of a predicate, so the edge loop of a polygon (up to 1024 iterations of FP64 per row) and the
// clauses run once per row, in a kernel that holds no other LDS to speak of.
//
// The scatter, per workgroup: the tile's positions come into LDS as consecutive doubles; every lane takes its row's three
// out of it, the selected ones go back into the SAME array at 3 x rank (rank <= lane, behind a barrier), and the compacted
// run leaves as consecutive doubles.  The source row of every output row stays in LDS: lane t then moves output row t of the
// tile column by column -- 8- and 12-byte rows as whole words, consecutive lanes consecutive addresses; the 1-, 2- and
// 3-byte rows as plain per-row stores (putting them together into dwords has not been measured).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <type_traits>

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
__device__ __forceinline__ uint32_t select_rank(bool in, uint32_t* s_wave, uint32_t* total, uint64_t* ballot = nullptr) {
  const uint32_t lane = threadIdx.x % WAVE, wave = threadIdx.x / WAVE;
  const uint64_t bal = __ballot(in);
  if (ballot) *ballot = bal;
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

// ---- regions: the box cut by planes or by a polygon in x-y
struct RegionNone {};  // the box alone

struct RegionPolygon {
  const double* xy;  // vertices x (x, y)
  uint32_t vertices;
};

// every plane: ((a*x + b*y) + c*z) + d >= 0, four separately rounded operations (the library is built without contraction)
__device__ __forceinline__ bool planes_inside(const RegionPlanes& P, double x, double y, double z) {
  bool in = true;
  for (uint32_t k = 0; k < P.count; ++k) in = in && ((P.p[k][0] * x + P.p[k][1] * y) + P.p[k][2] * z) + P.p[k][3] >= 0.0;
  return in;
}

// even-odd over the edges (v[i], v[(i+1) mod m]); the parity does not care that the closing edge comes first.  Every lane
// reads the same LDS address: a broadcast.
__device__ __forceinline__ bool polygon_inside(const double* s_xy, uint32_t m, double px, double py) {
  bool odd = false;
  double x0 = s_xy[2 * (m - 1)], y0 = s_xy[2 * (m - 1) + 1];
  for (uint32_t i = 0; i < m; ++i) {
    const double x1 = s_xy[2 * i], y1 = s_xy[2 * i + 1];
    if ((y0 > py) != (y1 > py)) {
      const double t = (x1 - x0) * (py - y0) - (px - x0) * (y1 - y0);
      odd ^= (t > 0.0) == (y1 > y0);
    }
    x0 = x1;
    y0 = y1;
  }
  return odd;
}

// ---- filters: clauses over the attribute columns, behind the region
struct FilterCols {
  const uint8_t* col[SWZ_FILTER_MAX_CLAUSES];  // clause k's column
};

// one clause on row r.  Every field of cl and col are the same for all lanes (kernel arguments: scalar registers); only the
// element is per lane.  The four words of a set are chosen by compares, not by an index a lane computes.
__device__ __forceinline__ bool clause_passes(const swz_filter_clause& cl, const uint8_t* __restrict__ col, uint64_t r) {
  bool pass;
  if ((cl.kind & 0xFFu) == SWZ_FILTER_SET) {
    const uint32_t b = col[r];  // the stored byte, unsigned
    const uint64_t w01 = (b & 64u) ? cl.set[1] : cl.set[0], w23 = (b & 64u) ? cl.set[3] : cl.set[2];
    pass = ((((b & 128u) ? w23 : w01) >> (b & 63u)) & 1ull) != 0;
  } else {
    double v;  // exact for every type
    switch (cl.attribute) {
      case SWZ_ATTR_GPS_TIME: v = reinterpret_cast<const double*>(col)[r]; break;
      case SWZ_ATTR_INTENSITY:
      case SWZ_ATTR_POINT_SOURCE_ID: v = (double)reinterpret_cast<const uint16_t*>(col)[r]; break;
      case SWZ_ATTR_SCAN_ANGLE_RANK: v = (double)reinterpret_cast<const int8_t*>(col)[r]; break;
      default: v = (double)col[r]; break;
    }
    pass = cl.lo <= v && v <= cl.hi;  // (a NaN fails both)
  }
  return pass != ((cl.kind & SWZ_FILTER_NOT) != 0u);
}

// ---- the count pass
struct Absent {};  // in place of a kernel parameter that an instantiation does not have: one byte of the argument block
template <bool HAS, class T>
using ArgIf = std::conditional_t<HAS, T, Absent>;
template <bool HAS, class T>
static ArgIf<HAS, T> arg_if(const T* v) {
  if constexpr (HAS) return *v;
  else return {};
}

// does select_count_kernel<R, FILTER> leave ballots for select_scatter_kernel<true>?  All but the box alone.
template <class R, bool FILTER>
constexpr bool COUNT_BALLOTS = FILTER || !std::is_same_v<R, RegionNone>;

// R is RegionNone, RegionPlanes (in the kernel arguments) or RegionPolygon (staged in LDS: 16 KiB at the most, which with the
// 16 bytes of the ranking leaves the 32 waves of a CU their room in its 160 KiB).  Box, then the region's test -- only the
// rows of the box walk a polygon's edges, and the box keeps NaN out of both tests --, then with FILTER the clauses in order:
// a lane loads a clause's element only while its row is still in (r < n then), and the loop over the clauses is the same
// for the whole wave.  ballots: one word per wave of every tile.  The parameters stay kernel parameters that the body reads
// directly: behind an argument struct the compiler loads the whole block up front (EXPERIMENTS.md).
template <class R, bool FILTER>
__global__ __launch_bounds__(SEL_TILE) void select_count_kernel(const double* __restrict__ xyz, uint32_t n, SelectBox box,
                                                                R region, ArgIf<FILTER, swz_filter> filter,
                                                                ArgIf<FILTER, FilterCols> cols, uint32_t* __restrict__ tile_count,
                                                                ArgIf<COUNT_BALLOTS<R, FILTER>, uint64_t* __restrict__> ballots) {
  __shared__ uint32_t s_wave[SEL_WAVES];
  const uint64_t r = (uint64_t)blockIdx.x * SEL_TILE + threadIdx.x;
  double x = 0, y = 0, z = 0;
  bool in = false;
  if (r < n) {
    x = xyz[3 * r];
    y = xyz[3 * r + 1];
    z = xyz[3 * r + 2];
    in = select_inside(box, x, y, z);
  }
  if constexpr (std::is_same_v<R, RegionPolygon>) {
    __shared__ double s_xy[2 * SWZ_REGION_MAX_VERTICES];
    for (uint32_t i = threadIdx.x; i < 2u * region.vertices; i += SEL_TILE) s_xy[i] = region.xy[i];
    __syncthreads();
    if (in) in = polygon_inside(s_xy, region.vertices, x, y);
  } else if constexpr (std::is_same_v<R, RegionPlanes>) {
    if (in) in = planes_inside(region, x, y, z);
  }
  if constexpr (FILTER)
    for (uint32_t k = 0; k < filter.count; ++k)
      if (in) in = clause_passes(filter.clause[k], cols.col[k], r);
  uint32_t total;
  uint64_t bal;
  (void)select_rank(in, s_wave, &total, &bal);
  if constexpr (COUNT_BALLOTS<R, FILTER>)
    if (threadIdx.x % WAVE == 0) ballots[(uint64_t)blockIdx.x * SEL_WAVES + threadIdx.x / WAVE] = bal;
  if (threadIdx.x == 0) tile_count[blockIdx.x] = total;
}

// the launch of one instantiation; `a` holds the rows and the box, filter and cols are read only with FILTER
template <class R, bool FILTER>
static void select_count_launch(hipStream_t stream, uint32_t nb, const SelectArgs& a, const R& region, const swz_filter* filter,
                                const FilterCols* cols, uint32_t* d_tiles, uint64_t* d_ballots) {
  hipLaunchKernelGGL((select_count_kernel<R, FILTER>), dim3(nb), dim3(SEL_TILE), 0, stream, a.xyz, a.n, a.box, region, arg_if<FILTER>(filter),
                     arg_if<FILTER>(cols), d_tiles, arg_if<COUNT_BALLOTS<R, FILTER>>(&d_ballots));
}

// ---- the scatter
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

// The scatter, instantiated over who decides a row.  BALLOTS false: the box test, here (the box alone; `ballots` is not
// read).  BALLOTS true: the count pass has decided every row and left its waves' ballots.
template <bool BALLOTS>
__global__ __launch_bounds__(SEL_TILE) void select_scatter_kernel(SelectArgs a, const uint64_t* __restrict__ ballots) {
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
    if constexpr (BALLOTS) in = ((ballots[(uint64_t)blockIdx.x * SEL_WAVES + t / WAVE] >> (t % WAVE)) & 1ull) != 0;
    else in = select_inside(a.box, x, y, z);
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

const char* attribute_name(int attribute) {
  static const char* const names[SWZ_ATTR_COUNT] = {"SWZ_ATTR_RGB", "SWZ_ATTR_NORMAL", "SWZ_ATTR_INTENSITY", "SWZ_ATTR_CLASSIFICATION",
                                                    "SWZ_ATTR_EDGE_OF_FLIGHT_LINE", "SWZ_ATTR_GPS_TIME", "SWZ_ATTR_NUMBER_OF_RETURNS",
                                                    "SWZ_ATTR_RETURN_NUMBER", "SWZ_ATTR_POINT_SOURCE_ID", "SWZ_ATTR_SCAN_DIRECTION_FLAG",
                                                    "SWZ_ATTR_SCAN_ANGLE_RANK", "SWZ_ATTR_USER_DATA"};
  return attribute >= 0 && attribute < SWZ_ATTR_COUNT ? names[attribute] : "an attribute outside the table";
}

// the rules of include/swz_gpu.h, the one place they live
int filter_check(swz_ctx* c, const char* who, const swz_filter* f, uint32_t* attrs_out) {
  auto refuse = [&](const std::string& what) { return fail(c, SWZ_ERR_BAD_ARG, std::string(who) + ": " + what); };
  if (attrs_out) *attrs_out = 0;
  if (!f) return SWZ_OK;
  if (f->count > SWZ_FILTER_MAX_CLAUSES) return refuse("a filter holds " + std::to_string(SWZ_FILTER_MAX_CLAUSES) + " clauses at the most");
  if (f->reserved) return refuse("the filter's reserved must be 0");
  uint32_t attrs = 0;
  for (uint32_t k = 0; k < f->count; ++k) {
    const swz_filter_clause& cl = f->clause[k];
    auto no = [&](const std::string& what) { return refuse("clause " + std::to_string(k) + ": " + what); };
    if (cl.attribute < 0 || cl.attribute >= SWZ_ATTR_COUNT) return no("an attribute outside the table");
    if (cl.attribute == SWZ_ATTR_RGB || cl.attribute == SWZ_ATTR_NORMAL)
      return no(std::string(attribute_name(cl.attribute)) + " is not a scalar column");
    if (cl.kind & ~(0xFFu | SWZ_FILTER_NOT)) return no("an unknown flag bit in kind");
    const uint32_t kind = cl.kind & 0xFFu;
    if (kind != SWZ_FILTER_RANGE && kind != SWZ_FILTER_SET) return no("an unknown kind");
    const bool any_set = (cl.set[0] | cl.set[1] | cl.set[2] | cl.set[3]) != 0;
    if (kind == SWZ_FILTER_SET) {
      if (ATTR_BYTES[cl.attribute] != 1) return no(std::string("a SET on ") + attribute_name(cl.attribute) + ", a column wider than a byte");
      if (!(cl.lo == 0.0 && cl.hi == 0.0)) return no("a SET with a lo or hi that is not 0");
    } else {
      if (std::isnan(cl.lo) || std::isnan(cl.hi)) return no("a RANGE with a NaN bound");
      if (cl.lo > cl.hi) return no("a RANGE with lo > hi");
      if (any_set) return no("a RANGE with a set that is not 0");
    }
    attrs |= 1u << cl.attribute;
  }
  if (attrs_out) *attrs_out = attrs;
  return SWZ_OK;
}

int region_check(swz_ctx* c, const char* who, const swz_region* region, RegionHost* out) {
  auto refuse = [&](const std::string& what) { return fail(c, SWZ_ERR_BAD_ARG, std::string(who) + ": " + what); };
  *out = RegionHost{};
  if (!region) return SWZ_OK;
  if (region->kind != SWZ_REGION_BOX && region->kind != SWZ_REGION_PLANES && region->kind != SWZ_REGION_POLYGON)
    return refuse("an unknown kind of region");
  if (region->reserved) return refuse("the region's reserved must be 0");
  if (region->kind == SWZ_REGION_BOX) {
    if (region->count) return refuse("a box region with a count that is not 0");
    return SWZ_OK;
  }
  const bool planes = region->kind == SWZ_REGION_PLANES;
  if (planes && (region->count < 1 || region->count > SWZ_REGION_MAX_PLANES)) return refuse("a region of planes holds 1 to 16 of them");
  if (!planes && (region->count < 3 || region->count > SWZ_REGION_MAX_VERTICES)) return refuse("a polygon region holds 3 to 1024 vertices");
  if (!region->values) return refuse("a region with NULL values");
  const size_t len = (size_t)region->count * (planes ? 4 : 2);
  for (size_t i = 0; i < len; ++i)
    if (!std::isfinite(region->values[i])) return refuse(planes ? "a coefficient of a plane is not finite" : "a vertex of the polygon is not finite");
  if (planes)
    for (uint32_t k = 0; k < region->count; ++k)
      if (region->values[4 * k] == 0.0 && region->values[4 * k + 1] == 0.0 && region->values[4 * k + 2] == 0.0)
        return refuse("a plane with a = b = c = 0");
  out->kind = region->kind;
  out->count = region->count;
  out->v.assign(region->values, region->values + len);
  return SWZ_OK;
}

bool region_polygon_inside(const RegionHost& r, double px, double py) {
  const uint32_t m = r.count;
  bool odd = false;
  for (uint32_t i = 0; i < m; ++i) {
    const double x0 = r.v[2 * i], y0 = r.v[2 * i + 1], x1 = r.v[2 * ((i + 1) % m)], y1 = r.v[2 * ((i + 1) % m) + 1];
    if ((y0 > py) != (y1 > py)) {
      const double t = (x1 - x0) * (py - y0) - (px - x0) * (y1 - y0);
      odd ^= (t > 0.0) == (y1 > y0);
    }
  }
  return odd;
}

int region_upload(swz_ctx* c, const RegionHost& r, RegionDev* out) {
  *out = RegionDev{};
  out->kind = r.kind;
  if (r.kind == SWZ_REGION_PLANES) {
    out->planes.count = r.count;
    memcpy(out->planes.p, r.v.data(), r.v.size() * sizeof(double));
  } else if (r.kind == SWZ_REGION_POLYGON) {
    double* d_xy = nullptr;
    SWZ_HIP(c, hipSetDevice(c->device));
    SWZ_TRY(c->get("sel_poly", (size_t)2 * SWZ_REGION_MAX_VERTICES, &d_xy));
    SWZ_HIP(c, hipMemcpyAsync(d_xy, r.v.data(), r.v.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
    SWZ_HIP(c, hipStreamSynchronize(c->stream));  // (r.v is the caller's)
    out->d_xy = d_xy;
    out->vertices = r.count;
  }
  return SWZ_OK;
}

static bool overlap(const void* a, uint64_t a_bytes, const void* b, uint64_t b_bytes) {
  if (!a || !b || !a_bytes || !b_bytes) return false;
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return a0 < b0 + b_bytes && b0 < a0 + a_bytes;
}

int region_select(swz_ctx* c, const char* who, const double* d_xyz, uint64_t n, const swz_attribute_columns* d_in, uint32_t mask,
                  const Selection& sel, uint64_t capacity, double* d_xyz_out, const swz_attribute_columns* d_out, uint32_t* d_row_out,
                  uint64_t* count_out) {
  const double *box_min = sel.box_min, *box_max = sel.box_max;
  const int kind = sel.region ? sel.region->kind : sel.uploaded ? sel.uploaded->kind : SWZ_REGION_BOX;
  const swz_filter* filter = sel.filter && sel.filter->count ? sel.filter : nullptr;  // no clause: no filter
  uint32_t fmask = 0;  // the columns the clauses read
  for (uint32_t k = 0; filter && k < filter->count; ++k) fmask |= 1u << filter->clause[k].attribute;
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
  for (int k = 0; k < SWZ_ATTR_COUNT; ++k) {
    if (!((fmask >> k) & 1u)) continue;
    if (!d_in || !d_in->column[k]) return refuse(std::string("the filter names ") + attribute_name(k) + ", which has no input column");
    if ((uintptr_t)d_in->column[k] % ATTR_BYTES[k]) return refuse("a column that is not aligned to its element");  // (1, 2 or 8 bytes)
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
        alias = alias || ((((mask | fmask) >> k) & 1u) && overlap(outs[o], out_bytes[o], d_in->column[k], (uint64_t)ATTR_BYTES[k] * n));
      if (alias) return refuse("an output aliases an input");
    }
  }
  if (n == 0) return SWZ_OK;

  SWZ_HIP(c, hipSetDevice(c->device));
  const RegionDev* region = sel.uploaded;
  RegionDev uploaded;
  if (sel.region) {
    SWZ_TRY(region_upload(c, *sel.region, &uploaded));
    region = &uploaded;
  }
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
  // all but the box alone: the count pass decides every row and hands its ballots to the scatter
  const bool ballots = filter || kind != SWZ_REGION_BOX;
  const uint64_t ballot_bytes = ballots ? 8ull * nb * SEL_WAVES : 0;
  uint64_t* d_ballots = nullptr;
  if (ballots) SWZ_TRY(c->get("sel_ballots", (size_t)nb * SEL_WAVES, &d_ballots));
  FilterCols fc{};
  uint64_t col_bytes = 0;  // (at the most: a lane reads only while its row is in)
  for (uint32_t k = 0; filter && k < filter->count; ++k) {
    fc.col[k] = static_cast<const uint8_t*>(d_in->column[filter->clause[k].attribute]);
    col_bytes += ATTR_BYTES[filter->clause[k].attribute];
  }
  static const char* const scopes[4][2] = {{"box_select_count", "box_select_scatter"},
                                           {"planes_select_count", "planes_select_scatter"},
                                           {"polygon_select_count", "polygon_select_scatter"},
                                           {"filter_select_count", "filter_select_scatter"}};
  static_assert(SWZ_REGION_BOX == 0 && SWZ_REGION_PLANES == 1 && SWZ_REGION_POLYGON == 2, "the rows of scopes");
  const char* const* scope = scopes[filter ? 3 : kind];
  {
    ProfScope ps(c, scope[0], (24 + col_bytes) * n + ballot_bytes, 1);
    auto count = [&](const auto& r) {
      using R = std::decay_t<decltype(r)>;
      (filter ? select_count_launch<R, true> : select_count_launch<R, false>)(c->stream, nb, a, r, filter, &fc, d_tiles, d_ballots);
    };
    if (kind == SWZ_REGION_PLANES) count(region->planes);
    else if (kind == SWZ_REGION_POLYGON) count(RegionPolygon{region->d_xy, region->vertices});
    else count(RegionNone{});
    SWZ_LAUNCH_CHECK(c);
  }
  SWZ_TRY(scan_exclusive_u32(c, d_tiles, d_tiles, nb, d_total, "sel"));
  uint32_t total = 0;
  SWZ_TRY(read_u32(c, d_total, &total));
  *count_out = total;
  if (count_only || total == 0) return SWZ_OK;
  if (total > capacity)
    return refuse("capacity " + std::to_string(capacity) + " is less than the " + std::to_string(total) +
                  (filter ? " rows that pass the filter" : kind == SWZ_REGION_BOX ? " rows of the box" : " rows of the region"));
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
    ProfScope ps(c, scope[1], 24 * n + ballot_bytes + row_bytes * total, 1);
    if (ballots) hipLaunchKernelGGL(select_scatter_kernel<true>, dim3(nb), dim3(SEL_TILE), 0, c->stream, a, (const uint64_t*)d_ballots);
    else hipLaunchKernelGGL(select_scatter_kernel<false>, dim3(nb), dim3(SEL_TILE), 0, c->stream, a, (const uint64_t*)nullptr);
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
  const Selection sel{box_min, box_max, nullptr, nullptr, nullptr};
  return region_select(c, "swz_box_select_device", d_xyz, n, d_in, attribute_mask, sel, capacity, d_xyz_out, d_out, d_row_out, count_out);
}

int swz_region_select_device(swz_ctx* c, const double* d_xyz, uint64_t n, const swz_attribute_columns* d_in, uint32_t attribute_mask,
                             const double box_min[3], const double box_max[3], const swz_region* region, uint64_t capacity,
                             double* d_xyz_out, const swz_attribute_columns* d_out, uint32_t* d_row_out, uint64_t* count_out) {
  if (!c) return SWZ_ERR_BAD_ARG;
  const char* who = "swz_region_select_device";
  RegionHost host;
  SWZ_TRY(region_check(c, who, region, &host));
  const Selection sel{box_min, box_max, &host, nullptr, nullptr};
  return region_select(c, who, d_xyz, n, d_in, attribute_mask, sel, capacity, d_xyz_out, d_out, d_row_out, count_out);
}

int swz_filter_check(const swz_filter* filter, char* why_out, uint64_t why_bytes) {
  swz_ctx text;  // (only its error text is used: no device is touched)
  return why_text(filter_check(&text, "swz_filter_check", filter, nullptr), text, why_out, why_bytes);
}

int swz_filter_select_device(swz_ctx* c, const double* d_xyz, uint64_t n, const swz_attribute_columns* d_in, uint32_t attribute_mask,
                             const double box_min[3], const double box_max[3], const swz_region* region, const swz_filter* filter,
                             uint64_t capacity, double* d_xyz_out, const swz_attribute_columns* d_out, uint32_t* d_row_out,
                             uint64_t* count_out) {
  if (!c) return SWZ_ERR_BAD_ARG;
  const char* who = "swz_filter_select_device";
  RegionHost host;
  SWZ_TRY(region_check(c, who, region, &host));
  SWZ_TRY(filter_check(c, who, filter, nullptr));
  const Selection sel{box_min, box_max, &host, nullptr, filter};
  return region_select(c, who, d_xyz, n, d_in, attribute_mask, sel, capacity, d_xyz_out, d_out, d_row_out, count_out);
}

}  // extern "C"
