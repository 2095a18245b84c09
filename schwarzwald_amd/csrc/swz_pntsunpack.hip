// swz_pntsunpack.hip -- .pnts node files unpacked on the device: the inverse of pnts_pack_kernel (swz_pnts.hip) and the 3D
// Tiles counterpart of swz_binunpack.hip, whose staging it shares (swz_unpackstage.h).
//
// A SEGMENT is what one file contributes: up to three arrays -- POSITION (3 x f32), RGB (3 x u8), INTENSITY (u16) -- each
// wherever the file's JSON puts it, so at any residue of the raw image and in any order.  One workgroup takes PNTU_TILE
// consecutive output rows whatever segments they belong to, lists the segments of those rows in LDS and then, array by array,
// stages the aligned dwords that cover the tile's part of every segment's run and lets every lane take its row's value out of
// the stage as shifted dwords.  Positions are widened with the plain cast -- exact for every float -- into a second LDS array
// that holds the tile's rows as they lie in the output, and leave from there as consecutive 16-byte pieces on consecutive
// lanes (a lane storing its own row would make three 8-byte stores at a stride of 24).
//
// LDS of a workgroup: 3 KB of first rows, counts and masks, 6 KB of array offsets, 5136 bytes of stage (12 * 256 / 4 + 2 *
// 256 + 4 dwords), 6 KB of widened positions: 20.5 KB, so a CU's 160 KB keep its eight workgroups of 256 threads resident.
#include <string>
#include <vector>

#include "swz_convert.h"
#include "swz_device.h"
#include "swz_hostio.h"
#include "swz_unpackstage.h"

static_assert(sizeof(swz_pnts_segment) == 48, "swz_pnts_segment as include/swz_gpu.h and the bindings lay it out");

namespace swz {

constexpr uint32_t PNTU_TILE = 256;  // output rows per workgroup, one per thread
constexpr uint32_t PNTU_PIECES = 3;  // POSITION, RGB, INTENSITY
constexpr uint32_t PNTU_STAGE = 12 * PNTU_TILE / 4 + 2 * PNTU_TILE + 4;
constexpr uint64_t PNTU_MAX_POINTS = 0xFFFFFFFFull - 65535ull;
constexpr uint32_t PNTU_MASK_ALL = SWZ_PNTS_RGB | SWZ_PNTS_INTENSITY;

struct PntsUnpackArgs {
  const uint8_t* raw;
  uint64_t raw_bytes;
  const swz_pnts_segment* segs;  // the segments that hold points; first_row ascends, every row belongs to exactly one
  uint32_t num_segs;
  uint32_t n;  // rows
  double* xyz;  // null: skipped, like the two columns
  uint8_t* rgb;
  uint16_t* intensity;
};

__global__ __launch_bounds__(PNTU_TILE) void pnts_unpack_kernel(PntsUnpackArgs a) {
  __shared__ uint32_t s_first[PNTU_TILE];  // first rows of the segments k0 .. k0 + PNTU_TILE - 1 (past the table: no row)
  __shared__ uint32_t s_count[PNTU_TILE];
  __shared__ uint32_t s_mask[PNTU_TILE];   // bit p: the segment holds piece p
  __shared__ uint64_t s_at[PNTU_PIECES][PNTU_TILE];
  __shared__ uint32_t s_stage[PNTU_STAGE];
  __shared__ __align__(16) double s_xyz[3 * PNTU_TILE];
  const uint32_t t = threadIdx.x;
  const uint32_t r0 = blockIdx.x * PNTU_TILE;
  const uint32_t r1 = (uint32_t)min((uint64_t)r0 + PNTU_TILE, (uint64_t)a.n);

  const uint32_t k0 = unpack_first_segment(a.segs, a.num_segs, r0);
  {
    const bool listed = k0 + t < a.num_segs;
    const swz_pnts_segment* sg = a.segs + k0 + t;
    s_first[t] = listed ? (uint32_t)sg->first_row : 0xFFFFFFFFu;
    s_count[t] = listed ? (uint32_t)sg->count : 0u;
    s_mask[t] = listed ? 1u | ((sg->mask & SWZ_PNTS_RGB) ? 2u : 0u) | ((sg->mask & SWZ_PNTS_INTENSITY) ? 4u : 0u) : 0u;
    s_at[0][t] = listed ? sg->position_offset : 0ull;
    s_at[1][t] = listed ? sg->rgb_offset : 0ull;
    s_at[2][t] = listed ? sg->intensity_offset : 0ull;
  }
  __syncthreads();

  const uint32_t nwin = unpack_window_size<PNTU_TILE>(s_first, r1);
  // this lane's row and its entry
  const uint32_t r = r0 + t;
  const bool live = r < r1;
  const uint32_t my = live ? unpack_row_entry(s_first, nwin, r) : 0u;
  const uintptr_t raw_begin = (uintptr_t)a.raw, raw_end = raw_begin + a.raw_bytes;

  for (uint32_t piece = 0; piece < PNTU_PIECES; ++piece) {
    if (piece == 0u ? !a.xyz : piece == 1u ? !a.rgb : !a.intensity) continue;  // (block-uniform)
    const uint32_t w = piece == 0u ? 12u : piece == 1u ? 3u : 2u;
    // where entry e's run of this piece lies: rows [lo, lo + len) of the tile, bytes [G, G + w len) of memory, from dword
    // S of the stage on; len == 0: the entry's segment lacks the array
    auto run = [&](uint32_t e, uint32_t* lo, uint32_t* len, uintptr_t* G, uint32_t* S) {
      const uint32_t first = s_first[e], count = s_count[e];
      *lo = max(first, r0);
      const uint32_t hi = min(first + count, r1);
      *len = ((s_mask[e] >> piece) & 1u) ? hi - *lo : 0u;
      *G = raw_begin + (uintptr_t)s_at[piece][e] + (uintptr_t)w * (*lo - first);
      *S = ((w * (*lo - r0)) >> 2) + 2u * e;
    };

    stage_fill<PNTU_TILE>(s_stage, s_first, nwin, w, r0, r1, raw_begin, raw_end, run);
    __syncthreads();

    // ---- every lane its row's value out of the stage, zeros where the segment lacks the array
    uint32_t q = 0;
    bool present = false;
    if (live) {
      uint32_t lo, len, S;
      uintptr_t G;
      run(my, &lo, &len, &G, &S);
      present = len != 0u;
      q = 4u * S + (uint32_t)(G & 3u) + w * (r - lo);
    }
    if (piece == 0u) {
      // the tile's rows as they lie in the output, then 16-byte pieces of that on consecutive lanes
      if (live) {
#pragma unroll
        for (uint32_t i = 0; i < 3u; ++i) s_xyz[3u * t + i] = present ? (double)__uint_as_float(stage_word(s_stage, q + 4u * i)) : 0.0;
      }
      __syncthreads();  // (the stage is the next piece's after it, too)
      const uint32_t doubles = 3u * (r1 - r0);
      double* const dst = a.xyz + 3u * (size_t)r0;  // 6144 bytes per tile: as aligned as a.xyz is
      if (((uintptr_t)a.xyz & 15u) == 0u) {
        for (uint32_t x = t; x < (doubles >> 1); x += PNTU_TILE)
          reinterpret_cast<double2*>(dst)[x] = reinterpret_cast<const double2*>(s_xyz)[x];
        if ((doubles & 1u) && t == 0u) dst[doubles - 1u] = s_xyz[doubles - 1u];
      } else {
        for (uint32_t x = t; x < doubles; x += PNTU_TILE) dst[x] = s_xyz[x];
      }
      continue;  // (s_xyz is written once per launch)
    }
    if (live) {
      if (piece == 1u) {
        const uint32_t v = present ? stage_word(s_stage, q) : 0u;
        uint8_t* const o = a.rgb + (size_t)r * 3u;
        o[0] = (uint8_t)v;
        o[1] = (uint8_t)(v >> 8);
        o[2] = (uint8_t)(v >> 16);
      } else {
        a.intensity[r] = present ? (uint16_t)stage_word(s_stage, q) : (uint16_t)0;
      }
    }
    __syncthreads();  // the stage is the next piece's
  }
}

int pnts_unpack_launch(swz_ctx* c, hipStream_t stream, const uint8_t* d_raw, uint64_t raw_bytes, const swz_pnts_segment* d_table,
                       uint32_t num_segs, uint32_t rows, double* d_xyz_out, const swz_attribute_columns* d_out) {
  if (!rows || !num_segs) return SWZ_OK;
  PntsUnpackArgs a{};
  a.raw = d_raw;
  a.raw_bytes = raw_bytes;
  a.segs = d_table;
  a.num_segs = num_segs;
  a.n = rows;
  a.xyz = d_xyz_out;
  a.rgb = static_cast<uint8_t*>(d_out ? d_out->column[SWZ_ATTR_RGB] : nullptr);
  a.intensity = static_cast<uint16_t*>(d_out ? d_out->column[SWZ_ATTR_INTENSITY] : nullptr);
  hipLaunchKernelGGL(pnts_unpack_kernel, dim3(div_up(rows, PNTU_TILE)), dim3(PNTU_TILE), 0, stream, a);
  SWZ_LAUNCH_CHECK(c);
  return SWZ_OK;
}

}  // namespace swz

using namespace swz;

extern "C" {

uint32_t swz_pnts_unpack_tile(void) { return PNTU_TILE; }

int swz_pnts_unpack_segments_device(swz_ctx* c, const uint8_t* d_raw, uint64_t raw_bytes, const swz_pnts_segment* segments,
                                    uint64_t num_segments, double* d_xyz_out, const swz_attribute_columns* d_out) {
  if (!c) return SWZ_ERR_BAD_ARG;
  auto refuse = [&](const char* what) { return c->fail(SWZ_ERR_BAD_ARG, std::string("swz_pnts_unpack_segments_device: ") + what); };
  // everything is checked on the host before anything is launched
  if (num_segments && !segments) return refuse("NULL segments");
  for (int a = 0; d_out && a < SWZ_ATTR_COUNT; ++a)
    if (d_out->column[a] && a != SWZ_ATTR_RGB && a != SWZ_ATTR_INTENSITY)
      return refuse("a .pnts file holds RGB and intensity besides the positions: no other output column can be filled");
  if (d_out && d_out->column[SWZ_ATTR_INTENSITY] && ((uintptr_t)d_out->column[SWZ_ATTR_INTENSITY] & 1u))
    return refuse("the intensity column must be 2-byte aligned");
  if ((uintptr_t)d_xyz_out & 7u) return refuse("the positions must be 8-byte aligned");
  auto inside = [&](uint64_t offset, uint64_t bytes) { return offset <= raw_bytes && bytes <= raw_bytes - offset; };
  std::vector<swz_pnts_segment> table;
  uint64_t rows = 0, bytes = 0;
  for (uint64_t s = 0; s < num_segments; ++s) {
    const swz_pnts_segment& sg = segments[s];
    if (sg.first_row != rows) return refuse("the rows of the segments must ascend contiguously from 0");
    if (sg.mask & ~PNTU_MASK_ALL) return refuse("the mask names an array a .pnts file does not hold");
    if (sg.reserved != 0u) return refuse("reserved must be 0");
    if (sg.count > PNTU_MAX_POINTS || rows + sg.count > PNTU_MAX_POINTS) return refuse("more than 2^32-65536 rows");
    if (!inside(sg.position_offset, 12 * sg.count) || ((sg.mask & SWZ_PNTS_RGB) && !inside(sg.rgb_offset, 3 * sg.count)) ||
        ((sg.mask & SWZ_PNTS_INTENSITY) && !inside(sg.intensity_offset, 2 * sg.count)))
      return refuse("an array of a segment passes raw_bytes");
    rows += sg.count;
    bytes += sg.count * (12 + ((sg.mask & SWZ_PNTS_RGB) ? 3 : 0) + ((sg.mask & SWZ_PNTS_INTENSITY) ? 2 : 0));
    if (sg.count) table.push_back(sg);
  }
  if (rows == 0) return SWZ_OK;
  if (!d_raw) return refuse("NULL image");
  SWZ_HIP(c, hipSetDevice(c->device));
  swz_pnts_segment* d_table = nullptr;
  SWZ_TRY(c->get("pnts_segments", table.size(), &d_table));
  SWZ_HIP(c, hipMemcpyAsync(d_table, table.data(), table.size() * sizeof(swz_pnts_segment), hipMemcpyHostToDevice, c->stream));
  {
    ProfScope ps(c, "pnts_unpack_segments", 3 * bytes, 1);
    SWZ_TRY(pnts_unpack_launch(c, c->stream, d_raw, raw_bytes, d_table, (uint32_t)table.size(), (uint32_t)rows, d_xyz_out, d_out));
  }
  SWZ_HIP(c, hipStreamSynchronize(c->stream));  // (the table's host copy lives until here)
  return SWZ_OK;
}

}  // extern "C"
