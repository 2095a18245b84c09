// swz_binunpack.hip -- BinaryPersistence node files unpacked on the device: the inverse of swz_binpack.hip and the BIN / BINZ
// counterpart of the LAS segment kernel (swz_tinput.hip).
//
// The raw image holds SEGMENTS, one uncompressed file image each: 12 bytes of mask and count, count x 24 bytes of positions,
// then the arrays of the segment's mask in FILE_ORDER.  An array begins wherever the arrays in front of it end -- after 3 n
// bytes of RGB with n odd the intensities sit on odd addresses, the GPS doubles on any residue -- and the image itself may
// begin anywhere.  One workgroup takes BINU_TILE consecutive output rows, whatever segments they belong to: it finds the
// segment of its first row with one binary search in the table and puts the BINU_TILE segments from there on into LDS (a
// tile of one-point files spans that many).  Then, ARRAY BY ARRAY: what the tile holds of the array in one segment is one run
// of bytes of the image; the aligned dwords that cover the run go into a stage in LDS, consecutive lanes consecutive dwords,
// so the run lies in the stage with the residue it has in memory; a dword that does not lie wholly inside [raw, raw +
// raw_bytes) is put together from the bytes that do.  Every lane then takes its row's value out of the stage as dwords
// shifted into place -- bit copies, nothing is computed -- and stores it; a lane whose segment lacks the array stores zeros.
#include <string>
#include <vector>

#include "swz_convert.h"
#include "swz_device.h"
#include "swz_hostio.h"
#include "swz_unpackstage.h"

namespace swz {

constexpr uint32_t BINU_TILE = 256;                      // output rows per workgroup, one per thread
constexpr uint32_t BINU_PIECES = SWZ_ATTR_COUNT + 1;     // positions, then the attribute arrays in file order
constexpr uint64_t BINU_MAX_POINTS = 0xFFFFFFFFull - 65535ull;
constexpr uint32_t BINU_MASK_ALL = (1u << SWZ_ATTR_COUNT) - 1u;
// the stage of the widest piece (swz_unpackstage.h)
constexpr uint32_t BINU_STAGE = 24 * BINU_TILE / 4 + 2 * BINU_TILE + 4;
// nibble j: bytes of a row of the j-th attribute array in file order (FILE_ORDER / ATTR_BYTES of swz_hostio.h)
constexpr uint64_t BINU_WIDTHS = 0x1112118112C3ull;

struct BinUnpackArgs {
  const uint8_t* raw;
  uint64_t raw_bytes;
  const BinUnpackSeg* segs;  // the segments that hold points; first_row ascends, every row belongs to exactly one
  uint32_t num_segs;
  uint32_t n;                // rows
  void* out[BINU_PIECES];    // [0] positions, [1 + j] the column of the j-th array in file order; null: skipped
};

__device__ __host__ __forceinline__ uint32_t binu_width(uint32_t piece) {
  return piece == 0u ? 24u : (uint32_t)(BINU_WIDTHS >> (4u * (piece - 1u))) & 15u;
}
// bytes of a row in front of `piece` in an image with the arrays of file_mask
__device__ __host__ __forceinline__ uint32_t binu_prefix(uint32_t file_mask, uint32_t piece) {
  if (piece == 0u) return 0u;
  uint32_t at = 24u;
  for (uint32_t j = 0; j + 1u < piece; ++j)
    if ((file_mask >> j) & 1u) at += binu_width(j + 1u);
  return at;
}

__global__ __launch_bounds__(BINU_TILE) void bin_unpack_kernel(BinUnpackArgs a) {
  __shared__ uint32_t s_first[BINU_TILE];  // first rows of the segments k0 .. k0 + BINU_TILE - 1 (past the table: no row)
  __shared__ uint32_t s_count[BINU_TILE];
  __shared__ uint32_t s_fmask[BINU_TILE];
  __shared__ uint64_t s_base[BINU_TILE];
  __shared__ uint32_t s_stage[BINU_STAGE];
  const uint32_t t = threadIdx.x;
  const uint32_t r0 = blockIdx.x * BINU_TILE;
  const uint32_t r1 = (uint32_t)min((uint64_t)r0 + BINU_TILE, (uint64_t)a.n);

  const uint32_t k0 = unpack_first_segment(a.segs, a.num_segs, r0);
  {
    const bool listed = k0 + t < a.num_segs;
    const BinUnpackSeg* sg = a.segs + k0 + t;
    s_first[t] = listed ? sg->first_row : 0xFFFFFFFFu;
    s_count[t] = listed ? sg->count : 0u;
    s_fmask[t] = listed ? sg->file_mask : 0u;
    s_base[t] = listed ? sg->byte_offset : 0ull;
  }
  __syncthreads();

  const uint32_t nwin = unpack_window_size<BINU_TILE>(s_first, r1);
  // this lane's row and its entry
  const uint32_t r = r0 + t;
  const bool live = r < r1;
  const uint32_t my = live ? unpack_row_entry(s_first, nwin, r) : 0u;
  const uintptr_t raw_begin = (uintptr_t)a.raw, raw_end = raw_begin + a.raw_bytes;

  for (uint32_t piece = 0; piece < BINU_PIECES; ++piece) {
    uint8_t* const out = static_cast<uint8_t*>(a.out[piece]);
    if (!out) continue;  // (block-uniform)
    const uint32_t w = binu_width(piece);
    // where entry e's run of this piece lies: rows [lo, lo + len) of the tile, bytes [G, G + w len) of memory, from dword
    // S of the stage on; len == 0: the entry's image lacks the array
    auto run = [&](uint32_t e, uint32_t* lo, uint32_t* len, uintptr_t* G, uint32_t* S) {
      const uint32_t first = s_first[e], count = s_count[e], fmask = s_fmask[e];
      *lo = max(first, r0);
      const uint32_t hi = min(first + count, r1);
      const bool present = piece == 0u || ((fmask >> (piece - 1u)) & 1u);
      *len = present ? hi - *lo : 0u;
      *G = raw_begin + (uintptr_t)s_base[e] + 12u + (uintptr_t)count * binu_prefix(fmask, piece) + (uintptr_t)w * (*lo - first);
      *S = ((w * (*lo - r0)) >> 2) + 2u * e;
    };

    stage_fill<BINU_TILE>(s_stage, s_first, nwin, w, r0, r1, raw_begin, raw_end, run);
    __syncthreads();

    // ---- every lane its row's value: bit copies out of the stage, zeros where the segment lacks the array
    if (live) {
      uint32_t lo, len, S;
      uintptr_t G;
      run(my, &lo, &len, &G, &S);
      const bool present = len != 0u;
      const uint32_t q = 4u * S + (uint32_t)(G & 3u) + w * (r - lo);
      uint8_t* const o = out + (size_t)r * w;
      switch (w) {
        case 24: {
          uint64_t* const o8 = reinterpret_cast<uint64_t*>(o);
#pragma unroll
          for (uint32_t i = 0; i < 3u; ++i)
            o8[i] = present ? ((uint64_t)stage_word(s_stage, q + 8u * i + 4u) << 32) | stage_word(s_stage, q + 8u * i) : 0ull;
          break;
        }
        case 12: {
          uint32_t* const o4 = reinterpret_cast<uint32_t*>(o);
#pragma unroll
          for (uint32_t i = 0; i < 3u; ++i) o4[i] = present ? stage_word(s_stage, q + 4u * i) : 0u;
          break;
        }
        case 8:
          *reinterpret_cast<uint64_t*>(o) = present ? ((uint64_t)stage_word(s_stage, q + 4u) << 32) | stage_word(s_stage, q) : 0ull;
          break;
        case 3: {
          const uint32_t v = present ? stage_word(s_stage, q) : 0u;
          o[0] = (uint8_t)v;
          o[1] = (uint8_t)(v >> 8);
          o[2] = (uint8_t)(v >> 16);
          break;
        }
        case 2: *reinterpret_cast<uint16_t*>(o) = present ? (uint16_t)stage_word(s_stage, q) : (uint16_t)0; break;
        default: o[0] = present ? reinterpret_cast<const uint8_t*>(s_stage)[q] : (uint8_t)0; break;
      }
    }
    __syncthreads();  // the stage is the next piece's
  }
}

BinUnpackSeg bin_unpack_seg(uint64_t byte_offset, uint64_t first_row, uint64_t count, uint32_t mask) {
  uint32_t file_mask = 0;
  for (int j = 0; j < SWZ_ATTR_COUNT; ++j)
    if ((mask >> FILE_ORDER[j]) & 1u) file_mask |= 1u << j;
  return BinUnpackSeg{byte_offset, (uint32_t)first_row, (uint32_t)count, file_mask, 0u};
}

uint64_t bin_image_bytes(uint64_t count, uint32_t mask) {
  uint64_t row = 24;
  for (int a = 0; a < SWZ_ATTR_COUNT; ++a)
    if ((mask >> a) & 1u) row += ATTR_BYTES[a];
  return 12 + count * row;
}

int bin_unpack_launch(swz_ctx* c, hipStream_t stream, const uint8_t* d_raw, uint64_t raw_bytes, const BinUnpackSeg* d_table,
                      uint32_t num_segs, uint32_t rows, double* d_xyz_out, const swz_attribute_columns* d_out) {
  if (!rows || !num_segs) return SWZ_OK;
  BinUnpackArgs a{};
  a.raw = d_raw;
  a.raw_bytes = raw_bytes;
  a.segs = d_table;
  a.num_segs = num_segs;
  a.n = rows;
  a.out[0] = d_xyz_out;
  for (int j = 0; j < SWZ_ATTR_COUNT; ++j) a.out[1 + j] = d_out ? d_out->column[FILE_ORDER[j]] : nullptr;
  hipLaunchKernelGGL(bin_unpack_kernel, dim3(div_up(rows, BINU_TILE)), dim3(BINU_TILE), 0, stream, a);
  SWZ_LAUNCH_CHECK(c);
  return SWZ_OK;
}

}  // namespace swz

using namespace swz;

extern "C" {

uint32_t swz_bin_unpack_tile(void) { return BINU_TILE; }

int swz_bin_unpack_segments_device(swz_ctx* c, const uint8_t* d_raw, uint64_t raw_bytes, const swz_bin_segment* segments,
                                   uint64_t num_segments, double* d_xyz_out, const swz_attribute_columns* d_out) {
  if (!c) return SWZ_ERR_BAD_ARG;
  auto refuse = [&](const char* what) { return c->fail(SWZ_ERR_BAD_ARG, std::string("swz_bin_unpack_segments_device: ") + what); };
  // everything is checked on the host before anything is launched
  if (num_segments && !segments) return refuse("NULL segments");
  static_assert(((BINU_WIDTHS >> 4) & 15u) == 12u && ((BINU_WIDTHS >> 20) & 15u) == 8u, "BINU_WIDTHS: normals and GPS times in file order");
  std::vector<BinUnpackSeg> table;
  uint64_t rows = 0, bytes = 0;
  for (uint64_t s = 0; s < num_segments; ++s) {
    const swz_bin_segment& sg = segments[s];
    if (sg.first_row != rows) return refuse("the rows of the segments must ascend contiguously from 0");
    if (sg.mask & ~BINU_MASK_ALL) return refuse("the mask names an attribute that does not exist");
    if (sg.count > BINU_MAX_POINTS || rows + sg.count > BINU_MAX_POINTS) return refuse("more than 2^32-65536 rows");
    const uint64_t image = bin_image_bytes(sg.count, sg.mask);
    if (sg.byte_offset > raw_bytes || image > raw_bytes - sg.byte_offset) return refuse("the image of a segment passes raw_bytes");
    rows += sg.count;
    bytes += image;
    if (sg.count) table.push_back(bin_unpack_seg(sg.byte_offset, sg.first_row, sg.count, sg.mask));
  }
  if (rows == 0) return SWZ_OK;
  if (!d_raw) return refuse("NULL image");
  SWZ_HIP(c, hipSetDevice(c->device));
  BinUnpackSeg* d_table = nullptr;
  SWZ_TRY(c->get("bin_segments", table.size(), &d_table));
  SWZ_HIP(c, hipMemcpyAsync(d_table, table.data(), table.size() * sizeof(BinUnpackSeg), hipMemcpyHostToDevice, c->stream));
  {
    ProfScope ps(c, "bin_unpack_segments", 2 * bytes, 1);
    SWZ_TRY(bin_unpack_launch(c, c->stream, d_raw, raw_bytes, d_table, (uint32_t)table.size(), (uint32_t)rows, d_xyz_out, d_out));
  }
  SWZ_HIP(c, hipStreamSynchronize(c->stream));  // (the table's host copy lives until here)
  return SWZ_OK;
}

}  // extern "C"
