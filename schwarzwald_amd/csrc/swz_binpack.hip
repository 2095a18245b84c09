// swz_binpack.hip -- BinaryPersistence node files packed on the device (reference: core/io/BinaryPersistence.h:45-193).
//
// A node file is: u32 properties mask, u64 count, count x 24 bytes of positions, then every attribute array the mask names in
// FILE_ORDER (swz_hostio.h), no padding.  That whole file is the node's BODY; the bodies of all nodes of a table, one behind
// the other and each zero-padded to a multiple of 8, are the IMAGE that swz_bin_pack_device writes in one pass.  Nothing is
// converted -- the format is lossless --, so the kernel is a permuted gather whose difficulty is the layout: an array of a
// body begins wherever the arrays in front of it end (positions at 12, the normals' floats at 12 + 27 * count, GPS doubles at
// odd offsets), and the image must leave as aligned dwords.
#include <cstring>
#include <string>
#include <vector>

#include "swz_internal.h"
#include "swz_device.h"
#include "swz_hostio.h"
#include "swz_nodepack.h"

namespace swz {

constexpr uint32_t BIN_MASK_ALL = (1u << SWZ_ATTR_COUNT) - 1u;
constexpr uint64_t BIN_MAX_POINTS = 0xFFFFFFFFull - 65535ull;  // the library's limit of points per batch (2^32 - 65536)
constexpr uint32_t BIN_HEADER_BYTES = 12;

constexpr int BIN_TILE = 256;                        // stored rows per block, one per thread
constexpr uint32_t BIN_PIECES = SWZ_ATTR_COUNT + 1;  // the arrays of a body: positions, then the attributes
constexpr uint32_t BIN_ROW_MAX = 24 + 58;            // bytes of a row with all twelve attributes
constexpr uint32_t BIN_STAGE = BIN_ROW_MAX * BIN_TILE;
constexpr uint32_t BIN_HEADER_SLOTS = 3, BIN_PAD_SLOTS = 3;

static uint64_t bin_row_bytes(uint32_t mask) {
  uint64_t row = 24;
  for (int a = 0; a < SWZ_ATTR_COUNT; ++a)
    if ((mask >> a) & 1u) row += ATTR_BYTES[a];
  return row;
}
static uint64_t bin_file_size(uint64_t count, uint64_t row_bytes) { return BIN_HEADER_BYTES + count * row_bytes; }

struct BinNode {  // an entry of the pack table (swz_nodepack.h)
  uint32_t start, count;
  uint64_t base;  // of the body in the image, a multiple of 8
};

// The arrays of a body as PIECES: piece 0 the positions, piece k the k-th attribute array of the file.  prefix[k] is what a
// row holds in front of piece k, so the array lies at 12 + count * prefix[k] of a body, and the rows of the tile at
// BIN_TILE * prefix[k] of the LDS stage.
struct BinPackArgs {
  const uint32_t* perm;
  const uint32_t* order;  // may be null: identity
  uint32_t n;
  const double* xyz;
  const uint8_t* col[BIN_PIECES];  // [0] unused
  uint32_t width[BIN_PIECES];
  uint32_t prefix[BIN_PIECES];
  uint32_t pieces;
  uint32_t mask;
  const BinNode* nodes;
  uint32_t num_nodes;
  uint8_t* image;
};

// the aligned dwords that L bytes at any address reach into, at most
__device__ __forceinline__ uint32_t bin_slots(uint32_t bytes) { return (bytes + 3u) / 4u + 1u; }

// Slot s of a run of L bytes that lie at G in the image and at byte q0 of the stage: the aligned dword (G & ~3) + 4 s.  The
// part of it inside the run leaves as one dword put together from two dwords of LDS, or -- at the ends of the run, where the
// rest of the dword belongs to another array, another node or another block -- as the halfword or the bytes that are the
// run's.
__device__ __forceinline__ void bin_emit(uint8_t* __restrict__ image, uint64_t G, uint32_t L, const uint32_t* stage, uint32_t q0,
                                         uint32_t s) {
  const uint64_t A = (G & ~3ull) + 4ull * s;
  const uint64_t lo = A > G ? A : G;
  const uint64_t hi = A + 4u < G + L ? A + 4u : G + L;
  if (lo >= hi) return;
  const uint32_t q = q0 + (uint32_t)(lo - G);
  const uint32_t bytes = (uint32_t)(hi - lo);
  if (bytes == 4u) {
    const uint32_t w0 = stage[q >> 2], w1 = stage[(q >> 2) + 1u];
    *reinterpret_cast<uint32_t*>(image + lo) = (uint32_t)((((uint64_t)w1 << 32) | w0) >> (8u * (q & 3u)));
    return;
  }
  const uint8_t* const stage8 = reinterpret_cast<const uint8_t*>(stage);
  if (bytes == 2u && (lo & 1ull) == 0) {
    *reinterpret_cast<uint16_t*>(image + lo) = (uint16_t)((uint32_t)stage8[q] | ((uint32_t)stage8[q + 1u] << 8));
    return;
  }
  for (uint32_t b = 0; b < bytes; ++b) image[lo + b] = stage8[q + b];
}

// One block takes BIN_TILE consecutive stored rows.  It finds the node of its first row with one binary search in the table
// and lists the nodes of its rows in a window (swz_nodepack.h).  Each lane loads its row through perm[order[r]] -- scattered
// reads -- and puts it into LDS array by array, so that what the tile holds of one array of one node is one run of bytes in
// LDS and one run of bytes in the image.  A node's part of the tile is a SEGMENT; its runs -- the header if the tile holds the
// node's first row, one run per array, the zero padding if it holds the last row -- are cut into SLOTS, one per aligned dword
// of the image.  The slots of all segments of the tile are numbered through, and lane t takes the slots t, t + 256, ...:
// consecutive lanes write consecutive dwords of a run.  Every byte of the image is written once, nothing is read back.
__global__ __launch_bounds__(BIN_TILE) void bin_pack_kernel(BinPackArgs a) {
  __shared__ uint32_t s_start[BIN_TILE];
  __shared__ uint32_t s_count[BIN_TILE];
  __shared__ uint64_t s_base[BIN_TILE];
  __shared__ uint32_t s_slots[BIN_TILE];  // slots of the window's segments
  __shared__ uint32_t s_first[BIN_TILE];  // ... and the first slot of each
  __shared__ uint32_t s_total;
  __shared__ __align__(8) uint32_t s_stage[BIN_STAGE / 4 + 4];  // the rows by array; eight zero bytes (the padding's source), four spare
  const uint32_t t = threadIdx.x;
  const uint32_t r0 = blockIdx.x * (uint32_t)BIN_TILE;
  const uint32_t r1 = (uint32_t)min((uint64_t)r0 + BIN_TILE, (uint64_t)a.n);
  const uint32_t row_bytes = a.prefix[a.pieces - 1u] + a.width[a.pieces - 1u];

  const uint32_t k0 = pack_first_node(a.nodes, a.num_nodes, r0);
  const BinNode* const listed = pack_fill_window(a.nodes, a.num_nodes, k0, r1, s_start, s_count);
  s_base[t] = listed ? listed->base : 0ull;
  {
    // the slots of window entry t's segment: rows [lo, hi) of the tile
    uint32_t slots = 0;
    if (listed) {
      const uint32_t lo = max(listed->start, r0), hi = min(listed->start + listed->count, r1);
      if (hi > lo) {
        const uint32_t len = hi - lo;
        if (lo == listed->start) slots += BIN_HEADER_SLOTS;
        for (uint32_t k = 0; k < a.pieces; ++k) slots += bin_slots(a.width[k] * len);
        if (hi == listed->start + listed->count) slots += BIN_PAD_SLOTS;
      }
    }
    s_slots[t] = slots;
  }
  if (t < 4u) s_stage[BIN_STAGE / 4 + t] = 0u;
  __syncthreads();

  // entries are valid up to the first filler
  uint32_t nwin;
  {
    uint32_t l = 0, h = BIN_TILE;
    while (l < h) {
      const uint32_t mid = (l + h) / 2;
      if (s_start[mid] != PACK_FILLER) l = mid + 1; else h = mid;
    }
    nwin = l;
  }
  if (nwin == 0) return;  // no row of the tile is in a node
  if (t < nwin) {
    uint32_t first = 0;
    for (uint32_t i = 0; i < t; ++i) first += s_slots[i];
    s_first[t] = first;
    if (t + 1u == nwin) s_total = first + s_slots[t];
  }

  // the rows into LDS
  const uint32_t r = r0 + t;
  uint32_t e;
  if (pack_row_node<BIN_TILE>(s_start, s_count, r, r1, &e)) {
    double pos[3];
    const uint32_t src = pack_source_row(a.perm, a.order, a.xyz, r, pos);
    double* const sp = reinterpret_cast<double*>(s_stage) + 3u * t;
    sp[0] = pos[0];
    sp[1] = pos[1];
    sp[2] = pos[2];
    uint8_t* const stage8 = reinterpret_cast<uint8_t*>(s_stage);
    for (uint32_t k = 1; k < a.pieces; ++k) {
      const uint32_t w = a.width[k];
      const uint8_t* const in = a.col[k] + (size_t)src * w;
      uint8_t* const out = stage8 + (uint32_t)BIN_TILE * a.prefix[k] + w * t;
      switch (w) {
        case 1: out[0] = in[0]; break;
        case 2: *reinterpret_cast<uint16_t*>(out) = *reinterpret_cast<const uint16_t*>(in); break;
        case 3:
          out[0] = in[0];
          out[1] = in[1];
          out[2] = in[2];
          break;
        case 8: *reinterpret_cast<uint64_t*>(out) = *reinterpret_cast<const uint64_t*>(in); break;
        default:  // 12: three floats
          reinterpret_cast<uint32_t*>(out)[0] = reinterpret_cast<const uint32_t*>(in)[0];
          reinterpret_cast<uint32_t*>(out)[1] = reinterpret_cast<const uint32_t*>(in)[1];
          reinterpret_cast<uint32_t*>(out)[2] = reinterpret_cast<const uint32_t*>(in)[2];
          break;
      }
    }
  }
  __syncthreads();

  const uint32_t total = s_total;
  for (uint32_t x = t; x < total; x += BIN_TILE) {
    // the last segment that begins at or before slot x (an entry without rows in the tile has no slots and is passed over)
    uint32_t l = 0, h = nwin;
    while (l < h) {
      const uint32_t mid = (l + h) / 2;
      if (s_first[mid] <= x) l = mid + 1; else h = mid;
    }
    const uint32_t en = l - 1u;
    uint32_t y = x - s_first[en];
    const uint32_t start = s_start[en], count = s_count[en];
    const uint32_t lo = max(start, r0), hi = min(start + count, r1);
    const uint32_t len = hi - lo, j0 = lo - start;  // rows [j0, j0 + len) of the node
    const uint64_t base = s_base[en];
    if (j0 == 0u) {
      if (y < BIN_HEADER_SLOTS) {  // the body begins on a multiple of 8: the header is three dwords (the count's high one is 0)
        *reinterpret_cast<uint32_t*>(a.image + base + 4u * y) = y == 0u ? a.mask : (y == 1u ? count : 0u);
        continue;
      }
      y -= BIN_HEADER_SLOTS;
    }
    bool done = false;
    for (uint32_t k = 0; k < a.pieces; ++k) {
      const uint32_t w = a.width[k], slots = bin_slots(w * len);
      if (y < slots) {
        const uint64_t G = base + BIN_HEADER_BYTES + (uint64_t)count * a.prefix[k] + (uint64_t)w * j0;
        bin_emit(a.image, G, w * len, s_stage, (uint32_t)BIN_TILE * a.prefix[k] + w * (lo - r0), y);
        done = true;
        break;
      }
      y -= slots;
    }
    if (done) continue;
    // behind the node's last row: the zeros up to the multiple of 8
    const uint64_t file = BIN_HEADER_BYTES + (uint64_t)count * row_bytes;
    bin_emit(a.image, base + file, (uint32_t)(((file + 7ull) & ~7ull) - file), s_stage, BIN_STAGE, y);
  }
}

static int check_mask(swz_ctx* c, const char* who, const swz_attribute_columns* cols, uint32_t mask) {
  if (mask & ~BIN_MASK_ALL) return fail(c, SWZ_ERR_BAD_ARG, std::string(who) + ": the mask names an attribute that does not exist");
  for (int a = 0; a < SWZ_ATTR_COUNT; ++a)
    if (((mask >> a) & 1u) && (!cols || !cols->column[a]))
      return fail(c, SWZ_ERR_BAD_ARG, std::string(who) + ": the mask names a column that is absent");
  return SWZ_OK;
}

}  // namespace swz

using namespace swz;

extern "C" {

uint32_t swz_bin_pack_tile(void) { return (uint32_t)BIN_TILE; }

int swz_bin_layout(uint64_t num_nodes, const uint64_t* node_count, uint32_t mask, uint64_t* body_offset_out, uint64_t* body_size_out,
                   uint64_t* file_size_out, uint64_t* total_out) {
  if ((num_nodes && !node_count) || (mask & ~BIN_MASK_ALL)) return SWZ_ERR_BAD_ARG;
  const uint64_t row = bin_row_bytes(mask);
  uint64_t at = 0;
  for (uint64_t k = 0; k < num_nodes; ++k) {
    if (node_count[k] > BIN_MAX_POINTS) return SWZ_ERR_BAD_ARG;
    // (a node without points has no file: swz_bin_write_node writes nothing)
    const uint64_t file = node_count[k] ? bin_file_size(node_count[k], row) : 0;
    const uint64_t size = (file + 7) & ~7ull;
    if (body_offset_out) body_offset_out[k] = at;
    if (body_size_out) body_size_out[k] = size;
    if (file_size_out) file_size_out[k] = file;
    at += size;
  }
  if (total_out) *total_out = at;
  return SWZ_OK;
}

int swz_bin_pack_device(swz_ctx* c, const uint32_t* d_perm, const uint32_t* d_order, uint64_t n, const double* d_xyz,
                        const swz_attribute_columns* d_in, uint64_t num_nodes, const uint64_t* node_offset, const uint64_t* node_count,
                        uint32_t mask, void* d_image_out, uint64_t image_bytes) {
  if (!c) return SWZ_ERR_BAD_ARG;
  // everything is checked on the host before anything is launched
  if (n > BIN_MAX_POINTS) return c->fail(SWZ_ERR_BAD_ARG, "swz_bin_pack_device: more than 2^32-65536 rows");
  SWZ_TRY(check_mask(c, "swz_bin_pack_device", d_in, mask));
  if (num_nodes && (!node_offset || !node_count)) return c->fail(SWZ_ERR_BAD_ARG, "swz_bin_pack_device: NULL node table");
  const uint64_t row = bin_row_bytes(mask);
  const PackNames names{"swz_bin_pack_device", "swz_bin_layout", "bin_nodes"};
  PackTable<BinNode> table;
  SWZ_TRY(pack_build_table(
    c, names, n, num_nodes, node_offset, node_count, [](uint64_t, BinNode*) -> const char* { return nullptr; },
    [&](uint64_t cnt, uint64_t* bytes) -> const char* {
      *bytes = (bin_file_size(cnt, row) + 7) & ~7ull;
      return nullptr;
    },
    &table));

  BinPackArgs a{};
  SWZ_TRY(pack_upload_table(c, names, table, d_perm, d_xyz, d_image_out, image_bytes, &a.nodes));
  if (!a.nodes) return SWZ_OK;
  a.perm = d_perm;
  a.order = d_order;
  a.n = (uint32_t)n;
  a.xyz = d_xyz;
  a.mask = mask;
  a.image = static_cast<uint8_t*>(d_image_out);
  a.num_nodes = (uint32_t)table.nodes.size();
  a.width[0] = 24;
  a.prefix[0] = 0;
  a.pieces = 1;
  for (int k = 0; k < SWZ_ATTR_COUNT; ++k) {
    const int at = FILE_ORDER[k];
    if (!((mask >> at) & 1u)) continue;
    a.col[a.pieces] = static_cast<const uint8_t*>(d_in->column[at]);
    a.width[a.pieces] = ATTR_BYTES[at];
    a.prefix[a.pieces] = a.prefix[a.pieces - 1] + a.width[a.pieces - 1];
    ++a.pieces;
  }
  {
    ProfScope ps(c, "bin_pack", n * (d_order ? 8 : 4) + table.prev_end * row + table.image_bytes, 1);
    // rows behind the last node belong to no body: the grid ends with it
    hipLaunchKernelGGL(bin_pack_kernel, dim3(div_up(table.prev_end, BIN_TILE)), dim3(BIN_TILE), 0, c->stream, a);
    SWZ_LAUNCH_CHECK(c);
  }
  SWZ_HIP(c, hipStreamSynchronize(c->stream));
  return SWZ_OK;
}

int swz_bin_persist_nodes_image(swz_ctx* c, const char* dir, uint64_t num_nodes, const int8_t* node_level, const uint64_t* node_key,
                                const uint64_t* node_count, const void* image, uint64_t image_bytes, uint32_t mask, int compressed) {
  if (!dir || (num_nodes && (!node_level || !node_key || !node_count)))
    return fail(c, SWZ_ERR_BAD_ARG, "swz_bin_persist_nodes_image: NULL argument");
  std::vector<uint64_t> at(num_nodes), file(num_nodes);
  uint64_t total = 0;
  if (swz_bin_layout(num_nodes, node_count, mask, at.data(), nullptr, file.data(), &total) != SWZ_OK)
    return fail(c, SWZ_ERR_BAD_ARG, "swz_bin_persist_nodes_image: bad mask, or a node of more than 2^32-65536 points");
  if (total > image_bytes || (total && !image))
    return fail(c, SWZ_ERR_BAD_ARG, "swz_bin_persist_nodes_image: the image is smaller than the table's layout");
  for (uint64_t k = 0; k < num_nodes; ++k) {
    char name[24];
    if (swz_node_name(node_level[k], node_key[k], name) != SWZ_OK) return fail(c, SWZ_ERR_BAD_ARG, "bad node level");
  }
  std::string first_err;
  const int st = run_tickets(c, num_nodes, [&](uint64_t k, std::string* err) {
    if (node_count[k] == 0) return (int)SWZ_OK;  // persist_points returns before opening the file
    char name[24];
    (void)swz_node_name(node_level[k], node_key[k], name);
    const std::string path = std::string(dir) + "/" + name + (compressed ? ".binz" : ".bin");
    const unsigned char* body = static_cast<const unsigned char*>(image) + at[k];
    if (compressed) return write_file_zlib(path, body, (size_t)file[k], err);
    return write_file(path, {{body, (size_t)file[k]}}, err);
  }, &first_err);
  return st == SWZ_OK ? SWZ_OK : fail(c, st, first_err);
}

}  // extern "C"
