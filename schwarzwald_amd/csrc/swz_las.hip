// swz_las.hip -- LAS node files whose point records are packed on the device, and the Entwine (EPT) metadata
// (reference: core/io/LASPersistence.cpp:16-271, core/io/EntwinePersistence.cpp:31-130, 197-333).
//
// A node file is a LAS 1.2 file: the 227-byte public header, no VLRs, then `count` point records of format
// (gps time ? 1 : 0) + (colour ? 2 : 0), 20 + 8 * gps + 6 * rgb bytes each.  The records of a node are its BODY; the bodies
// of all nodes of a table, one behind the other and each zero-padded to a multiple of 8, are the IMAGE that
// swz_las_pack_device writes in one pass (permuted gather + quantisation + bit packing + colour shift + final layout).
//
// The header fields the reference sets are written as it sets them (LASPersistence.cpp:113-136); every other byte is what a
// fresh laszip_header happens to hold, which is not pinned against LASzip here: file source id, global encoding, GUID,
// system identifier, creation day and year are zeros, the generating software is padded with zeros.
//
// Quantisation (laszip_set_coordinates): X = I32_QUANTIZE((x - offset) / scale), I32_QUANTIZE(n) = n >= 0 ? (int32)(n + 0.5)
// : (int32)(n - 0.5) -- one double subtraction, one division, one addition, not contracted, then truncation.  The reference's
// cast of a value outside int32 is undefined; OURS saturates to INT32_MIN / INT32_MAX and writes 0 for NaN.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include <sys/stat.h>

#include "swz_internal.h"
#include "swz_device.h"
#include "swz_hostio.h"
#include "swz_nodepack.h"

namespace swz {

constexpr uint32_t LAS_MASK_ALL = (1u << SWZ_ATTR_COUNT) - 1u;
constexpr uint64_t LAS_MAX_POINTS = 0xFFFFFFFFull - 65535ull;  // the library's limit of points per batch (2^32 - 65536)
constexpr uint32_t LAS_HEADER_BYTES = 227;

__host__ __device__ inline uint32_t las_format(uint32_t mask) {
  return ((mask >> SWZ_ATTR_GPS_TIME) & 1u) + 2u * ((mask >> SWZ_ATTR_RGB) & 1u);
}
__host__ __device__ inline uint32_t las_record_bytes(uint32_t format) { return 20u + 8u * (format & 1u) + 6u * (format >> 1); }
inline uint64_t las_body_size(uint64_t count, uint32_t record_bytes) { return (count * record_bytes + 7) & ~7ull; }

// I32_QUANTIZE of (x - offset) / scale, saturating (see the head of the file)
__host__ __device__ inline int32_t las_quantize(double x, double offset, double scale) {
  const double n = (x - offset) / scale;
  const double v = n >= 0 ? n + 0.5 : n - 0.5;
  if (!(v == v)) return 0;
  if (v >= 2147483648.0) return 2147483647;
  if (v <= -2147483649.0) return -2147483647 - 1;
  return (int32_t)v;
}

// One point record as dwords (the last one half used in formats 2 and 3).  A NULL column is an untouched laszip_point: 0.
struct LasColumns {
  const uint8_t* rgb;
  const uint16_t* intensity;
  const uint8_t* classification;
  const uint8_t* edge;
  const double* gps;
  const uint8_t* num_returns;
  const uint8_t* return_number;
  const uint16_t* source_id;
  const uint8_t* scan_direction;
  const int8_t* scan_angle;
  const uint8_t* user_data;
};

static LasColumns las_columns(const swz_attribute_columns* cols, uint32_t mask) {
  auto col = [&](int a) -> const void* { return (cols && ((mask >> a) & 1u)) ? cols->column[a] : nullptr; };
  LasColumns c;
  c.rgb = static_cast<const uint8_t*>(col(SWZ_ATTR_RGB));
  c.intensity = static_cast<const uint16_t*>(col(SWZ_ATTR_INTENSITY));
  c.classification = static_cast<const uint8_t*>(col(SWZ_ATTR_CLASSIFICATION));
  c.edge = static_cast<const uint8_t*>(col(SWZ_ATTR_EDGE_OF_FLIGHT_LINE));
  c.gps = static_cast<const double*>(col(SWZ_ATTR_GPS_TIME));
  c.num_returns = static_cast<const uint8_t*>(col(SWZ_ATTR_NUMBER_OF_RETURNS));
  c.return_number = static_cast<const uint8_t*>(col(SWZ_ATTR_RETURN_NUMBER));
  c.source_id = static_cast<const uint16_t*>(col(SWZ_ATTR_POINT_SOURCE_ID));
  c.scan_direction = static_cast<const uint8_t*>(col(SWZ_ATTR_SCAN_DIRECTION_FLAG));
  c.scan_angle = static_cast<const int8_t*>(col(SWZ_ATTR_SCAN_ANGLE_RANK));
  c.user_data = static_cast<const uint8_t*>(col(SWZ_ATTR_USER_DATA));
  return c;
}

// row `src` of the columns and the position p, quantised against the node's offset and scale, as the record of FORMAT
template <uint32_t FORMAT>
__host__ __device__ inline void las_compose(uint32_t rec[9], const double p[3], const LasColumns& c, size_t src, const double offset[3],
                                            double scale) {
  rec[0] = (uint32_t)las_quantize(p[0], offset[0], scale);
  rec[1] = (uint32_t)las_quantize(p[1], offset[1], scale);
  rec[2] = (uint32_t)las_quantize(p[2], offset[2], scale);
  // the bit-fields of laszip_point: return number : 3, number of returns : 3, scan direction : 1, edge of flight line : 1,
  // then classification : 5 with the three flag bits zero
  uint32_t bits = 0, cls = 0;
  if (c.return_number) bits |= (uint32_t)c.return_number[src] & 7u;
  if (c.num_returns) bits |= ((uint32_t)c.num_returns[src] & 7u) << 3;
  if (c.scan_direction) bits |= ((uint32_t)c.scan_direction[src] & 1u) << 6;
  if (c.edge) bits |= ((uint32_t)c.edge[src] & 1u) << 7;
  if (c.classification) cls = (uint32_t)c.classification[src] & 31u;
  rec[3] = (c.intensity ? (uint32_t)c.intensity[src] : 0u) | (bits << 16) | (cls << 24);
  rec[4] = (c.scan_angle ? (uint32_t)(uint8_t)c.scan_angle[src] : 0u) | ((c.user_data ? (uint32_t)c.user_data[src] : 0u) << 8) |
           ((c.source_id ? (uint32_t)c.source_id[src] : 0u) << 16);
  uint32_t at = 5;
  if (FORMAT & 1u) {
    double g = c.gps[src];
    uint64_t u;
    memcpy(&u, &g, 8);
    rec[5] = (uint32_t)u;
    rec[6] = (uint32_t)(u >> 32);
    at = 7;
  }
  if (FORMAT & 2u) {  // LASPersistence.cpp:215-217: the 8-bit colour shifted into the high byte
    const uint8_t* q = c.rgb + 3 * src;
    rec[at] = ((uint32_t)q[0] << 8) | ((uint32_t)q[1] << 24);
    rec[at + 1] = (uint32_t)q[2] << 8;
  }
}

// ---------------------------------------------------------------------------------- the pack kernel
constexpr int LAS_TILE = 256;                 // stored rows per block, one per thread
constexpr uint32_t LAS_STAGE = 34 * LAS_TILE;  // bytes of LDS the records pass through

struct LasNode {  // an entry of the pack table (swz_nodepack.h)
  uint32_t start, count;
  uint64_t base;  // of the body in the image, a multiple of 8
  double offset[3];
  double scale;
};

struct LasPackArgs {
  const uint32_t* perm;
  const uint32_t* order;  // may be null: identity
  uint32_t n;
  const double* xyz;
  LasColumns cols;
  const LasNode* nodes;
  uint32_t num_nodes;
  uint8_t* image;
};

// One block takes LAS_TILE consecutive stored rows.  It finds the node of its first row with one binary search in the table
// and walks forward from there (swz_nodepack.h).  The bodies
// of consecutive nodes of the table lie one behind the other, so whatever the block's rows hold -- parts of nodes, whole nodes
// with their padding, rows of no node in between -- their bytes are ONE range [lo, hi) of the image, every byte of which is
// this block's and nobody else's.  Each lane loads its row (scattered reads), composes the record in registers and puts it
// where it lies in that range into LDS, the last row of a node the node's zero padding behind it; the block then writes the
// range from LDS as aligned dwords, consecutive lanes consecutive dwords.  Records and bodies begin on even addresses, so
// the range may begin or end in the middle of a dword whose other half belongs to the neighbouring block (record lengths 26
// and 34): that dword leaves as the halfword that is this block's.  Nothing is written twice or read back.  The range of a
// tile of one- and two-point nodes of 34 bytes (40 and 72 with the padding) is longer than the LDS stage: it passes through
// in two windows.
template <uint32_t FORMAT>
__global__ __launch_bounds__(LAS_TILE) void las_pack_kernel(LasPackArgs a) {
  constexpr uint32_t RB = 20u + 8u * (FORMAT & 1u) + 6u * (FORMAT >> 1);
  constexpr uint32_t HALVES = RB / 2;
  __shared__ uint32_t s_start[LAS_TILE];
  __shared__ uint32_t s_count[LAS_TILE];
  __shared__ uint32_t s_rel[LAS_TILE];  // base of the body relative to the anchor
  __shared__ uint32_t s_stage[LAS_STAGE / 4];
  const uint32_t t = threadIdx.x;
  const uint32_t r0 = blockIdx.x * (uint32_t)LAS_TILE;
  const uint32_t r1 = (uint32_t)min((uint64_t)r0 + LAS_TILE, (uint64_t)a.n);

  const uint32_t k0 = pack_first_node(a.nodes, a.num_nodes, r0);
  // Offsets in the image are kept as 32-bit distances from an ANCHOR just in front of the block's range: where node k0's
  // rows in front of the tile end, rounded down to 8.  The base of node k0 itself may lie 2^32 bytes and more in front of
  // it; its distance and RB * (row in the node) wrap, their sum -- a place inside the range -- does not.
  uint64_t anchor;
  {
    const LasNode* nd = a.nodes + k0;
    const uint32_t before = nd->start < r0 ? min(r0 - nd->start, nd->count) : 0u;
    anchor = nd->base + (((uint64_t)RB * before) & ~7ull);
  }
  const LasNode* const listed = pack_fill_window(a.nodes, a.num_nodes, k0, r1, s_start, s_count);
  s_rel[t] = listed ? (uint32_t)(listed->base - anchor) : 0u;
  __syncthreads();

  // the block's range of the image, relative to the anchor: from the first listed node that reaches into the tile ...
  const uint32_t first = (s_start[0] != PACK_FILLER && s_start[0] + s_count[0] > r0) ? 0u : 1u;
  if (first >= (uint32_t)LAS_TILE || s_start[first] == PACK_FILLER) return;  // no row of the tile is in a node
  const uint32_t range_lo = s_rel[first] + (s_start[first] < r0 ? RB * (r0 - s_start[first]) : 0u);
  // ... to the last one (entries are valid up to the first filler)
  uint32_t l = first, h = LAS_TILE;
  while (l < h) {
    const uint32_t mid = (l + h) / 2;
    if (s_start[mid] != PACK_FILLER) l = mid + 1; else h = mid;
  }
  const uint32_t last = l - 1;
  const uint32_t last_rows = min(s_count[last], r1 - s_start[last]);
  const uint32_t range_hi = s_rel[last] + (last_rows == s_count[last] ? ((RB * s_count[last] + 7u) & ~7u) : RB * last_rows);
  const uint32_t mirror_lo = range_lo & ~3u;  // what LDS byte 0 of the first window stands for

  const uint32_t r = r0 + t;
  uint32_t e;
  const bool in_node = pack_row_node<LAS_TILE>(s_start, s_count, r, r1, &e);
  uint32_t rec[9];
  uint32_t at = 0, pad_halves = 0;  // where the record lies in the range, and the zeros behind it
  if (in_node) {
    double pos[3];
    const uint32_t src = pack_source_row(a.perm, a.order, a.xyz, r, pos);
    const LasNode* nd = a.nodes + k0 + e;
    const double off[3] = {nd->offset[0], nd->offset[1], nd->offset[2]};
    las_compose<FORMAT>(rec, pos, a.cols, src, off, nd->scale);
    const uint32_t j = r - s_start[e];
    at = s_rel[e] + RB * j - mirror_lo;
    if (j + 1 == s_count[e]) pad_halves = (((RB * s_count[e] + 7u) & ~7u) - RB * s_count[e]) / 2;
  }

  uint16_t* const stage16 = reinterpret_cast<uint16_t*>(s_stage);
  uint8_t* const out = a.image + anchor + mirror_lo;
  const uint32_t span = range_hi - mirror_lo;
  for (uint32_t win = 0; win < span; win += LAS_STAGE) {
    if (win) __syncthreads();  // the window before has left
    if (in_node) {
      const uint32_t rel = at - win;  // wraps below the window: then every test against LAS_STAGE fails for the bytes in front
      if ((rel & 3u) == 0 && rel <= LAS_STAGE - 4u * ((RB + 3u) / 4u)) {
#pragma unroll
        for (uint32_t d = 0; d < RB / 4; ++d) s_stage[rel / 4 + d] = rec[d];
        if (RB & 2u) stage16[rel / 2 + HALVES - 1] = (uint16_t)rec[RB / 4];
      } else {
#pragma unroll
        for (uint32_t k = 0; k < HALVES; ++k) {
          const uint32_t b = rel + 2u * k;
          if (b < LAS_STAGE) stage16[b / 2] = (uint16_t)(rec[k / 2] >> (16u * (k & 1u)));
        }
      }
      for (uint32_t k = 0; k < pad_halves; ++k) {
        const uint32_t b = rel + RB + 2u * k;
        if (b < LAS_STAGE) stage16[b / 2] = 0;
      }
    }
    __syncthreads();
    const uint32_t bytes = min(span - win, LAS_STAGE);
    for (uint32_t w = t; 4u * w < bytes; w += LAS_TILE) {
      const uint32_t g = win + 4u * w;  // relative to mirror_lo
      const uint32_t v = s_stage[w];
      if (mirror_lo + g < range_lo) {
        *reinterpret_cast<uint16_t*>(out + g + 2) = (uint16_t)(v >> 16);  // the low half is the block's in front
      } else if (g + 4u > span) {
        *reinterpret_cast<uint16_t*>(out + g) = (uint16_t)v;  // the high half is the next block's
      } else {
        *reinterpret_cast<uint32_t*>(out + g) = v;
      }
    }
  }
}

// ---------------------------------------------------------------------------------- host helpers
static bool scale_ok(double s) { return std::isfinite(s) && s > 0; }

static int check_mask(swz_ctx* c, const char* who, const swz_attribute_columns* cols, uint32_t mask) {
  if (mask & ~LAS_MASK_ALL) return fail(c, SWZ_ERR_BAD_ARG, std::string(who) + ": the mask names an attribute that does not exist");
  for (int a = 0; a < SWZ_ATTR_COUNT; ++a) {
    if (a == SWZ_ATTR_NORMAL || !((mask >> a) & 1u)) continue;  // normals: no LAS field takes them
    if (!cols || !cols->column[a]) return fail(c, SWZ_ERR_BAD_ARG, std::string(who) + ": the mask names a column that is absent");
  }
  return SWZ_OK;
}

static void put_u16(unsigned char* p, uint32_t v) {
  p[0] = (unsigned char)v;
  p[1] = (unsigned char)(v >> 8);
}
static void put_u32(unsigned char* p, uint32_t v) {
  put_u16(p, v);
  put_u16(p + 2, v >> 16);
}
static void put_f64(unsigned char* p, double v) { memcpy(p, &v, 8); }
static uint32_t get_u16(const unsigned char* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }
static uint32_t get_u32(const unsigned char* p) { return get_u16(p) | (get_u16(p + 2) << 16); }
static double get_f64(const unsigned char* p) {
  double v;
  memcpy(&v, p, 8);
  return v;
}

// the LAS 1.2 public header block as LASPersistence::persist_points fills it (LASPersistence.cpp:113-136)
// (extent: what max / min x, y, z hold when it is not the node box -- the box of the stored records; null = the node box)
static void las_header(unsigned char h[LAS_HEADER_BYTES], uint64_t count, uint32_t format, const double box_min[3], const double box_max[3],
                       double scale, const double* extent_min = nullptr, const double* extent_max = nullptr) {
  memset(h, 0, LAS_HEADER_BYTES);
  memcpy(h, "LASF", 4);
  h[24] = 1;  // version 1.2
  h[25] = 2;
  memcpy(h + 58, "pointcloud_tiler", 16);  // generating software, 32 bytes
  put_u16(h + 94, LAS_HEADER_BYTES);       // header size
  put_u32(h + 96, LAS_HEADER_BYTES);       // offset to point data
  h[104] = (unsigned char)format;
  put_u16(h + 105, las_record_bytes(format));
  put_u32(h + 107, (uint32_t)count);  // number of point records
  put_u32(h + 111, (uint32_t)count);  // ... by return: {count, 0, 0, 0, 0}
  for (int k = 0; k < 3; ++k) {
    put_f64(h + 131 + 8 * k, scale);
    put_f64(h + 155 + 8 * k, box_min[k]);   // the offsets are the box minimum
    put_f64(h + 179 + 16 * k, extent_max ? extent_max[k] : box_max[k]);  // max x, min x, max y, min y, max z, min z
    put_f64(h + 187 + 16 * k, extent_min ? extent_min[k] : box_min[k]);
  }
}

// no context: the files of a table are written by several threads
static int las_write_file(const char* path, uint64_t count, const void* body, uint32_t format, const double box_min[3],
                          const double box_max[3], double scale, std::string* err, const double* extent_min = nullptr,
                          const double* extent_max = nullptr) {
  unsigned char h[LAS_HEADER_BYTES];
  las_header(h, count, format, box_min, box_max, scale, extent_min, extent_max);
  return write_file(path, {{h, sizeof(h)}, {body, (size_t)(count * las_record_bytes(format))}}, err);
}

static int check_file_args(swz_ctx* c, const char* who, uint64_t count, const double box_min[3], const double box_max[3], double scale) {
  if (!box_min || !box_max || !finite3(box_min) || !finite3(box_max))
    return fail(c, SWZ_ERR_BAD_ARG, std::string(who) + ": the node box is not finite");
  if (!scale_ok(scale)) return fail(c, SWZ_ERR_BAD_ARG, std::string(who) + ": the scale is not finite and positive");
  if (count > 0xFFFFFFFFull) return fail(c, SWZ_ERR_BAD_ARG, std::string(who) + ": a LAS 1.2 header counts at most 2^32-1 records");
  return SWZ_OK;
}

template <uint32_t FORMAT>
static void las_convert_rows(unsigned char* body, uint64_t count, const double* xyz, const LasColumns& cols, const double offset[3],
                             double scale) {
  const uint32_t rb = las_record_bytes(FORMAT);
  for (uint64_t i = 0; i < count; ++i) {
    uint32_t rec[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    las_compose<FORMAT>(rec, xyz + 3 * i, cols, (size_t)i, offset, scale);
    unsigned char* out = body + i * rb;
    for (uint32_t k = 0; k < rb / 2; ++k) put_u16(out + 2 * k, rec[k / 2] >> (16u * (k & 1u)));
  }
}

struct LasFile {
  std::vector<unsigned char> data;
  uint64_t count = 0;
  uint32_t data_at = 0;
  swz_las_layout layout{};
};

static int las_parse(swz_ctx* c, const char* path, LasFile* f) {
  SWZ_TRY(read_whole_file(c, path, &f->data));
  const std::string where = std::string(" in ") + path;
  const unsigned char* h = f->data.data();
  const uint64_t size = f->data.size();
  if (size < LAS_HEADER_BYTES) return fail(c, SWZ_ERR_BAD_ARG, "shorter than a LAS 1.2 header" + where);
  if (memcmp(h, "LASF", 4) != 0) return fail(c, SWZ_ERR_BAD_ARG, "not a LAS file (signature)" + where);
  const uint64_t header_size = get_u16(h + 94), data_at = get_u32(h + 96);
  if (header_size < LAS_HEADER_BYTES || header_size > size || data_at < header_size || data_at > size)
    return fail(c, SWZ_ERR_BAD_ARG, "the header size or the offset to the point data passes the file" + where);
  const uint32_t format = h[104], rb = get_u16(h + 105);
  if (format > 3)
    return fail(c, SWZ_ERR_BAD_ARG, "point data record formats 0-3 are read here; swz_las_decode_device decodes the others" + where);
  if (rb < las_record_bytes(format)) return fail(c, SWZ_ERR_BAD_ARG, "the record length is below the format's" + where);
  const uint64_t count = get_u32(h + 107);
  if (count > (size - data_at) / rb) return fail(c, SWZ_ERR_BAD_ARG, "the point records pass the end of the file" + where);
  f->count = count;
  f->data_at = (uint32_t)data_at;
  for (int k = 0; k < 3; ++k) {
    f->layout.scale[k] = get_f64(h + 131 + 8 * k);
    f->layout.offset[k] = get_f64(h + 155 + 8 * k);
    f->layout.max[k] = get_f64(h + 179 + 16 * k);
    f->layout.min[k] = get_f64(h + 187 + 16 * k);
  }
  f->layout.point_format = format;
  f->layout.record_bytes = rb;
  return SWZ_OK;
}

static int make_dir(const std::string& path) {
  if (mkdir(path.c_str(), 0777) == 0) return 0;
  struct stat st;
  return (stat(path.c_str(), &st) == 0 && S_ISDIR(st.st_mode)) ? 0 : -1;
}

static void put_string(std::string& s, const char* text) {
  s += '"';
  for (const char* p = text ? text : ""; *p; ++p) {
    const unsigned char ch = (unsigned char)*p;
    if (ch == '"' || ch == '\\') {
      s += '\\';
      s += (char)ch;
    } else if (ch < 0x20) {
      char buf[8];
      snprintf(buf, sizeof(buf), "\\u%04x", ch);
      s += buf;
    } else {
      s += (char)ch;
    }
  }
  s += '"';
}

// a node as (depth = number of octants, the key's bits above that depth): what orders and names the hierarchy's entries
struct EptNode {
  int depth;
  uint64_t prefix;
  bool operator<(const EptNode& o) const { return depth != o.depth ? depth < o.depth : prefix < o.prefix; }
};
static EptNode ept_ancestor(EptNode n, int depth) { return {depth, n.prefix >> (3 * (n.depth - depth))}; }
static std::string ept_name(EptNode n) {
  char name[72];
  (void)swz_node_name_entwine((int8_t)(n.depth - 1), n.depth ? n.prefix << (3 * (MAX_LEVELS - n.depth)) : 0, name);
  return name;
}

}  // namespace swz

using namespace swz;

extern "C" {

double swz_las_scale_from_bounds(const double box_min[3], const double box_max[3]) {
  // compute_las_scale_from_bounds (LASPersistence.cpp:16-28) on extent().length()
  const double ex = box_max[0] - box_min[0], ey = box_max[1] - box_min[1], ez = box_max[2] - box_min[2];
  const double diagonal = std::sqrt(ex * ex + ey * ey + ez * ez);
  if (diagonal > 1000000) return 0.01;
  if (diagonal > 1) return 0.001;  // (the reference has a branch of its own above 100 000 with the same value)
  return 0.0001;
}

int swz_las_stored_box(const double box_min[3], const double box_max[3], const double las_offset[3], double scale,
                       double min_out[3], double max_out[3]) {
  if (!box_min || !box_max || !las_offset || !min_out || !max_out || !scale_ok(scale)) return SWZ_ERR_BAD_ARG;
  for (int ax = 0; ax < 3; ++ax) {  // las_quantize, then swz_las_read_node's offset + X * scale
    min_out[ax] = las_offset[ax] + (double)las_quantize(box_min[ax], las_offset[ax], scale) * scale;
    max_out[ax] = las_offset[ax] + (double)las_quantize(box_max[ax], las_offset[ax], scale) * scale;
  }
  return SWZ_OK;
}

int swz_las_record_layout(uint32_t mask, uint32_t* point_format_out, uint32_t* record_bytes_out) {
  if (mask & ~LAS_MASK_ALL) return SWZ_ERR_BAD_ARG;
  const uint32_t format = las_format(mask);
  if (point_format_out) *point_format_out = format;
  if (record_bytes_out) *record_bytes_out = las_record_bytes(format);
  return SWZ_OK;
}

uint32_t swz_las_pack_tile(void) { return (uint32_t)LAS_TILE; }

int swz_las_image_layout(uint64_t num_nodes, const uint64_t* node_count, uint32_t mask, uint64_t* body_offset_out,
                         uint64_t* body_size_out, uint64_t* total_out) {
  if ((num_nodes && !node_count) || (mask & ~LAS_MASK_ALL)) return SWZ_ERR_BAD_ARG;
  const uint32_t rb = las_record_bytes(las_format(mask));
  uint64_t at = 0;
  for (uint64_t k = 0; k < num_nodes; ++k) {
    if (node_count[k] > 0xFFFFFFFFull) return SWZ_ERR_BAD_ARG;  // a header's number of point records is a u32
    const uint64_t size = las_body_size(node_count[k], rb);
    if (body_offset_out) body_offset_out[k] = at;
    if (body_size_out) body_size_out[k] = size;
    at += size;
  }
  if (total_out) *total_out = at;
  return SWZ_OK;
}

int swz_las_pack_device(swz_ctx* c, const uint32_t* d_perm, const uint32_t* d_order, uint64_t n, const double* d_xyz,
                        const swz_attribute_columns* d_in, uint64_t num_nodes, const uint64_t* node_offset, const uint64_t* node_count,
                        const double* node_las_offset, const double* node_las_scale, uint32_t mask, void* d_image_out,
                        uint64_t image_bytes) {
  if (!c) return SWZ_ERR_BAD_ARG;
  // everything is checked on the host before anything is launched
  if (n > LAS_MAX_POINTS) return c->fail(SWZ_ERR_BAD_ARG, "swz_las_pack_device: more than 2^32-65536 rows");
  SWZ_TRY(check_mask(c, "swz_las_pack_device", d_in, mask));
  if (num_nodes && (!node_offset || !node_count || !node_las_offset || !node_las_scale))
    return c->fail(SWZ_ERR_BAD_ARG, "swz_las_pack_device: NULL node table");
  const uint32_t format = las_format(mask), rb = las_record_bytes(format);
  const PackNames names{"swz_las_pack_device", "swz_las_image_layout", "las_nodes"};
  PackTable<LasNode> table;
  SWZ_TRY(pack_build_table(
    c, names, n, num_nodes, node_offset, node_count,
    [&](uint64_t k, LasNode* nd) -> const char* {
      if (!scale_ok(node_las_scale[k])) return "a scale is not finite and positive";
      if (!finite3(node_las_offset + 3 * k)) return "an offset is not finite";
      for (int a = 0; a < 3; ++a) nd->offset[a] = node_las_offset[3 * k + a];
      nd->scale = node_las_scale[k];
      return nullptr;
    },
    [&](uint64_t cnt, uint64_t* bytes) -> const char* {
      *bytes = las_body_size(cnt, rb);
      return nullptr;
    },
    &table));
  const uint64_t at = table.image_bytes, prev_end = table.prev_end;

  LasPackArgs a{};
  SWZ_TRY(pack_upload_table(c, names, table, d_perm, d_xyz, d_image_out, image_bytes, &a.nodes));
  if (!a.nodes) return SWZ_OK;
  a.perm = d_perm;
  a.order = d_order;
  a.n = (uint32_t)n;
  a.xyz = d_xyz;
  a.cols = las_columns(d_in, mask);
  a.image = static_cast<uint8_t*>(d_image_out);
  a.num_nodes = (uint32_t)table.nodes.size();
  {
    uint64_t row = 24;
    for (int k = 0; k < SWZ_ATTR_COUNT; ++k)
      if (k != SWZ_ATTR_NORMAL && ((mask >> k) & 1u)) row += swz_attribute_row_bytes(k);
    ProfScope ps(c, "las_pack", n * (d_order ? 8 : 4) + prev_end * row + at, 1);
    // rows behind the last node belong to no body: the grid ends with it
    const dim3 grid(div_up(prev_end, LAS_TILE)), block(LAS_TILE);
    switch (format) {
      case 0: hipLaunchKernelGGL(las_pack_kernel<0>, grid, block, 0, c->stream, a); break;
      case 1: hipLaunchKernelGGL(las_pack_kernel<1>, grid, block, 0, c->stream, a); break;
      case 2: hipLaunchKernelGGL(las_pack_kernel<2>, grid, block, 0, c->stream, a); break;
      default: hipLaunchKernelGGL(las_pack_kernel<3>, grid, block, 0, c->stream, a); break;
    }
    SWZ_LAUNCH_CHECK(c);
  }
  SWZ_HIP(c, hipStreamSynchronize(c->stream));
  return SWZ_OK;
}

int swz_las_write_node(swz_ctx* c, const char* path, uint64_t count, const void* body, uint32_t mask, const double box_min[3],
                       const double box_max[3], double scale) {
  if (!path) return fail(c, SWZ_ERR_BAD_ARG, "swz_las_write_node: NULL path");
  if (mask & ~LAS_MASK_ALL) return fail(c, SWZ_ERR_BAD_ARG, "swz_las_write_node: the mask names an attribute that does not exist");
  SWZ_TRY(check_file_args(c, "swz_las_write_node", count, box_min, box_max, scale));
  if (count == 0) return SWZ_OK;  // like swz_bin_write_node: an empty node has no file
  if (!body) return fail(c, SWZ_ERR_BAD_ARG, "swz_las_write_node: NULL body");
  std::string err;
  const int st = las_write_file(path, count, body, las_format(mask), box_min, box_max, scale, &err);
  return st == SWZ_OK ? SWZ_OK : fail(c, st, err);
}

int swz_las_write_node_extent(swz_ctx* c, const char* path, uint64_t count, const void* body, uint32_t mask, const double box_min[3],
                              const double box_max[3], double scale, const double extent_min[3], const double extent_max[3]) {
  if (!path) return fail(c, SWZ_ERR_BAD_ARG, "swz_las_write_node_extent: NULL path");
  if (mask & ~LAS_MASK_ALL) return fail(c, SWZ_ERR_BAD_ARG, "swz_las_write_node_extent: the mask names an attribute that does not exist");
  SWZ_TRY(check_file_args(c, "swz_las_write_node_extent", count, box_min, box_max, scale));
  if (count == 0) return SWZ_OK;
  if (!body) return fail(c, SWZ_ERR_BAD_ARG, "swz_las_write_node_extent: NULL body");
  if (!extent_min || !extent_max || !finite3(extent_min) || !finite3(extent_max))
    return fail(c, SWZ_ERR_BAD_ARG, "swz_las_write_node_extent: the extent is not finite");
  std::string err;
  const int st = las_write_file(path, count, body, las_format(mask), box_min, box_max, scale, &err, extent_min, extent_max);
  return st == SWZ_OK ? SWZ_OK : fail(c, st, err);
}

int swz_las_write_node_rows(swz_ctx* c, const char* path, uint64_t count, const double* xyz, const swz_attribute_columns* columns,
                            uint32_t mask, const double box_min[3], const double box_max[3], double scale) {
  if (!path) return fail(c, SWZ_ERR_BAD_ARG, "swz_las_write_node_rows: NULL path");
  SWZ_TRY(check_mask(c, "swz_las_write_node_rows", columns, mask));
  SWZ_TRY(check_file_args(c, "swz_las_write_node_rows", count, box_min, box_max, scale));
  if (count == 0) return SWZ_OK;
  if (!xyz) return fail(c, SWZ_ERR_BAD_ARG, "swz_las_write_node_rows: NULL positions");
  const uint32_t format = las_format(mask);
  std::vector<unsigned char> body((size_t)(count * las_record_bytes(format)));
  const LasColumns cols = las_columns(columns, mask);
  switch (format) {
    case 0: las_convert_rows<0>(body.data(), count, xyz, cols, box_min, scale); break;
    case 1: las_convert_rows<1>(body.data(), count, xyz, cols, box_min, scale); break;
    case 2: las_convert_rows<2>(body.data(), count, xyz, cols, box_min, scale); break;
    default: las_convert_rows<3>(body.data(), count, xyz, cols, box_min, scale); break;
  }
  std::string err;
  const int st = las_write_file(path, count, body.data(), format, box_min, box_max, scale, &err);
  return st == SWZ_OK ? SWZ_OK : fail(c, st, err);
}

int swz_las_persist_nodes(swz_ctx* c, const char* dir, uint64_t num_nodes, const int8_t* node_level, const uint64_t* node_key,
                          const uint64_t* node_count, const double* node_box_min, const double* node_box_max, const double* node_scale,
                          const void* image, uint64_t image_bytes, uint32_t mask, int naming) {
  if (!dir || (num_nodes && (!node_level || !node_key || !node_count || !node_box_min || !node_box_max || !node_scale)))
    return fail(c, SWZ_ERR_BAD_ARG, "swz_las_persist_nodes: NULL argument");
  if (naming != SWZ_LAS_NAMING_POTREE && naming != SWZ_LAS_NAMING_ENTWINE)
    return fail(c, SWZ_ERR_BAD_ARG, "swz_las_persist_nodes: unknown naming");
  std::vector<uint64_t> at(num_nodes);
  uint64_t total = 0;
  if (swz_las_image_layout(num_nodes, node_count, mask, at.data(), nullptr, &total) != SWZ_OK)
    return fail(c, SWZ_ERR_BAD_ARG, "swz_las_persist_nodes: bad mask, or a node too large for a LAS 1.2 file");
  if (total > image_bytes || (total && !image)) return fail(c, SWZ_ERR_BAD_ARG, "swz_las_persist_nodes: the image is smaller than the table's layout");
  for (uint64_t k = 0; k < num_nodes; ++k) {
    char name[72];
    if (swz_node_name_entwine(node_level[k], node_key[k], name) != SWZ_OK) return fail(c, SWZ_ERR_BAD_ARG, "bad node level");
    SWZ_TRY(check_file_args(c, "swz_las_persist_nodes", node_count[k], node_box_min + 3 * k, node_box_max + 3 * k, node_scale[k]));
  }
  const uint32_t format = las_format(mask);
  std::string first_err;
  const int st = run_tickets(c, num_nodes, [&](uint64_t k, std::string* err) {
    if (node_count[k] == 0) return (int)SWZ_OK;
    char name[72];
    if (naming == SWZ_LAS_NAMING_ENTWINE) (void)swz_node_name_entwine(node_level[k], node_key[k], name);
    else (void)swz_node_name(node_level[k], node_key[k], name);
    const std::string path = std::string(dir) + "/" + name + ".las";
    return las_write_file(path.c_str(), node_count[k], static_cast<const unsigned char*>(image) + at[k], format, node_box_min + 3 * k,
                          node_box_max + 3 * k, node_scale[k], err);
  }, &first_err);
  return st == SWZ_OK ? SWZ_OK : fail(c, st, first_err);
}

int swz_las_read_header(swz_ctx* c, const char* path, uint64_t* count_out, uint32_t* point_format_out, uint32_t* record_bytes_out,
                        uint32_t* offset_to_point_data_out, swz_las_layout* layout_out) {
  if (!path) return fail(c, SWZ_ERR_BAD_ARG, "swz_las_read_header: NULL path");
  LasFile f;
  SWZ_TRY(las_parse(c, path, &f));
  if (count_out) *count_out = f.count;
  if (point_format_out) *point_format_out = f.layout.point_format;
  if (record_bytes_out) *record_bytes_out = f.layout.record_bytes;
  if (offset_to_point_data_out) *offset_to_point_data_out = f.data_at;
  if (layout_out) *layout_out = f.layout;
  return SWZ_OK;
}

int swz_las_read_node(swz_ctx* c, const char* path, double* xyz_out, const swz_attribute_columns* columns_out) {
  if (!path) return fail(c, SWZ_ERR_BAD_ARG, "swz_las_read_node: NULL path");
  LasFile f;
  SWZ_TRY(las_parse(c, path, &f));
  const swz_las_layout& L = f.layout;
  auto col = [&](int a) -> void* { return columns_out ? columns_out->column[a] : nullptr; };
  const uint32_t gps_at = 20, rgb_at = (L.point_format & 1u) ? 28 : 20;
  for (uint64_t i = 0; i < f.count; ++i) {
    const unsigned char* r = f.data.data() + f.data_at + i * L.record_bytes;
    if (xyz_out) {
      // position_from_las_point (LASFile.cpp:79-94): offset + X * scale, then min(max, max(min, p)) per axis
      for (int ax = 0; ax < 3; ++ax) {
        double p = L.offset[ax] + (double)(int32_t)get_u32(r + 4 * ax) * L.scale[ax];
        p = std::min(L.max[ax], std::max(L.min[ax], p));
        xyz_out[3 * i + ax] = p;
      }
    }
    if (void* o = col(SWZ_ATTR_INTENSITY)) static_cast<uint16_t*>(o)[i] = (uint16_t)get_u16(r + 12);
    if (void* o = col(SWZ_ATTR_RETURN_NUMBER)) static_cast<uint8_t*>(o)[i] = r[14] & 7u;
    if (void* o = col(SWZ_ATTR_NUMBER_OF_RETURNS)) static_cast<uint8_t*>(o)[i] = (r[14] >> 3) & 7u;
    if (void* o = col(SWZ_ATTR_SCAN_DIRECTION_FLAG)) static_cast<uint8_t*>(o)[i] = (r[14] >> 6) & 1u;
    if (void* o = col(SWZ_ATTR_EDGE_OF_FLIGHT_LINE)) static_cast<uint8_t*>(o)[i] = (r[14] >> 7) & 1u;
    if (void* o = col(SWZ_ATTR_CLASSIFICATION)) static_cast<uint8_t*>(o)[i] = r[15] & 31u;
    if (void* o = col(SWZ_ATTR_SCAN_ANGLE_RANK)) static_cast<int8_t*>(o)[i] = (int8_t)r[16];
    if (void* o = col(SWZ_ATTR_USER_DATA)) static_cast<uint8_t*>(o)[i] = r[17];
    if (void* o = col(SWZ_ATTR_POINT_SOURCE_ID)) static_cast<uint16_t*>(o)[i] = (uint16_t)get_u16(r + 18);
    if (void* o = col(SWZ_ATTR_GPS_TIME)) static_cast<double*>(o)[i] = (L.point_format & 1u) ? get_f64(r + gps_at) : 0.0;
    if (void* o = col(SWZ_ATTR_RGB)) {
      // las_read_points_into (LASFile.cpp:592-597): static_cast<uint8_t>(rgb[k] >> 8)
      for (int k = 0; k < 3; ++k)
        static_cast<uint8_t*>(o)[3 * i + k] = (L.point_format & 2u) ? (uint8_t)(get_u16(r + rgb_at + 2 * k) >> 8) : 0;
    }
  }
  return SWZ_OK;
}

int swz_ept_create_dirs(swz_ctx* c, const char* dir) {
  if (!dir) return fail(c, SWZ_ERR_BAD_ARG, "swz_ept_create_dirs: NULL directory");
  const std::string root = dir;
  for (const char* sub : {"", "/ept-data", "/ept-hierarchy", "/ept-sources"})
    if (make_dir(root + sub) != 0) return fail(c, SWZ_ERR_BAD_ARG, "swz_ept_create_dirs: cannot create " + root + sub);
  return SWZ_OK;
}

int swz_ept_hierarchy_write(swz_ctx* c, const char* dir, uint64_t num_nodes, const int8_t* node_level, const uint64_t* node_key,
                            const uint64_t* node_count) {
  if (!dir || (num_nodes && (!node_level || !node_key || !node_count)))
    return fail(c, SWZ_ERR_BAD_ARG, "swz_ept_hierarchy_write: NULL argument");
  // create_hierarchy_files (EntwinePersistence.cpp:51-130): a node goes into the file of its nearest ancestor-or-self whose
  // depth is a multiple of SPLIT_DEPTH; such a subtree root is entered with -1 in the file of the subtree root above it
  constexpr int SPLIT_DEPTH = 5;
  std::map<EptNode, std::map<EptNode, int64_t>> files;
  for (uint64_t k = 0; k < num_nodes; ++k) {
    if (node_level[k] < -1 || node_level[k] >= (int)MAX_LEVELS) return fail(c, SWZ_ERR_BAD_ARG, "swz_ept_hierarchy_write: bad node level");
    if (node_count[k] == 0) continue;
    const int depth = node_level[k] + 1;
    const EptNode node{depth, depth ? node_key[k] >> (3 * (MAX_LEVELS - depth)) : 0};
    const EptNode root = ept_ancestor(node, depth - depth % SPLIT_DEPTH);
    if (!files.count(root)) {
      for (EptNode r = root; r.depth > 0;) {
        const EptNode above = ept_ancestor(r, r.depth - SPLIT_DEPTH);
        files[above][r] = -1;
        r = above;
      }
    }
    files[root][node] = (int64_t)node_count[k];
  }
  std::vector<const std::pair<const EptNode, std::map<EptNode, int64_t>>*> list;
  for (const auto& kv : files) list.push_back(&kv);
  std::string first_err;
  const int st = run_tickets(c, list.size(), [&](uint64_t k, std::string* err) {
    std::string s = "{";
    for (const auto& entry : list[k]->second) {
      if (s.size() > 1) s += ",";
      s += "\"" + ept_name(entry.first) + "\":" + std::to_string(entry.second);
    }
    s += "}";
    return write_file(std::string(dir) + "/ept-hierarchy/" + ept_name(list[k]->first) + ".json", {{s.data(), s.size()}}, err);
  }, &first_err);
  return st == SWZ_OK ? SWZ_OK : fail(c, st, first_err);
}

int swz_ept_json_write(swz_ctx* c, const char* path, const swz_ept_json* ept) {
  if (!path || !ept) return fail(c, SWZ_ERR_BAD_ARG, "swz_ept_json_write: NULL argument");
  if (ept->attribute_mask & ~LAS_MASK_ALL) return fail(c, SWZ_ERR_BAD_ARG, "swz_ept_json_write: the mask names an attribute that does not exist");
  if (!finite3(ept->bounds_min) || !finite3(ept->bounds_max) || !finite3(ept->conforming_min) || !finite3(ept->conforming_max) ||
      !std::isfinite(ept->span))
    return fail(c, SWZ_ERR_BAD_ARG, "swz_ept_json_write: a number is not finite");
  // write_ept_json (EntwinePersistence.cpp:197-269)
  std::string s = "{";
  const double* boxes[2][2] = {{ept->bounds_min, ept->bounds_max}, {ept->conforming_min, ept->conforming_max}};
  for (int b = 0; b < 2; ++b) {
    s += b ? ",\"boundsConforming\":[" : "\"bounds\":[";
    for (int k = 0; k < 6; ++k) {
      if (k) s += ",";
      put_number(s, boxes[b][k / 3][k % 3]);
    }
    s += "]";
  }
  s += ",\"dataType\":\"las\",\"hierarchyType\":\"json\",\"points\":" + std::to_string(ept->points) + ",\"schema\":[";
  // point_attributes_to_ept_schema (:132-194); the reference iterates an unordered set, here: position, then by SWZ_ATTR_*
  struct Entry {
    int attribute;
    const char* name;
    int size;
    const char* type;
  };
  static const Entry entries[] = {
    {-1, "X", 4, "signed"}, {-1, "Y", 4, "signed"}, {-1, "Z", 4, "signed"},
    {SWZ_ATTR_RGB, "Red", 2, "unsigned"}, {SWZ_ATTR_RGB, "Green", 2, "unsigned"}, {SWZ_ATTR_RGB, "Blue", 2, "unsigned"},
    {SWZ_ATTR_NORMAL, "NX", 4, "float"}, {SWZ_ATTR_NORMAL, "NY", 4, "float"}, {SWZ_ATTR_NORMAL, "NZ", 4, "float"},
    {SWZ_ATTR_INTENSITY, "Intensity", 2, "unsigned"}, {SWZ_ATTR_CLASSIFICATION, "Classification", 1, "unsigned"},
    {SWZ_ATTR_EDGE_OF_FLIGHT_LINE, "EdgeOfFlightLine", 1, "unsigned"}, {SWZ_ATTR_GPS_TIME, "GpsTime", 8, "float"},
    {SWZ_ATTR_NUMBER_OF_RETURNS, "NumberOfReturns", 1, "unsigned"}, {SWZ_ATTR_RETURN_NUMBER, "ReturnNumber", 1, "unsigned"},
    {SWZ_ATTR_POINT_SOURCE_ID, "PointSourceID", 2, "unsigned"}, {SWZ_ATTR_SCAN_DIRECTION_FLAG, "ScanDirectionFlag", 1, "unsigned"},
    {SWZ_ATTR_SCAN_ANGLE_RANK, "ScanAngleRank", 1, "signed"}, {SWZ_ATTR_USER_DATA, "UserData", 1, "unsigned"}};
  bool any = false;
  for (const Entry& e : entries) {
    if (e.attribute >= 0 && !((ept->attribute_mask >> e.attribute) & 1u)) continue;
    if (any) s += ",";
    any = true;
    s += std::string("{\"name\":\"") + e.name + "\",\"size\":" + std::to_string(e.size) + ",\"type\":\"" + e.type + "\"";
    if (e.attribute < 0) s += ",\"offset\":0,\"scale\":1";
    s += "}";
  }
  s += "],\"span\":";
  put_number(s, ept->span);
  s += ",\"srs\":{\"authority\":";
  put_string(s, ept->srs_authority);
  s += ",\"horizontal\":";
  put_string(s, ept->srs_horizontal);
  s += ",\"wkt\":";
  put_string(s, ept->srs_wkt);
  s += "},\"version\":";
  put_string(s, ept->version);
  s += "}";
  std::string err;
  const int st = write_file(path, {{s.data(), s.size()}}, &err);
  return st == SWZ_OK ? SWZ_OK : fail(c, st, err);
}

}  // extern "C"
