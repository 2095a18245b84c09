// swz_pnts.hip -- 3D Tiles output: .pnts node files whose bodies are packed on the device, and the tileset JSON files
// (reference: core/io/PNTSWriter.cpp:109-264, 507-527, core/io/Cesium3DTilesPersistence.cpp:53-210,
// core/io/TileSetWriter.cpp:15-210, core/pointcloud/Tileset.cpp:94-118).
//
// A .pnts file is a 28-byte header, the feature-table JSON padded with spaces to a multiple of 8 (counted from the start
// of the JSON, as the reference has it) and the feature-table binary: POSITION (3 x f32), RGB (3 x u8), INTENSITY (u16),
// each array at the running offset rounded up to its alignment (4, 1, 2), the whole zero-padded to a multiple of 8.  The
// binary of a node is its BODY; the bodies of all nodes of a table, one behind the other, are the IMAGE that
// swz_pnts_pack_device writes in one pass (permuted gather + narrowing + colour mapping + final layout).
//
// Numbers in JSON are written in the shortest text that parses back to the same double (std::to_chars).  The reference's
// rapidjson does not always find the shortest form (Grisu2), so a file agrees with the reference's in every parsed value and
// in every byte of the binary, but not necessarily in the length of the JSON text; the spelling of a number is no part of
// either format.
#include <charconv>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <algorithm>
#include <limits>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include <sys/stat.h>

#include "swz_internal.h"
#include "swz_convert.h"
#include "swz_device.h"
#include "swz_hostio.h"
#include "swz_nodepack.h"
#include "swz_srs.h"

namespace swz {

constexpr uint32_t PNTS_MASK_ALL = SWZ_PNTS_RGB | SWZ_PNTS_INTENSITY;
constexpr uint64_t PNTS_MAX_POINTS = 0xFFFFFFFFull - 65535ull;  // the library's limit of points per batch (2^32 - 65536)
constexpr uint64_t PNTS_MAX_BODY = 0xFFFFFFFFull - 28ull - 1024ull;  // byteLength is a u32: header + JSON + body must fit

// The body of a node of `count` points: POSITION at 0, RGB at rgb (12 * count), INTENSITY at intensity (the end of what
// lies in front of it, rounded up to 2), size = the end rounded up to 8.  rgb_end: where the padded RGB array ends (the
// start of the next array, or the end of the body).
template <typename U>
struct PntsBody {
  U rgb, rgb_end, intensity, size;
};
template <typename U>
__host__ __device__ inline PntsBody<U> pnts_body(U count, uint32_t mask) {
  PntsBody<U> b;
  b.rgb = 12 * count;
  U end = (mask & SWZ_PNTS_RGB) ? 15 * count : 12 * count;
  b.intensity = (end + 1) & ~(U)1;
  if (mask & SWZ_PNTS_INTENSITY) end = b.intensity + 2 * count;
  b.size = (end + 7) & ~(U)7;
  b.rgb_end = (mask & SWZ_PNTS_INTENSITY) ? b.intensity : b.size;
  if (!(mask & SWZ_PNTS_RGB)) b.rgb = 0;
  if (!(mask & SWZ_PNTS_INTENSITY)) b.intensity = 0;
  if (count == 0) b.rgb = b.rgb_end = b.intensity = b.size = 0;
  return b;
}

// ---------------------------------------------------------------------------------- the grey table
// RGBFromIntensityAttribute (PNTSWriter.cpp:507-527).  LINEAR: intensity >> 8.  LOG: (uint8_t)(255 * std::log((float)
// intensity + 1) / std::log(65535)) -- the numerator is a float product of logf, the division is in double, the cast
// truncates.  Evaluated with the HOST's libm, once, for all 65 536 intensities: logf on the device is not guaranteed to
// round like glibc's, and one ulp changes a truncated value.
static uint8_t grey_of(int mapping, uint16_t intensity) {
  if (mapping == SWZ_PNTS_RGB_FROM_INTENSITY_LINEAR) return static_cast<uint8_t>(intensity >> 8);
  if (mapping == SWZ_PNTS_RGB_FROM_INTENSITY_LOG) {
    const float numerator = 255 * std::log(static_cast<float>(intensity) + 1);
    const double denominator = std::log(static_cast<double>(65535));
    return static_cast<uint8_t>(numerator / denominator);
  }
  return 0;
}
static const uint8_t* grey_table(int mapping) {
  static std::once_flag once;
  static uint8_t table[2][65536];
  std::call_once(once, [] {
    for (uint32_t i = 0; i < 65536; ++i) {
      table[0][i] = grey_of(SWZ_PNTS_RGB_FROM_INTENSITY_LINEAR, (uint16_t)i);
      table[1][i] = grey_of(SWZ_PNTS_RGB_FROM_INTENSITY_LOG, (uint16_t)i);
    }
  });
  return table[mapping == SWZ_PNTS_RGB_FROM_INTENSITY_LOG ? 1 : 0];
}

// ---------------------------------------------------------------------------------- the pack kernel
constexpr int PNTS_TILE = 256;  // stored rows per block, one per thread

struct PntsNode {  // an entry of the pack table (swz_nodepack.h)
  uint32_t start, count;
  uint64_t base;  // of the body in the image, a multiple of 8
};

struct PntsPackArgs {
  const uint32_t* perm;
  const uint32_t* order;  // may be null: identity
  uint32_t n;
  const double* xyz;
  const uint8_t* rgb;
  const uint16_t* intensity;
  const uint8_t* grey;  // 65 536 grey values when RGB is mapped from the intensity, else null
  const PntsNode* nodes;
  uint32_t num_nodes;
  uint32_t mask;
  uint8_t* image;
  const double* origin;  // swz_pnts_pack_origin_device: 3 per entry of `nodes`, else null
};

// The part of one byte array (rows of RB bytes) of a node that this thread writes.  `body` is the node's body in the image,
// the array lies at [off, pad_end) of it: count rows, then zeros up to where the next array (or the body) ends.  The block
// holds the rows [seg_lo, seg_hi) of the node; their bytes lie in LDS from lds on.  Every aligned dword of the body belongs
// to the row that holds the dword's first byte (the block's first row of the node also takes the dword its bytes begin
// in, the node's last row everything up to pad_end).  A dword that lies inside what this block holds of the array leaves as
// one dword store; one that reaches beyond -- into another array, or into rows of the neighbouring block -- leaves as byte
// stores of the part that is this block's, so that no byte is written twice or read back.
template <uint32_t RB>
__device__ __forceinline__ void pnts_emit_bytes(uint8_t* __restrict__ body, const uint8_t* lds, uint32_t off, uint32_t pad_end,
                                                uint32_t j, uint32_t count, uint32_t seg_lo, uint32_t seg_hi) {
  const uint32_t a0 = off + RB * j;
  const uint32_t d0 = off + RB * seg_lo, d1_data = off + RB * seg_hi;
  const uint32_t d1 = seg_hi == count ? pad_end : d1_data;
  const uint32_t end = j + 1 == count ? pad_end : a0 + RB;
  for (uint32_t w = j == seg_lo ? (a0 & ~3u) : ((a0 + 3u) & ~3u); w < end; w += 4) {
    const uint32_t lo = max(w, d0), hi = min(w + 4u, d1);
    uint32_t v = 0;
    for (uint32_t b = lo; b < hi; ++b) {
      const uint32_t byte = b < d1_data ? (uint32_t)lds[b - d0] : 0u;
      v |= byte << (8u * (b - w));
    }
    if (hi - lo == 4u) {
      *reinterpret_cast<uint32_t*>(body + w) = v;
    } else {
      for (uint32_t b = lo; b < hi; ++b) body[b] = (uint8_t)(v >> (8u * (b - w)));
    }
  }
}

// One block takes PNTS_TILE consecutive stored rows.  It finds the node of its first row with one binary search in the
// table, walks forward from there (swz_nodepack.h), loads its rows -- scattered 24-byte position reads, the narrowing is
// the plain cast (round to nearest even) -- into LDS and writes from there:
// positions as dwords in the order of the image, the 3- and 2-byte rows as aligned dwords put together from LDS.
// ORIGIN (swz_pnts_pack_origin_device): the window also keeps every node's origin, and a position is narrowed after the
// origin has been subtracted from it in double; nothing else differs.
template <bool ORIGIN>
__global__ __launch_bounds__(PNTS_TILE) void pnts_pack_kernel(PntsPackArgs a) {
  __shared__ uint32_t s_start[PNTS_TILE];
  __shared__ uint32_t s_count[PNTS_TILE];
  __shared__ uint64_t s_base[PNTS_TILE];
  __shared__ uint32_t s_pos[PNTS_TILE * 3];
  __shared__ uint32_t s_rgb[PNTS_TILE * 3 / 4];
  __shared__ uint16_t s_int[PNTS_TILE];
  __shared__ uint16_t s_node[PNTS_TILE];
  __shared__ double s_origin[ORIGIN ? PNTS_TILE * 3 : 1];
  const uint32_t t = threadIdx.x;
  const uint32_t r0 = blockIdx.x * (uint32_t)PNTS_TILE;
  const uint32_t r1 = (uint32_t)min((uint64_t)r0 + PNTS_TILE, (uint64_t)a.n);

  const uint32_t k0 = pack_first_node(a.nodes, a.num_nodes, r0);
  const PntsNode* const listed = pack_fill_window(a.nodes, a.num_nodes, k0, r1, s_start, s_count);
  s_base[t] = listed ? listed->base : 0ull;
  if constexpr (ORIGIN) {
#pragma unroll
    for (int k = 0; k < 3; ++k) s_origin[3 * t + k] = listed ? a.origin[3 * (size_t)(k0 + t) + k] : 0.0;
  }
  __syncthreads();

  const uint32_t r = r0 + t;
  uint32_t e;
  const bool in_node = pack_row_node<PNTS_TILE>(s_start, s_count, r, r1, &e);
  uint8_t* const rgb_bytes = reinterpret_cast<uint8_t*>(s_rgb);
  if (in_node) {
    double pos[3];
    const uint32_t src = pack_source_row(a.perm, a.order, a.xyz, r, pos);
    if constexpr (ORIGIN) {
#pragma unroll
      for (int k = 0; k < 3; ++k) pos[k] = pos[k] - s_origin[3 * e + k];
    }
    s_pos[3 * t + 0] = __float_as_uint((float)pos[0]);
    s_pos[3 * t + 1] = __float_as_uint((float)pos[1]);
    s_pos[3 * t + 2] = __float_as_uint((float)pos[2]);
    uint16_t in = 0;
    if (a.intensity) in = a.intensity[src];
    if (a.mask & SWZ_PNTS_RGB) {
      if (a.grey) {
        const uint8_t g = a.grey[in];
        rgb_bytes[3 * t + 0] = g;
        rgb_bytes[3 * t + 1] = g;
        rgb_bytes[3 * t + 2] = g;
      } else {
        const uint8_t* c = a.rgb + (size_t)src * 3;
        rgb_bytes[3 * t + 0] = c[0];
        rgb_bytes[3 * t + 1] = c[1];
        rgb_bytes[3 * t + 2] = c[2];
      }
    }
    if (a.mask & SWZ_PNTS_INTENSITY) s_int[t] = in;
  }
  s_node[t] = in_node ? (uint16_t)e : (uint16_t)0xFFFFu;
  __syncthreads();

  // positions: dword w of the tile's rows, consecutive threads write consecutive dwords of a body
  for (uint32_t w = t; w < 3u * PNTS_TILE; w += PNTS_TILE) {
    const uint32_t row = w / 3u, c = w - 3u * row;
    const uint32_t en = s_node[row];
    if (en != 0xFFFFu) {
      const uint32_t j = r0 + row - s_start[en];
      *reinterpret_cast<uint32_t*>(a.image + s_base[en] + 12ull * j + 4u * c) = s_pos[w];
    }
  }
  if (!in_node) return;
  const uint32_t start = s_start[e], count = s_count[e];
  uint8_t* const body = a.image + s_base[e];
  const uint32_t j = r - start;
  const uint32_t seg_lo = start < r0 ? r0 - start : 0u;
  const uint32_t seg_hi = min(count, r1 - start);
  const uint32_t lds_row = start + seg_lo - r0;  // the tile row of the block's first row of this node
  const PntsBody<uint32_t> b = pnts_body<uint32_t>(count, a.mask);
  if (a.mask == 0u) {
    // positions only: an odd count leaves four bytes up to the multiple of 8
    if (j + 1 == count && b.size != 12u * count) *reinterpret_cast<uint32_t*>(body + 12u * count) = 0u;
    return;
  }
  if (a.mask & SWZ_PNTS_RGB) pnts_emit_bytes<3>(body, rgb_bytes + 3u * lds_row, b.rgb, b.rgb_end, j, count, seg_lo, seg_hi);
  if (a.mask & SWZ_PNTS_INTENSITY)
    pnts_emit_bytes<2>(body, reinterpret_cast<const uint8_t*>(s_int) + 2u * lds_row, b.intensity, b.size, j, count, seg_lo, seg_hi);
}

// ---------------------------------------------------------------------------------- host helpers
static bool mask_ok(uint32_t mask) { return (mask & ~PNTS_MASK_ALL) == 0; }
static bool mapping_ok(int m) {
  return m == SWZ_PNTS_RGB_FROM_COLOR || m == SWZ_PNTS_RGB_FROM_INTENSITY_LINEAR || m == SWZ_PNTS_RGB_FROM_INTENSITY_LOG;
}

// header + feature-table JSON of a node file (PNTSWriter::flush / createFeatureTableBlob, PNTSWriter.cpp:109-264)
static std::string pnts_file_head(uint64_t count, uint32_t mask, const double rtc[3], uint64_t body_bytes) {
  const PntsBody<uint64_t> b = pnts_body<uint64_t>(count, mask);
  std::string json = "{\"POINTS_LENGTH\":" + std::to_string(count) + ",\"RTC_CENTER\":[";
  for (int k = 0; k < 3; ++k) {
    if (k) json += ",";
    put_number(json, rtc ? rtc[k] : 0.0);
  }
  json += "],\"POSITION\":{\"byteOffset\":0}";
  if (mask & SWZ_PNTS_RGB) json += ",\"RGB\":{\"byteOffset\":" + std::to_string(b.rgb) + "}";
  if (mask & SWZ_PNTS_INTENSITY) json += ",\"INTENSITY\":{\"byteOffset\":" + std::to_string(b.intensity) + "}";
  json += "}";
  while (json.size() % 8) json.push_back(' ');  // aligned from the start of the JSON, not of the file (PNTSWriter.cpp:241-258)
  const uint32_t head[7] = {0x73746e70u /* "pnts" */, 1u, (uint32_t)(28 + json.size() + body_bytes), (uint32_t)json.size(),
                            (uint32_t)body_bytes, 0u, 0u};
  return std::string(reinterpret_cast<const char*>(head), 28) + json;
}

// no context: the files of a table are written by several threads
static int pnts_write_file(const char* path, uint64_t count, const void* body, uint64_t body_bytes, uint32_t mask, const double rtc[3],
                           std::string* err) {
  const std::string head = pnts_file_head(count, mask, rtc, body_bytes);
  return write_file(path, {{head.data(), head.size()}, {body, (size_t)body_bytes}}, err);
}

static int check_columns(swz_ctx* c, const char* who, const swz_attribute_columns* cols, uint32_t mask, int mapping) {
  if (!mask_ok(mask)) return fail(c, SWZ_ERR_BAD_ARG, std::string(who) + ": the mask names an attribute a .pnts file does not hold");
  if (!mapping_ok(mapping)) return fail(c, SWZ_ERR_BAD_ARG, std::string(who) + ": unknown RGB mapping");
  const void* rgb = cols ? cols->column[SWZ_ATTR_RGB] : nullptr;
  const void* in = cols ? cols->column[SWZ_ATTR_INTENSITY] : nullptr;
  if (mapping != SWZ_PNTS_RGB_FROM_COLOR && !in)
    return fail(c, SWZ_ERR_BAD_ARG, std::string(who) + ": RGB from intensity needs the intensity column");
  if ((mask & SWZ_PNTS_RGB) && mapping == SWZ_PNTS_RGB_FROM_COLOR && !rgb)
    return fail(c, SWZ_ERR_BAD_ARG, std::string(who) + ": the mask names RGB but the column is absent");
  if ((mask & SWZ_PNTS_INTENSITY) && !in)
    return fail(c, SWZ_ERR_BAD_ARG, std::string(who) + ": the mask names INTENSITY but the column is absent");
  return SWZ_OK;
}

// ---------------------------------------------------------------------------------- a reader for the feature-table JSON
// One object whose members are numbers, arrays of numbers, or objects holding "byteOffset"; everything else a JSON text may
// hold is skipped.  Works on [p, end) only.
struct JsonCursor {
  const char* p;
  const char* end;
  void ws() {
    while (p < end && (*p == ' ' || *p == '\t' || *p == '\n' || *p == '\r')) ++p;
  }
  bool eat(char ch) {
    ws();
    if (p < end && *p == ch) {
      ++p;
      return true;
    }
    return false;
  }
  bool string(std::string* out) {
    ws();
    if (p >= end || *p != '"') return false;
    ++p;
    out->clear();
    while (p < end && *p != '"') {
      if (*p == '\\') {
        if (++p >= end) return false;
      }
      out->push_back(*p++);
    }
    if (p >= end) return false;
    ++p;
    return true;
  }
  bool number(double* out) {
    ws();
    const char* q = p;
    while (q < end && (*q == '-' || *q == '+' || *q == '.' || *q == 'e' || *q == 'E' || (*q >= '0' && *q <= '9'))) ++q;
    if (q == p || *p == '+') return false;
    const auto r = std::from_chars(p, q, *out);
    if (r.ec != std::errc() || r.ptr != q) return false;
    p = q;
    return true;
  }
  bool literal(const char* word) {
    const size_t n = strlen(word);
    if ((size_t)(end - p) < n || memcmp(p, word, n) != 0) return false;
    p += n;
    return true;
  }
  // any value; numbers of a flat array go to nums, the "byteOffset" of an object to *byte_offset
  bool value(int depth, std::vector<double>* nums, double* byte_offset, bool* is_number, double* number_out) {
    if (depth > 16) return false;
    ws();
    if (p >= end) return false;
    if (is_number) *is_number = false;
    if (*p == '{') {
      ++p;
      if (eat('}')) return true;
      for (;;) {
        std::string key;
        if (!string(&key) || !eat(':')) return false;
        bool num = false;
        double v = 0;
        if (!value(depth + 1, nullptr, nullptr, &num, &v)) return false;
        if (byte_offset && num && key == "byteOffset") *byte_offset = v;
        if (eat(',')) continue;
        return eat('}');
      }
    }
    if (*p == '[') {
      ++p;
      if (eat(']')) return true;
      for (;;) {
        bool num = false;
        double v = 0;
        if (!value(depth + 1, nullptr, nullptr, &num, &v)) return false;
        if (nums && num) nums->push_back(v);
        if (eat(',')) continue;
        return eat(']');
      }
    }
    if (*p == '"') {
      std::string s;
      return string(&s);
    }
    if (*p == 't') return literal("true");
    if (*p == 'f') return literal("false");
    if (*p == 'n') return literal("null");
    double v = 0;
    if (!number(&v)) return false;
    if (is_number) *is_number = true;
    if (number_out) *number_out = v;
    return true;
  }
};

static bool offset_ok(double v, uint64_t bytes, uint64_t binary_bytes, uint64_t* out) {
  if (!(v >= 0) || v != std::floor(v) || v > 4294967295.0) return false;
  const uint64_t o = (uint64_t)v;
  if (o > binary_bytes || bytes > binary_bytes - o) return false;
  *out = o;
  return true;
}

// Every check of a .pnts file, on the first head_bytes bytes of a file of file_bytes bytes: head_bytes reaches at least to
// the end of the feature-table JSON wherever the header's lengths add up to file_bytes (the whole file, or what pnts_read_head
// read of it).  Nothing outside [head, head + head_bytes) is read.  What is wrong goes to *why; no context: reader threads
// call this.
static int pnts_parse_bytes(const unsigned char* head, uint64_t head_bytes, uint64_t file_bytes, PntsImage* f, std::string* why) {
  auto refuse = [&](const char* what) {
    *why = what;
    return (int)SWZ_ERR_BAD_ARG;
  };
  *f = PntsImage{};
  if (file_bytes < 28 || head_bytes < 28) return refuse("shorter than a .pnts header");
  if (memcmp(head, "pnts", 4) != 0) return refuse("not a .pnts file (magic)");
  uint32_t h[6];
  memcpy(h, head + 4, 24);
  if (h[0] != 1u) return refuse("unknown .pnts version");
  const uint64_t json_bytes = h[2], binary_bytes = h[3];
  if ((uint64_t)h[1] != file_bytes || 28ull + json_bytes + binary_bytes + h[4] + h[5] != (uint64_t)h[1])
    return refuse("the lengths of the header do not add up to the file");
  if (head_bytes < 28 + json_bytes) return refuse("the feature-table JSON was not read to its end");
  const uint64_t binary_at = 28 + json_bytes;
  JsonCursor js{reinterpret_cast<const char*>(head) + 28, reinterpret_cast<const char*>(head) + 28 + json_bytes};
  bool have_count = false, have_pos = false, have_rgb = false, have_int = false;
  double o_pos = 0, o_rgb = 0, o_int = 0;
  bool ok = js.eat('{');
  if (ok && !js.eat('}')) {
    for (;;) {
      std::string key;
      if (!js.string(&key) || !js.eat(':')) {
        ok = false;
        break;
      }
      std::vector<double> nums;
      double off = std::nan(""), num = 0;  // (an array's member that carries no byteOffset cannot be found)
      bool is_num = false;
      if (!js.value(0, &nums, &off, &is_num, &num)) {
        ok = false;
        break;
      }
      if (key == "POINTS_LENGTH") {
        if (!is_num || !(num >= 0) || num != std::floor(num) || num > 4294967295.0) {
          ok = false;
          break;
        }
        f->count = (uint64_t)num;
        have_count = true;
      } else if (key == "RTC_CENTER" && nums.size() == 3) {
        for (int k = 0; k < 3; ++k) f->rtc[k] = nums[k];
      } else if (key == "POSITION" || key == "RGB" || key == "INTENSITY") {
        if (std::isnan(off)) {
          ok = false;
          break;
        }
        if (key == "POSITION") {
          o_pos = off;
          have_pos = true;
        } else if (key == "RGB") {
          o_rgb = off;
          have_rgb = true;
        } else {
          o_int = off;
          have_int = true;
        }
      }
      if (js.eat(',')) continue;
      ok = js.eat('}');
      break;
    }
  }
  if (ok) {
    js.ws();
    ok = js.p == js.end;  // only the padding may follow
  }
  if (!ok || !have_count) return refuse("cannot read the feature-table JSON");
  if (!have_pos) return refuse("the feature table has no POSITION array (POSITION_QUANTIZED is not read)");
  if (!offset_ok(o_pos, 12 * f->count, binary_bytes, &f->position) ||
      (have_rgb && !offset_ok(o_rgb, 3 * f->count, binary_bytes, &f->rgb)) ||
      (have_int && !offset_ok(o_int, 2 * f->count, binary_bytes, &f->intensity)))
    return refuse("an attribute array passes the end of the binary");
  f->position += binary_at;  // from the first byte of the file on
  if (have_rgb) f->rgb += binary_at;
  if (have_int) f->intensity += binary_at;
  f->mask = (have_rgb ? SWZ_PNTS_RGB : 0u) | (have_int ? SWZ_PNTS_INTENSITY : 0u);
  f->file_bytes = file_bytes;
  return SWZ_OK;
}

int pnts_parse_image(const unsigned char* file, uint64_t file_bytes, PntsImage* out, std::string* why) {
  return pnts_parse_bytes(file, file_bytes, file_bytes, out, why);
}

// the header and the feature-table JSON of a file, not its arrays; *why names the file
int pnts_read_head(const char* path, PntsImage* out, std::string* why) {
  Fd f;
  f.fd = open(path, O_RDONLY | O_CLOEXEC);
  struct stat sb;
  if (f.fd < 0 || fstat(f.fd, &sb) != 0) {
    *why = std::string("cannot open ") + path;
    return SWZ_ERR_BAD_ARG;
  }
  const uint64_t file_bytes = (uint64_t)sb.st_size;
  std::vector<unsigned char> head((size_t)std::min<uint64_t>(file_bytes, 28));
  uint32_t json_bytes = 0;
  bool ok = pread_all(f.fd, head.data(), head.size(), 0);
  if (ok && head.size() == 28) {
    memcpy(&json_bytes, head.data() + 12, 4);
    head.resize((size_t)std::min<uint64_t>(file_bytes, 28ull + json_bytes));
    ok = pread_all(f.fd, head.data() + 28, head.size() - 28, 28);
  }
  if (!ok) {
    *why = std::string("cannot read the header of ") + path;
    return SWZ_ERR_BAD_ARG;
  }
  const int st = pnts_parse_bytes(head.data(), head.size(), file_bytes, out, why);
  if (st != SWZ_OK) *why += std::string(" in ") + path;
  return st;
}

// the whole file and where its arrays are
static int pnts_parse(swz_ctx* c, const char* path, std::vector<unsigned char>* data, PntsImage* f) {
  SWZ_TRY(read_whole_file(c, path, data));
  std::string why;
  const int st = pnts_parse_bytes(data->data(), data->size(), data->size(), f, &why);
  return st == SWZ_OK ? SWZ_OK : fail(c, st, why + " in " + path);
}

// ---------------------------------------------------------------------------------- tileset JSON
// the axis-aligned box of an entry: boundingBoxFromAABB (Tileset.cpp:94-118): centre = min + extent / 2 (AABB.h:70) and the
// FULL extent on the diagonal; a `tight` entry the half extent
static void put_box(std::string& s, const swz_tileset_node& t) {
  double e[3];
  for (int k = 0; k < 3; ++k) {
    e[k] = t.bounds_max[k] - t.bounds_min[k];
    put_number(s, t.bounds_min[k] + e[k] / 2);
    s += ",";
  }
  if (t.tight) {
    // OURS (swz_tileset_build_boxes): the HALF extent, as the 3D Tiles specification defines the box -- the largest of the
    // centre's distances to the two faces (the centre is rounded), then ulp by ulp until centre -/+ half, evaluated in
    // double like a reader does, encloses the bounds: rounding is monotonic, so a half that is large enough as a real is
    for (int k = 0; k < 3; ++k) {
      const double centre = t.bounds_min[k] + e[k] / 2;
      e[k] = std::max(e[k] / 2, std::max(centre - t.bounds_min[k], t.bounds_max[k] - centre));
      for (int step = 0; step < 8 && (centre - e[k] > t.bounds_min[k] || centre + e[k] < t.bounds_max[k]); ++step)
        e[k] = std::nextafter(e[k], std::numeric_limits<double>::infinity());
    }
  }
  for (int k = 0; k < 9; ++k) {
    put_number(s, k % 4 == 0 ? e[k / 4] : 0.0);
    if (k < 8) s += ",";
  }
}

// obb (may be null; swz_tileset_write_oriented): 12 numbers per entry, written as they are for every entry that is not `tight`
static void put_tile(std::string& s, const swz_tileset_node* nodes, const double* obb, uint64_t i, uint32_t remaining_levels) {
  const swz_tileset_node& t = nodes[i];
  char name[24];
  (void)swz_node_name(t.level, t.key, name);
  s += "{\"boundingVolume\":{\"box\":[";
  if (obb && !t.tight) {
    for (int k = 0; k < 12; ++k) {
      put_number(s, obb[12 * i + k]);
      if (k < 11) s += ",";
    }
  } else {
    put_box(s, t);
  }
  s += "]},\"geometricError\":";
  put_number(s, t.geometric_error);
  // write_tileset (TileSetWriter.cpp:42-79): at the bottom of a file the entry refers to the next file and has no children
  s += std::string(",\"refine\":\"ADD\",\"content\":{\"uri\":\"") + name + (remaining_levels == 0 ? ".json" : ".pnts") + "\"}";
  if (t.num_children && remaining_levels) {
    s += ",\"children\":[";
    for (uint32_t k = 0; k < t.num_children; ++k) {
      if (k) s += ",";
      put_tile(s, nodes, obb, (uint64_t)t.first_child + k, remaining_levels - 1);
    }
    s += "]";
  }
  s += "}";
}

}  // namespace swz

using namespace swz;

extern "C" {

uint8_t swz_pnts_rgb_from_intensity(int mapping, uint16_t intensity) {
  if (mapping != SWZ_PNTS_RGB_FROM_INTENSITY_LINEAR && mapping != SWZ_PNTS_RGB_FROM_INTENSITY_LOG) return 0;
  return grey_table(mapping)[intensity];
}

int swz_pnts_layout(uint64_t num_nodes, const uint64_t* node_count, uint32_t mask, int rgb_mapping, uint64_t* body_offset_out,
                    uint64_t* body_size_out, uint64_t* rgb_offset_out, uint64_t* intensity_offset_out, uint64_t* total_out) {
  if ((num_nodes && !node_count) || !mask_ok(mask) || !mapping_ok(rgb_mapping)) return SWZ_ERR_BAD_ARG;
  uint64_t at = 0;
  for (uint64_t k = 0; k < num_nodes; ++k) {
    if (node_count[k] > PNTS_MAX_BODY / 17) return SWZ_ERR_BAD_ARG;  // a file's byteLength is a u32
    const PntsBody<uint64_t> b = pnts_body<uint64_t>(node_count[k], mask);
    if (b.size > PNTS_MAX_BODY) return SWZ_ERR_BAD_ARG;
    if (body_offset_out) body_offset_out[k] = at;
    if (body_size_out) body_size_out[k] = b.size;
    if (rgb_offset_out) rgb_offset_out[k] = b.rgb;
    if (intensity_offset_out) intensity_offset_out[k] = b.intensity;
    at += b.size;
  }
  if (total_out) *total_out = at;
  return SWZ_OK;
}

// swz_pnts_pack_device (node_origin null) and swz_pnts_pack_origin_device: the checks, the table and the launch
static int pnts_pack(swz_ctx* c, const char* who, const uint32_t* d_perm, const uint32_t* d_order, uint64_t n, const double* d_xyz,
                     const swz_attribute_columns* d_in, uint64_t num_nodes, const uint64_t* node_offset, const uint64_t* node_count,
                     uint32_t mask, int rgb_mapping, void* d_image_out, uint64_t image_bytes, const double* node_origin) {
  // everything is checked on the host before anything is launched
  if (n > PNTS_MAX_POINTS) return c->fail(SWZ_ERR_BAD_ARG, std::string(who) + ": more than 2^32-65536 rows");
  SWZ_TRY(check_columns(c, who, d_in, mask, rgb_mapping));
  if (num_nodes && (!node_offset || !node_count)) return c->fail(SWZ_ERR_BAD_ARG, std::string(who) + ": NULL node table");
  const PackNames names{who, "swz_pnts_layout", "pnts_nodes"};
  PackTable<PntsNode> table;
  std::vector<double> origins;  // of the nodes that hold points, in the table's order
  SWZ_TRY(pack_build_table(
    c, names, n, num_nodes, node_offset, node_count,
    [&](uint64_t k, PntsNode*) -> const char* {
      if (!node_origin || node_count[k] == 0) return nullptr;
      if (!finite3(node_origin + 3 * k)) return "the origin of a node that holds points is not finite";
      origins.insert(origins.end(), node_origin + 3 * k, node_origin + 3 * k + 3);
      return nullptr;
    },
    [&](uint64_t cnt, uint64_t* bytes) -> const char* {
      if (cnt > PNTS_MAX_BODY / 17) return "a node too large for a .pnts file";
      *bytes = pnts_body<uint64_t>(cnt, mask).size;
      return nullptr;
    },
    &table));
  const uint64_t at = table.image_bytes, prev_end = table.prev_end;

  PntsPackArgs a{};
  SWZ_TRY(pack_upload_table(c, names, table, d_perm, d_xyz, d_image_out, image_bytes, &a.nodes));
  if (!a.nodes) return SWZ_OK;
  a.perm = d_perm;
  a.order = d_order;
  a.n = (uint32_t)n;
  a.xyz = d_xyz;
  a.rgb = static_cast<const uint8_t*>(d_in ? d_in->column[SWZ_ATTR_RGB] : nullptr);
  a.intensity = static_cast<const uint16_t*>(d_in ? d_in->column[SWZ_ATTR_INTENSITY] : nullptr);
  a.mask = mask;
  a.image = static_cast<uint8_t*>(d_image_out);
  a.num_nodes = (uint32_t)table.nodes.size();
  if ((mask & SWZ_PNTS_RGB) && rgb_mapping != SWZ_PNTS_RGB_FROM_COLOR) {
    // (64 KiB per call: the workspace may have been released since the last one)
    uint8_t* d_grey = nullptr;
    SWZ_TRY(c->get("pnts_grey", (size_t)65536, &d_grey));
    SWZ_HIP(c, hipMemcpyAsync(d_grey, grey_table(rgb_mapping), 65536, hipMemcpyHostToDevice, c->stream));
    a.grey = d_grey;
  }
  if (node_origin) {
    double* d_origin = nullptr;
    SWZ_TRY(c->get("pnts_origins", origins.size(), &d_origin));
    SWZ_HIP(c, hipMemcpyAsync(d_origin, origins.data(), origins.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
    a.origin = d_origin;
  }
  {
    const uint64_t row = 24 + ((mask & SWZ_PNTS_RGB) ? 3 : 0) + ((mask & SWZ_PNTS_INTENSITY) || a.grey ? 2 : 0);
    ProfScope ps(c, "pnts_pack", n * (d_order ? 8 : 4) + prev_end * row + at, 1);
    // rows behind the last node belong to no body: the grid ends with it
    if (node_origin) hipLaunchKernelGGL(pnts_pack_kernel<true>, dim3(div_up(prev_end, PNTS_TILE)), dim3(PNTS_TILE), 0, c->stream, a);
    else hipLaunchKernelGGL(pnts_pack_kernel<false>, dim3(div_up(prev_end, PNTS_TILE)), dim3(PNTS_TILE), 0, c->stream, a);
    SWZ_LAUNCH_CHECK(c);
  }
  SWZ_HIP(c, hipStreamSynchronize(c->stream));
  return SWZ_OK;
}

int swz_pnts_pack_device(swz_ctx* c, const uint32_t* d_perm, const uint32_t* d_order, uint64_t n, const double* d_xyz,
                         const swz_attribute_columns* d_in, uint64_t num_nodes, const uint64_t* node_offset,
                         const uint64_t* node_count, uint32_t mask, int rgb_mapping, void* d_image_out, uint64_t image_bytes) {
  if (!c) return SWZ_ERR_BAD_ARG;
  return pnts_pack(c, "swz_pnts_pack_device", d_perm, d_order, n, d_xyz, d_in, num_nodes, node_offset, node_count, mask, rgb_mapping,
                   d_image_out, image_bytes, nullptr);
}

int swz_pnts_pack_origin_device(swz_ctx* c, const uint32_t* d_perm, const uint32_t* d_order, uint64_t n, const double* d_xyz,
                                const swz_attribute_columns* d_in, uint64_t num_nodes, const uint64_t* node_offset,
                                const uint64_t* node_count, uint32_t mask, int rgb_mapping, void* d_image_out, uint64_t image_bytes,
                                const double* node_origin) {
  if (!c) return SWZ_ERR_BAD_ARG;
  if (num_nodes && !node_origin) return c->fail(SWZ_ERR_BAD_ARG, "swz_pnts_pack_origin_device: NULL origins");
  static const double none[3] = {0, 0, 0};  // (no nodes: the instantiation is chosen by the pointer, nothing is read)
  return pnts_pack(c, "swz_pnts_pack_origin_device", d_perm, d_order, n, d_xyz, d_in, num_nodes, node_offset, node_count, mask,
                   rgb_mapping, d_image_out, image_bytes, node_origin ? node_origin : none);
}

int swz_pnts_write_node(swz_ctx* c, const char* path, uint64_t count, const void* body, uint64_t body_bytes, uint32_t mask,
                        const double rtc_center[3]) {
  if (!path) return fail(c, SWZ_ERR_BAD_ARG, "swz_pnts_write_node: NULL path");
  if (!mask_ok(mask)) return fail(c, SWZ_ERR_BAD_ARG, "swz_pnts_write_node: the mask names an attribute a .pnts file does not hold");
  if (count == 0) return SWZ_OK;  // like swz_bin_write_node: an empty node has no file
  if (!body) return fail(c, SWZ_ERR_BAD_ARG, "swz_pnts_write_node: NULL body");
  if (rtc_center && !finite3(rtc_center)) return fail(c, SWZ_ERR_BAD_ARG, "swz_pnts_write_node: RTC_CENTER is not finite");
  if (count > PNTS_MAX_BODY / 17 || pnts_body<uint64_t>(count, mask).size != body_bytes)
    return fail(c, SWZ_ERR_BAD_ARG, "swz_pnts_write_node: the body does not have the size swz_pnts_layout gives this count");
  std::string err;
  const int st = pnts_write_file(path, count, body, body_bytes, mask, rtc_center, &err);
  return st == SWZ_OK ? SWZ_OK : fail(c, st, err);
}

int swz_pnts_write_node_rows(swz_ctx* c, const char* path, uint64_t count, const double* xyz, const swz_attribute_columns* columns,
                             uint32_t mask, int rgb_mapping, const double rtc_center[3]) {
  if (!path) return fail(c, SWZ_ERR_BAD_ARG, "swz_pnts_write_node_rows: NULL path");
  SWZ_TRY(check_columns(c, "swz_pnts_write_node_rows", columns, mask, rgb_mapping));
  if (count == 0) return SWZ_OK;
  if (!xyz) return fail(c, SWZ_ERR_BAD_ARG, "swz_pnts_write_node_rows: NULL positions");
  if (rtc_center && !finite3(rtc_center)) return fail(c, SWZ_ERR_BAD_ARG, "swz_pnts_write_node_rows: RTC_CENTER is not finite");
  if (count > PNTS_MAX_BODY / 17) return fail(c, SWZ_ERR_BAD_ARG, "swz_pnts_write_node_rows: a node too large for a .pnts file");
  const PntsBody<uint64_t> b = pnts_body<uint64_t>(count, mask);
  std::vector<unsigned char> body((size_t)b.size, 0);
  float* pos = reinterpret_cast<float*>(body.data());
  for (uint64_t i = 0; i < 3 * count; ++i) pos[i] = static_cast<float>(xyz[i]);  // PNTSWriter narrows with static_cast<float>
  const uint16_t* in = columns ? static_cast<const uint16_t*>(columns->column[SWZ_ATTR_INTENSITY]) : nullptr;
  if (mask & SWZ_PNTS_RGB) {
    unsigned char* out = body.data() + b.rgb;
    if (rgb_mapping == SWZ_PNTS_RGB_FROM_COLOR) {
      memcpy(out, columns->column[SWZ_ATTR_RGB], (size_t)(3 * count));
    } else {
      const uint8_t* grey = grey_table(rgb_mapping);
      for (uint64_t i = 0; i < count; ++i) out[3 * i] = out[3 * i + 1] = out[3 * i + 2] = grey[in[i]];
    }
  }
  if (mask & SWZ_PNTS_INTENSITY) memcpy(body.data() + b.intensity, in, (size_t)(2 * count));
  std::string err;
  const int st = pnts_write_file(path, count, body.data(), b.size, mask, rtc_center, &err);
  return st == SWZ_OK ? SWZ_OK : fail(c, st, err);
}

// swz_pnts_persist_nodes (one centre, may be null) and swz_pnts_persist_nodes_rtc (node_rtc: 3 per node)
static int pnts_persist(swz_ctx* c, const std::string& who, const char* dir, uint64_t num_nodes, const int8_t* node_level,
                        const uint64_t* node_key, const uint64_t* node_count, const void* image, uint64_t image_bytes, uint32_t mask,
                        const double* rtc_center, const double* node_rtc) {
  if (!dir || (num_nodes && (!node_level || !node_key || !node_count))) return fail(c, SWZ_ERR_BAD_ARG, who + ": NULL argument");
  if (!mask_ok(mask)) return fail(c, SWZ_ERR_BAD_ARG, who + ": the mask names an attribute a .pnts file does not hold");
  if (rtc_center && !finite3(rtc_center)) return fail(c, SWZ_ERR_BAD_ARG, who + ": RTC_CENTER is not finite");
  for (uint64_t k = 0; node_rtc && k < num_nodes; ++k)
    if (node_count[k] && !finite3(node_rtc + 3 * k)) return fail(c, SWZ_ERR_BAD_ARG, who + ": the RTC_CENTER of a node that holds points is not finite");
  std::vector<uint64_t> at(num_nodes), size(num_nodes);
  uint64_t total = 0;
  if (swz_pnts_layout(num_nodes, node_count, mask, SWZ_PNTS_RGB_FROM_COLOR, at.data(), size.data(), nullptr, nullptr, &total) != SWZ_OK)
    return fail(c, SWZ_ERR_BAD_ARG, who + ": a node too large for a .pnts file");
  if (total > image_bytes || (total && !image)) return fail(c, SWZ_ERR_BAD_ARG, who + ": the image is smaller than the table's layout");
  for (uint64_t k = 0; k < num_nodes; ++k) {
    char name[24];
    if (swz_node_name(node_level[k], node_key[k], name) != SWZ_OK) return fail(c, SWZ_ERR_BAD_ARG, "bad node level");
  }
  std::string first_err;
  const int st = run_tickets(c, num_nodes, [&](uint64_t k, std::string* err) {
    if (node_count[k] == 0) return (int)SWZ_OK;
    char name[24];
    (void)swz_node_name(node_level[k], node_key[k], name);
    const std::string path = std::string(dir) + "/" + name + ".pnts";
    return pnts_write_file(path.c_str(), node_count[k], static_cast<const unsigned char*>(image) + at[k], size[k], mask,
                           node_rtc ? node_rtc + 3 * k : rtc_center, err);
  }, &first_err);
  return st == SWZ_OK ? SWZ_OK : fail(c, st, first_err);
}

int swz_pnts_persist_nodes(swz_ctx* c, const char* dir, uint64_t num_nodes, const int8_t* node_level, const uint64_t* node_key,
                           const uint64_t* node_count, const void* image, uint64_t image_bytes, uint32_t mask,
                           const double rtc_center[3]) {
  return pnts_persist(c, "swz_pnts_persist_nodes", dir, num_nodes, node_level, node_key, node_count, image, image_bytes, mask, rtc_center,
                      nullptr);
}

int swz_pnts_persist_nodes_rtc(swz_ctx* c, const char* dir, uint64_t num_nodes, const int8_t* node_level, const uint64_t* node_key,
                               const uint64_t* node_count, const void* image, uint64_t image_bytes, uint32_t mask,
                               const double* node_rtc_center) {
  if (num_nodes && !node_rtc_center) return fail(c, SWZ_ERR_BAD_ARG, "swz_pnts_persist_nodes_rtc: NULL argument");
  static const double none[3] = {0, 0, 0};
  return pnts_persist(c, "swz_pnts_persist_nodes_rtc", dir, num_nodes, node_level, node_key, node_count, image, image_bytes, mask, nullptr,
                      node_rtc_center ? node_rtc_center : none);
}

int swz_pnts_read_header(swz_ctx* c, const char* path, uint64_t* count_out, uint32_t* mask_out, double rtc_center_out[3]) {
  if (!path || !count_out || !mask_out) return fail(c, SWZ_ERR_BAD_ARG, "swz_pnts_read_header: NULL argument");
  PntsImage f;
  std::string why;
  const int st = pnts_read_head(path, &f, &why);
  if (st != SWZ_OK) return fail(c, st, why);
  *count_out = f.count;
  *mask_out = f.mask;
  if (rtc_center_out)
    for (int k = 0; k < 3; ++k) rtc_center_out[k] = f.rtc[k];
  return SWZ_OK;
}

int swz_pnts_parse_image(swz_ctx* c, const void* file, uint64_t file_bytes, uint64_t* count_out, uint32_t* mask_out,
                         double rtc_center_out[3], uint64_t* position_offset_out, uint64_t* rgb_offset_out,
                         uint64_t* intensity_offset_out) {
  if (!file && file_bytes) return fail(c, SWZ_ERR_BAD_ARG, "swz_pnts_parse_image: NULL image");
  PntsImage f;
  std::string why;
  const int st = pnts_parse_image(static_cast<const unsigned char*>(file), file_bytes, &f, &why);
  if (st != SWZ_OK) return fail(c, st, "swz_pnts_parse_image: " + why);
  if (count_out) *count_out = f.count;
  if (mask_out) *mask_out = f.mask;
  if (rtc_center_out)
    for (int k = 0; k < 3; ++k) rtc_center_out[k] = f.rtc[k];
  if (position_offset_out) *position_offset_out = f.position;
  if (rgb_offset_out) *rgb_offset_out = f.rgb;
  if (intensity_offset_out) *intensity_offset_out = f.intensity;
  return SWZ_OK;
}

int swz_pnts_read_node(swz_ctx* c, const char* path, double* xyz_out, const swz_attribute_columns* columns_out) {
  if (!path) return fail(c, SWZ_ERR_BAD_ARG, "swz_pnts_read_node: NULL path");
  std::vector<unsigned char> data;
  PntsImage f;
  SWZ_TRY(pnts_parse(c, path, &data, &f));
  const unsigned char* file = data.data();
  if (xyz_out) {
    for (uint64_t i = 0; i < 3 * f.count; ++i) {
      float v;
      memcpy(&v, file + f.position + 4 * i, 4);
      xyz_out[i] = v;  // the format is lossy: the stored float, widened
    }
  }
  if (columns_out && columns_out->column[SWZ_ATTR_RGB] && (f.mask & SWZ_PNTS_RGB))
    memcpy(columns_out->column[SWZ_ATTR_RGB], file + f.rgb, (size_t)(3 * f.count));
  if (columns_out && columns_out->column[SWZ_ATTR_INTENSITY] && (f.mask & SWZ_PNTS_INTENSITY))
    memcpy(columns_out->column[SWZ_ATTR_INTENSITY], file + f.intensity, (size_t)(2 * f.count));
  return SWZ_OK;
}

int swz_tileset_build_boxes(uint64_t num_nodes, const int8_t* node_level, const uint64_t* node_key, const double* node_box_min,
                            const double* node_box_max, const double root_min[3], const double root_max[3], float spacing_at_root,
                            const double global_offset[3], uint64_t max_out, swz_tileset_node* out, uint64_t* num_out) {
  if (num_nodes && (!node_box_min || !node_box_max)) return SWZ_ERR_BAD_ARG;
  SWZ_TRY(swz_tileset_build(num_nodes, node_level, node_key, root_min, root_max, spacing_at_root, global_offset, max_out, out, num_out));
  if (!out) return SWZ_OK;
  const uint64_t num = *num_out;
  // the table's node of an entry: both are ordered by (level, key), the entries hold the table's nodes and their ancestors
  std::map<std::pair<int, uint64_t>, uint64_t> row;
  for (uint64_t j = 0; j < num_nodes; ++j) {
    const int lv = node_level[j];
    row[{lv, lv < 0 ? 0ull : ((node_key[j] >> level_shift(lv)) << level_shift(lv))}] = j;
  }
  const double inf = std::numeric_limits<double>::infinity();
  std::vector<double> lo(3 * num, inf), hi(3 * num, -inf);
  // one pass from the back: children lie behind their parent, so an entry is complete when it is reached
  for (uint64_t i = num; i-- > 0;) {
    swz_tileset_node& t = out[i];
    if (t.has_content) {
      const uint64_t j = row[{(int)t.level, t.key}];
      for (int ax = 0; ax < 3; ++ax) {
        if (!(node_box_min[3 * j + ax] <= node_box_max[3 * j + ax])) continue;  // a node without points
        const double off = global_offset ? global_offset[ax] : 0.0;
        lo[3 * i + ax] = std::min(lo[3 * i + ax], node_box_min[3 * j + ax] + off);
        hi[3 * i + ax] = std::max(hi[3 * i + ax], node_box_max[3 * j + ax] + off);
      }
    }
    if (lo[3 * i] <= hi[3 * i] && lo[3 * i + 1] <= hi[3 * i + 1] && lo[3 * i + 2] <= hi[3 * i + 2]) {
      t.tight = 1;
      for (int ax = 0; ax < 3; ++ax) {
        t.bounds_min[ax] = lo[3 * i + ax];
        t.bounds_max[ax] = hi[3 * i + ax];
      }
    }
    if (t.parent >= 0) {
      for (int ax = 0; ax < 3; ++ax) {
        lo[3 * t.parent + ax] = std::min(lo[3 * t.parent + ax], lo[3 * i + ax]);
        hi[3 * t.parent + ax] = std::max(hi[3 * t.parent + ax], hi[3 * i + ax]);
      }
    }
  }
  return SWZ_OK;
}

// swz_tileset_write (obb null) and swz_tileset_write_oriented
static int tileset_write(swz_ctx* c, const std::string& who, const swz_tileset_node* nodes, uint64_t num, const double* obb,
                         const char* dir) {
  if (!dir || (num && !nodes)) return fail(c, SWZ_ERR_BAD_ARG, who + ": NULL argument");
  // the array must be what swz_tileset_build hands out: children behind their parent, inside the array, one level down
  for (uint64_t i = 0; i < num; ++i) {
    const swz_tileset_node& t = nodes[i];
    bool ok = t.level >= -1 && t.level <= 20;
    if (ok && t.num_children)
      ok = t.first_child > (int64_t)i && (uint64_t)t.first_child < num && t.num_children <= num - (uint64_t)t.first_child;
    for (uint32_t k = 0; ok && k < t.num_children; ++k) ok = nodes[t.first_child + k].level == t.level + 1;
    if (!ok || !std::isfinite(t.geometric_error) || !finite3(t.bounds_min) || !finite3(t.bounds_max))
      return fail(c, SWZ_ERR_BAD_ARG, who + ": not a tileset tree of swz_tileset_build");
    for (int k = 0; obb && !t.tight && k < 12; ++k)
      if (!std::isfinite(obb[12 * i + k])) return fail(c, SWZ_ERR_BAD_ARG, who + ": an oriented box is not finite");
  }
  std::vector<uint64_t> roots;
  for (uint64_t i = 0; i < num; ++i)
    if (nodes[i].is_tileset_root) roots.push_back(i);
  std::string first_err;
  const int st = run_tickets(c, roots.size(), [&](uint64_t k, std::string* err) {
    const swz_tileset_node& t = nodes[roots[k]];
    // writeTilesetJSON (TileSetWriter.cpp:81-210) with MAX_DEPTH + 1 = 3 levels below the file's root
    std::string s = "{\"asset\":{\"version\":\"0.0\"},\"geometricError\":";
    put_number(s, t.geometric_error);
    s += ",\"root\":";
    put_tile(s, nodes, obb, roots[k], 3);
    s += "}";
    char name[24];
    (void)swz_node_name(t.level, t.key, name);
    const std::string path = std::string(dir) + "/" + name + ".json";
    return write_file(path, {{s.data(), s.size()}}, err);
  }, &first_err);
  return st == SWZ_OK ? SWZ_OK : fail(c, st, first_err);
}

int swz_tileset_write(swz_ctx* c, const swz_tileset_node* nodes, uint64_t num, const char* dir) {
  return tileset_write(c, "swz_tileset_write", nodes, num, nullptr, dir);
}

int swz_tileset_write_oriented(swz_ctx* c, const swz_tileset_node* nodes, uint64_t num, const double* obb, const char* dir) {
  if (num && !obb) return fail(c, SWZ_ERR_BAD_ARG, "swz_tileset_write_oriented: NULL argument");
  static const double none[12] = {0};
  return tileset_write(c, "swz_tileset_write_oriented", nodes, num, obb ? obb : none, dir);
}

int swz_tileset_oriented_boxes(const swz_srs* srs, const swz_tileset_node* nodes, uint64_t num, double* obb_out) {
  if ((srs && !srs_valid(srs)) || (num && (!nodes || !obb_out))) return SWZ_ERR_BAD_ARG;
  for (uint64_t i = 0; i < num; ++i) {
    const swz_tileset_node& t = nodes[i];
    // boundingBoxFromAABB(aabb, transform) (Tileset.cpp:52-92): the centre (min + extent / 2, AABB.h:70) and the centres of
    // the three upper faces
    double c3[3];
    for (int k = 0; k < 3; ++k) c3[k] = t.bounds_min[k] + (t.bounds_max[k] - t.bounds_min[k]) / 2;
    double p[12] = {c3[0], c3[1], c3[2], t.bounds_max[0], c3[1], c3[2], c3[0], t.bounds_max[1], c3[2], c3[0], c3[1], t.bounds_max[2]};
    if (srs) (void)swz_srs_transform(srs, SWZ_SRS_ECEF, p, 4);
    double* out = obb_out + 12 * i;
    for (int k = 0; k < 3; ++k) out[k] = p[k];
    for (int v = 1; v < 4; ++v)
      for (int k = 0; k < 3; ++k) out[3 * v + k] = p[3 * v + k] - p[k];
  }
  return SWZ_OK;
}

}  // extern "C"
