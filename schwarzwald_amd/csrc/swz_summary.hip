// swz_summary.hip -- per-node attribute summaries: what every scalar column of a node holds, reduced on the device
// (swz_node_summaries_device), the sidecar file node-summaries.swz that keeps the result beside a written data set
// (swz_dataset_summaries_write / _read), so that a filtered query can skip the node files no row of which can pass, and
// swz_dataset_summarize, which streams a data set chunk by chunk (SourceLoop::each_chunk, swz_source.hip), reduces every chunk
// and writes that file.
//
// The rows are in stored order (a chunk's columns as the unpack kernels leave them), so the rows of a node are neighbours.  One
// block takes SUM_TILE consecutive rows, one per thread, and finds their nodes with the window helpers of swz_nodepack.h.  The
// columns are handled one after the other, an element per lane, so the LDS window holds ONE column's partial result per window
// entry, four 64-bit words: the 256-bit set of a one-byte column; min and max of a uint16 column as two 32-bit words; min and
// max of the GPS times as order-preserving codes (swz_nodebox.h) and a flag word for NaN, which stays out of min and max.  A
// wave combines the runs of lanes of one node with shuffles, the first lane of every run combines into its entry in LDS, and
// each window entry that has rows in the tile leaves with one round of atomics on the table in global memory: 64-bit OR for
// the set words that are not 0, 32-bit min / max, 64-bit min / max on the codes.  A small kernel presets the table; OR, min
// and max are idempotent and commute, so neither the workspace's old bytes nor the order of the atomics shows.
#include <cstddef>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "swz_internal.h"
#include "swz_convert.h"
#include "swz_device.h"
#include "swz_hostio.h"
#include "swz_nodebox.h"
#include "swz_nodepack.h"
#include "swz_select.h"
#include "swz_summary.h"

static_assert(sizeof(swz_attr_summary) == 56 && offsetof(swz_attr_summary, set) == 16 && offsetof(swz_attr_summary, flags) == 48,
              "an entry as include/swz_gpu.h and the sidecar lay it out");
static_assert(SWZ_SUMMARY_SCALARS == (((1u << SWZ_ATTR_COUNT) - 1u) & ~((1u << SWZ_ATTR_RGB) | (1u << SWZ_ATTR_NORMAL))), "the scalar columns");

namespace swz {

constexpr int SUM_TILE = 256;  // stored rows per block, one per thread
enum { SUM_BYTE = 0, SUM_U16 = 1, SUM_F64 = 2 };
constexpr uint64_t SUM_U16_PRESET = 0x00000000FFFFFFFFull;  // low word: the minimum, from 2^32 - 1; high word: the maximum, from 0

struct SumArgs {
  const void* col[SUMMARY_MAX_COLS];  // the summarised columns, by ascending SWZ_ATTR_*
  uint8_t kind[SUMMARY_MAX_COLS + 2];
  uint32_t cols;
  uint32_t n;  // one past the last row of the last node
  const BoxNode* nodes;
  uint32_t num_nodes;
  uint64_t* table;  // per listed node and column four words (BoxNode::base: 32 x cols x its place)
};

__host__ __device__ inline uint64_t sum_preset_word(uint32_t kind, uint32_t w) {
  if (kind == SUM_U16) return w == 0 ? SUM_U16_PRESET : 0;
  if (kind == SUM_F64) return w == 0 ? BOX_CODE_POS_INF : w == 1 ? BOX_CODE_NEG_INF : 0;
  return 0;
}

__global__ void node_summaries_preset_kernel(SumArgs a, uint32_t words) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < words) a.table[i] = sum_preset_word(a.kind[(i / 4u) % a.cols], i % 4u);
}

__global__ __launch_bounds__(SUM_TILE) void node_summaries_kernel(SumArgs a) {
  __shared__ uint32_t s_start[SUM_TILE];
  __shared__ uint32_t s_count[SUM_TILE];
  __shared__ unsigned long long s_part[SUM_TILE * 4];  // window entry e: words 4e .. 4e + 3 of the column in hand
  const uint32_t t = threadIdx.x;
  const uint32_t lane = t & 63u;
  const uint32_t r0 = blockIdx.x * (uint32_t)SUM_TILE;
  const uint32_t r1 = (uint32_t)min((uint64_t)r0 + SUM_TILE, (uint64_t)a.n);

  const uint32_t k0 = pack_first_node(a.nodes, a.num_nodes, r0);
  const BoxNode* listed = pack_fill_window(a.nodes, a.num_nodes, k0, r1, s_start, s_count);
  if (listed && (uint64_t)listed->start + listed->count <= r0) listed = nullptr;  // the first entry may end in front of the tile
  {
    const uint32_t kind0 = a.kind[0];
#pragma unroll
    for (uint32_t w = 0; w < 4; ++w) s_part[4 * t + w] = sum_preset_word(kind0, w);
  }
  __syncthreads();

  const uint32_t r = r0 + t;
  uint32_t e;
  const bool in_node = pack_row_node<SUM_TILE>(s_start, s_count, r, r1, &e);
  if (!in_node) e = BOX_NO_ENTRY;
  // the lanes of one entry are neighbours: bit i of `same` says that lane + 2^i is in this wave and in this lane's entry
  uint32_t same = 0;
#pragma unroll
  for (uint32_t i = 0; i < 6; ++i) {
    const uint32_t e_far = __shfl_down(e, 1u << i, 64);
    if (lane + (1u << i) < 64u && e_far == e) same |= 1u << i;
  }
  const uint32_t e_before = __shfl_up(e, 1u, 64);
  const bool run_first = in_node && (lane == 0u || e_before != e);  // one combine per wave and entry
  unsigned long long* const part = s_part + 4 * (in_node ? e : 0u);
  uint32_t* const part32 = reinterpret_cast<uint32_t*>(part);

  for (uint32_t j = 0; j < a.cols; ++j) {
    const uint32_t kind = a.kind[j];
    if (kind == SUM_BYTE) {
      const uint32_t v = in_node ? static_cast<const uint8_t*>(a.col[j])[r] : 0u;
      unsigned long long m[4];
#pragma unroll
      for (uint32_t w = 0; w < 4; ++w) m[w] = (in_node && (v >> 6) == w) ? 1ull << (v & 63u) : 0ull;
#pragma unroll
      for (uint32_t i = 0; i < 6; ++i) {
#pragma unroll
        for (uint32_t w = 0; w < 4; ++w) {
          const unsigned long long far = __shfl_down(m[w], 1u << i, 64);
          if ((same >> i) & 1u) m[w] |= far;
        }
      }
      if (run_first) {
#pragma unroll
        for (uint32_t w = 0; w < 4; ++w)
          if (m[w]) atomicOr(part + w, m[w]);
      }
    } else if (kind == SUM_U16) {
      uint32_t lo = 0xFFFFFFFFu, hi = 0u;
      if (in_node) lo = hi = static_cast<const uint16_t*>(a.col[j])[r];
#pragma unroll
      for (uint32_t i = 0; i < 6; ++i) {
        const uint32_t lo_far = __shfl_down(lo, 1u << i, 64);
        const uint32_t hi_far = __shfl_down(hi, 1u << i, 64);
        if ((same >> i) & 1u) {
          lo = min(lo, lo_far);
          hi = max(hi, hi_far);
        }
      }
      if (run_first) {
        atomicMin(part32, lo);
        atomicMax(part32 + 1, hi);
      }
    } else {
      unsigned long long lo = BOX_CODE_POS_INF, hi = BOX_CODE_NEG_INF;
      uint32_t nan = 0;
      if (in_node) {
        const double v = static_cast<const double*>(a.col[j])[r];
        if (v != v) nan = SWZ_SUMMARY_HAS_NAN;  // stays out of min and max: its code would sort behind +inf or in front of -inf
        else lo = hi = box_code(v);
      }
#pragma unroll
      for (uint32_t i = 0; i < 6; ++i) {
        const unsigned long long lo_far = __shfl_down(lo, 1u << i, 64);
        const unsigned long long hi_far = __shfl_down(hi, 1u << i, 64);
        const uint32_t nan_far = __shfl_down(nan, 1u << i, 64);
        if ((same >> i) & 1u) {
          lo = min(lo, lo_far);
          hi = max(hi, hi_far);
          nan |= nan_far;
        }
      }
      if (run_first) {
        if (lo != BOX_CODE_POS_INF || hi != BOX_CODE_NEG_INF) {  // (a run of NaN alone has neither)
          atomicMin(part, lo);
          atomicMax(part + 1, hi);
        }
        if (nan) atomicOr(part + 2, (unsigned long long)nan);
      }
    }
    __syncthreads();
    // window entry t: one round of atomics when the node has rows in this tile; then the entry is the next column's
    unsigned long long* const mine = s_part + 4 * t;
    if (listed) {
      unsigned long long* const out = reinterpret_cast<unsigned long long*>(a.table) + listed->base / 8 + 4ull * j;
      if (kind == SUM_BYTE) {
#pragma unroll
        for (uint32_t w = 0; w < 4; ++w)
          if (mine[w]) (void)__hip_atomic_fetch_or(out + w, mine[w], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      } else if (kind == SUM_U16) {
        uint32_t* const out32 = reinterpret_cast<uint32_t*>(out);
        (void)__hip_atomic_fetch_min(out32, (uint32_t)(mine[0] & 0xFFFFFFFFull), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        (void)__hip_atomic_fetch_max(out32 + 1, (uint32_t)(mine[0] >> 32), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      } else {
        if (mine[0] != BOX_CODE_POS_INF || mine[1] != BOX_CODE_NEG_INF) {
          (void)__hip_atomic_fetch_min(out, mine[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          (void)__hip_atomic_fetch_max(out + 1, mine[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        if (mine[2]) (void)__hip_atomic_fetch_or(out + 2, mine[2], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
    if (j + 1 < a.cols) {
      const uint32_t next = a.kind[j + 1];
#pragma unroll
      for (uint32_t w = 0; w < 4; ++w) mine[w] = sum_preset_word(next, w);
    }
    __syncthreads();
  }
}

static uint32_t summary_kind(int attribute) {
  return attribute == SWZ_ATTR_GPS_TIME ? SUM_F64 : ATTR_BYTES[attribute] == 2 ? SUM_U16 : SUM_BYTE;
}

// lo / hi of a one-byte column out of its set; the scan-angle rank reads the byte as signed
static void summary_byte_bounds(int attribute, swz_attr_summary* e) {
  const bool is_signed = attribute == SWZ_ATTR_SCAN_ANGLE_RANK;
  for (int b = 0; b < 256; ++b) {
    if (!((e->set[b >> 6] >> (b & 63)) & 1ull)) continue;
    const double v = is_signed ? (double)(int8_t)(uint8_t)b : (double)b;
    e->lo = std::min(e->lo, v);
    e->hi = std::max(e->hi, v);
  }
}

int node_summaries(swz_ctx* c, const char* who, uint64_t n, const swz_attribute_columns* d_in, uint32_t mask, uint64_t num_nodes,
                   const uint64_t* node_offset, const uint64_t* node_count, swz_attr_summary* out) {
  auto refuse = [&](const std::string& what) { return c->fail(SWZ_ERR_BAD_ARG, std::string(who) + ": " + what); };
  // everything is checked on the host before anything is launched
  if (n > BOX_MAX_POINTS) return refuse("more than 2^32-65536 rows");
  if (mask & ~((1u << SWZ_ATTR_COUNT) - 1u)) return refuse("a bit of the mask that names no attribute");
  for (int a : {SWZ_ATTR_RGB, SWZ_ATTR_NORMAL})
    if ((mask >> a) & 1u) return refuse(std::string(attribute_name(a)) + " is not a scalar column");
  SumArgs a{};
  int attr_of[SUMMARY_MAX_COLS];
  for (int at = 0; at < SWZ_ATTR_COUNT; ++at) {
    if (!((mask >> at) & 1u)) continue;
    const void* col = d_in ? d_in->column[at] : nullptr;
    if (n && !col) return refuse(std::string("the mask names ") + attribute_name(at) + ", which has no input column");
    if ((uintptr_t)col % ATTR_BYTES[at]) return refuse(std::string("the column of ") + attribute_name(at) + " is not aligned to its element");
    attr_of[a.cols] = at;
    a.col[a.cols] = col;
    a.kind[a.cols] = (uint8_t)summary_kind(at);
    ++a.cols;
  }
  const uint32_t cols = a.cols;
  if (num_nodes && (!node_offset || !node_count || (cols && !out))) return refuse("NULL node table");
  const PackNames names{who, who, "summary_nodes"};
  PackTable<BoxNode> table;
  SWZ_TRY(pack_build_table(
    c, names, n, num_nodes, node_offset, node_count, [](uint64_t, BoxNode*) -> const char* { return nullptr; },
    [cols](uint64_t, uint64_t* bytes) -> const char* {
      *bytes = 32ull * cols;
      return nullptr;
    },
    &table));
  const uint64_t listed = table.nodes.size(), prev_end = table.prev_end;
  for (uint64_t i = 0; i < num_nodes * cols; ++i) out[i] = summary_empty();  // a node without points, and every node when nothing is launched
  if (!listed || !cols) return SWZ_OK;
  const uint64_t words = listed * cols * 4;
  if (words > 0xFFFFFFFFull) return refuse("more than 2^32 words of summaries in one call");

  SWZ_HIP(c, hipSetDevice(c->device));
  uint64_t* d_table = nullptr;
  SWZ_TRY(c->get("summary_table", (size_t)words, &d_table));
  SWZ_TRY(pack_upload_table(c, names, table, d_table, d_table, d_table, words * 8, &a.nodes));
  if (!a.nodes) return SWZ_OK;
  a.n = (uint32_t)prev_end;
  a.num_nodes = (uint32_t)listed;
  a.table = d_table;
  {
    uint64_t row_bytes = 0;
    for (uint32_t j = 0; j < cols; ++j) row_bytes += ATTR_BYTES[attr_of[j]];
    ProfScope ps(c, "node_summaries", prev_end * row_bytes + listed * (sizeof(BoxNode) + 64ull * cols), 2);
    hipLaunchKernelGGL(node_summaries_preset_kernel, dim3(div_up(words, 256)), dim3(256), 0, c->stream, a, (uint32_t)words);
    SWZ_LAUNCH_CHECK(c);
    // rows behind the last node belong to no node: the grid ends with it
    hipLaunchKernelGGL(node_summaries_kernel, dim3(div_up(prev_end, SUM_TILE)), dim3(SUM_TILE), 0, c->stream, a);
    SWZ_LAUNCH_CHECK(c);
  }
  std::vector<uint64_t> got((size_t)words);
  SWZ_HIP(c, hipMemcpyAsync(got.data(), d_table, got.size() * 8, hipMemcpyDeviceToHost, c->stream));
  SWZ_HIP(c, hipStreamSynchronize(c->stream));
  uint64_t place = 0;
  for (uint64_t k = 0; k < num_nodes; ++k) {
    if (node_count[k] == 0) continue;
    for (uint32_t j = 0; j < cols; ++j) {
      const uint64_t* w = &got[(place * cols + j) * 4];
      swz_attr_summary& e = out[k * cols + j];
      if (a.kind[j] == SUM_BYTE) {
        memcpy(e.set, w, 32);
        summary_byte_bounds(attr_of[j], &e);
      } else if (a.kind[j] == SUM_U16) {
        e.lo = (double)(uint32_t)(w[0] & 0xFFFFFFFFull);
        e.hi = (double)(uint32_t)(w[0] >> 32);
      } else {
        e.lo = box_decode(w[0]);  // (a node whose times are all NaN: the preset, +inf / -inf)
        e.hi = box_decode(w[1]);
        e.flags = (uint32_t)w[2];
      }
    }
    ++place;
  }
  return SWZ_OK;
}

// ---------------------------------------------------------------------------------- the sidecar file
static const char SIDECAR_NAME[] = "node-summaries.swz";
static const unsigned char SIDECAR_MAGIC[8] = {'S', 'W', 'Z', 'N', 'S', 'U', 'M', 0};
constexpr uint64_t SIDECAR_HEAD = 48, SIDECAR_NODE = 24;

static void put_le(unsigned char* p, uint64_t v, int bytes) {
  for (int i = 0; i < bytes; ++i) p[i] = (unsigned char)(v >> (8 * i));
}
static uint64_t get_le(const unsigned char* p, int bytes) {
  uint64_t v = 0;
  for (int i = 0; i < bytes; ++i) v |= (uint64_t)p[i] << (8 * i);
  return v;
}
// an entry's fields one after the other, little-endian (the struct's own bytes on the hosts the library runs on)
static void put_entry(unsigned char* p, const swz_attr_summary& e) {
  uint64_t b;
  memcpy(&b, &e.lo, 8);
  put_le(p, b, 8);
  memcpy(&b, &e.hi, 8);
  put_le(p + 8, b, 8);
  for (int w = 0; w < 4; ++w) put_le(p + 16 + 8 * w, e.set[w], 8);
  put_le(p + 48, e.flags, 4);
  put_le(p + 52, e.reserved, 4);
}
static swz_attr_summary get_entry(const unsigned char* p) {
  swz_attr_summary e{};
  uint64_t b = get_le(p, 8);
  memcpy(&e.lo, &b, 8);
  b = get_le(p + 8, 8);
  memcpy(&e.hi, &b, 8);
  for (int w = 0; w < 4; ++w) e.set[w] = get_le(p + 16 + 8 * w, 8);
  e.flags = (uint32_t)get_le(p + 48, 4);
  e.reserved = (uint32_t)get_le(p + 52, 4);
  return e;
}

int sidecar_write(const std::string& dir, int32_t format, uint32_t mask, uint64_t num_nodes, const int8_t* level, const uint64_t* key,
                  const uint64_t* count, const swz_attr_summary* entries, std::string* why) {
  auto refuse = [&](const std::string& what) {
    *why = what;
    return SWZ_ERR_BAD_ARG;
  };
  if (format < SWZ_OUT_BIN || format > SWZ_OUT_ENTWINE_LAS) return refuse("an unknown format");
  if (mask & ~(uint32_t)SWZ_SUMMARY_SCALARS) return refuse("a bit of the mask that names no scalar column");
  const uint32_t cols = (uint32_t)__builtin_popcount(mask);
  if (num_nodes && (!level || !key || !count || (cols && !entries))) return refuse("NULL node table");
  uint64_t points = 0;
  for (uint64_t k = 0; k < num_nodes; ++k) {
    if (k && !(level[k - 1] != level[k] ? level[k - 1] < level[k] : key[k - 1] < key[k]))
      return refuse("the nodes are not in (level, Morton index) order");
    points += count[k];
  }
  std::vector<unsigned char> image((size_t)(SIDECAR_HEAD + num_nodes * SIDECAR_NODE + num_nodes * cols * sizeof(swz_attr_summary)), 0);
  unsigned char* p = image.data();
  memcpy(p, SIDECAR_MAGIC, 8);
  put_le(p + 8, 1, 4);
  put_le(p + 12, (uint32_t)format, 4);
  put_le(p + 16, mask, 4);
  put_le(p + 20, sizeof(swz_attr_summary), 4);
  put_le(p + 24, num_nodes, 8);
  put_le(p + 32, points, 8);
  p += SIDECAR_HEAD;
  for (uint64_t k = 0; k < num_nodes; ++k, p += SIDECAR_NODE) {
    put_le(p, key[k], 8);
    put_le(p + 8, count[k], 8);
    p[16] = (unsigned char)level[k];
  }
  for (uint64_t i = 0; i < num_nodes * cols; ++i, p += sizeof(swz_attr_summary)) {
    if (entries[i].reserved) return refuse("an entry's reserved must be 0");
    put_entry(p, entries[i]);
  }
  const std::string path = dir + "/" + SIDECAR_NAME, tmp = path + ".tmp";
  const int st = write_file(tmp, {{image.data(), image.size()}}, why);
  if (st != SWZ_OK) {
    (void)remove(tmp.c_str());
    return st;
  }
  if (rename(tmp.c_str(), path.c_str()) != 0) {
    (void)remove(tmp.c_str());
    *why = "cannot rename " + tmp + " to " + path;
    return SWZ_ERR_INTERNAL;
  }
  return SWZ_OK;
}

int sidecar_read(const std::string& dir, Sidecar* out, std::string* why) {
  *out = Sidecar{};
  const std::string path = dir + "/" + SIDECAR_NAME;
  auto refuse = [&](const std::string& what) {
    *why = path + ": " + what;
    return SWZ_ERR_BAD_ARG;
  };
  if (access(path.c_str(), F_OK) != 0) return SWZ_OK;  // no sidecar: not an error
  std::vector<unsigned char> image;
  if (read_whole_file(nullptr, path.c_str(), &image) != SWZ_OK) return refuse("cannot be opened");
  if (image.size() < SIDECAR_HEAD) return refuse("a wrong file size: shorter than its header");
  const unsigned char* p = image.data();
  if (memcmp(p, SIDECAR_MAGIC, 8) != 0) return refuse("a wrong magic: not a node-summaries file");
  if (get_le(p + 8, 4) != 1) return refuse("a wrong version: " + std::to_string(get_le(p + 8, 4)) + " (this library reads version 1)");
  const uint64_t format = get_le(p + 12, 4), mask = get_le(p + 16, 4), entry = get_le(p + 20, 4), nodes = get_le(p + 24, 8);
  if (entry != sizeof(swz_attr_summary)) return refuse("a wrong entry size: " + std::to_string(entry) + " bytes, not 56");
  if (format > SWZ_OUT_ENTWINE_LAS) return refuse("an unknown format");
  if (mask & ~(uint64_t)SWZ_SUMMARY_SCALARS) return refuse("a bit of the mask that names no scalar column");
  if (get_le(p + 40, 8) != 0) return refuse("a nonzero reserved field in the header");
  const uint32_t cols = (uint32_t)__builtin_popcount((uint32_t)mask);
  const uint64_t per_node = SIDECAR_NODE + (uint64_t)cols * sizeof(swz_attr_summary);
  if (nodes > (image.size() - SIDECAR_HEAD) / SIDECAR_NODE || SIDECAR_HEAD + nodes * per_node != image.size())
    return refuse("a wrong file size: " + std::to_string(image.size()) + " bytes for " + std::to_string(nodes) + " nodes of " +
                  std::to_string(cols) + " columns");
  out->format = (int32_t)format;
  out->mask = (uint32_t)mask;
  out->cols = cols;
  out->level.resize(nodes);
  out->key.resize(nodes);
  out->count.resize(nodes);
  p += SIDECAR_HEAD;
  uint64_t points = 0;
  for (uint64_t k = 0; k < nodes; ++k, p += SIDECAR_NODE) {
    out->key[k] = get_le(p, 8);
    out->count[k] = get_le(p + 8, 8);
    out->level[k] = (int8_t)p[16];
    if (get_le(p + 17, 7) != 0) return refuse("a nonzero reserved field in node " + std::to_string(k));
    if (k) {
      if (out->level[k - 1] == out->level[k] && out->key[k - 1] == out->key[k]) return refuse("node " + std::to_string(k) + " is there twice");
      if (!(out->level[k - 1] != out->level[k] ? out->level[k - 1] < out->level[k] : out->key[k - 1] < out->key[k]))
        return refuse("nodes out of order at node " + std::to_string(k));
    }
    points += out->count[k];
  }
  if (points != get_le(image.data() + 32, 8)) return refuse("the header's points are not the sum of the nodes' counts");
  out->entries.resize(nodes * cols);
  for (uint64_t i = 0; i < nodes * cols; ++i, p += sizeof(swz_attr_summary)) {
    out->entries[i] = get_entry(p);
    if (out->entries[i].reserved) return refuse("a nonzero reserved field in entry " + std::to_string(i));
  }
  out->points = points;
  out->present = true;
  return SWZ_OK;
}

// ---------------------------------------------------------------------------------- a data set's summaries
// swz_dataset_summarize: every node of the source through the query's stream (SourceLoop::each_chunk, swz_source.hip), the
// summaries kernel on every chunk, the sidecar.  A source without scalar columns gets its empty sidecar without a stream.
static int summarize(swz_ctx* c, const char* who, const char* dir, uint32_t source_flags, uint64_t chunk_points, swz_summarize_stats* stats) {
  auto refuse = [&](const std::string& what) { return c->fail(SWZ_ERR_BAD_ARG, std::string(who) + ": " + what); };
  const auto t_wall = std::chrono::steady_clock::now();
  if (stats) *stats = swz_summarize_stats{};
  if (!dir) return refuse("NULL argument");
  if (source_flags & ~(uint32_t)SWZ_CONVERT_LOSSY_SOURCE) return refuse("an unknown bit in source_flags");
  DatasetScan scan;
  SWZ_TRY(source_open(c, who, dir, -1, source_flags, &scan, nullptr));
  uint32_t mask = scan.info.attribute_mask & (uint32_t)SWZ_SUMMARY_SCALARS;
  if (scan.info.format == SWZ_OUT_3DTILES) mask &= 1u << SWZ_ATTR_INTENSITY;  // all a .pnts file carries beside RGB
  const uint32_t cols = (uint32_t)__builtin_popcount(mask);
  const uint64_t nn = scan.count.size();
  std::vector<swz_attr_summary> entries((size_t)(nn * cols), summary_empty());
  SourceLoopStats ls;
  SourceLoop loop{c, who, scan, mask, chunk_points};
  if (cols) {
    SWZ_HIP(c, hipSetDevice(c->device));
    std::vector<uint64_t> offset;
    const SourceChunkBody body = [&](const SourceChunkView& ch) -> int {
      offset.assign(ch.k1 - ch.k0, 0);
      for (uint64_t k = ch.k0 + 1; k < ch.k1; ++k) offset[k - ch.k0] = offset[k - ch.k0 - 1] + scan.count[k - 1];
      return node_summaries(c, who, ch.rows, ch.cols, mask, ch.k1 - ch.k0, offset.data(), scan.count.data() + ch.k0,
                            entries.data() + ch.k0 * cols);
    };
    SWZ_TRY(loop.each_chunk(body, &ls));
  }
  std::string why;
  const int st = sidecar_write(dir, scan.info.format, mask, nn, scan.level.data(), scan.key.data(), scan.count.data(), entries.data(), &why);
  if (st != SWZ_OK) return c->fail(st, std::string(who) + ": " + why);
  if (stats) {
    stats->nodes = nn;
    stats->points = scan.info.points;
    stats->bytes_read = ls.bytes_read;
    stats->chunks = ls.chunks;
    stats->read_ms = ls.read_ms;
    stats->unpack_ms = ls.unpack_ms;
    stats->summary_ms = ls.body_ms;
    stats->copy_ms = ls.copy_ms;
    stats->wall_ms = ms_since(t_wall);
  }
  return SWZ_OK;
}

}  // namespace swz

using namespace swz;

extern "C" {

uint32_t swz_node_summaries_tile(void) { return (uint32_t)SUM_TILE; }

int swz_dataset_summarize(swz_ctx* c, const char* dir, uint32_t source_flags, uint64_t chunk_points, swz_summarize_stats* stats) {
  if (!c) return SWZ_ERR_BAD_ARG;
  return summarize(c, "swz_dataset_summarize", dir, source_flags, chunk_points, stats);
}

int swz_node_summaries_device(swz_ctx* c, uint64_t n, const swz_attribute_columns* d_in, uint32_t attribute_mask, uint64_t num_nodes,
                              const uint64_t* node_offset, const uint64_t* node_count, swz_attr_summary* summaries_out) {
  if (!c) return SWZ_ERR_BAD_ARG;
  return node_summaries(c, "swz_node_summaries_device", n, d_in, attribute_mask, num_nodes, node_offset, node_count, summaries_out);
}

int swz_dataset_summaries_write(const char* dir, int32_t format, uint32_t mask, uint64_t num_nodes, const int8_t* level,
                                const uint64_t* key, const uint64_t* count, const swz_attr_summary* entries, char* why_out,
                                uint64_t why_bytes) {
  swz_ctx text;
  std::string why;
  int st = dir ? sidecar_write(dir, format, mask, num_nodes, level, key, count, entries, &why) : SWZ_ERR_BAD_ARG;
  if (!dir) why = "NULL argument";
  if (st != SWZ_OK) text.fail(st, "swz_dataset_summaries_write: " + why);
  return why_text(st, text, why_out, why_bytes);
}

int swz_dataset_summaries_read(const char* dir, int32_t* present_out, int32_t* format_out, uint32_t* mask_out, uint64_t* num_nodes_out,
                               uint64_t* points_out, uint64_t max_nodes, int8_t* level_out, uint64_t* key_out, uint64_t* count_out,
                               swz_attr_summary* entries_out, char* why_out, uint64_t why_bytes) {
  swz_ctx text;
  auto done = [&](int st, const std::string& why) {
    if (st != SWZ_OK) text.fail(st, "swz_dataset_summaries_read: " + why);
    return why_text(st, text, why_out, why_bytes);
  };
  if (!dir || !present_out) return done(SWZ_ERR_BAD_ARG, "NULL argument");
  Sidecar s;
  std::string why;
  const int st = sidecar_read(dir, &s, &why);
  if (st != SWZ_OK) return done(st, why);
  *present_out = s.present ? 1 : 0;
  if (format_out) *format_out = s.format;
  if (mask_out) *mask_out = s.mask;
  if (num_nodes_out) *num_nodes_out = s.key.size();
  if (points_out) *points_out = s.points;
  if (!level_out && !key_out && !count_out && !entries_out) return done(SWZ_OK, "");
  if (s.key.size() > max_nodes) return done(SWZ_ERR_BAD_ARG, "max_nodes too small");
  for (uint64_t k = 0; k < s.key.size(); ++k) {
    if (level_out) level_out[k] = s.level[k];
    if (key_out) key_out[k] = s.key[k];
    if (count_out) count_out[k] = s.count[k];
  }
  if (entries_out && !s.entries.empty()) memcpy(entries_out, s.entries.data(), s.entries.size() * sizeof(swz_attr_summary));
  return done(SWZ_OK, "");
}

}  // extern "C"
