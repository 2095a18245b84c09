// swz_nodebox.h -- the table of node boxes that swz_nodebox.hip and swz_srsbox.hip share: six ORDER-PRESERVING codes per node
// that holds points (min x, y, z, max x, y, z), preset to the codes of +inf / -inf and combined with 64-bit integer atomics.
#pragma once
#include <cstring>

#include "swz_internal.h"

namespace swz {

constexpr uint64_t BOX_MAX_POINTS = 0xFFFFFFFFull - 65535ull;  // the library's limit of points per batch (2^32 - 65536)
constexpr uint32_t BOX_NO_ENTRY = 0xFFFFFFFFu;
constexpr uint64_t BOX_CODE_POS_INF = 0xFFF0000000000000ull;  // box_code(+inf): what a minimum starts from
constexpr uint64_t BOX_CODE_NEG_INF = 0x000FFFFFFFFFFFFFull;  // box_code(-inf): what a maximum starts from

struct BoxNode {  // an entry of the pack table (swz_nodepack.h)
  uint32_t start, count;
  uint64_t base;  // of the node's six codes in the table, in bytes: 48 x its place among the nodes that hold points
};

// all bits of a negative flipped, the sign bit of a non-negative set: the codes ascend with the values, -0.0 just below +0.0
__host__ __device__ inline uint64_t box_code(double v) {
#ifdef __HIP_DEVICE_COMPILE__
  const uint64_t b = (uint64_t)__double_as_longlong(v);
#else
  uint64_t b;
  memcpy(&b, &v, 8);
#endif
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
inline double box_decode(uint64_t code) {
  const uint64_t b = (code >> 63) ? (code & 0x7FFFFFFFFFFFFFFFull) : ~code;
  double v;
  memcpy(&v, &b, 8);
  return v;
}

// the small kernel that presets `entries` codes (six per node) on c's stream; no synchronisation (swz_nodebox.hip)
int node_boxes_preset(swz_ctx* c, uint64_t* d_table, uint32_t entries);

}  // namespace swz
