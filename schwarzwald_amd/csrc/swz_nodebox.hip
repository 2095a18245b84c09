// swz_nodebox.hip -- the tight box of every node of a table: a segmented min/max over the stored rows, on the device.
//
// Row i of node k is d_xyz[d_perm[d_order[node_offset[k] + i]]], the composition the pack kernels of the node-file writers
// take (swz_nodepack.h), and the table is checked, listed and uploaded by that header's functions.  One block takes
// BOX_TILE consecutive stored rows, one per thread.  A double is compared as its ORDER-PRESERVING unsigned code (all bits of
// a negative flipped, the sign bit of a non-negative set: the codes ascend with the values, -0.0 just below +0.0), so min
// and max are integer min and max and nothing is ever computed on a value.  The rows of a node are contiguous within a
// tile: a wave reduces its lanes by window entry with shuffles, the first lane of every run combines into the entry's six
// codes in LDS, and each window entry that has rows in the tile leaves with six 64-bit atomics on the table in global
// memory.  A small kernel presets that table to the codes of +inf / -inf, so nothing depends on what the buffer held;
// min and max commute, so the order of the atomics does not show.  The codes are decoded on the host after the copy back.
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "swz_internal.h"
#include "swz_device.h"
#include "swz_nodebox.h"
#include "swz_nodepack.h"

namespace swz {

constexpr int BOX_TILE = 256;  // stored rows per block, one per thread

struct BoxArgs {
  const uint32_t* perm;
  const uint32_t* order;  // may be null: identity
  uint32_t n;
  const double* xyz;
  const BoxNode* nodes;
  uint32_t num_nodes;
  uint64_t* table;  // per listed node: min x, y, z, max x, y, z as codes
};

__global__ void node_boxes_preset_kernel(uint64_t* table, uint32_t entries) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < entries) table[i] = (i % 6u) < 3u ? BOX_CODE_POS_INF : BOX_CODE_NEG_INF;
}

__global__ __launch_bounds__(BOX_TILE) void node_boxes_kernel(BoxArgs a) {
  __shared__ uint32_t s_start[BOX_TILE];
  __shared__ uint32_t s_count[BOX_TILE];
  __shared__ unsigned long long s_box[BOX_TILE * 6];
  const uint32_t t = threadIdx.x;
  const uint32_t r0 = blockIdx.x * (uint32_t)BOX_TILE;
  const uint32_t r1 = (uint32_t)min((uint64_t)r0 + BOX_TILE, (uint64_t)a.n);

  const uint32_t k0 = pack_first_node(a.nodes, a.num_nodes, r0);
  const BoxNode* const listed = pack_fill_window(a.nodes, a.num_nodes, k0, r1, s_start, s_count);
#pragma unroll
  for (int k = 0; k < 6; ++k) s_box[6 * t + k] = k < 3 ? BOX_CODE_POS_INF : BOX_CODE_NEG_INF;
  __syncthreads();

  const uint32_t r = r0 + t;
  uint32_t e;
  const bool in_node = pack_row_node<BOX_TILE>(s_start, s_count, r, r1, &e);
  if (!in_node) e = BOX_NO_ENTRY;
  unsigned long long lo[3] = {BOX_CODE_POS_INF, BOX_CODE_POS_INF, BOX_CODE_POS_INF};
  unsigned long long hi[3] = {BOX_CODE_NEG_INF, BOX_CODE_NEG_INF, BOX_CODE_NEG_INF};
  if (in_node) {
    double pos[3];
    (void)pack_source_row(a.perm, a.order, a.xyz, r, pos);
#pragma unroll
    for (int k = 0; k < 3; ++k) lo[k] = hi[k] = box_code(pos[k]);
  }
  // the lanes of one entry are neighbours: after the step of distance d a lane holds its run's rows [lane, lane + 2d)
  const uint32_t lane = t & 63u;
#pragma unroll
  for (uint32_t d = 1; d < 64u; d <<= 1) {
    const uint32_t e_far = __shfl_down(e, d, 64);
    const bool same = lane + d < 64u && e_far == e;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const unsigned long long lo_far = __shfl_down(lo[k], d, 64);
      const unsigned long long hi_far = __shfl_down(hi[k], d, 64);
      if (same) {
        lo[k] = min(lo[k], lo_far);
        hi[k] = max(hi[k], hi_far);
      }
    }
  }
  const uint32_t e_before = __shfl_up(e, 1u, 64);
  if (in_node && (lane == 0u || e_before != e)) {  // the first lane of a run: one combine per wave and entry
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      atomicMin(&s_box[6 * e + k], lo[k]);
      atomicMax(&s_box[6 * e + 3 + k], hi[k]);
    }
  }
  __syncthreads();
  // window entry t: six atomics when the node has rows in this tile (the first entry may end in front of it)
  if (listed && (uint64_t)listed->start + listed->count > r0) {
    unsigned long long* const out = reinterpret_cast<unsigned long long*>(a.table) + listed->base / 8;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      (void)__hip_atomic_fetch_min(out + k, s_box[6 * t + k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      (void)__hip_atomic_fetch_max(out + 3 + k, s_box[6 * t + 3 + k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

int node_boxes_preset(swz_ctx* c, uint64_t* d_table, uint32_t entries) {
  hipLaunchKernelGGL(node_boxes_preset_kernel, dim3(div_up(entries, 256)), dim3(256), 0, c->stream, d_table, entries);
  SWZ_LAUNCH_CHECK(c);
  return SWZ_OK;
}

}  // namespace swz

using namespace swz;

extern "C" {

uint32_t swz_node_boxes_tile(void) { return (uint32_t)BOX_TILE; }

int swz_node_boxes_device(swz_ctx* c, const uint32_t* d_perm, const uint32_t* d_order, uint64_t n, const double* d_xyz,
                          uint64_t num_nodes, const uint64_t* node_offset, const uint64_t* node_count, double* box_min_out,
                          double* box_max_out) {
  if (!c) return SWZ_ERR_BAD_ARG;
  // everything is checked on the host before anything is launched
  if (n > BOX_MAX_POINTS) return c->fail(SWZ_ERR_BAD_ARG, "swz_node_boxes_device: more than 2^32-65536 rows");
  if (num_nodes && (!node_offset || !node_count || !box_min_out || !box_max_out))
    return c->fail(SWZ_ERR_BAD_ARG, "swz_node_boxes_device: NULL node table");
  const PackNames names{"swz_node_boxes_device", "swz_node_boxes_device", "nodebox_nodes"};
  PackTable<BoxNode> table;
  SWZ_TRY(pack_build_table(
    c, names, n, num_nodes, node_offset, node_count, [](uint64_t, BoxNode*) -> const char* { return nullptr; },
    [](uint64_t, uint64_t* bytes) -> const char* {
      *bytes = 48;
      return nullptr;
    },
    &table));
  const uint64_t listed = table.nodes.size(), prev_end = table.prev_end;
  if (listed && (!d_perm || !d_xyz)) return c->fail(SWZ_ERR_BAD_ARG, "swz_node_boxes_device: NULL buffer");

  const double inf = std::numeric_limits<double>::infinity();
  for (uint64_t i = 0; i < 3 * num_nodes; ++i) {  // a node without points, and every node when nothing is launched
    box_min_out[i] = inf;
    box_max_out[i] = -inf;
  }
  BoxArgs a{};
  uint64_t* d_table = nullptr;
  if (listed) {
    SWZ_HIP(c, hipSetDevice(c->device));
    SWZ_TRY(c->get("nodebox_table", (size_t)listed * 6, &d_table));
  }
  SWZ_TRY(pack_upload_table(c, names, table, d_perm, d_xyz, d_table, listed * 48, &a.nodes));
  if (!a.nodes) return SWZ_OK;
  a.perm = d_perm;
  a.order = d_order;
  a.n = (uint32_t)n;
  a.xyz = d_xyz;
  a.num_nodes = (uint32_t)listed;
  a.table = d_table;
  {
    ProfScope ps(c, "node_boxes", prev_end * (d_order ? 8 : 4) + prev_end * 24 + listed * (sizeof(BoxNode) + 96), 2);
    const uint32_t entries = (uint32_t)(listed * 6);
    SWZ_TRY(node_boxes_preset(c, d_table, entries));
    // rows behind the last node belong to no node: the grid ends with it
    hipLaunchKernelGGL(node_boxes_kernel, dim3(div_up(prev_end, BOX_TILE)), dim3(BOX_TILE), 0, c->stream, a);
    SWZ_LAUNCH_CHECK(c);
  }
  std::vector<uint64_t> codes((size_t)listed * 6);
  SWZ_HIP(c, hipMemcpyAsync(codes.data(), d_table, codes.size() * 8, hipMemcpyDeviceToHost, c->stream));
  SWZ_HIP(c, hipStreamSynchronize(c->stream));
  uint64_t j = 0;
  for (uint64_t k = 0; k < num_nodes; ++k) {
    if (node_count[k] == 0) continue;
    for (int ax = 0; ax < 3; ++ax) {
      box_min_out[3 * k + ax] = box_decode(codes[6 * j + ax]);
      box_max_out[3 * k + ax] = box_decode(codes[6 * j + 3 + ax]);
    }
    ++j;
  }
  return SWZ_OK;
}

}  // extern "C"
