// swz_nodepack.h -- what the pack kernels of the node-file writers share (swz_pnts.hip, swz_las.hip).  A PACK TABLE lists the
// nodes that hold points by ascending first row: { start, count, base of the body in the image, a multiple of 8 } and
// whatever else the format keeps per node.  One block takes TILE consecutive stored rows, one per thread; the device helpers
// find the nodes of those rows, the host functions check a node table, build the pack table and upload it.
#pragma once

#include <string>
#include <vector>

#include "swz_internal.h"

namespace swz {

// ---------------------------------------------------------------------------------- device: the nodes of a tile's rows
constexpr uint32_t PACK_FILLER = 0xFFFFFFFFu;  // (a row number is below 2^32 - 65536: the filler sorts behind every row)

// the last node that starts at or before r0 (the first node when there is none)
template <typename Node>
__device__ __forceinline__ uint32_t pack_first_node(const Node* nodes, uint32_t num_nodes, uint32_t r0) {
  uint32_t lo = 0, hi = num_nodes;
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (nodes[mid].start <= r0) lo = mid + 1; else hi = mid;
  }
  return lo ? lo - 1 : 0;
}

// Entry threadIdx.x of the block's window: node k0 + threadIdx.x when it starts in front of r1, else the filler (a tile
// holds at most TILE nodes: they are not empty).  Returns the node it listed, or null: what else the block keeps of a node
// is the caller's.  The caller synchronises.
template <typename Node>
__device__ __forceinline__ const Node* pack_fill_window(const Node* nodes, uint32_t num_nodes, uint32_t k0, uint32_t r1,
                                                        uint32_t* s_start, uint32_t* s_count) {
  const uint32_t t = threadIdx.x;
  const Node* nd = nullptr;
  if ((uint64_t)k0 + t < num_nodes && nodes[k0 + t].start < r1) nd = nodes + k0 + t;
  s_start[t] = nd ? nd->start : PACK_FILLER;
  s_count[t] = nd ? nd->count : 0u;
  return nd;
}

// the window entry *e whose node holds row r; false (and *e = 0) when r lies behind the tile or in no node
template <int TILE>
__device__ __forceinline__ bool pack_row_node(const uint32_t* s_start, const uint32_t* s_count, uint32_t r, uint32_t r1, uint32_t* e) {
  *e = 0;
  if (r >= r1) return false;
  uint32_t l = 0, h = TILE;
  while (l < h) {
    const uint32_t mid = (l + h) / 2;
    if (s_start[mid] <= r) l = mid + 1; else h = mid;
  }
  if (!l) return false;
  *e = l - 1;
  return r - s_start[*e] < s_count[*e];
}

// the source row of stored row r (order may be null: identity) and its position
__device__ __forceinline__ uint32_t pack_source_row(const uint32_t* perm, const uint32_t* order, const double* xyz, uint32_t r,
                                                    double pos[3]) {
  const uint32_t src = perm[order ? order[r] : r];
  const double* p = xyz + (size_t)src * 3;
  pos[0] = p[0];
  pos[1] = p[1];
  pos[2] = p[2];
  return src;
}

// ---------------------------------------------------------------------------------- host: from a node table to the launch
struct PackNames {
  const char* who;     // the entry point, in front of every error text
  const char* layout;  // the function that gives the image its size
  const char* buffer;  // the workspace buffer of the uploaded table
};

template <typename Node>
struct PackTable {
  std::vector<Node> nodes;
  uint64_t image_bytes = 0;  // the bodies of all nodes, one behind the other
  uint64_t prev_end = 0;     // one past the last row of the last node
};

// Checks the node table (ascending, no overlap, inside the n rows) and lists the nodes that hold points.  per_node(k, &node)
// runs for EVERY node, empty ones included, and fills what the format keeps per node besides start, count and base;
// body_size(count, &bytes) gives the size of a body.  Both return null or what is wrong, which is refused in `who`'s name.
template <typename Node, typename PerNode, typename BodySize>
int pack_build_table(swz_ctx* c, const PackNames& names, uint64_t n, uint64_t num_nodes, const uint64_t* node_offset,
                     const uint64_t* node_count, PerNode&& per_node, BodySize&& body_size, PackTable<Node>* out) {
  auto refuse = [&](const char* what) { return c->fail(SWZ_ERR_BAD_ARG, std::string(names.who) + ": " + what); };
  uint64_t prev_offset = 0;
  for (uint64_t k = 0; k < num_nodes; ++k) {
    const uint64_t off = node_offset[k], cnt = node_count[k];
    if (off < prev_offset) return refuse("node offsets are not ascending");
    prev_offset = off;
    Node nd{};
    if (const char* what = per_node(k, &nd)) return refuse(what);
    if (cnt == 0) continue;
    if (off < out->prev_end) return refuse("node ranges overlap");
    if (off > n || cnt > n - off) return refuse("a node range passes the last row");
    uint64_t bytes = 0;
    if (const char* what = body_size(cnt, &bytes)) return refuse(what);
    out->prev_end = off + cnt;
    nd.start = (uint32_t)off;
    nd.count = (uint32_t)cnt;
    nd.base = out->image_bytes;
    out->nodes.push_back(nd);
    out->image_bytes += bytes;
  }
  return SWZ_OK;
}

// What lies between the table and the launch: the checks of the buffers, then the table's upload on the context's stream.
// *d_nodes_out stays null when no node holds points (n == 0, no nodes, or only empty ones): nothing to write.
template <typename Node>
int pack_upload_table(swz_ctx* c, const PackNames& names, const PackTable<Node>& table, const void* d_perm, const void* d_xyz,
                      const void* d_image_out, uint64_t image_bytes, const Node** d_nodes_out) {
  auto refuse = [&](const std::string& what) { return c->fail(SWZ_ERR_BAD_ARG, std::string(names.who) + ": " + what); };
  *d_nodes_out = nullptr;
  if (table.image_bytes > image_bytes) return refuse(std::string("the image buffer is smaller than ") + names.layout + "'s total");
  if (table.nodes.empty()) return SWZ_OK;
  if (!d_perm || !d_xyz || !d_image_out) return refuse("NULL buffer");
  if (((uintptr_t)d_image_out & 7u) != 0) return refuse("the image must be 8-byte aligned");
  SWZ_HIP(c, hipSetDevice(c->device));
  Node* d_nodes = nullptr;
  SWZ_TRY(c->get(names.buffer, table.nodes.size(), &d_nodes));
  SWZ_HIP(c, hipMemcpyAsync(d_nodes, table.nodes.data(), table.nodes.size() * sizeof(Node), hipMemcpyHostToDevice, c->stream));
  *d_nodes_out = d_nodes;
  return SWZ_OK;
}

}  // namespace swz
