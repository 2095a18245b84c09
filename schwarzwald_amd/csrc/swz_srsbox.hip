// swz_srsbox.hip -- a chunk of stored rows projected in place and the box of every node's PROJECTED rows, in one launch
// (swz_srs_project_node_boxes_device): what swz_convert_dataset_world runs between the unpack and the pack of a chunk.
//
// A workgroup takes tiles of SRS_BOX_TILE rows, grid-stride, and stages a tile's 24-byte rows through LDS exactly as
// srs_transform_kernel does (swz_srs.hip); every lane maps its own row with the inlined map of swz_srs.h -- the target is a
// kernel argument as it is there, and contraction is off inside the map, so the stored bits are those of
// swz_srs_transform_device.  The rows are in stored order, so the rows of a node are neighbours: the block finds the nodes
// of its tile with the window helpers of swz_nodepack.h, a wave reduces the runs of lanes of one node with shuffles on the
// order-preserving codes of swz_nodebox.h, and the first lane of every run leaves with one 64-bit atomic min and one
// atomic max per axis on the table in global memory, which the preset kernel of swz_nodebox.hip set to +inf / -inf.
#include <limits>
#include <string>
#include <vector>

#include "swz_internal.h"
#include "swz_device.h"
#include "swz_nodebox.h"
#include "swz_nodepack.h"
#include "swz_srs.h"

namespace swz {

constexpr int SRS_BOX_TILE = 256;  // rows per workgroup and turn, one per thread: swz_srs_tile()

struct SrsBoxArgs {
  swz_srs s;
  int target;   // SWZ_SRS_ECEF
  int project;  // 0: the rows stay as they are, only the boxes are reduced
  double* xyz;
  uint32_t n;
  const BoxNode* nodes;  // the nodes that hold points, by ascending first row (may be null: no boxes)
  uint32_t num_nodes;
  uint64_t* table;  // per listed node: min x, y, z, max x, y, z as codes
};

__global__ __launch_bounds__(SRS_BOX_TILE) void srs_project_node_boxes_kernel(SrsBoxArgs a) {
  __shared__ double s_row[3 * SRS_BOX_TILE];
  __shared__ uint32_t s_start[SRS_BOX_TILE];
  __shared__ uint32_t s_count[SRS_BOX_TILE];
  const uint32_t t = threadIdx.x;
  const uint32_t lane = t & 63u;
  const uint32_t tiles = (uint32_t)(((uint64_t)a.n + SRS_BOX_TILE - 1) / SRS_BOX_TILE);
  for (uint32_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const uint32_t r0 = tile * (uint32_t)SRS_BOX_TILE;
    const uint32_t rows = min((uint32_t)SRS_BOX_TILE, a.n - r0);
    const uint32_t r1 = r0 + rows;
    double* const g = a.xyz + 3 * (size_t)r0;
    for (uint32_t w = t; w < 3 * rows; w += SRS_BOX_TILE) s_row[w] = g[w];
    const uint32_t k0 = pack_first_node(a.nodes, a.num_nodes, r0);
    (void)pack_fill_window(a.nodes, a.num_nodes, k0, r1, s_start, s_count);
    __syncthreads();

    double x = 0.0, y = 0.0, z = 0.0;
    if (t < rows) {
      x = s_row[3 * t];
      y = s_row[3 * t + 1];
      z = s_row[3 * t + 2];
      if (a.project) {
        srs_to_target(a.s, a.target, x, y, z);
        s_row[3 * t] = x;
        s_row[3 * t + 1] = y;
        s_row[3 * t + 2] = z;
      }
    }
    uint32_t e;
    const bool in_node = pack_row_node<SRS_BOX_TILE>(s_start, s_count, r0 + t, r1, &e);
    if (!in_node) e = BOX_NO_ENTRY;
    unsigned long long lo[3] = {BOX_CODE_POS_INF, BOX_CODE_POS_INF, BOX_CODE_POS_INF};
    unsigned long long hi[3] = {BOX_CODE_NEG_INF, BOX_CODE_NEG_INF, BOX_CODE_NEG_INF};
    if (in_node) {
      lo[0] = hi[0] = box_code(x);
      lo[1] = hi[1] = box_code(y);
      lo[2] = hi[2] = box_code(z);
    }
    // the lanes of one entry are neighbours: after the step of distance d a lane holds its run's rows [lane, lane + 2d)
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
    if (in_node && (lane == 0u || e_before != e)) {  // the first lane of a run: window entry e is listed node k0 + e
      unsigned long long* const out = reinterpret_cast<unsigned long long*>(a.table) + 6ull * ((uint64_t)k0 + e);
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        (void)__hip_atomic_fetch_min(out + k, lo[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        (void)__hip_atomic_fetch_max(out + 3 + k, hi[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
    __syncthreads();
    if (a.project)
      for (uint32_t w = t; w < 3 * rows; w += SRS_BOX_TILE) g[w] = s_row[w];
    __syncthreads();  // the next tile's loads write what these stores read, and its window replaces this one
  }
}

}  // namespace swz

using namespace swz;

extern "C" {

int swz_srs_project_node_boxes_device(swz_ctx* c, const swz_srs* srs, double* d_xyz, uint64_t n, uint64_t num_nodes,
                                      const uint64_t* node_offset, const uint64_t* node_count, double* box_min_out,
                                      double* box_max_out) {
  if (!c) return SWZ_ERR_BAD_ARG;
  const char* who = "swz_srs_project_node_boxes_device";
  // everything is checked on the host before anything is launched
  if (srs && !srs_valid(srs)) return c->fail(SWZ_ERR_BAD_ARG, std::string(who) + ": not a definition swz_srs_parse made");
  if (n > BOX_MAX_POINTS) return c->fail(SWZ_ERR_TOO_MANY_POINTS, std::string(who) + ": more than 2^32-65536 rows");
  if (num_nodes && (!node_offset || !node_count || !box_min_out || !box_max_out))
    return c->fail(SWZ_ERR_BAD_ARG, std::string(who) + ": NULL node table");
  const PackNames names{who, who, "srsbox_nodes"};
  PackTable<BoxNode> table;
  SWZ_TRY(pack_build_table(
    c, names, n, num_nodes, node_offset, node_count, [](uint64_t, BoxNode*) -> const char* { return nullptr; },
    [](uint64_t, uint64_t* bytes) -> const char* {
      *bytes = 48;
      return nullptr;
    },
    &table));
  const uint64_t listed = table.nodes.size();
  const double inf = std::numeric_limits<double>::infinity();
  for (uint64_t i = 0; i < 3 * num_nodes; ++i) {  // a node without points, and every node when nothing is launched
    box_min_out[i] = inf;
    box_max_out[i] = -inf;
  }
  if (n == 0 || (!srs && !listed)) return SWZ_OK;
  if (!d_xyz) return c->fail(SWZ_ERR_BAD_ARG, std::string(who) + ": NULL positions");

  SWZ_HIP(c, hipSetDevice(c->device));
  SrsBoxArgs a{};
  uint64_t* d_table = nullptr;
  if (listed) {
    SWZ_TRY(c->get("srsbox_table", (size_t)listed * 6, &d_table));
    SWZ_TRY(pack_upload_table(c, names, table, d_xyz, d_xyz, d_table, listed * 48, &a.nodes));
  }
  if (srs) a.s = *srs;
  a.target = SWZ_SRS_ECEF;
  a.project = srs ? 1 : 0;
  a.xyz = d_xyz;
  a.n = (uint32_t)n;
  a.num_nodes = (uint32_t)listed;
  a.table = d_table;
  {
    ProfScope ps(c, "srs_project_node_boxes", n * (srs ? 48 : 24) + listed * (sizeof(BoxNode) + 96), listed ? 2 : 1);
    if (listed) SWZ_TRY(node_boxes_preset(c, d_table, (uint32_t)(listed * 6)));
    // grid-stride like srs_transform_kernel; without a projection the rows behind the last node are not read
    const uint64_t rows = srs ? n : table.prev_end;
    a.n = (uint32_t)rows;
    const uint64_t tiles = (rows + SRS_BOX_TILE - 1) / SRS_BOX_TILE;
    const uint32_t grid = (uint32_t)std::min<uint64_t>(tiles, 256u * 32u);
    hipLaunchKernelGGL(srs_project_node_boxes_kernel, dim3(grid), dim3(SRS_BOX_TILE), 0, c->stream, a);
    SWZ_LAUNCH_CHECK(c);
  }
  std::vector<uint64_t> codes((size_t)listed * 6);
  if (listed) SWZ_HIP(c, hipMemcpyAsync(codes.data(), d_table, codes.size() * 8, hipMemcpyDeviceToHost, c->stream));
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
