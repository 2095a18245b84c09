// swz_level.hip -- one level of the level-synchronous octree tiling: node segmentation (K3), the level's sampler,
// stream compaction (K5), and the host's plan of a level.  The grid samplers live in swz_grid.hip, MIN_DISTANCE behind
// swz_md.hip (MIN_DISTANCE_FAST: swz_mdfast.hip in front of it); the drivers that loop over the levels in swz_session.hip, swz_shard.hip and swz_tiler.hip.
//
// The reference recurses top-down per node (TilingAlgorithmBase::do_tiling_for_node /
// tile_node / tile_internal_node, core/tiling/TilingAlgorithms.cpp:499-561, 351-492, 247-349): sample
// a node's Morton-sorted points (stable partition), persist the taken ones, split the rest into the
// <= 8 child octants (:116-162) and recurse.  Here all nodes of one level are processed together:
// the "active set" is the Morton-sorted array of points not yet taken; a node is a run of equal key
// prefix, a sampling-grid cell a run of a longer prefix; taken points get their level recorded and
// the survivors are stream-compacted (stable) into the next level's active set.
#include <algorithm>
#include <cmath>

#include "swz_md.h"
#include "swz_scan.h"

namespace swz {

// ----------------------------------------------------------------------------- node segmentation
// fused form: node-head flag computed from the keys inside the scan, node id / node start written by it
struct NodeHeadF {
  const uint64_t* akey;
  uint32_t nsh;
  __device__ uint32_t operator()(uint32_t i) const {
    return (i == 0) ? 1u : (uint32_t)((akey[i] >> nsh) != (akey[i - 1] >> nsh));
  }
};
struct NodeAssignG {
  uint32_t* nid;
  uint32_t* nstart;
  uint32_t m;
  __device__ void operator()(uint32_t i, uint32_t excl, uint32_t head) const {
    const uint32_t id = excl + head - 1u;
    nid[i] = id;
    if (head) nstart[id] = i;
    if (i == m - 1) nstart[id + 1] = m;
  }
};
// ---- segmentation by search: the nodes of a level are children of the nodes of the level above, and the active set is
// sorted by node prefix, so child o of parent P starts at the lower bound of (P, o) among the keys.  Nine searches per
// parent node instead of two passes over the keys of every point (20 bytes per point: the segmentation was as expensive
// as the sort's histogram passes); the node id per point, which the samplers look up, is then filled from the node starts.
__global__ __launch_bounds__(256) void node_child_bounds_kernel(const uint64_t* __restrict__ akey, uint32_t m, uint32_t nsh,
                                                                const uint64_t* __restrict__ pprefix, uint32_t parents,
                                                                uint32_t* __restrict__ cb) {
  const uint32_t t = blockIdx.x * 256 + threadIdx.x;
  const uint32_t j = t >> 4, o = t & 15u;
  if (j >= parents || o > 8u) return;
  const uint64_t target = (pprefix[j] >> nsh) + o;
  uint32_t lo = 0, hi = m;
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if ((akey[mid] >> nsh) < target) lo = mid + 1; else hi = mid;
  }
  cb[j * 9u + o] = lo;
}
struct ChildExistsF {
  const uint32_t* cb;
  uint32_t parents, m;
  uint32_t* counters;
  __device__ uint32_t operator()(uint32_t e) const {
    const uint32_t j = e >> 3, o = e & 7u;
    if (o == 0) {  // the parents' ranges must tile the active set: a point under none of them would belong to no node
      const uint32_t b = cb[j * 9u], en = cb[j * 9u + 8u];
      const bool ok = (j == 0 ? b == 0u : b == cb[(j - 1u) * 9u + 8u]) && (j + 1u < parents || en == m);
      if (!ok) atomicMax(&counters[CTR_ERROR], (uint32_t)SWZ_ERR_INTERNAL);
    }
    return cb[j * 9u + o + 1u] > cb[j * 9u + o] ? 1u : 0u;
  }
};
struct ChildStartG {
  const uint32_t* cb;
  uint32_t* nstart;
  __device__ void operator()(uint32_t e, uint32_t excl, uint32_t exists) const {
    if (!exists) return;
    const uint32_t j = e >> 3, o = e & 7u;
    nstart[excl] = cb[j * 9u + o];
    nstart[excl + 1u] = cb[j * 9u + o + 1u];  // (the next child writes the same value; the last one closes the table)
  }
};
constexpr uint32_t NF_TILE = 1024;  // points per workgroup: four per thread, one 16-byte store
// (lazy: the grid samplers look a point's node up only on levels that have take-all nodes -- the counters node_mode_kernel
// has just written say so --, and most levels of a large batch have none)
__global__ __launch_bounds__(256) void node_fill_kernel(const uint32_t* __restrict__ nstart, const uint32_t* __restrict__ counters,
                                                        uint32_t m, uint32_t* __restrict__ nid, int lazy) {
  __shared__ uint32_t s_lo, s_hi;
  __shared__ uint32_t ss[NF_TILE + 1];
  const uint32_t nn = counters[CTR_NUM_NODES];
  if (lazy && counters[CTR_SAMPLE_NODES] == nn) return;
  // (an inconsistent segmentation -- ChildExistsF raises CTR_ERROR -- must not be walked: the host reads the counter later)
  if (counters[CTR_ERROR] != 0u || nn == 0u) return;
  const uint32_t tid = threadIdx.x;
  const uint32_t i0 = blockIdx.x * NF_TILE;
  const uint32_t last = (m - i0) > NF_TILE ? i0 + NF_TILE - 1u : m - 1u;
  auto node_of = [&](uint32_t i) {  // the last node that starts at or before i
    uint32_t lo = 0, hi = nn;
    while (lo < hi) {
      const uint32_t mid = lo + (hi - lo) / 2;
      if (nstart[mid] <= i) lo = mid + 1; else hi = mid;
    }
    return lo - 1u;
  };
  if (tid < 2) {  // (two lanes of one wavefront: see tl_merge_rank_kernel, swz_tlevel.hip)
    const uint32_t r = node_of(tid ? last : i0);
    if (tid) s_hi = r; else s_lo = r;
  }
  __syncthreads();
  const uint32_t lo = s_lo, span = min(s_hi - s_lo + 1u, (uint32_t)NF_TILE);  // (at most one node starts per point: span <= NF_TILE)
  for (uint32_t k = tid; k <= span; k += 256u) ss[k] = (lo + k < nn) ? nstart[lo + k] : 0xFFFFFFFFu;  // ss[k]: start of node lo + k
  __syncthreads();
  const uint32_t i = i0 + tid * 4u;
  if (i >= m) return;
  uint32_t a = 0, b = span;  // the last k < span with ss[k] <= i
  while (a < b) {
    const uint32_t mid = a + (b - a) / 2;
    if (ss[mid] <= i) a = mid + 1; else b = mid;
  }
  uint32_t k = a - 1u;
  uint32_t v[4];
#pragma unroll
  for (uint32_t q = 0; q < 4u; ++q) {
    while (k + 1u <= span && ss[k + 1u] <= i + q) ++k;
    v[q] = lo + k;
  }
  if (i + 4u <= m) {
    *reinterpret_cast<uint4*>(nid + i) = make_uint4(v[0], v[1], v[2], v[3]);
  } else {
    for (uint32_t q = 0; i + q < m; ++q) nid[i + q] = v[q];
  }
}
__global__ __launch_bounds__(256) void node_prefix_kernel(const uint32_t* __restrict__ nstart, const uint64_t* __restrict__ akey,
                                                          uint32_t nsh, uint32_t nn, uint64_t* __restrict__ out) {
  const uint32_t j = blockIdx.x * 256 + threadIdx.x;
  if (j < nn) out[j] = nsh >= 63u ? 0ull : ((akey[nstart[j]] >> nsh) << nsh);
}
__global__ void single_node_kernel(uint32_t* __restrict__ nstart, uint32_t* __restrict__ num_nodes, uint32_t m) {
  nstart[0] = 0;
  nstart[1] = m;
  *num_nodes = 1;
}
// fused stable compaction: survivors move to the next level's active set, taken points get their level
struct KeepF {
  const uint8_t* taken;
  __device__ uint32_t operator()(uint32_t i) const { return taken[i] ? 0u : 1u; }
};
template <>
struct FsCountsZeroBytes<KeepF> {
  static constexpr bool value = true;
};
struct CompactG {
  const uint64_t* akey;
  const uint32_t* aidx;
  int8_t level;
  int8_t* level_out;
  uint64_t* okey;
  uint32_t* oidx;
  __device__ void operator()(uint32_t i, uint32_t excl, uint32_t keep) const {
    const uint32_t p = aidx ? aidx[i] : i;
    if (keep) {
      okey[excl] = akey[i];
      oidx[excl] = p;
    } else {
      level_out[p] = level;
    }
  }
};

__global__ __launch_bounds__(256) void node_head_kernel(const uint64_t* __restrict__ akey, uint32_t m,
                                                        uint32_t nsh, uint32_t* __restrict__ flags) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= m) return;
  flags[i] = (i == 0) ? 1u : (uint32_t)((akey[i] >> nsh) != (akey[i - 1] >> nsh));
}

__global__ __launch_bounds__(256) void node_finish_kernel(const uint32_t* __restrict__ flags,
                                                          uint32_t* __restrict__ nid, uint32_t m,
                                                          uint32_t* __restrict__ nstart) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= m) return;
  const uint32_t f = flags[i];
  const uint32_t id = nid[i] + f - 1u;  // exclusive count of heads before i -> node index of i
  nid[i] = id;
  if (f) nstart[id] = i;
  if (i == m - 1) nstart[id + 1] = m;
}

// ---- a level that shares its arrays with the level above (ActiveSet::gone): the open points before point i, from the
// open points before i's tile of FS_TILE (level_live_counts) and the bytes of that tile in front of i
__device__ __forceinline__ uint32_t live_before(const uint8_t* __restrict__ gone, const uint32_t* __restrict__ tiles, uint32_t i) {
  uint32_t off = i & ~(uint32_t)(FS_TILE - 1);
  uint32_t cnt = tiles[i / (uint32_t)FS_TILE];  // (i == m on a tile boundary reads the total behind the last tile)
  for (; off + 16u <= i; off += 16u) {
    const uint4 v = *reinterpret_cast<const uint4*>(gone + off);
    cnt += fs_zero_bytes(v.x) + fs_zero_bytes(v.y) + fs_zero_bytes(v.z) + fs_zero_bytes(v.w);
  }
  for (; off < i; ++off) cnt += gone[off] == 0 ? 1u : 0u;
  return cnt;
}
// tiles[t] = open points before tile t, tiles[tiles of m] = *live = all of them: one pass over the bytes
static int level_live_counts(swz_ctx* c, const uint8_t* gone, uint32_t m, const uint32_t** tiles_out, uint32_t* live) {
  ProfScope ps(c, "level_live_count", (uint64_t)m, 1);
  const uint32_t nb = div_up(m, FS_TILE);
  uint32_t* tiles = nullptr;
  SWZ_TRY(c->get("lvl_gone_tiles", (size_t)nb + 1, &tiles));
  hipLaunchKernelGGL(fscan_partial_zero_bytes_kernel, dim3(div_up(nb, (uint32_t)(FS_THREADS / 32))), dim3(FS_THREADS), 0, c->stream, gone,
                     m, nb, tiles);
  SWZ_LAUNCH_CHECK(c);
  SWZ_TRY(scan_exclusive_u32(c, tiles, tiles, nb, tiles + nb, "gone"));
  SWZ_TRY(read_u32(c, tiles + nb, live));
  *tiles_out = tiles;
  return SWZ_OK;
}
// the compaction that ends a chain: every taken point gets the level its code stands for
struct CompactCodedG {
  const uint64_t* akey;
  const uint32_t* aidx;
  const uint8_t* gone;
  int8_t* level_out;
  uint64_t* okey;
  uint32_t* oidx;
  __device__ void operator()(uint32_t i, uint32_t excl, uint32_t keep) const {
    const uint32_t p = aidx ? aidx[i] : i;
    if (keep) {
      okey[excl] = akey[i];
      oidx[excl] = p;
    } else {
      level_out[p] = (int8_t)((int)gone[i] - 2);
    }
  }
};

// tile_node / tile_internal_node decisions per node: terminal nodes and nodes with <= max_points
// points (SamplingBehaviour::TakeAllWhenCountBelowMaxPoints, Sampling.h:201-208) keep everything.
__global__ __launch_bounds__(256) void node_mode_kernel(const uint32_t* __restrict__ nstart,
                                                        uint8_t* __restrict__ nmode, uint32_t* __restrict__ counters,
                                                        uint64_t max_points, int force_sample, int terminal,
                                                        int reroot, const uint64_t* __restrict__ akey, uint32_t nsh,
                                                        const uint64_t* __restrict__ ckey, uint32_t nc,
                                                        const uint8_t* __restrict__ gone, const uint32_t* __restrict__ gone_tiles) {
  // grid-stride over the nodes: their number is only known on the device, and it is small next to the points
  const uint32_t nnodes = counters[CTR_NUM_NODES];
  for (uint32_t j = blockIdx.x * 256 + threadIdx.x; j < nnodes; j += gridDim.x * 256u) {
    uint32_t cnt = nstart[j + 1] - nstart[j];
    if (gone) {
      // the arrays still hold the points taken further up: a node is what it holds of OPEN points, and one that holds none
      // does not exist -- its entry stays in the table as a take-all node with nothing to take and is counted nowhere
      cnt = live_before(gone, gone_tiles, nstart[j + 1]) - live_before(gone, gone_tiles, nstart[j]);
      if (cnt == 0u) {
        nmode[j] = MODE_TAKE_ALL;
        continue;
      }
      atomicAdd(&counters[CTR_LIVE_NODES], 1u);
    }
    bool cached = false;  // previously_taken_points_count > 0 (TilingAlgorithms.cpp:272-275)
    if (nc) {
      const uint64_t prefix = akey[nstart[j]] >> nsh;
      uint32_t lo = 0, hi = nc;
      while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if ((ckey[mid] >> nsh) < prefix) lo = mid + 1; else hi = mid;
      }
      cached = lo < nc && (ckey[lo] >> nsh) == prefix;
    }
    const bool sample = !terminal && (force_sample || cached || (uint64_t)cnt > max_points);
    nmode[j] = sample ? MODE_SAMPLE : MODE_TAKE_ALL;
    if (sample) {
      if (reroot) atomicMax(&counters[CTR_ERROR], (uint32_t)SWZ_ERR_REROOT_UNSUPPORTED);
      atomicAdd(&counters[CTR_SAMPLE_NODES], 1u);
      atomicAdd(&counters[CTR_SAMPLE_POINTS], cnt);
    }
  }
}

// MIN_DISTANCE: the points of take-all nodes (the grid samplers flag them in their own pass)
__global__ __launch_bounds__(256) void take_all_kernel(uint32_t m, const uint32_t* __restrict__ nid,
                                                       const uint8_t* __restrict__ nmode,
                                                       uint8_t* __restrict__ taken, uint8_t code, int open_only) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= m) return;
  // (open_only: the bytes of points taken further up hold those levels' codes, ActiveSet::gone)
  if (nmode[nid[i]] == MODE_TAKE_ALL && !(open_only && taken[i])) taken[i] = code;
}

// ----------------------------------------------------------------------------- host: level plans
// candidate_level_in_octree -- Sampling.h:210-229 (std::log2f on the double ratio narrowed to float)
static int candidate_level_host(double root_extent_x, float spacing_at_root, int node_level) {
  const auto spacing_at_this_node = spacing_at_root / std::pow(2, node_level + 1);
  return std::max(-1, (int)std::floor(std::log2f(root_extent_x / spacing_at_this_node)) - 1);
}
// get_node_level_to_sample_from / first_node_level_obeying_spacing -- core/tiling/Node.cpp:37-57
static int node_level_to_sample_from_host(double root_extent_x, float root_max_spacing, int node_level) {
  const auto spacing_at_target_node = root_max_spacing / std::pow(2, node_level + 1);
  const float target_spacing = (float)spacing_at_target_node;
  return std::max(-1, (int)std::floor(std::log2f(root_extent_x / target_spacing)) - 1);
}
static uint32_t prev_pow2_host(uint32_t x) {
  x = x | (x >> 1);
  x = x | (x >> 2);
  x = x | (x >> 4);
  x = x | (x >> 8);
  x = x | (x >> 16);
  return x - (x >> 1);
}
// required_morton_index_depth -- core/tiling/Sampling.cpp:29-62
int required_depth_host(int sampler, int node_level, double root_extent_x, float root_max_spacing) {
  switch (sampler) {
    case SWZ_RANDOM_GRID:
    case SWZ_GRID_CENTER:
      return node_level_to_sample_from_host(root_extent_x, root_max_spacing, node_level);
    case SWZ_MIN_DISTANCE:
    case SWZ_MIN_DISTANCE_FAST:  // (Sampling.cpp:45-47)
      return node_level;
    default: {
      const auto spacing_at_this_node = root_max_spacing / std::pow(2, node_level + 1);
      const auto perfect_cell_count = (root_extent_x / std::pow(2, node_level + 1)) / spacing_at_this_node;
      const double clamped = perfect_cell_count >= 4294967295.0 ? 4294967295.0 : perfect_cell_count;
      const auto actual_cell_count = prev_pow2_host(static_cast<uint32_t>(clamped));
      const uint32_t levels = static_cast<uint32_t>(std::log2(actual_cell_count));
      return static_cast<int32_t>(static_cast<uint32_t>(node_level + levels));
    }
  }
}

}  // namespace swz
extern "C" int32_t swz_required_morton_index_depth(int sampler, int32_t node_level, const double root_min[3],
                                                   const double root_max[3], float spacing_at_root) {
  if (!root_min || !root_max) return INT32_MIN;
  return swz::required_depth_host(sampler, node_level, root_max[0] - root_min[0], spacing_at_root);
}
namespace swz {

LevelPlan make_plan(int level, int sampler, uint64_t max_points, float spacing_at_root, uint32_t max_depth,
                           const double bmin[3], const double bmax[3], bool force_sample, bool tiler_rules) {
  LevelPlan p;
  p.level = level;
  p.node_shift = level < 0 ? 63u : level_shift(level);
  p.sampler = sampler;
  p.max_points = max_points;
  p.force_sample = force_sample;
  p.root = Box{bmin[0], bmin[1], bmin[2], bmax[0], bmax[1], bmax[2]};
  const double ext_x = bmax[0] - bmin[0];
  if (tiler_rules) {
    // tile_node, TilingAlgorithms.cpp:408-444
    const int req = required_depth_host(sampler, level, ext_x, spacing_at_root);
    const bool deeper = req > level;
    const int max_level = (int)std::min<uint32_t>(MAX_LEVELS - 1, max_depth);
    if (!deeper) {
      p.terminal = req >= max_level;
    } else {
      p.terminal = level >= max_level;
      p.reroot = !p.terminal && req >= (int)MAX_LEVELS;
    }
  }
  p.cand = candidate_level_host(ext_x, spacing_at_root, level);
  p.spacing_node = spacing_at_root / std::pow(2, level + 1);
  p.jitter_start = (3u * static_cast<uint32_t>(level + 1)) % 16u;
  const float sf = static_cast<float>(p.spacing_node);  // PoissonDiskSampling, Sampling.h:448-449
  const float sq = sf * sf;                             // SparseGrid::SparseGrid, SparseGrid.cpp:13
  p.sq_spacing = (double)sq;                            // widened at the compare, GridCell.cpp:44,52
  // finest subdivision of a node whose cells are still at least one spacing wide on every axis (with
  // a 2^-20 relative margin so that quantisation of the key never lets two points closer than the
  // spacing sit in non-adjacent cells); node extent / spacing is the same at every level
  double min_ext = std::min(bmax[0] - bmin[0], std::min(bmax[1] - bmin[1], bmax[2] - bmin[2]));
  const double need = (double)spacing_at_root * (1.0 + 0x1.0p-20);
  int mg = 0;
  while (mg < 20 && min_ext / 2 >= need) {
    min_ext /= 2;
    ++mg;
  }
  p.cell_levels_geo = std::min(mg, 20 - level);
  return p;
}

bool level_decides_on_keys(const swz_ctx* c, const LevelPlan& plan, const SortedPoints& sp) {
  if (plan.sampler == SWZ_RANDOM_GRID) return true;
  if (greedy_sampler(plan.sampler)) return min_distance_level_uses_keys(c, plan, sp);
  return grid_level_uses_keys(c, plan, sp);
}

// what a kernel of the level raised in CTR_ERROR, in words
const char* level_error_message(int code) {
  switch (code) {
    case SWZ_ERR_JITTER_GRID_TOO_SMALL: return "Grids smaller than 16x16 are not supported currently!";
    case SWZ_ERR_JITTER_NODE_TOO_DEEP: return "node is too small to be sampled with JITTERED";
    case SWZ_ERR_REROOT_UNSUPPORTED: return "a node needs Morton re-rooting, which this call's per-point outputs cannot express: use swz_tile_nodes_begin_device / _end_device (one batch as node files) or a swz_tiler";
    case SWZ_ERR_INTERNAL: return "level segmentation inconsistent, or a MIN_DISTANCE sweep / a peer shard failed";
    default: return "a kernel of the level raised an error";
  }
}

// ----------------------------------------------------------------------------- one level
// Samples every node of the level.  When okey/oidx are given the survivors are compacted into them
// and level_out receives plan.level for the taken points; otherwise only lb.taken is produced.
int level_step(swz_ctx* c, const LevelPlan& plan, const ActiveSet& as, const SortedPoints& sp,
                      const LevelBuffers& lb, int8_t* level_out, uint64_t* okey, uint32_t* oidx,
                      LevelResult* res, const LevelChain* chain) {
  const uint32_t m = as.m;
  const uint32_t nb = div_up(m, 256);
  // inside a chain: lb.taken IS as.gone and holds the codes of the levels above
  const bool shared = as.gone != nullptr;
  if (shared && !(as.gone == lb.taken && as.gone_tiles && as.parent_prefix && as.parents && m > 0 && plan.node_shift < 63u &&
                  plan.sampler == SWZ_MIN_DISTANCE && !plan.md_property && !as.ckey && okey && !c->opt("SWZ_LEVEL_NODES_SCAN"))) {
    res->needs_flush = true;
    return SWZ_OK;
  }
  SWZ_HIP(c, hipMemsetAsync(lb.counters, 0, CTR_COUNT * sizeof(uint32_t), c->stream));
  {  // ---- segment the nodes
    ProfScope ps(c, "level_nodes", (uint64_t)m * 8ull, 3);
    bool fill_after_modes = false;
    if (plan.node_shift >= 63u && m > 0) {
      // the root (Morton keys have 63 bits): one node, nothing to segment -- two passes over the keys saved
      // (node ids: zeros -- unless the one node is going to be sampled and the sampler is one that then never looks, see
      // node_fill_kernel)
      const bool sampled_for_sure = !plan.terminal && (plan.force_sample || (uint64_t)m > plan.max_points);
      if (greedy_sampler(plan.sampler) || !sampled_for_sure)
        SWZ_HIP(c, hipMemsetAsync(lb.nid, 0, (size_t)m * sizeof(uint32_t), c->stream));
      hipLaunchKernelGGL(single_node_kernel, dim3(1), dim3(1), 0, c->stream, lb.nstart, lb.counters + CTR_NUM_NODES, m);
      SWZ_LAUNCH_CHECK(c);
    } else if (as.parent_prefix && as.parents && m > 0 && !c->opt("SWZ_LEVEL_NODES_SCAN")) {
      uint32_t* cb = nullptr;
      SWZ_TRY(c->get("lvl_child_bounds", (size_t)as.parents * 9u, &cb));
      hipLaunchKernelGGL(node_child_bounds_kernel, dim3(div_up(as.parents * 16u, 256u)), dim3(256), 0, c->stream, as.akey, m,
                         plan.node_shift, as.parent_prefix, as.parents, cb);
      SWZ_LAUNCH_CHECK(c);
      SWZ_TRY(fused_scan(c, ChildExistsF{cb, as.parents, m, lb.counters}, ChildStartG{cb, lb.nstart}, as.parents * 8u,
                         lb.counters + CTR_NUM_NODES, "lvl"));
      fill_after_modes = true;
    } else {
      SWZ_TRY(fused_scan(c, NodeHeadF{as.akey, plan.node_shift}, NodeAssignG{lb.nid, lb.nstart, m}, m,
                         lb.counters + CTR_NUM_NODES, "lvl"));
    }
    hipLaunchKernelGGL(node_mode_kernel, dim3(std::min(nb, 2048u)), dim3(256), 0, c->stream, lb.nstart, lb.nmode, lb.counters,
                       plan.max_points, plan.force_sample ? 1 : 0, plan.terminal ? 1 : 0, plan.reroot ? 1 : 0, as.akey,
                       plan.node_shift, as.ckey, as.nc, as.gone, as.gone_tiles);
    SWZ_LAUNCH_CHECK(c);
    if (fill_after_modes) {  // the node id per point, from the node starts (MIN_DISTANCE reads it on every level)
      hipLaunchKernelGGL(node_fill_kernel, dim3(div_up(m, NF_TILE)), dim3(256), 0, c->stream, lb.nstart, lb.counters, m, lb.nid,
                         greedy_sampler(plan.sampler) ? 0 : 1);
      SWZ_LAUNCH_CHECK(c);
    }
  }

  // ---- sample: lb.taken of every point (the grid samplers flag the points of take-all nodes themselves)
  if (plan.sampler == SWZ_RANDOM_GRID) {
    SWZ_TRY(random_grid_level(c, plan, as, lb));
  } else if (plan.sampler == SWZ_GRID_CENTER || plan.sampler == SWZ_JITTERED) {
    SWZ_TRY(grid_level(c, plan, as, sp, lb));
  } else if (plan.sampler == SWZ_MIN_DISTANCE_FAST && plan.cand < 0) {
    // AdaptivePoissonDiskSampling, Sampling.h:510-512: "just take the first point" of every sampled node, no sweep
    SWZ_TRY(random_grid_level(c, plan, as, lb));
  } else {  // MIN_DISTANCE; MIN_DISTANCE_FAST: the same on every n-th point of a node
    if (!shared) SWZ_HIP(c, hipMemsetAsync(lb.taken, 0, m, c->stream));
    uint32_t h[CTR_COUNT];
    SWZ_HIP(c, hipMemcpyAsync(h, lb.counters, sizeof(h), hipMemcpyDeviceToHost, c->stream));
    SWZ_HIP(c, hipStreamSynchronize(c->stream));
    if (h[CTR_ERROR]) return c->fail((int)h[CTR_ERROR], level_error_message((int)h[CTR_ERROR]));
    // only levels that have take-all nodes pay for the pass
    const bool take_all = h[CTR_SAMPLE_NODES] < (shared ? h[CTR_LIVE_NODES] : h[CTR_NUM_NODES]);
    // (inside a chain after the sampler: it may still hand the level back untouched, and the two write disjoint nodes)
    if (take_all && !shared) {
      hipLaunchKernelGGL(take_all_kernel, dim3(nb), dim3(256), 0, c->stream, m, lb.nid, lb.nmode, lb.taken, plan.take_code, 0);
      SWZ_LAUNCH_CHECK(c);
    }
    const uint32_t stride = plan.sampler == SWZ_MIN_DISTANCE_FAST ? (uint32_t)swz_min_distance_fast_stride(plan.level) : 1u;
    if (h[CTR_SAMPLE_NODES] > 0 && stride > 1u) {
      SWZ_TRY(min_distance_fast_level(c, plan, as, sp, lb, stride, h[CTR_NUM_NODES], h[CTR_SAMPLE_NODES], &res->md_rounds));
    } else if (h[CTR_SAMPLE_NODES] > 0) {
      SWZ_TRY(min_distance_level(c, plan, as, sp, lb, h[CTR_NUM_NODES], h[CTR_SAMPLE_NODES], h[CTR_SAMPLE_POINTS],
                                 &res->md_rounds, &res->md_keys_direct, &res->needs_flush));
      if (res->needs_flush) {
        c->prof_collect();
        return SWZ_OK;
      }
    }
    if (take_all && shared) {
      hipLaunchKernelGGL(take_all_kernel, dim3(nb), dim3(256), 0, c->stream, m, lb.nid, lb.nmode, lb.taken, plan.take_code, 1);
      SWZ_LAUNCH_CHECK(c);
    }
  }

  // ---- the survivors: left where they are for the next level of the chain (lb.taken becomes its ActiveSet::gone), or compacted
  uint32_t live = 0;
  if (okey && chain && chain->may_defer && res->md_keys_direct) {
    SWZ_TRY(level_live_counts(c, lb.taken, m, &res->gone_tiles, &live));
    res->deferred = live > 0u && (double)(m - live) < chain->max_gone * (double)m;
  }
  if (okey && !res->deferred) {
    ProfScope ps(c, "level_compact", (uint64_t)m * 14ull, 2);
    if (shared)  // every level of the chain at once
      SWZ_TRY(fused_scan(c, KeepF{lb.taken}, CompactCodedG{as.akey, as.aidx, lb.taken, level_out, okey, oidx}, m,
                         lb.counters + CTR_REMAINING, "lvl"));
    else
      SWZ_TRY(fused_scan(c, KeepF{lb.taken}, CompactG{as.akey, as.aidx, (int8_t)plan.level, level_out, okey, oidx}, m,
                         lb.counters + CTR_REMAINING, "lvl"));
  }
  // ---- read the counters
  uint32_t h[CTR_COUNT];
  SWZ_HIP(c, hipMemcpyAsync(h, lb.counters, sizeof(h), hipMemcpyDeviceToHost, c->stream));
  SWZ_HIP(c, hipStreamSynchronize(c->stream));
  c->prof_collect();
  if (h[CTR_ERROR]) {
    const int code = (int)h[CTR_ERROR];
    return c->fail(code, level_error_message(code));
  }
  res->remaining = res->deferred ? live : h[CTR_REMAINING];
  res->num_nodes = shared ? h[CTR_LIVE_NODES] : h[CTR_NUM_NODES];
  res->table_nodes = h[CTR_NUM_NODES];
  res->node_prefix = nullptr;
  // ---- publish the node prefixes
  // (all entries of the table: the children of a node without an open point hold none either and drop out the same way)
  if (okey && res->remaining && res->table_nodes) {  // for the next level's segmentation (two buffers: the one of the level above is still read)
    uint64_t* np = nullptr;
    SWZ_TRY(c->get((plan.level & 1) ? "lvl_node_prefix_1" : "lvl_node_prefix_0", (size_t)res->table_nodes, &np));
    hipLaunchKernelGGL(node_prefix_kernel, dim3(div_up(res->table_nodes, 256)), dim3(256), 0, c->stream, lb.nstart, as.akey,
                       plan.node_shift, res->table_nodes, np);
    SWZ_LAUNCH_CHECK(c);
    res->node_prefix = np;
  }
  return SWZ_OK;
}

int level_flush_chain(swz_ctx* c, const ActiveSet& as, const LevelBuffers& lb, int8_t* level_out, uint64_t* okey, uint32_t* oidx,
                      uint32_t* remaining) {
  ProfScope ps(c, "level_compact", (uint64_t)as.m * 14ull, 2);
  SWZ_TRY(fused_scan(c, KeepF{as.gone}, CompactCodedG{as.akey, as.aidx, as.gone, level_out, okey, oidx}, as.m, lb.counters + CTR_REMAINING,
                     "lvl"));
  return read_u32(c, lb.counters + CTR_REMAINING, remaining);
}

int alloc_level_buffers(swz_ctx* c, uint32_t m, LevelBuffers* lb) {
  SWZ_TRY(c->get("lvl_flags", (size_t)m, &lb->flags));
  SWZ_TRY(c->get("lvl_nid", (size_t)m, &lb->nid));
  SWZ_TRY(c->get("lvl_nstart", (size_t)m + 1, &lb->nstart));
  SWZ_TRY(c->get("lvl_nmode", (size_t)m, &lb->nmode));
  SWZ_TRY(c->get("lvl_taken", (size_t)m, &lb->taken));
  SWZ_TRY(c->get("lvl_counters", (size_t)CTR_COUNT, &lb->counters));
  return SWZ_OK;
}

}  // namespace swz
