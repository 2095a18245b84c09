// swz_grid.hip -- the three grid samplers of a level: RANDOM_GRID (K4a), GRID_CENTER (K4b) and JITTERED (K4d).
//
// A sampling-grid cell is a run of equal key prefix inside a node's run of the Morton-sorted active set (swz_level.hip).
// RANDOM_GRID takes the first point of every run.  GRID_CENTER and JITTERED take the point nearest to a target inside
// the cell, a segmented arg-min: on key coordinates where the level allows it (the exact positions only for the runs the
// keys cannot decide), on positions in Morton order otherwise.  level_step hands a level to random_grid_level or
// grid_level; which kernels sample it, with which tables, is decided here.
#include <algorithm>
#include <cmath>

#include "swz_level.h"

namespace swz {

#define SWZ_JITTER_TABLE(W) __constant__ uint8_t PERMUTATIONS_##W[16 * W]
#include "jitter_tables.inc"
#undef SWZ_JITTER_TABLE

__device__ __forceinline__ uint32_t spos_of(const uint32_t* aidx, uint32_t i) { return aidx ? aidx[i] : i; }

// ----------------------------------------------------------------------------- RANDOM_GRID (K4a)
// RandomSortedGridSampling::sample_points, Sampling.h:187-308: the first point of every run of equal
// truncate_to_level(candidate_level) is taken.  candidate_level == -1 takes the first point only.
// (when every node of the level is sampled -- the counters of node_mode_kernel say so -- nobody looks at nid / nmode)
// Four consecutive points per thread: two 16-byte key loads and ONE 4-byte store of the four flags (a wavefront's byte
// stores fill 64 bytes of a line each).
constexpr uint32_t RG_IPT = 4;
__global__ __launch_bounds__(256) void random_grid_kernel(const uint64_t* __restrict__ akey, uint32_t m,
                                                          const uint32_t* __restrict__ nid,
                                                          const uint8_t* __restrict__ nmode, uint32_t csh,
                                                          uint8_t* __restrict__ taken, const uint32_t* __restrict__ counters) {
  const uint64_t i0 = ((uint64_t)blockIdx.x * 256 + threadIdx.x) * RG_IPT;
  if (i0 >= m) return;
  const bool all_sampled = counters[CTR_SAMPLE_NODES] == counters[CTR_NUM_NODES];
  if (i0 + RG_IPT <= m) {
    const ulonglong2 ka = *reinterpret_cast<const ulonglong2*>(akey + i0);
    const ulonglong2 kb = *reinterpret_cast<const ulonglong2*>(akey + i0 + 2);
    const uint64_t prev = i0 ? akey[i0 - 1] : 0ull;
    const uint64_t k[RG_IPT + 1] = {prev >> csh, ka.x >> csh, ka.y >> csh, kb.x >> csh, kb.y >> csh};
    uint32_t packed = 0;
#pragma unroll
    for (uint32_t j = 0; j < RG_IPT; ++j) {
      uint32_t t = 1;
      if (all_sampled || nmode[nid[i0 + j]] == MODE_SAMPLE) t = (i0 + j == 0) || (k[j + 1] != k[j]);
      packed |= t << (8u * j);
    }
    *reinterpret_cast<uint32_t*>(taken + i0) = packed;
    return;
  }
  for (uint64_t i = i0; i < m; ++i) {  // the last thread's partial group
    uint8_t t = 1;
    if (all_sampled || nmode[nid[i]] == MODE_SAMPLE) t = (i == 0) || ((akey[i] >> csh) != (akey[i - 1] >> csh));
    taken[i] = t;
  }
}

// ----------------------------------------------------------------------------- GRID_CENTER / JITTERED (K4b, K4d)
// Both pick, per run of equal grid-cell prefix, the first point with the smallest squared distance
// to a per-cell target (std::min_element, Sampling.h:392-403 / :741-750): a segmented arg-min.
#ifndef SWZ_GA_THREADS
#define SWZ_GA_THREADS 256
#endif
#ifndef SWZ_GA_IPT
#define SWZ_GA_IPT 2
#endif
constexpr int GA_THREADS = SWZ_GA_THREADS;
constexpr int GA_IPT = SWZ_GA_IPT;
constexpr int GA_TILE = GA_THREADS * GA_IPT;
// the kernel that decides on keys (grid_argmin_keys_kernel) takes four points per thread: its loads are the keys alone, and
// the segmented scan across the lanes -- a third of its instructions -- is paid per thread (measured at 1 B points,
// GRID_CENTER / JITTERED sampling per step: 26.0 / 27.9 ms with two, 24.0 / 23.5 ms with four)
#ifndef SWZ_GAK_IPT
#define SWZ_GAK_IPT 4
#endif
constexpr int GAK_IPT = SWZ_GAK_IPT;
constexpr int GAK_TILE = GA_THREADS * GAK_IPT;
constexpr uint32_t NONE = 0xFFFFFFFFu;

struct Agg {
  double d;    // smallest squared distance since the last run start (or since the range began)
  uint32_t i;  // active index of the first point attaining it
  uint32_t f;  // 1 when a run start lies inside the covered range
};
__device__ __forceinline__ bool agg_less(double d1, uint32_t i1, double d2, uint32_t i2) {
  return d1 < d2 || (d1 == d2 && i1 < i2);
}
__device__ __forceinline__ Agg agg_combine(Agg a, Agg b) {  // a covers earlier points than b
  const bool take_b = b.f != 0 || agg_less(b.d, b.i, a.d, a.i);  // selects only: no branches, nothing on the stack
  Agg r;
  r.d = take_b ? b.d : a.d;
  r.i = take_b ? b.i : a.i;
  r.f = a.f | b.f;
  return r;
}
__device__ __forceinline__ Agg agg_shfl_up(Agg a, int delta) {
  Agg r;
  r.d = __shfl_up(a.d, delta, WAVE);
  r.i = __shfl_up(a.i, delta, WAVE);
  r.f = __shfl_up(a.f, delta, WAVE);
  return r;
}
// One step of the wave's inclusive scan over DPP: the aggregate of the lanes the control word names (the identity
// where it names none) combined in front of the lane's own.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ Agg agg_dpp_step(Agg v) {
  const uint64_t db = (uint64_t)__double_as_longlong(v.d);
  const uint64_t inf = 0x7FF0000000000000ull;
  const uint32_t lo = (uint32_t)__builtin_amdgcn_update_dpp((int)(uint32_t)inf, (int)(uint32_t)db, CTRL, ROW_MASK, 0xF, false);
  const uint32_t hi =
    (uint32_t)__builtin_amdgcn_update_dpp((int)(uint32_t)(inf >> 32), (int)(uint32_t)(db >> 32), CTRL, ROW_MASK, 0xF, false);
  Agg o;
  o.d = __longlong_as_double((long long)(((uint64_t)hi << 32) | lo));
  o.i = (uint32_t)__builtin_amdgcn_update_dpp((int)0xFFFFFFFFu, (int)v.i, CTRL, ROW_MASK, 0xF, false);
  o.f = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v.f, CTRL, ROW_MASK, 0xF, false);
  return agg_combine(o, v);
}
__device__ __forceinline__ Agg agg_wave_incl_scan(Agg v) {
  v = agg_dpp_step<0x111, 0xF>(v);  // row_shr:1
  v = agg_dpp_step<0x112, 0xF>(v);  // row_shr:2
  v = agg_dpp_step<0x114, 0xF>(v);  // row_shr:4
  v = agg_dpp_step<0x118, 0xF>(v);  // row_shr:8
  v = agg_dpp_step<0x142, 0xA>(v);  // row_bcast:15 -> rows 1, 3
  v = agg_dpp_step<0x143, 0xC>(v);  // row_bcast:31 -> rows 2, 3
  return v;
}

struct TileSummary {
  double head_d;  // leading partial run (continues a run of the previous tile), if the first point is no start
  double tail_d;  // trailing run that starts in this tile and continues into the next one
  uint32_t head_i;
  uint32_t tail_i;
  uint32_t has_start;  // some run starts inside this tile
  uint32_t last_open;  // the last run continues into the next tile
};

struct GridParams {
  Box root;
  int level;              // node level
  int sampler;            // SWZ_GRID_CENTER or SWZ_JITTERED
  int cand;               // GRID_CENTER candidate level (>= 0 here)
  double spacing_node;    // JITTERED
  uint32_t jitter_start;  // JITTERED
  // bounds of every octree cell at depth table_depth, indexed by the key's first table_depth octants (0: no table).
  // The points of a cell all walk the same halving chain; its first table_depth steps are looked up instead (the
  // table is small enough to stay in the caches, and neighbouring lanes read the same entry).
  const Box* box_table;
  int table_depth;
  const struct JitNode* jit_table;  // JITTERED: what the sampler derives from a node's bounds, per node prefix (or null)
};
// JitteredSampling's per-node quantities (Sampling.h:621-668): every point of a node derives the same ones
struct alignas(16) JitNode {
  double minx, miny, minz;  // the node's bounds_from_key minimum
  double cell_size, perm_size;
  uint32_t cells, levels;
  int32_t err;  // SWZ_ERR_JITTER_* or 0
  uint32_t pad;
};
constexpr int GRID_TABLE_MAX_DEPTH = 6;  // 8^6 boxes of 48 bytes = 12.6 MB (deeper tables were measured: no faster)
__global__ __launch_bounds__(256) void grid_box_table_kernel(Box root, int depth, Box* __restrict__ table) {
  const uint32_t t = blockIdx.x * 256 + threadIdx.x;
  if (t >= (1u << (3 * depth))) return;
  table[t] = bounds_from_key((uint64_t)t << level_shift(depth - 1), root, depth);
}

// get_prev_power_of_two -- core/util/stuff.cpp:340-349
__device__ __forceinline__ uint32_t prev_pow2(uint32_t x) {
  x = x | (x >> 1);
  x = x | (x >> 2);
  x = x | (x >> 4);
  x = x | (x >> 8);
  x = x | (x >> 16);
  return x - (x >> 1);
}

// Depth of the bounds chain a point's target starts from: the candidate cell (GRID_CENTER) or the node (JITTERED).
__device__ __forceinline__ int cell_box_depth(const GridParams& g) {
  return g.sampler == SWZ_GRID_CENTER ? g.cand + 1 : g.level + 1;
}
// GridCenterSampling, Sampling.h:387-390: centre of kb = get_bounds_from_morton_index(key, root, cand + 1)
__device__ __forceinline__ void grid_center_target(const Box& kb, double& tx, double& ty, double& tz) {
  tx = kb.minx + (kb.maxx - kb.minx) / 2;  // AABB::getCenter, AABB.h:70
  ty = kb.miny + (kb.maxy - kb.miny) / 2;
  tz = kb.minz + (kb.maxz - kb.minz) / 2;
}
// JitteredSampling, Sampling.h:621-668: the grid of a node with bounds nb = bounds_from_key(key, root, level + 1)
__device__ __forceinline__ JitNode jitter_node(const Box& nb, double spacing_node, int level) {
  JitNode n;
  n.minx = nb.minx;
  n.miny = nb.miny;
  n.minz = nb.minz;
  n.pad = 0;
  n.err = 0;
  const double ext_x = nb.maxx - nb.minx;
  const double perfect = ext_x / spacing_node;
  const uint32_t perfect_u = perfect >= 4294967295.0 ? 4294967295u : (uint32_t)perfect;
  n.cells = prev_pow2(perfect_u);
  n.levels = n.cells ? 31u - (uint32_t)__clz((int)n.cells) : 0u;  // (uint32_t)std::log2(power of two)
  if (n.cells < 16) n.err = SWZ_ERR_JITTER_GRID_TOO_SMALL;
  else if ((uint32_t)level + n.levels >= MAX_LEVELS) n.err = SWZ_ERR_JITTER_NODE_TOO_DEEP;
  // ext_x / cells and cell_size / cells: cells = 2^levels, so the quotients are the scaled operands (ldexp rounds a
  // result that underflows once, like the division)
  n.cell_size = ldexp(ext_x, -(int)n.levels);
  n.perm_size = ldexp(n.cell_size, -(int)n.levels);
  return n;
}
// Sampling.h:669-739: cell prefix shift and jittered target of the grid cell `key` falls in (n.err == 0)
__device__ __forceinline__ void jitter_target(const GridParams& g, uint64_t key, const JitNode& n, uint32_t& csh, double& tx,
                                              double& ty, double& tz) {
  const uint32_t cells = n.cells, levels = n.levels;
  csh = level_shift((int)((uint32_t)g.level + levels));
  const uint64_t rel = (key >> csh) & ((1ull << (3u * levels)) - 1ull);
  const uint64_t mask = (1ull << levels) - 1ull;
  uint32_t gx, gy, gz;  // OctreeNodeIndex64::to_grid_index, OctreeNodeIndex.h:357-363 (below 2^levels <= 2^20)
  if (levels <= 10u) {  // the usual case (grids up to 1024 cells a side): rel has at most 30 bits, half the instructions
    const uint32_t r = (uint32_t)rel, m32 = (uint32_t)mask;
    gz = contract_bits_by_3_u32(r) & m32;
    gy = contract_bits_by_3_u32(r >> 1) & m32;
    gx = contract_bits_by_3_u32(r >> 2) & m32;
  } else {
    gz = (uint32_t)(contract_bits_by_3(rel) & mask);
    gy = (uint32_t)(contract_bits_by_3(rel >> 1) & mask);
    gx = (uint32_t)(contract_bits_by_3(rel >> 2) & mask);
  }
  const uint8_t* table;
  uint32_t width;
  if (cells <= 16) {
    table = PERMUTATIONS_16;
    width = 16;
  } else if (cells <= 32) {
    table = PERMUTATIONS_32;
    width = 32;
  } else {
    table = PERMUTATIONS_64;
    width = 64;
  }
  // length of the permutation in use: min(cells, 64), a power of two like cells -- "% plen" is a mask (the 64-bit
  // remainder the expression would otherwise compile to costs more than the rest of the function).  (The three rows in
  // use copied to LDS instead of three dependent byte loads from memory: measured, no faster.)
  const uint32_t plen_mask = (cells < 64 ? cells : 64) - 1u;
  const uint32_t s0 = g.jitter_start, s1 = (g.jitter_start + 1) % 16, s2 = (g.jitter_start + 2) % 16;
  const uint32_t px = (uint32_t)table[s0 * width + ((gy + gz) & plen_mask)] - 1u;
  const uint32_t py = (uint32_t)table[s1 * width + ((gx + gz) & plen_mask)] - 1u;
  const uint32_t pz = (uint32_t)table[s2 * width + ((gx + gy) & plen_mask)] - 1u;
  tx = n.minx + ((double)gx * n.cell_size + (double)px * n.perm_size);
  ty = n.miny + ((double)gy * n.cell_size + (double)py * n.perm_size);
  tz = n.minz + ((double)gz * n.cell_size + (double)pz * n.perm_size);
}
__global__ __launch_bounds__(256) void jitter_node_table_kernel(Box root, int level, double spacing_node,
                                                                JitNode* __restrict__ table) {
  const uint32_t t = blockIdx.x * 256 + threadIdx.x;
  if (t >= (1u << (3 * (level + 1)))) return;
  const Box nb = level < 0 ? root : bounds_from_key((uint64_t)t << level_shift(level), root, level + 1);
  table[t] = jitter_node(nb, spacing_node, level);
}

#ifndef SWZ_GA_MINW
#define SWZ_GA_MINW 1
#endif
__global__ __launch_bounds__(GA_THREADS, SWZ_GA_MINW) void grid_argmin_kernel(
  const uint64_t* __restrict__ akey, const uint32_t* __restrict__ aidx, uint32_t m, const uint32_t* __restrict__ nid,
  const uint8_t* __restrict__ nmode, const double* __restrict__ X, const double* __restrict__ Y,
  const double* __restrict__ Z, GridParams g, uint32_t node_shift, uint8_t* __restrict__ taken,
  TileSummary* __restrict__ summaries, uint32_t* __restrict__ counters) {
  __shared__ Agg wave_tot[GA_THREADS / WAVE];
  const uint32_t tid = threadIdx.x, w = tid / WAVE, l = lane_id();
  const uint32_t tile_base = blockIdx.x * GA_TILE;
  const uint32_t tile_end = (m - tile_base) < (uint32_t)GA_TILE ? m : tile_base + GA_TILE;
  const uint32_t last_valid = tile_end - 1;
  const uint32_t first = tile_base + tid * GA_IPT;
  const bool all_sampled = counters[CTR_SAMPLE_NODES] == counters[CTR_NUM_NODES];  // then nobody looks at nid / nmode

  // Every load an item needs is issued before the arithmetic starts: the bounds chain below is a loop of dependent
  // f64 operations, and the loads of the next item must not queue up behind it.
  uint64_t key[GA_IPT];
  uint32_t spos[GA_IPT];
  bool sample[GA_IPT];
  double px[GA_IPT], py[GA_IPT], pz[GA_IPT];
  uint64_t prev_key = 0;
  bool have_prev = false;
  if (first < tile_end && first > 0) {
    prev_key = akey[first - 1];
    have_prev = true;
  }
  if (GA_IPT == 2 && first + 2 <= tile_end) {  // the usual case: two-item vector loads
    const ulonglong2 k2 = *reinterpret_cast<const ulonglong2*>(akey + first);
    key[0] = k2.x;
    key[GA_IPT - 1] = k2.y;
    if (aidx) {
      const uint2 p2 = *reinterpret_cast<const uint2*>(aidx + first);
      spos[0] = p2.x;
      spos[GA_IPT - 1] = p2.y;
    } else {
      spos[0] = first;
      spos[GA_IPT - 1] = first + 1;
    }
  } else {
#pragma unroll
    for (int j = 0; j < GA_IPT; ++j) {
      const uint32_t gc = first + j < tile_end ? first + j : last_valid;
      key[j] = akey[gc];
      spos[j] = spos_of(aidx, gc);
    }
  }
#pragma unroll
  for (int j = 0; j < GA_IPT; ++j) {
    const uint32_t gc = first + j < tile_end ? first + j : last_valid;
    sample[j] = all_sampled || nmode[nid[gc]] == MODE_SAMPLE;
  }
  if (GA_IPT == 2 && first + 2 <= tile_end && !aidx) {
    const double2 x2 = *reinterpret_cast<const double2*>(X + first);
    const double2 y2 = *reinterpret_cast<const double2*>(Y + first);
    const double2 z2 = *reinterpret_cast<const double2*>(Z + first);
    px[0] = x2.x, px[GA_IPT - 1] = x2.y;
    py[0] = y2.x, py[GA_IPT - 1] = y2.y;
    pz[0] = z2.x, pz[GA_IPT - 1] = z2.y;
  } else {
#pragma unroll
    for (int j = 0; j < GA_IPT; ++j) {
      px[j] = X[spos[j]];
      py[j] = Y[spos[j]];
      pz[j] = Z[spos[j]];
    }
  }
  Box kb[GA_IPT];
  JitNode jn[GA_IPT];
  if (g.jit_table) {  // JITTERED with a table: nothing of the node is computed here
    const uint32_t tsh = g.level < 0 ? 63u : level_shift(g.level);
#pragma unroll
    for (int j = 0; j < GA_IPT; ++j) jn[j] = g.jit_table[key[j] >> tsh];
  } else {
    if (g.table_depth > 0) {
      const uint32_t tsh = level_shift(g.table_depth - 1);
#pragma unroll
      for (int j = 0; j < GA_IPT; ++j) kb[j] = g.box_table[key[j] >> tsh];
    } else {
#pragma unroll
      for (int j = 0; j < GA_IPT; ++j) kb[j] = g.root;
    }
    bounds_from_keys<GA_IPT>(key, g.table_depth, cell_box_depth(g), kb);
    if (g.sampler != SWZ_GRID_CENTER) {
#pragma unroll
      for (int j = 0; j < GA_IPT; ++j) jn[j] = jitter_node(kb[j], g.spacing_node, g.level);
    }
  }

  double dist[GA_IPT];
  bool head[GA_IPT];
  uint32_t last_csh = node_shift;  // shift of the last valid item (for the last_open test)
  uint64_t last_key = 0;
  bool any_head = false;
#pragma unroll
  for (int j = 0; j < GA_IPT; ++j) {
    const uint32_t gi = first + j;
    dist[j] = __builtin_inf();
    head[j] = false;
    if (gi < tile_end) {
      uint32_t csh = node_shift;
      if (sample[j]) {
        double tx = 0, ty = 0, tz = 0;
        int err = 0;
        if (g.sampler == SWZ_GRID_CENTER) {
          csh = level_shift(g.cand);
          grid_center_target(kb[j], tx, ty, tz);
        } else {
          err = jn[j].err;
          if (!err) jitter_target(g, key[j], jn[j], csh, tx, ty, tz);
        }
        if (err) {
          atomicMax(&counters[CTR_ERROR], (uint32_t)err);
          csh = node_shift;
        } else {
          dist[j] = sq_dist(px[j], py[j], pz[j], tx, ty, tz);
        }
      } else {
        taken[gi] = 1;  // take-all node
      }
      head[j] = !have_prev || ((key[j] >> csh) != (prev_key >> csh));
      any_head |= head[j];
      prev_key = key[j];
      have_prev = true;
      last_csh = csh;
      last_key = key[j];
    }
  }

  // thread aggregate over its items, then block-wide exclusive segmented scan
  Agg a{__builtin_inf(), NONE, 0};
#pragma unroll
  for (int j = 0; j < GA_IPT; ++j) {
    const uint32_t gi = first + j;
    if (gi < tile_end) {
      if (head[j]) {
        a.d = dist[j];
        a.i = gi;
        a.f = 1;
      } else if (agg_less(dist[j], gi, a.d, a.i)) {
        a.d = dist[j];
        a.i = gi;
      }
    }
  }
  const Agg incl = agg_wave_incl_scan(a);
  if (l == WAVE - 1) wave_tot[w] = incl;
  const Agg up = agg_shfl_up(incl, 1);
  Agg excl;
  excl.d = l == 0 ? __builtin_inf() : up.d;
  excl.i = l == 0 ? NONE : up.i;
  excl.f = l == 0 ? 0u : up.f;
  const int tile_has_start = __syncthreads_or(any_head ? 1 : 0);
  Agg carry{__builtin_inf(), NONE, 0};
#pragma unroll
  for (uint32_t i = 0; i + 1 < (uint32_t)(GA_THREADS / WAVE); ++i) {
    const Agg t = wave_tot[i];
    const Agg cc = agg_combine(carry, t);
    carry.d = i < w ? cc.d : carry.d;
    carry.i = i < w ? cc.i : carry.i;
    carry.f = i < w ? cc.f : carry.f;
  }
  carry = agg_combine(carry, excl);

  // second pass: close runs, emit winners / partial aggregates
  bool started = carry.f != 0;
  double rd = carry.d;
  uint32_t ri = carry.i;
  TileSummary* sum = &summaries[blockIdx.x];
#pragma unroll
  for (int j = 0; j < GA_IPT; ++j) {
    const uint32_t gi = first + j;
    if (gi < tile_end) {
      if (head[j]) {
        if (gi != tile_base) {  // the run ending at gi-1 closes inside this tile
          if (started) {
            if (ri != NONE) taken[ri] = 1;
          } else {
            sum->head_d = rd;
            sum->head_i = ri;
          }
        }
        rd = dist[j];
        ri = gi;
        started = true;
      } else if (agg_less(dist[j], gi, rd, ri)) {
        rd = dist[j];
        ri = gi;
      }
      if (gi == last_valid) {
        const bool last_open = (tile_end < m) && ((akey[tile_end] >> last_csh) == (last_key >> last_csh));
        if (!last_open) {
          if (started) {
            if (ri != NONE) taken[ri] = 1;
          } else {
            sum->head_d = rd;
            sum->head_i = ri;
          }
        } else if (started) {
          sum->tail_d = rd;
          sum->tail_i = ri;
        } else {
          sum->head_d = rd;
          sum->head_i = ri;
        }
        sum->has_start = (uint32_t)tile_has_start;
        sum->last_open = last_open ? 1u : 0u;
      }
    }
  }
}

// runs that cross tile borders: the thread of the tile in which the run starts walks forward
__global__ __launch_bounds__(256) void grid_resolve_kernel(const TileSummary* __restrict__ summaries,
                                                           uint32_t ntiles, uint8_t* __restrict__ taken) {
  const uint32_t t = blockIdx.x * 256 + threadIdx.x;
  if (t >= ntiles) return;
  const TileSummary s = summaries[t];
  if (!(s.has_start && s.last_open)) return;
  double d = s.tail_d;
  uint32_t i = s.tail_i;
  for (uint32_t u = t + 1; u < ntiles; ++u) {
    const TileSummary h = summaries[u];
    if (agg_less(h.head_d, h.head_i, d, i)) {
      d = h.head_d;
      i = h.head_i;
    }
    if (h.has_start || !h.last_open) break;
  }
  if (i != NONE) taken[i] = 1;
}

// ----------------------------------------------------------------------------- GRID_CENTER / JITTERED on key coordinates
// The arg-min above reads every point's position (24 bytes, in Morton order: a gather of the whole batch after the sort).
// But the Morton key IS the position, quantised to 2^-21 of the bounds per axis (calculate_morton_index,
// OctreeAlgorithms.h:64-87): a point with key coordinate i lies in [i, i + 1] key cells, so its distance to a target is
// known to +- half a cell per axis from the key alone.  Per grid cell the kernel below keeps the point with the smallest
// UPPER bound of that distance, that point's lower bound, and the smallest lower bound among all the others: when even
// that exceeds the leader's upper bound the leader is the arg-min whatever the exact positions are (and the first one:
// equal distances would overlap).  Otherwise -- two points whose distances to the target differ by less than the
// quantisation -- the run goes on a list and a second kernel repeats it with the reference's own arithmetic (target from
// the halving chain of the bounds, sq_dist in double on the ORIGINAL positions, read through the permutation;
// Sampling.h:387-403 / :741-750).  No position is moved; runs of one point (most runs of the deeper levels) never need it.
// hk = 0.5 + slack: the slack covers the rounding of the encoder's (p - min) * scale (1e-9 cells) and the difference
// between the ideal target and the reference's, computed from bounds that went through up to 21 halvings (make_grid_keys).
struct KAgg {
  float ub, lb;    // leader: upper / lower bound of its squared distance (in units of the widest key cell, squared)
  float m2;        // smallest lower bound among the run's other points
  uint32_t i;      // leader (first one with the smallest upper bound)
  uint32_t start;  // the run's first point, NONE when it lies before the covered range
  uint32_t f;      // 1 when a run start lies inside the covered range
};
__device__ __forceinline__ KAgg kagg_combine(KAgg a, KAgg b) {  // a covers earlier points than b; selects only
  const bool bwin = b.ub < a.ub || (b.ub == a.ub && b.i < a.i);
  const bool bf = b.f != 0;
  const float l_lb = bwin ? a.lb : b.lb;
  KAgg r;
  r.ub = (bf || bwin) ? b.ub : a.ub;
  r.lb = (bf || bwin) ? b.lb : a.lb;
  r.i = (bf || bwin) ? b.i : a.i;
  r.m2 = bf ? b.m2 : fminf(fminf(a.m2, b.m2), l_lb);
  r.start = bf ? b.start : a.start;
  r.f = a.f | b.f;
  return r;
}
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ KAgg kagg_dpp_step(KAgg v) {
  const int inf = 0x7F800000;
  KAgg o;
  o.ub = __int_as_float(__builtin_amdgcn_update_dpp(inf, __float_as_int(v.ub), CTRL, ROW_MASK, 0xF, false));
  o.lb = __int_as_float(__builtin_amdgcn_update_dpp(inf, __float_as_int(v.lb), CTRL, ROW_MASK, 0xF, false));
  o.m2 = __int_as_float(__builtin_amdgcn_update_dpp(inf, __float_as_int(v.m2), CTRL, ROW_MASK, 0xF, false));
  o.i = (uint32_t)__builtin_amdgcn_update_dpp((int)0xFFFFFFFFu, (int)v.i, CTRL, ROW_MASK, 0xF, false);
  o.start = (uint32_t)__builtin_amdgcn_update_dpp((int)0xFFFFFFFFu, (int)v.start, CTRL, ROW_MASK, 0xF, false);
  o.f = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v.f, CTRL, ROW_MASK, 0xF, false);
  return kagg_combine(o, v);
}
__device__ __forceinline__ KAgg kagg_wave_incl_scan(KAgg v) {
  v = kagg_dpp_step<0x111, 0xF>(v);
  v = kagg_dpp_step<0x112, 0xF>(v);
  v = kagg_dpp_step<0x114, 0xF>(v);
  v = kagg_dpp_step<0x118, 0xF>(v);
  v = kagg_dpp_step<0x142, 0xA>(v);
  v = kagg_dpp_step<0x143, 0xC>(v);
  return v;
}
__device__ __forceinline__ KAgg kagg_identity() { return KAgg{__builtin_inff(), __builtin_inff(), __builtin_inff(), NONE, NONE, 0u}; }

struct KTileSummary {
  KAgg head;          // leading partial run (continues a run of the previous tile), if the first point is no start
  KAgg tail;          // trailing run that starts in this tile and continues into the next one (tail.start: where)
  uint32_t head_end;  // where the leading partial run ends: the tile's first run start, or the tile's end
  uint32_t has_start;
  uint32_t last_open;
  uint32_t pad;
};

struct GridKeys {
  float w[3];   // key cell width per axis relative to the widest one
  double hk;    // half a key cell plus the slack (see above)
  // the same for the kernel's single-precision bounds, rounded to the safe side: hk up, the widths down for the lower and
  // up for the upper bound (grid_argmin_keys_kernel)
  float hk_f, w_lo[3], w_hi[3];
  uint2* amb;   // runs the keys cannot decide: {first, end} active index
  uint32_t* amb_count;
};

// a run is closed: the leader is taken, or the run goes to the exact pass
__device__ __forceinline__ void kagg_close(const KAgg& r, uint32_t end, const GridKeys& gk, uint8_t* __restrict__ taken) {
  if (r.i == NONE) return;
  if (r.m2 <= r.ub && r.ub < __builtin_inff()) {
    const uint32_t at = atomicAdd(gk.amb_count, 1u);
    gk.amb[at] = make_uint2(r.start, end);
  } else {
    taken[r.i] = 1;
  }
}

__global__ __launch_bounds__(GA_THREADS) void grid_argmin_keys_kernel(
  const uint64_t* __restrict__ akey, uint32_t m, const uint32_t* __restrict__ nid, const uint8_t* __restrict__ nmode, GridParams g,
  GridKeys gk, uint32_t node_shift, uint8_t* __restrict__ taken, KTileSummary* __restrict__ summaries, uint32_t* __restrict__ counters) {
  __shared__ KAgg wave_tot[GA_THREADS / WAVE];
  const uint32_t tid = threadIdx.x, w = tid / WAVE, l = lane_id();
  const uint32_t tile_base = blockIdx.x * GAK_TILE;
  const uint32_t tile_end = (m - tile_base) < (uint32_t)GAK_TILE ? m : tile_base + GAK_TILE;
  const uint32_t last_valid = tile_end - 1;
  const uint32_t first = tile_base + tid * GAK_IPT;
  const bool all_sampled = counters[CTR_SAMPLE_NODES] == counters[CTR_NUM_NODES];

  uint64_t key[GAK_IPT];
  bool sample[GAK_IPT];
  uint64_t prev_key = 0;
  bool have_prev = false;
  if (first < tile_end && first > 0) {
    prev_key = akey[first - 1];
    have_prev = true;
  }
#pragma unroll
  for (int j = 0; j < GAK_IPT; ++j) {
    const uint32_t gc = first + j < tile_end ? first + j : last_valid;
    key[j] = akey[gc];
    sample[j] = all_sampled || nmode[nid[gc]] == MODE_SAMPLE;
  }
  JitNode jn[GAK_IPT];
  if (g.sampler != SWZ_GRID_CENTER) {  // what JITTERED derives from the node's box: grid size, levels, error (as above)
    if (g.jit_table) {
      const uint32_t tsh = g.level < 0 ? 63u : level_shift(g.level);
#pragma unroll
      for (int j = 0; j < GAK_IPT; ++j) jn[j] = g.jit_table[key[j] >> tsh];
    } else {
      Box kb[GAK_IPT];
      if (g.table_depth > 0) {
        const uint32_t tsh = level_shift(g.table_depth - 1);
#pragma unroll
        for (int j = 0; j < GAK_IPT; ++j) kb[j] = g.box_table[key[j] >> tsh];
      } else {
#pragma unroll
        for (int j = 0; j < GAK_IPT; ++j) kb[j] = g.root;
      }
      bounds_from_keys<GAK_IPT>(key, g.table_depth, g.level + 1, kb);
#pragma unroll
      for (int j = 0; j < GAK_IPT; ++j) jn[j] = jitter_node(kb[j], g.spacing_node, g.level);
    }
  }

  float ub[GAK_IPT], lb[GAK_IPT];
  bool head[GAK_IPT];
  uint32_t last_csh = node_shift;
  uint64_t last_key = 0;
  bool any_head = false;
#pragma unroll
  for (int j = 0; j < GAK_IPT; ++j) {
    const uint32_t gi = first + j;
    ub[j] = __builtin_inff();
    lb[j] = __builtin_inff();
    head[j] = false;
    if (gi < tile_end) {
      uint32_t csh = node_shift;
      if (sample[j]) {
        int err = 0;
        // Offset of the point's key cell centre from the target, per axis, in key cells -- in single precision, exactly:
        // a half-integer below 2^21 (GRID_CENTER), or a multiple of the permutation step 2^(sbits - levels) >= 2^-6 below
        // 2^sbits with levels <= 6 (JITTERED): at most 22 significant bits either way.
        float ox = 0.f, oy = 0.f, oz = 0.f;
        uint32_t ix, iy, iz;
        key_coords_u32(key[j], ix, iy, iz);
        if (g.sampler == SWZ_GRID_CENTER) {
          csh = level_shift(g.cand);
          const uint32_t sbits = csh / 3u, mask = (1u << sbits) - 1u;
          const float half = ldexpf(1.0f, (int)sbits - 1);  // (0.5 for a cell one key cell wide)
          ox = (float)(ix & mask) + 0.5f - half;
          oy = (float)(iy & mask) + 0.5f - half;
          oz = (float)(iz & mask) + 0.5f - half;
        } else {
          err = jn[j].err;
          if (!err) {
            const uint32_t levels = jn[j].levels, cells = jn[j].cells;
            csh = level_shift((int)((uint32_t)g.level + levels));
            const uint32_t sbits = csh / 3u, mask = (1u << sbits) - 1u, gmask = cells - 1u;
            const uint32_t gx = (ix >> sbits) & gmask, gy = (iy >> sbits) & gmask, gz = (iz >> sbits) & gmask;  // to_grid_index
            const uint8_t* table;
            uint32_t width;
            if (cells <= 16) {
              table = PERMUTATIONS_16;
              width = 16;
            } else if (cells <= 32) {
              table = PERMUTATIONS_32;
              width = 32;
            } else {
              table = PERMUTATIONS_64;
              width = 64;
            }
            const uint32_t plen_mask = (cells < 64 ? cells : 64) - 1u;
            const uint32_t s0 = g.jitter_start, s1 = (g.jitter_start + 1) % 16, s2 = (g.jitter_start + 2) % 16;
            const uint32_t px = (uint32_t)table[s0 * width + ((gy + gz) & plen_mask)] - 1u;
            const uint32_t py = (uint32_t)table[s1 * width + ((gx + gz) & plen_mask)] - 1u;
            const uint32_t pz = (uint32_t)table[s2 * width + ((gx + gy) & plen_mask)] - 1u;
            const float perm = ldexpf(1.0f, (int)sbits - (int)levels);  // perm_size = cell_size / cells, in key cells
            ox = (float)(ix & mask) + 0.5f - (float)px * perm;
            oy = (float)(iy & mask) + 0.5f - (float)py * perm;
            oz = (float)(iz & mask) + 0.5f - (float)pz * perm;
          }
        }
        if (err) {
          atomicMax(&counters[CTR_ERROR], (uint32_t)err);
          csh = node_shift;
        } else {
          // Bounds of the squared distance, rounded outwards.  hk_f >= hk and w_lo <= w <= w_hi are rounded to the safe side
          // already; what is left are the roundings of this arithmetic on non-negative terms -- the sum / difference with
          // hk_f, the product with the width, the square, two additions: five at 2^-24 relative each along any path --, which
          // the factors 1 -+ 2^-20 cover several times over.  (Until round 4 this ran in double: half the rate and twice the
          // registers for bounds that end up as floats.)
          const float ax = fabsf(ox), ay = fabsf(oy), az = fabsf(oz);
          const float lx = fmaxf(ax - gk.hk_f, 0.f) * gk.w_lo[0], ly = fmaxf(ay - gk.hk_f, 0.f) * gk.w_lo[1], lz = fmaxf(az - gk.hk_f, 0.f) * gk.w_lo[2];
          const float ux = (ax + gk.hk_f) * gk.w_hi[0], uy = (ay + gk.hk_f) * gk.w_hi[1], uz = (az + gk.hk_f) * gk.w_hi[2];
          lb[j] = (lx * lx + ly * ly + lz * lz) * (1.0f - 0x1.0p-20f);
          ub[j] = (ux * ux + uy * uy + uz * uz) * (1.0f + 0x1.0p-20f);
        }
      } else {
        taken[gi] = 1;  // take-all node
      }
      head[j] = !have_prev || ((key[j] >> csh) != (prev_key >> csh));
      any_head |= head[j];
      prev_key = key[j];
      have_prev = true;
      last_csh = csh;
      last_key = key[j];
    }
  }

  // thread aggregate over its items, then block-wide exclusive segmented scan
  KAgg a = kagg_identity();
#pragma unroll
  for (int j = 0; j < GAK_IPT; ++j) {
    const uint32_t gi = first + j;
    if (gi < tile_end) {
      KAgg it{ub[j], lb[j], __builtin_inff(), gi, head[j] ? gi : NONE, head[j] ? 1u : 0u};
      a = kagg_combine(a, it);
    }
  }
  const KAgg incl = kagg_wave_incl_scan(a);
  if (l == WAVE - 1) wave_tot[w] = incl;
  KAgg excl;
  excl.ub = __shfl_up(incl.ub, 1, WAVE);
  excl.lb = __shfl_up(incl.lb, 1, WAVE);
  excl.m2 = __shfl_up(incl.m2, 1, WAVE);
  excl.i = __shfl_up(incl.i, 1, WAVE);
  excl.start = __shfl_up(incl.start, 1, WAVE);
  excl.f = __shfl_up(incl.f, 1, WAVE);
  if (l == 0) excl = kagg_identity();
  const int tile_has_start = __syncthreads_or(any_head ? 1 : 0);
  KAgg carry = kagg_identity();
#pragma unroll
  for (uint32_t i = 0; i + 1 < (uint32_t)(GA_THREADS / WAVE); ++i) {
    const KAgg cc = kagg_combine(carry, wave_tot[i]);
    if (i < w) carry = cc;
  }
  carry = kagg_combine(carry, excl);

  // second pass: close runs, emit winners / undecided runs / partial aggregates
  KAgg run = carry;
  KTileSummary* sum = &summaries[blockIdx.x];
#pragma unroll
  for (int j = 0; j < GAK_IPT; ++j) {
    const uint32_t gi = first + j;
    if (gi < tile_end) {
      if (head[j] && gi != tile_base) {  // the run ending at gi - 1 closes inside this tile
        if (run.f) {
          kagg_close(run, gi, gk, taken);
        } else {
          sum->head = run;
          sum->head_end = gi;
        }
      }
      KAgg it{ub[j], lb[j], __builtin_inff(), gi, head[j] ? gi : NONE, head[j] ? 1u : 0u};
      run = kagg_combine(run, it);
      if (gi == last_valid) {
        const bool last_open = (tile_end < m) && ((akey[tile_end] >> last_csh) == (last_key >> last_csh));
        if (!last_open) {
          if (run.f) {
            kagg_close(run, tile_end, gk, taken);
          } else {
            sum->head = run;
            sum->head_end = tile_end;
          }
        } else if (run.f) {
          sum->tail = run;
        } else {
          sum->head = run;
          sum->head_end = tile_end;
        }
        sum->has_start = (uint32_t)tile_has_start;
        sum->last_open = last_open ? 1u : 0u;
      }
    }
  }
}

// runs that cross tile borders: the thread of the tile in which the run starts walks forward
__global__ __launch_bounds__(256) void grid_resolve_keys_kernel(const KTileSummary* __restrict__ summaries, uint32_t ntiles, GridKeys gk,
                                                                uint8_t* __restrict__ taken) {
  const uint32_t t = blockIdx.x * 256 + threadIdx.x;
  if (t >= ntiles) return;
  if (!(summaries[t].has_start && summaries[t].last_open)) return;
  KAgg run = summaries[t].tail;
  uint32_t end = 0;
  for (uint32_t u = t + 1; u < ntiles; ++u) {
    const KAgg h = summaries[u].head;  // (no run start inside: it continues this run)
    run = kagg_combine(run, h);
    end = summaries[u].head_end;
    if (summaries[u].has_start || !summaries[u].last_open) break;
  }
  kagg_close(run, end, gk, taken);
}

// the runs the keys could not decide, one wavefront each, with the reference's arithmetic on the original positions
__global__ __launch_bounds__(256) void grid_exact_runs_kernel(const uint64_t* __restrict__ akey, const uint32_t* __restrict__ aidx,
                                                              SortedPoints sp, GridParams g, GridKeys gk, uint8_t* __restrict__ taken) {
  const uint32_t l = lane_id();
  const uint32_t nruns = *gk.amb_count;
  for (uint32_t r = blockIdx.x * (256u / WAVE) + threadIdx.x / WAVE; r < nruns; r += gridDim.x * (256u / WAVE)) {
    const uint2 se = gk.amb[r];
    double best = __builtin_inf();
    uint32_t besti = NONE;
    for (uint32_t i = se.x + l; i < se.y; i += WAVE) {
      const uint64_t key = akey[i];
      const double* pp = sorted_point_xyz(sp.xyz, sp.perm, sp.ghost_xyz, sp.ghosts, aidx ? aidx[i] : i);
      const double px = pp[0], py = pp[1], pz = pp[2];
      const Box kb = bounds_from_key(key, g.root, cell_box_depth(g));
      double tx = 0, ty = 0, tz = 0;
      if (g.sampler == SWZ_GRID_CENTER) {
        grid_center_target(kb, tx, ty, tz);
      } else {
        const JitNode n = jitter_node(kb, g.spacing_node, g.level);
        uint32_t csh;
        jitter_target(g, key, n, csh, tx, ty, tz);
      }
      const double d = sq_dist(px, py, pz, tx, ty, tz);
      if (agg_less(d, i, best, besti)) {
        best = d;
        besti = i;
      }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      const double od = __shfl_xor(best, off, WAVE);
      const uint32_t oi = (uint32_t)__shfl_xor((int)besti, off, WAVE);
      if (agg_less(od, oi, best, besti)) {
        best = od;
        besti = oi;
      }
    }
    if (l == 0 && besti != NONE) taken[besti] = 1;
  }
}

// ----------------------------------------------------------------------------- host
// GRID_CENTER / JITTERED: can this level be decided on key coordinates, and with which bounds?  Needs the original
// positions and the permutation for the undecided runs; JITTERED additionally cubic bounds (its grid cells are cubes of the
// node's x-extent along every axis, Sampling.h:621-668: with other bounds its targets do not sit where the key cells put them).
// SWZ_GRID_KEYS=0 switches it off; SWZ_GRID_KEYS_SLACK adds to the slack (tests: a huge one sends every run of more than
// one point through the exact pass, a negative one must change results).
static bool make_grid_keys(const swz_ctx* c, const LevelPlan& plan, const SortedPoints& sp, GridKeys& gk) {
  if (plan.sampler != SWZ_GRID_CENTER && plan.sampler != SWZ_JITTERED) return false;
  if (!sp.xyz || !sp.perm) return false;
  if (!c->opt_on("SWZ_GRID_KEYS", true)) return false;
  const double ext[3] = {plan.root.maxx - plan.root.minx, plan.root.maxy - plan.root.miny, plan.root.maxz - plan.root.minz};
  if (!(ext[0] > 0.0) || !(ext[1] > 0.0) || !(ext[2] > 0.0)) return false;
  if (plan.sampler == SWZ_JITTERED && !(ext[0] == ext[1] && ext[1] == ext[2])) return false;
  const double wmax = std::max(ext[0], std::max(ext[1], ext[2])), wmin = std::min(ext[0], std::min(ext[1], ext[2]));
  const double max_abs = std::max(std::max(std::max(std::fabs(plan.root.minx), std::fabs(plan.root.maxx)),
                                           std::max(std::fabs(plan.root.miny), std::fabs(plan.root.maxy))),
                                  std::max(std::fabs(plan.root.minz), std::fabs(plan.root.maxz)));
  // The reference's target comes out of bounds that went through up to 21 halvings and a few more operations, each
  // rounding at the magnitude of the coordinates: 128 ulp of the largest one, in key cells of the narrowest axis; plus
  // the rounding of the encoder's (p - min) * scale.
  double slack = 1e-6 + 128.0 * 0x1.0p-52 * max_abs / (wmin / 2097152.0);
  slack += c->opt_num("SWZ_GRID_KEYS_SLACK", 0.0);
  if (!(slack < 0.25) && !c->opt("SWZ_GRID_KEYS_SLACK")) return false;  // bounds far from the origin relative to their size
  for (int a = 0; a < 3; ++a) {
    gk.w[a] = (float)(ext[a] / wmax);
    const double wd = ext[a] / wmax;
    float lo = (float)wd, hi = (float)wd;
    if ((double)lo > wd) lo = std::nextafterf(lo, 0.f);
    if ((double)hi < wd) hi = std::nextafterf(hi, INFINITY);
    gk.w_lo[a] = lo;
    gk.w_hi[a] = hi;
  }
  gk.hk = 0.5 + slack;
  gk.hk_f = (float)gk.hk;
  if ((double)gk.hk_f < gk.hk) gk.hk_f = std::nextafterf(gk.hk_f, INFINITY);
  gk.amb = nullptr;
  gk.amb_count = nullptr;
  return true;
}
bool grid_level_uses_keys(const swz_ctx* c, const LevelPlan& plan, const SortedPoints& sp) {
  GridKeys gk;
  return make_grid_keys(c, plan, sp, gk);
}

int random_grid_level(swz_ctx* c, const LevelPlan& plan, const ActiveSet& as, const LevelBuffers& lb) {
  // candidate level -1: "just take the first point" (Sampling.h:290-298, :346-348)
  const bool first_only = plan.cand < 0;
  const uint32_t csh = first_only ? plan.node_shift : level_shift(plan.cand);
  if (!first_only && plan.cand >= (int)MAX_LEVELS) return c->fail(SWZ_ERR_REROOT_UNSUPPORTED, level_error_message(SWZ_ERR_REROOT_UNSUPPORTED));
  const uint32_t m = as.m;
  ProfScope ps(c, "sample_random_grid", (uint64_t)m * 9ull);
  hipLaunchKernelGGL(random_grid_kernel, dim3(div_up(m, 256u * RG_IPT)), dim3(256), 0, c->stream, as.akey, m, lb.nid, lb.nmode, csh,
                     lb.taken, lb.counters);
  SWZ_LAUNCH_CHECK(c);
  return SWZ_OK;
}

// All but the last three steps of the bounds chain from a table (worth it from a few thousand points per entry on);
// JITTERED on a shallow level instead one entry per node prefix: the node's box and everything the sampler derives from it.
static int grid_tables(swz_ctx* c, const LevelPlan& plan, uint32_t m, GridParams& g) {
  const int chain = plan.sampler == SWZ_GRID_CENTER ? plan.cand + 1 : plan.level + 1;
  int td = std::min(chain - 3, GRID_TABLE_MAX_DEPTH);
  td = std::min(std::min((int)c->opt_int("SWZ_GRID_TABLE_DEPTH", td), chain), GRID_TABLE_MAX_DEPTH);
  while (td > 0 && ((uint64_t)1 << (3 * td)) * 64u > (uint64_t)m) --td;
  if (plan.sampler == SWZ_JITTERED && chain <= GRID_TABLE_MAX_DEPTH && c->opt_on("SWZ_JITTER_TABLE", true)) {
    JitNode* d_nodes = nullptr;
    const uint32_t entries = 1u << (3 * chain);
    SWZ_TRY(c->get("grid_jitter_nodes", (size_t)entries, &d_nodes));
    hipLaunchKernelGGL(jitter_node_table_kernel, dim3(div_up(entries, 256)), dim3(256), 0, c->stream, plan.root, plan.level,
                       plan.spacing_node, d_nodes);
    SWZ_LAUNCH_CHECK(c);
    g.jit_table = d_nodes;
    td = 0;
  }
  if (td > 0) {
    Box* d_table = nullptr;
    SWZ_TRY(c->get("grid_boxes", (size_t)1 << (3 * td), &d_table));
    hipLaunchKernelGGL(grid_box_table_kernel, dim3(div_up(1u << (3 * td), 256)), dim3(256), 0, c->stream, plan.root, td, d_table);
    SWZ_LAUNCH_CHECK(c);
    g.box_table = d_table;
    g.table_depth = td;
  }
  return SWZ_OK;
}

int grid_level(swz_ctx* c, const LevelPlan& plan, const ActiveSet& as, const SortedPoints& sp, const LevelBuffers& lb) {
  if (plan.sampler == SWZ_GRID_CENTER && plan.cand < 0) return random_grid_level(c, plan, as, lb);  // the first point only
  if (plan.sampler == SWZ_GRID_CENTER && plan.cand >= (int)MAX_LEVELS)
    return c->fail(SWZ_ERR_REROOT_UNSUPPORTED, level_error_message(SWZ_ERR_REROOT_UNSUPPORTED));
  const uint32_t m = as.m;
  const uint32_t ntiles = div_up(m, GA_TILE);
  TileSummary* d_sum = nullptr;
  SWZ_TRY(c->get("grid_summaries", (size_t)ntiles, &d_sum));
  SWZ_HIP(c, hipMemsetAsync(lb.taken, 0, m, c->stream));
  GridParams g;
  g.root = plan.root;
  g.level = plan.level;
  g.sampler = plan.sampler;
  g.cand = plan.cand;
  g.spacing_node = plan.spacing_node;
  g.jitter_start = plan.jitter_start;
  g.box_table = nullptr;
  g.table_depth = 0;
  g.jit_table = nullptr;
  ProfScope ps(c, plan.sampler == SWZ_GRID_CENTER ? "sample_grid_center" : "sample_jittered", (uint64_t)m * 33ull, 2);
  SWZ_TRY(grid_tables(c, plan, m, g));
  GridKeys gk;
  if (make_grid_keys(c, plan, sp, gk)) {
    // decided on the key coordinates; the runs they cannot decide repeated on the original positions
    KTileSummary* d_ksum = nullptr;
    const uint32_t nktiles = div_up(m, GAK_TILE);
    SWZ_TRY(c->get("grid_key_summaries", (size_t)nktiles, &d_ksum));
    SWZ_TRY(c->get("grid_key_undecided", (size_t)m / 2 + 1024, &gk.amb));  // (a run of one point is always decided)
    gk.amb_count = lb.counters + CTR_NUM_CELLS;
    hipLaunchKernelGGL(grid_argmin_keys_kernel, dim3(nktiles), dim3(GA_THREADS), 0, c->stream, as.akey, m, lb.nid, lb.nmode, g, gk,
                       plan.node_shift, lb.taken, d_ksum, lb.counters);
    SWZ_LAUNCH_CHECK(c);
    hipLaunchKernelGGL(grid_resolve_keys_kernel, dim3(div_up(nktiles, 256)), dim3(256), 0, c->stream, d_ksum, nktiles, gk, lb.taken);
    SWZ_LAUNCH_CHECK(c);
    hipLaunchKernelGGL(grid_exact_runs_kernel, dim3(std::min<uint32_t>(div_up(m, 2048u), 4096u)), dim3(256), 0, c->stream, as.akey, as.aidx,
                       sp, g, gk, lb.taken);
    SWZ_LAUNCH_CHECK(c);
  } else {
    if (!sp.X) return c->fail(SWZ_ERR_INTERNAL, "GRID_CENTER / JITTERED: this level needs the positions in Morton order");
    hipLaunchKernelGGL(grid_argmin_kernel, dim3(ntiles), dim3(GA_THREADS), 0, c->stream, as.akey, as.aidx, m, lb.nid,
                       lb.nmode, sp.X, sp.Y, sp.Z, g, plan.node_shift, lb.taken, d_sum, lb.counters);
    SWZ_LAUNCH_CHECK(c);
    hipLaunchKernelGGL(grid_resolve_kernel, dim3(div_up(ntiles, 256)), dim3(256), 0, c->stream, d_sum, ntiles, lb.taken);
    SWZ_LAUNCH_CHECK(c);
  }
  return SWZ_OK;
}

}  // namespace swz
