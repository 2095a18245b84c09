// swz_mqbuild.hip -- the key sweep's tables (protocol: swz_mdkeys.hip): the cells of a level and their bounds, numbered
// directly or compacted, key coordinates and state bytes per point, the adjacent cells of every cell and the first
// round's queues, the list of dense cells -- the kernels and the host steps that launch them.
#include <algorithm>
#include <string>
#include <vector>

#include "swz_mdkeys.h"
#include "swz_scan.h"

namespace swz {

__device__ __forceinline__ uint64_t mq_pack(uint64_t key) {
  // octant = x << 2 | y << 1 | z (MortonIndex.h:62-79): bit 3j+2 of the key is bit j of x
  uint32_t x, y, z;
  key_coords_u32(key, x, y, z);
  return (uint64_t)x | ((uint64_t)y << 21) | ((uint64_t)z << 42);
}
__device__ __forceinline__ bool mq_is_head(const MqArgs& a, uint32_t i) {
  if (!a.all_sampled && a.nmode[a.nid[i]] != MODE_SAMPLE) return false;
  return i == 0 || ((a.akey[i] >> a.cell_shift) != (a.akey[i - 1] >> a.cell_shift));
}

// ----------------------------------------------------------------------------- build
__global__ __launch_bounds__(256) void mq_pack_kernel(const uint64_t* __restrict__ akey, uint32_t m, uint64_t* __restrict__ qpos,
                                                      uint8_t* __restrict__ state) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= m) return;
  qpos[i] = mq_pack(akey[i]);
  state[i] = QS_OPEN;
}

struct MqHeadF {
  MqArgs a;
  __device__ uint32_t operator()(uint32_t i) const { return mq_is_head(a, i) ? 1u : 0u; }
};
struct MqCellBuildG {
  MqArgs a;
  __device__ void operator()(uint32_t i, uint32_t c, uint32_t head) const {
    const uint64_t key = a.akey[i];  // (the scan's head functor has just read it: a cache hit)
    a.qpos[i] = mq_pack(key);
    a.state[i] = QS_OPEN;
    if (!head) return;
    a.cinfo[c].x = i;
    a.crel[c] = (uint32_t)((key >> a.cell_shift) & (a.cells_per_node - 1ull));
    a.csnode[c] = a.all_sampled ? a.nid[i] : a.snode_of[a.nid[i]];
  }
};

// Direct numbering: the cell of a point follows from its own key, so one pass over the keys builds everything per point and
// the bounds of every occupied cell -- no count, no scan.  A run of equal cell prefixes inside a sampled node is a cell
// (nodes are prefixes of cells: a run never crosses a node's end); its first point writes the start, its last one the end.
// cinfo has been zeroed: what no run touches stays {0, 0}, an empty cell.
// Four consecutive points per thread: 16-byte accesses (vec: the keys are 16-byte aligned; qpos / state always are), the
// state bytes of the four as one word.
__global__ __launch_bounds__(256) void mq_direct_build_kernel(MqArgs a, uint32_t vec) {
  const uint64_t i0 = ((uint64_t)blockIdx.x * 256u + threadIdx.x) * 4u;
  if (i0 >= a.m) return;
  const uint32_t n = a.m - i0 < 4u ? (uint32_t)(a.m - i0) : 4u;
  uint64_t key[6];  // [0]: the point in front of the four, [5]: the one behind them (cache hits)
  uint64_t q[4];
  if (vec && n == 4u) {
    const ulonglong2 v0 = *reinterpret_cast<const ulonglong2*>(a.akey + i0), v1 = *reinterpret_cast<const ulonglong2*>(a.akey + i0 + 2);
    key[1] = v0.x, key[2] = v0.y, key[3] = v1.x, key[4] = v1.y;
  } else {
#pragma unroll
    for (uint32_t j = 0; j < 4u; ++j) key[1 + j] = j < n ? a.akey[i0 + j] : 0ull;
  }
  key[0] = i0 ? a.akey[i0 - 1u] : 0ull;
  key[5] = i0 + 4u < a.m ? a.akey[i0 + 4u] : 0ull;
  if (!a.keep_qpos) {
#pragma unroll
    for (int j = 0; j < 4; ++j) q[j] = mq_pack(key[1 + j]);
  }
  if (n == 4u) {
    if (!a.keep_qpos) {
      ulonglong2 w0, w1;
      w0.x = q[0], w0.y = q[1], w1.x = q[2], w1.y = q[3];
      *reinterpret_cast<ulonglong2*>(a.qpos + i0) = w0;
      *reinterpret_cast<ulonglong2*>(a.qpos + i0 + 2) = w1;
    }
    uint32_t sw = 0x01010101u * (uint32_t)QS_OPEN;
    if (a.gone) {
      const uint32_t g = *reinterpret_cast<const uint32_t*>(a.gone + i0);
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if ((g >> (8 * j)) & 0xFFu) sw = (sw & ~(0xFFu << (8 * j))) | ((uint32_t)QS_DEAD << (8 * j));
    }
    *reinterpret_cast<uint32_t*>(a.state + i0) = sw;
  } else {
    for (uint32_t j = 0; j < n; ++j) {
      if (!a.keep_qpos) a.qpos[i0 + j] = q[j];
      a.state[i0 + j] = (a.gone && a.gone[i0 + j]) ? (uint8_t)QS_DEAD : (uint8_t)QS_OPEN;
    }
  }
#pragma unroll
  for (uint32_t j = 0; j < 4u; ++j) {
    if (j >= n) break;
    const uint32_t i = (uint32_t)i0 + j;
    const uint64_t pre = key[1 + j] >> a.cell_shift;
    const bool first = i == 0u || (key[j] >> a.cell_shift) != pre;
    const bool last = i + 1u == a.m || (key[2 + j] >> a.cell_shift) != pre;
    if (!first && !last) continue;
    const uint32_t node = a.nid[i];
    if (!a.all_sampled && a.nmode[node] != MODE_SAMPLE) continue;
    const uint64_t g = ((uint64_t)(a.all_sampled ? node : a.snode_of[node]) << a.cpn_shift) | (pre & (a.cells_per_node - 1ull));
    if (first) a.cinfo[g].x = i;
    if (last) a.cinfo[g].y = i + 1u;
  }
}

__global__ __launch_bounds__(256) void mq_cell_end_kernel(MqArgs a, uint32_t ncells) {
  const uint32_t c = blockIdx.x * 256 + threadIdx.x;
  if (c >= ncells) return;
  const uint32_t s = a.cinfo[c].x;
  const uint32_t node_end = a.nstart[a.nid[s] + 1];
  const uint32_t next = (c + 1 < ncells) ? a.cinfo[c + 1].x : a.m;
  const uint32_t e = next < node_end ? next : node_end;
  a.cinfo[c].y = e;
  a.gridmap[(uint64_t)a.csnode[c] * a.cells_per_node + a.crel[c]] = c;
  uint4* r = a.rec + ((size_t)c << a.rg2_shift);
  r[0] = make_uint4(s, 0u, 0u, e);
  r[a.rg] = make_uint4(s, 0u, 1u, e);
  a.qst[c] = make_uint4(QNONE, 0u, 0u, 0u);
}

// append `value` of every lane with want == true to the queue: one atomic per wavefront
__device__ __forceinline__ void mq_wave_push(bool want, uint32_t value, uint32_t* qout, uint32_t* cout) {
  const uint64_t m = __ballot(want);
  if (!m) return;
  const int leader = __ffsll((unsigned long long)m) - 1;
  uint32_t base = 0;
  if ((int)lane_id() == leader) base = atomicAdd(cout, (uint32_t)__popcll(m));
  base = __shfl(base, leader, WAVE);
  if (want) qout[base + (uint32_t)__popcll(m & lanemask_lt())] = value;
}

// where a level starts: the first round's queue of every node group
struct MqStart {
  uint32_t* queue[8];
  uint32_t* qctr[8];
  uint32_t groups;
  uint32_t lazy;
};

// The 26 adjacent cells by direction (codes by arithmetic on the dilated coordinates, as md_nbr_build_kernel does), 32
// lanes per cell -- and the start of the level, from the same lanes: not lazy, every cell is queued; lazy, only the
// cells without an earlier adjacent cell are, and every other cell sleeps on its latest earlier neighbour until that one
// has decided the given fraction of its points (sleeping on a cell that is not the real blocker is always safe: the cell
// looks again when it wakes up).
// Direct numbering: ncells counts the grid's entries.  The neighbour's id is the arithmetic alone, and it exists when its
// cinfo entry is not empty (a load whose address depends on no other load).  The same lanes write what the sweep expects to
// find of a new cell -- its two record headers and its stall state (mq_cell_end_kernel does that for compacted cells); an
// empty cell gets headers that read "at its end" and nothing else.
// the code of the cell adjacent to the one with code `rel` in direction k < 27 (k != 13) inside its node; false: the node ends there
__device__ __forceinline__ bool mq_adjacent_rel(const MqArgs& a, uint32_t rel, uint32_t k, uint32_t* nrel_out) {
  const uint32_t all = (uint32_t)(a.cells_per_node - 1ull);
  const uint32_t mz = all & 0x09249249u, my = mz << 1, mx = mz << 2;
  const uint32_t v[3] = {rel & mx, rel & my, rel & mz};
  const uint32_t mk[3] = {mx, my, mz};
  const uint32_t d[3] = {k / 9u, (k / 3u) % 3u, k % 3u};  // 0: minus one, 1: same, 2: plus one
  bool inside = true;
  uint32_t nrel = 0;
#pragma unroll
  for (int ax = 0; ax < 3; ++ax) {
    uint32_t w = v[ax];
    if (d[ax] == 0u) {
      inside &= w != 0u;
      w = (w - 1u) & mk[ax];
    } else if (d[ax] == 2u) {
      inside &= w != mk[ax];
      w = ((w | ~mk[ax]) + 1u) & mk[ax];
    }
    nrel |= w;
  }
  *nrel_out = nrel;
  return inside;
}

// The start of the level for lane k of cell c, whose adjacent cell in direction k is nb (every lane of the wavefront calls):
// the latest earlier adjacent cell of this shard (the maximum over the cell's 32 lanes), the sleeper's slot and stall, the
// first round's queues.  clear_qst: lane 2 of a cell that does not start asleep writes its empty stall state.
__device__ __forceinline__ void mq_start_cell(const MqArgs& a, const MqStart& st, uint64_t cbase, uint32_t c, uint32_t k, bool in, uint32_t nb,
                                              bool clear_qst) {
  uint32_t best = 0;  // id + 1
  if (st.lazy && in && k < 27u && nb != QNONE && (a.peers.shards <= 1u || (nb >> MQ_PEER_SHIFT) == 0u) && nb < c) best = nb + 1u;
  if (st.lazy) {
#pragma unroll
    for (int off = 16; off >= 1; off >>= 1) best = max(best, (uint32_t)__shfl_xor((int)best, off, 32));
    if (in && best && nb + 1u == best) {  // (the one lane that holds it: the ids of adjacent cells are distinct)
      const uint2 o = a.cinfo[best - 1u];
      const uint32_t bq = o.x + (uint32_t)((float)(o.y - 1u - o.x) * a.lazy_frac);
      a.slot[(size_t)(best - 1u) * 32 + (26u - k)] = (unsigned long long)bq;  // stamp 0: written before the first round
      a.qst[c] = make_uint4(a.cinfo[c].x, k, bq, 0u);
    }
  }
  if (clear_qst && k == 2u && best == 0u) a.qst[c] = make_uint4(QNONE, 0u, 0u, 0u);  // (a cell that starts asleep has its stall on record, above)
  const bool push = in && k == 13u && best == 0u;
  const uint32_t seg = (uint32_t)(cbase >> 3) & (a.nseg - 1u);  // (eight entries per step, spread evenly: a segment cannot overflow)
  if (st.groups == 1u) {
    mq_wave_push(push, c | MQ_WOKEN, st.queue[0] + (size_t)seg * a.segcap, st.qctr[0] + (size_t)seg * 32u);
  } else {
    const uint32_t g = push ? (a.direct ? c >> a.cpn_shift : a.csnode[c]) % st.groups : 0u;
    for (uint32_t gg = 0; gg < st.groups; ++gg)
      mq_wave_push(push && g == gg, c | MQ_WOKEN, st.queue[gg] + (size_t)seg * a.segcap, st.qctr[gg] + (size_t)seg * 32u);
  }
}

__global__ __launch_bounds__(256) void mq_nbr_build_kernel(MqArgs a, uint32_t ncells, MqStart st) {
  for (uint64_t cbase = (uint64_t)blockIdx.x * 8u; cbase < ncells; cbase += (uint64_t)gridDim.x * 8u) {
    const uint32_t c = (uint32_t)cbase + threadIdx.x / 32u;
    const uint32_t k = threadIdx.x & 31u;
    const bool in_grid = c < ncells;
    bool in = in_grid;
    if (a.direct && in_grid) {
      const uint2 ci = a.cinfo[c];
      if (k < 2u) a.rec[((size_t)c << a.rg2_shift) + k * a.rg] = make_uint4(ci.x, 0u, k, ci.y);
      in = ci.x != ci.y;
    }
    uint32_t nb = QNONE;
    if (in && k == 13u) {
      nb = c;
    } else if (in && k < 27u) {
      const uint32_t rel = a.direct ? (c & (uint32_t)(a.cells_per_node - 1ull)) : a.crel[c];
      uint32_t nrel = 0;
      if (mq_adjacent_rel(a, rel, k, &nrel)) {
        if (a.peers.shards > 1u) {
          // the root of a sharded batch: the cell code's first octant names the owner; cells of higher shards are later
          // ones, nobody here looks at them
          const uint32_t owner = (nrel >> (3u * (a.cell_levels - 1u))) * a.peers.shards / 8u;
          if (owner == a.peers.shard) {
            nb = a.gridmap[nrel];
          } else if (owner < a.peers.shard && a.peers.gridmap[owner]) {
            const uint32_t id = a.peers.gridmap[owner][nrel];
            if (id != QNONE) nb = ((owner + 1u) << MQ_PEER_SHIFT) | id;
          }
        } else if (a.direct) {
          const uint32_t g = (c - rel) | nrel;
          const uint2 cn = a.cinfo[g];
          if (cn.x != cn.y) nb = g;
        } else {
          nb = a.gridmap[(uint64_t)a.csnode[c] * a.cells_per_node + nrel];
        }
      }
    }
    if (in) a.qnbr[(size_t)c * 32 + k] = nb;
    mq_start_cell(a, st, cbase, c, k, in, nb, a.direct && in_grid);
  }
}

// ---- the same tables in two halves, for a level inside a chain whose grid is known before the level above has ended
// (DESIGN 4.1(d)).  EARLY: everything that follows from the raw keys, the cell size and the record size alone, under the
// guess that every node of the level exists and is sampled -- the node table is then the identity, a cell's id its key
// prefix.  LATE: what the level above decides (the state bytes) and what the survey decides (who starts asleep, the queues).
// Neither early kernel reads ActiveSet::gone, a state byte, a node mode or a count.
//
// Early 1: the bounds of every occupied cell (mq_direct_build_kernel's last loop); cinfo has been zeroed.
__global__ __launch_bounds__(256) void mq_cinfo_early_kernel(const uint64_t* __restrict__ akey, uint32_t m, uint32_t cell_shift, uint32_t ncells,
                                                             uint2* __restrict__ cinfo, uint32_t vec) {
  const uint64_t i0 = ((uint64_t)blockIdx.x * 256u + threadIdx.x) * 4u;
  if (i0 >= m) return;
  const uint32_t n = m - i0 < 4u ? (uint32_t)(m - i0) : 4u;
  uint64_t key[6];  // [0]: the point in front of the four, [5]: the one behind them (cache hits)
  if (vec && n == 4u) {
    const ulonglong2 v0 = *reinterpret_cast<const ulonglong2*>(akey + i0), v1 = *reinterpret_cast<const ulonglong2*>(akey + i0 + 2);
    key[1] = v0.x, key[2] = v0.y, key[3] = v1.x, key[4] = v1.y;
  } else {
#pragma unroll
    for (uint32_t j = 0; j < 4u; ++j) key[1 + j] = j < n ? akey[i0 + j] : 0ull;
  }
  key[0] = i0 ? akey[i0 - 1u] : 0ull;
  key[5] = i0 + 4u < m ? akey[i0 + 4u] : 0ull;
#pragma unroll
  for (uint32_t j = 0; j < 4u; ++j) {
    if (j >= n) break;
    const uint32_t i = (uint32_t)i0 + j;
    const uint64_t pre = key[1 + j] >> cell_shift;
    const bool first = i == 0u || (key[j] >> cell_shift) != pre;
    const bool last = i + 1u == m || (key[2 + j] >> cell_shift) != pre;
    if ((!first && !last) || pre >= ncells) continue;  // (a 63-bit key's prefix is inside the grid)
    if (first) cinfo[pre].x = i;
    if (last) cinfo[pre].y = i + 1u;
  }
}

// Early 2: record headers, empty stall states, the adjacent cells by arithmetic (mq_nbr_build_kernel without its start)
__global__ __launch_bounds__(256) void mq_nbr_early_kernel(MqArgs a, uint32_t ncells) {
  for (uint64_t cbase = (uint64_t)blockIdx.x * 8u; cbase < ncells; cbase += (uint64_t)gridDim.x * 8u) {
    const uint32_t c = (uint32_t)cbase + threadIdx.x / 32u;
    const uint32_t k = threadIdx.x & 31u;
    if (c >= ncells) continue;
    const uint2 ci = a.cinfo[c];
    if (k < 2u) a.rec[((size_t)c << a.rg2_shift) + k * a.rg] = make_uint4(ci.x, 0u, k, ci.y);
    if (k == 2u) a.qst[c] = make_uint4(QNONE, 0u, 0u, 0u);
    if (ci.x == ci.y) continue;
    uint32_t nb = QNONE;
    if (k == 13u) {
      nb = c;
    } else if (k < 27u) {
      const uint32_t rel = c & (uint32_t)(a.cells_per_node - 1ull);
      uint32_t nrel = 0;
      if (mq_adjacent_rel(a, rel, k, &nrel)) {
        const uint32_t g = (c - rel) | nrel;
        const uint2 cn = a.cinfo[g];
        if (cn.x != cn.y) nb = g;
      }
    }
    a.qnbr[(size_t)c * 32 + k] = nb;
  }
}

// Late 1: the state bytes -- a point taken further up starts dead (mq_direct_build_kernel's part that reads `gone`), 16 per thread
// (vec: both arrays are 16-byte aligned)
__global__ __launch_bounds__(256) void mq_state_late_kernel(const uint8_t* __restrict__ gone, uint32_t m, uint8_t* __restrict__ state, uint32_t vec) {
  const uint64_t i0 = ((uint64_t)blockIdx.x * 256u + threadIdx.x) * 16u;
  if (i0 >= m) return;
  if (vec && m - i0 >= 16u) {
    const uint4 g = *reinterpret_cast<const uint4*>(gone + i0);
    const uint32_t w[4] = {g.x, g.y, g.z, g.w};
    uint32_t s[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      uint32_t sw = 0x01010101u * (uint32_t)QS_OPEN;
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if ((w[q] >> (8 * j)) & 0xFFu) sw = (sw & ~(0xFFu << (8 * j))) | ((uint32_t)QS_DEAD << (8 * j));
      s[q] = sw;
    }
    *reinterpret_cast<uint4*>(state + i0) = make_uint4(s[0], s[1], s[2], s[3]);
  } else {
    for (uint64_t i = i0; i < m && i < i0 + 16u; ++i) state[i] = gone[i] ? (uint8_t)QS_DEAD : (uint8_t)QS_OPEN;
  }
}

// Late 2: the start of the level (mq_nbr_build_kernel's), from the adjacent cells the early kernel has written
__global__ __launch_bounds__(256) void mq_start_late_kernel(MqArgs a, uint32_t ncells, MqStart st) {
  for (uint64_t cbase = (uint64_t)blockIdx.x * 8u; cbase < ncells; cbase += (uint64_t)gridDim.x * 8u) {
    const uint32_t c = (uint32_t)cbase + threadIdx.x / 32u;
    const uint32_t k = threadIdx.x & 31u;
    bool in = c < ncells;
    if (in) {
      const uint2 ci = a.cinfo[c];
      in = ci.x != ci.y;
    }
    uint32_t nb = QNONE;
    if (in && k == 13u) nb = c;
    else if (in && k < 27u && st.lazy) nb = a.qnbr[(size_t)c * 32 + k];
    mq_start_cell(a, st, cbase, c, k, in, nb, false);
  }
}

// the cells mq_dense_reject_kernel (swz_mqsweep.hip) looks after
__global__ __launch_bounds__(256) void mq_dense_list_kernel(MqArgs a, uint32_t ncells, uint32_t* __restrict__ list, uint32_t* __restrict__ count) {
  const uint32_t c = blockIdx.x * 256 + threadIdx.x;
  if (c >= ncells) return;
  const uint2 ci = a.cinfo[c];
  if (ci.y - ci.x >= a.dense_min) list[atomicAdd(count, 1u)] = c;
}

// ----------------------------------------------------------------------------- host: the steps of the level that build
// How many entries the per-cell arrays have: the grid's with direct numbering, else the occupied cells, counted.
int mq_count_cells(swz_ctx* c, MqLevel& q) {
  MqArgs& a = q.a;
  const LevelBuffers& lb = q.L.lb;
  if (a.direct) {
    if (q.L.sample_points == 0) {
      q.over = true;
      return SWZ_OK;
    }
    q.ncells = (uint32_t)q.grid_entries;
  } else {
    // cells = runs of the cell prefix inside sampled nodes
    SWZ_TRY(fused_scan_sums(c, MqHeadF{a}, a.m, lb.counters + CTR_NUM_CELLS, "mqc", &q.d_cell_sums));
    SWZ_HIP(c, hipMemcpyAsync(&q.ncells, lb.counters + CTR_NUM_CELLS, 4, hipMemcpyDeviceToHost, c->stream));
    SWZ_HIP(c, hipStreamSynchronize(c->stream));
    if (q.ncells == 0 || q.ncells >= 0x7FFFFFFFu) {
      if (q.ncells) *q.used = false;
      q.over = true;
      return SWZ_OK;
    }
  }
  // occupied cells, for the scheduling rules: counted, or the caller's estimate
  q.occ_cells = a.direct ? std::max(1u, std::min<uint32_t>(q.L.occupied[q.cl], q.ncells)) : q.ncells;
  return SWZ_OK;
}

// Were the tables built ahead (mq_prebuild_launch) built for this level?  The key: the same raw keys, the grid the guess
// assumed -- cell size, record size, direct numbering, every node of the level present and sampled, so that the node table
// is the identity --, and a level inside a chain whose key coordinates are in place.
static bool mq_prebuilt_matches(const swz_ctx* c, const MqLevel& q) {
  const MqPrebuild& p = c->mq_pre;
  const MqArgs& a = q.a;
  const MdLevel& L = q.L;
  return p.valid && !p.done && c->opt_on("SWZ_MD_PREBUILD", true) && !q.sharded && p.akey == (const void*)a.akey && p.m == a.m &&
         p.node_shift == L.plan.node_shift && p.cl == (uint32_t)q.cl && p.rg == a.rg && a.direct != 0u &&
         a.cells_per_node == (1ull << (3u * p.cl)) && L.sample_nodes == p.nodes && a.all_sampled != 0u && L.num_nodes == p.nodes &&
         p.nodes == (1ull << (63u - L.plan.node_shift)) && p.ncells == q.ncells && a.gone != nullptr && a.keep_qpos != 0u;
}

int mq_alloc_arrays(swz_ctx* c, MqLevel& q) {
  MqArgs& a = q.a;
  const ActiveSet& as = q.L.as;
  const uint32_t m = a.m, ncells = q.ncells;
  const std::string& sfx = q.sfx;
  SWZ_TRY(c->get(("md_qpos" + sfx).c_str(), (size_t)m, &a.qpos));
  SWZ_TRY(c->get(("md_qstate" + sfx).c_str(), (size_t)m, &a.state));
  // the level's code for its taken points, where that is not the 1 the sweep stores: see mq_commit_kernel
  q.coded = as.gone != nullptr || q.L.plan.take_code != 1;
  if (q.coded) a.taken = a.state;
  a.gone = as.gone;
  a.keep_qpos = (as.gone && c->mq_qpos_buf == a.qpos && c->mq_qpos_keys == as.akey && c->mq_qpos_m == m) ? 1u : 0u;
  c->mq_qpos_buf = q.sharded ? nullptr : a.qpos;
  c->mq_qpos_keys = as.akey;
  c->mq_qpos_m = m;
  SWZ_TRY(c->get(("md_qovf" + sfx).c_str(), (size_t)m, &a.ovf));
  // The per-cell arrays.  Tables built ahead under the level before are taken when they were built for exactly this level
  // -- and are still where they were built --; whatever else was built is dropped here, and the level builds its own.
  MqPrebuild& pre = c->mq_pre;
  q.prebuilt = mq_prebuilt_matches(c, q);
  q.set = q.prebuilt ? pre.set : 0;
  const std::string cs = sfx + (q.set ? "_b" : "");
  SWZ_TRY(c->get(("md_qcinfo" + cs).c_str(), (size_t)ncells, &a.cinfo));
  if (!a.direct) {
    uint32_t* cellbuf = nullptr;
    SWZ_TRY(c->get(("md_qcells" + sfx).c_str(), (size_t)ncells * 2, &cellbuf));
    a.crel = cellbuf;
    a.csnode = cellbuf + ncells;
  }
  SWZ_TRY(c->get(("md_qnbr" + cs).c_str(), (size_t)ncells * 32, &a.qnbr));
  SWZ_TRY(c->get(("md_qrec" + cs).c_str(), (size_t)ncells * 2 * a.rg, &a.rec));
  SWZ_TRY(c->get(("md_qslot" + cs).c_str(), (size_t)ncells * 32, &a.slot));
  SWZ_TRY(c->get(("md_qst" + cs).c_str(), (size_t)ncells, &a.qst));
  if (q.prebuilt && !(pre.valid && pre.cinfo == a.cinfo && pre.qnbr == a.qnbr && pre.rec == a.rec && pre.slot == a.slot && pre.qst == a.qst))
    q.prebuilt = false;  // (the workspace gave one of them back meanwhile)
  if (pre.valid) c->prof_count(q.prebuilt ? "mq_prebuild_taken" : "mq_prebuild_dropped", 1);
  pre.valid = false;
  // (the slots stay a fill of their own: a cell that starts asleep writes into its blocker's row while the table is built)
  if (!q.prebuilt) SWZ_HIP(c, memset_large(a.slot, 0xFF, (size_t)ncells * 32 * sizeof(unsigned long long), c->stream));
  return SWZ_OK;
}

int mq_build_cell_tables(swz_ctx* c, MqLevel& q) {
  MqArgs& a = q.a;
  const uint32_t m = a.m, ncells = q.ncells;
  if (q.prebuilt) {  // the cell bounds are there: the state bytes alone
    hipLaunchKernelGGL(mq_state_late_kernel, dim3(div_up(m, 4096)), dim3(256), 0, c->stream, a.gone, m, a.state,
                       (((uintptr_t)a.gone | (uintptr_t)a.state) & 15u) == 0 ? 1u : 0u);
    SWZ_LAUNCH_CHECK(c);
    c->prof_count("mq_tables_late", 1);
  } else if (a.direct) {
    c->prof_count("mq_tables_at_setup", 1);
    SWZ_HIP(c, memset_large(a.cinfo, 0, (size_t)ncells * sizeof(uint2), c->stream));
    hipLaunchKernelGGL(mq_direct_build_kernel, dim3(div_up(m, 1024)), dim3(256), 0, c->stream, a,
                       ((uintptr_t)a.akey & 15u) == 0 ? 1u : 0u);
    SWZ_LAUNCH_CHECK(c);
  } else {
    SWZ_TRY(c->get(("md_gridmap" + q.sfx).c_str(), (size_t)q.grid_entries, &a.gridmap));
    SWZ_HIP(c, memset_large(a.gridmap, 0xFF, (size_t)q.grid_entries * 4, c->stream));
    SWZ_TRY(fused_scan_apply(c, MqHeadF{a}, MqCellBuildG{a}, m, q.d_cell_sums));
    hipLaunchKernelGGL(mq_cell_end_kernel, dim3(div_up(ncells, 256)), dim3(256), 0, c->stream, a, ncells);
    SWZ_LAUNCH_CHECK(c);
  }
  return SWZ_OK;
}

// dense cells: levels of large cells in one node group (mq_dense_reject_kernel)
int mq_list_dense_cells(swz_ctx* c, MqLevel& q) {
  MqArgs& a = q.a;
  const uint32_t m = a.m, ncells = q.ncells;
  q.ndense = 0;
  a.dense_min = 0;
  a.dirty = nullptr;
  if (!(q.big_cells && q.groups == 1 && !q.sharded)) return SWZ_OK;
  // (100 M clustered points, root: 2048 -> 99 ms, 4096 -> 95, 1024 -> 101, off -> 106; a sheet alone loses 4 ms of 34 to the extra rounds)
  const uint32_t dense_min = (uint32_t)std::max(0L, c->opt_int("SWZ_MD_DENSE_MIN", 4096));
  if (!dense_min || m < dense_min) return SWZ_OK;
  uint32_t* dl = nullptr;
  uint32_t* dcount = nullptr;
  SWZ_TRY(c->get("md_qdense", (size_t)(m / dense_min + 1u), &dl));
  SWZ_TRY(c->get("md_qdense_count", (size_t)4, &dcount));
  SWZ_HIP(c, hipMemsetAsync(dcount, 0, 4, c->stream));
  a.dense_min = dense_min;
  hipLaunchKernelGGL(mq_dense_list_kernel, dim3(div_up(ncells, 256)), dim3(256), 0, c->stream, a, ncells, dl, dcount);
  SWZ_LAUNCH_CHECK(c);
  SWZ_HIP(c, hipMemcpyAsync(&q.ndense, dcount, 4, hipMemcpyDeviceToHost, c->stream));
  SWZ_HIP(c, hipStreamSynchronize(c->stream));
  if (q.ndense) {
    SWZ_TRY(c->get("md_qdirty", (size_t)ncells, &a.dirty));
    SWZ_TRY(c->get("md_qbulk", (size_t)ncells, &a.bulk_round));
    SWZ_HIP(c, hipMemsetAsync(a.dirty, 0, (size_t)ncells, c->stream));
    SWZ_HIP(c, hipMemsetAsync(a.bulk_round, 0, (size_t)ncells * 4, c->stream));
    a.dlist = dl;
  } else {
    a.dense_min = 0;
  }
  return SWZ_OK;
}

// The queues, counters and stream of every node group, then -- in one pass -- the adjacent cells of every cell and the
// first round's queues.
int mq_start_groups(swz_ctx* c, MqLevel& q) {
  MqArgs& a = q.a;
  const uint32_t groups = q.groups, ncells = q.ncells;
  // the round's queue in segments with a counter each (a single counter word takes ~90 atomics per microsecond, and
  // every activation pushes): workgroup b reads segment b % nseg and pushes into it
  a.nseg_shift = 5;
  a.nseg = 1u << a.nseg_shift;
  a.segcap = (uint32_t)std::min<uint64_t>(0x7FFFFFF0ull, 2ull * ncells / a.nseg + 4096ull);
  q.ga.assign(groups, a);
  q.gs.assign(groups, c->stream);
  MqStart start{};
  start.groups = groups;
  start.lazy = q.lazy ? 1u : 0u;
  for (uint32_t g = 0; g < groups; ++g) {
    MqArgs& ag = q.ga[g];
    ag.group = g;
    ag.groups = groups;
    const std::string tag = std::to_string(g);
    SWZ_TRY(c->get(("md_qqueue0_g" + tag).c_str(), (size_t)a.nseg * a.segcap, &ag.queue[0]));
    SWZ_TRY(c->get(("md_qqueue1_g" + tag).c_str(), (size_t)a.nseg * a.segcap, &ag.queue[1]));
    SWZ_TRY(c->get(("md_qctr_g" + tag).c_str(), (size_t)6 * a.nseg * 32 + 32, &ag.qctr));
    ag.qhead = ag.qctr + (size_t)3 * a.nseg * 32;
    ag.qtotal = ag.qctr + (size_t)6 * a.nseg * 32;
    SWZ_HIP(c, hipMemsetAsync(ag.qctr, 0, ((size_t)6 * a.nseg * 32 + 32) * sizeof(uint32_t), c->stream));
    if (g > 0) {
      SWZ_TRY(c->get(("md_counters_g" + tag).c_str(), (size_t)CTR_COUNT, &ag.counters));
      SWZ_HIP(c, hipMemsetAsync(ag.counters, 0, CTR_COUNT * sizeof(uint32_t), c->stream));
      while (c->aux_streams.size() < g) {
        hipStream_t stn = nullptr;
        SWZ_HIP(c, hipStreamCreateWithFlags(&stn, hipStreamNonBlocking));
        c->aux_streams.push_back(stn);
      }
      q.gs[g] = c->aux_streams[g - 1];
    }
    start.queue[g] = ag.queue[0];
    start.qctr[g] = ag.qctr;
  }
  const dim3 nbr_grid(std::min<uint32_t>(div_up(ncells, 8), 1u << 20));
  if (q.prebuilt) {
    hipLaunchKernelGGL(mq_start_late_kernel, nbr_grid, dim3(256), 0, c->stream, q.ga[0], ncells, start);
    c->prof_count("mq_tables_late", 1);
  } else {
    hipLaunchKernelGGL(mq_nbr_build_kernel, nbr_grid, dim3(256), 0, c->stream, q.ga[0], ncells, start);
    if (a.direct) c->prof_count("mq_tables_at_setup", 1);
  }
  SWZ_LAUNCH_CHECK(c);
  SWZ_STAGE(c, "mq tables");
  return SWZ_OK;
}

// ---- the early tables of the level after this one, under this level's rounds
// Asked for by session_run_levels (MqPrebuild::wanted: the grid that level would most likely get), launched when this
// level is one whose arrays the next may share -- direct numbering --, when a second set of per-cell buffers fits beside
// this level's, and when the build stream is at most the process's fourth stream with work in flight.  Node group 0 runs
// on the context's stream and group g > 0 on aux stream g - 1 (mq_start_groups), so a level has q.groups streams in
// flight -- two as a rule, up to eight with SWZ_MD_GROUPS -- and the build stream is one more: q.groups + 1 <= 4.  Two fills and two kernels on that stream, ordered
// behind this level's own tables by an event; nothing waits for them until mq_prebuild_join.
int mq_prebuild_launch(swz_ctx* c, MqLevel& q) {
  MqPrebuild& p = c->mq_pre;
  if (!p.wanted) return SWZ_OK;
  p.wanted = false;
  p.valid = false;
  const MqArgs& a = q.a;
  if (!a.direct || q.sharded || q.groups + 1u > 4u || p.want_node_shift >= 63u) return SWZ_OK;
  const uint32_t rg = p.want_rg, cl = p.want_cl;
  const uint64_t nodes = 1ull << (63u - p.want_node_shift);
  const uint64_t ncells = nodes << (3u * cl);
  if (ncells > 0x7FFFFFF0ull) return SWZ_OK;
  // memory: both sets side by side, by the rule that admits a level's grid (mq_choose_records_and_numbering)
  const std::string cs = q.set ? "" : "_b";
  const char* base[5] = {"md_qcinfo", "md_qnbr", "md_qrec", "md_qslot", "md_qst"};
  const size_t bytes[5] = {ncells * sizeof(uint2), ncells * 32 * 4, ncells * 2 * rg * sizeof(uint4), ncells * 32 * 8, ncells * sizeof(uint4)};
  if (const char* mc = c->opt("SWZ_MD_DIRECT_MAX_CELLS")) {
    if ((uint64_t)q.ncells + ncells > (uint64_t)std::max(0LL, atoll(mc))) return SWZ_OK;
  }
  size_t grow = 0;
  bool grows[5] = {false, false, false, false, false};  // the buffers this call has to allocate or enlarge
  for (int i = 0; i < 5; ++i) {
    const auto it = c->bufs.find(base[i] + cs);
    grows[i] = it == c->bufs.end() || it->second.cap < bytes[i];
    if (grows[i]) grow += bytes[i] + bytes[i] / 16 + 256;
  }
  if (grow) {
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) free_b = 0;
    if ((double)grow > (double)free_b * 0.9) return SWZ_OK;
  }
  uint2* cinfo = nullptr;
  uint32_t* qnbr = nullptr;
  uint4* rec = nullptr;
  unsigned long long* slot = nullptr;
  uint4* qst = nullptr;
  void* got[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  for (int i = 0; i < 5; ++i)
    if (c->get((base[i] + cs).c_str(), bytes[i], &got[i]) != SWZ_OK) {  // (no room after all: the level is none the worse for it)
      c->err.clear();
      (void)hipGetLastError();
      // ... and the idle set keeps nothing of the attempt: what this call allocated or enlarged goes back; a buffer that
      // was large enough before stays, so that a later attempt in a timed step does not allocate it again
      for (int j = 0; j < 5; ++j) {
        const auto it = c->bufs.find(base[j] + cs);
        if (grows[j] && it != c->bufs.end()) c->free_buf(it->second);
      }
      return SWZ_OK;
    }
  cinfo = static_cast<uint2*>(got[0]);
  qnbr = static_cast<uint32_t*>(got[1]);
  rec = static_cast<uint4*>(got[2]);
  slot = static_cast<unsigned long long*>(got[3]);
  qst = static_cast<uint4*>(got[4]);
  MqArgs e{};
  e.akey = a.akey;
  e.m = a.m;
  e.direct = 1u;
  e.cpn_shift = 3u * cl;
  e.cells_per_node = 1ull << (3u * cl);
  e.cell_shift = p.want_node_shift - 3u * cl;
  e.rg = rg;
  e.rg2_shift = rg == 4u ? 3u : 4u;
  e.cinfo = cinfo;
  e.qnbr = qnbr;
  e.rec = rec;
  e.qst = qst;
  e.peers.shards = 1u;
  // From here on a HIP call that fails ends the attempt, not the level (the speculation never changes an error code): the
  // first failure is kept, nothing more is launched, whatever reached the build stream is waited for, the events go back.
  hipError_t bad = hipSuccess;
  auto ok = [&](hipError_t r) {
    if (bad == hipSuccess && r != hipSuccess) bad = r;
    return bad == hipSuccess;
  };
  if (!c->mq_build_stream) {
    int least = 0, greatest = 0;
    // (the lowest priority: a round's few thousand wavefronts must not queue behind a grid of a million workgroups)
    if (ok(hipDeviceGetStreamPriorityRange(&least, &greatest)) && !ok(hipStreamCreateWithPriority(&c->mq_build_stream, hipStreamNonBlocking, least)))
      c->mq_build_stream = nullptr;
  }
  hipStream_t bs = c->mq_build_stream;
  hipEvent_t fork = c->take_event();
  p.done = c->take_event();
  const bool timed = c->opt("SWZ_DEBUG") != nullptr;
  if (timed) {
    p.t0 = c->take_event();
    p.t1 = c->take_event();
  }
  if (bs && fork && p.done && (!timed || (p.t0 && p.t1)) && ok(hipEventRecord(fork, c->stream)) && ok(hipStreamWaitEvent(bs, fork, 0))) {
    if (timed) ok(hipEventRecord(p.t0, bs));
    if (ok(memset_large(cinfo, 0, bytes[0], bs))) {
      hipLaunchKernelGGL(mq_cinfo_early_kernel, dim3(div_up(e.m, 1024)), dim3(256), 0, bs, e.akey, e.m, e.cell_shift, (uint32_t)ncells, cinfo,
                         ((uintptr_t)e.akey & 15u) == 0 ? 1u : 0u);
      ok(hipGetLastError());
    }
    if (ok(memset_large(slot, 0xFF, bytes[3], bs))) {
      hipLaunchKernelGGL(mq_nbr_early_kernel, dim3(std::min<uint32_t>(div_up(ncells, 8), 1u << 20)), dim3(256), 0, bs, e, (uint32_t)ncells);
      ok(hipGetLastError());
    }
    if (timed) ok(hipEventRecord(p.t1, bs));
    ok(hipEventRecord(p.done, bs));
  } else if (bad == hipSuccess) {
    bad = hipErrorUnknown;  // (no stream or no event)
  }
  if (fork) c->event_pool.push_back(fork);
  if (bad != hipSuccess) {
    (void)hipGetLastError();
    if (bs) (void)hipStreamSynchronize(bs);
    for (hipEvent_t* ev : {&p.done, &p.t0, &p.t1}) {
      if (*ev) c->event_pool.push_back(*ev);
      *ev = nullptr;
    }
    return SWZ_OK;
  }
  // SWZ_TRACE synchronises after every stage: here too, so that (with SWZ_DEBUG) the early tables are timed with nothing beside them
  if (c->opt("SWZ_TRACE")) {
    const hipError_t te = hipStreamSynchronize(bs);
    fprintf(stderr, "[swz trace] %s:%d %s -> %s\n", __FILE__, __LINE__, "mq tables ahead", hipGetErrorString(te));
    fflush(stderr);
  }
  c->prof_count("mq_tables_ahead", 2);
  p.set = q.set ? 0 : 1;
  p.akey = a.akey;
  p.m = a.m;
  p.node_shift = p.want_node_shift;
  p.cl = cl;
  p.rg = rg;
  p.ncells = (uint32_t)ncells;
  p.nodes = (uint32_t)nodes;
  p.cinfo = cinfo;
  p.qnbr = qnbr;
  p.rec = rec;
  p.slot = slot;
  p.qst = qst;
  p.valid = true;
  ++p.serial;
  return SWZ_OK;
}

// the context's stream goes on behind the early kernels (no host wait); a product is taken only after this
int mq_prebuild_join(swz_ctx* c) {
  MqPrebuild& p = c->mq_pre;
  if (!p.done) return SWZ_OK;
  hipError_t e = hipStreamWaitEvent(c->stream, p.done, 0);
  if (e != hipSuccess) {  // no order on the device: the host waits instead, and nobody takes the tables
    (void)hipGetLastError();
    p.valid = false;
    e = c->mq_build_stream ? hipStreamSynchronize(c->mq_build_stream) : hipSuccess;
  }
  c->event_pool.push_back(p.done);
  p.done = nullptr;
  if (p.t0 && p.t1) {
    float ms = 0.f;
    (void)hipEventSynchronize(p.t1);
    (void)hipEventElapsedTime(&ms, p.t0, p.t1);
    fprintf(stderr, "[swz] MIN_DISTANCE tables built ahead: %u cells (cell levels %u, records of %u), %.2f ms on the build stream\n", p.ncells, p.cl,
            p.rg - 1u, ms);
    c->event_pool.push_back(p.t0);
    c->event_pool.push_back(p.t1);
  }
  p.t0 = p.t1 = nullptr;
  if (e != hipSuccess) {  // (a device that cannot even be waited for: the level's own next call reports it)
    (void)hipGetLastError();
    p.valid = false;
  }
  return SWZ_OK;
}

}  // namespace swz
