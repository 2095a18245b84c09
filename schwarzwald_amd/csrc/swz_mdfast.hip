// swz_mdfast.hip -- MIN_DISTANCE_FAST (AdaptivePoissonDiskSampling, Sampling.h:477-542): a sampled node offers only every
// n-th point of its Morton-ordered range to the greedy minimum-distance test, n = swz_min_distance_fast_stride(level): 4 at
// the root, 2 at level 0, 1 below.  The other points are neither taken nor do they block anything; they go down.
//
// A level with n > 1 is sampled here: the candidates of all sampled nodes are compacted into an active set of their own,
// with its own node segmentation, that set goes through min_distance_level like any level, and the decisions are scattered
// back.  Levels with n == 1 and levels that take the first point only never get here (level_step, swz_level.hip).
#include <algorithm>
#include <cmath>

#include "swz_md.h"
#include "swz_scan.h"

// density of a node level -- TilerProcess.cpp:500-508; nth as Sampling.h:522-523 evaluates it
extern "C" int32_t swz_min_distance_fast_stride(int32_t node_level) {
  const float density = node_level < 0 ? 0.25f : (node_level < 1 ? 0.5f : 1.f);
  return (int32_t)(uint32_t)std::round(1 / density);
}

namespace swz {

// ----------------------------------------------------------------------------- the candidates' node segmentation
// Sampled node j of the level offers ceil(count / n) candidates: the exclusive scan of that number over the nodes is where
// its candidates start, and -- the candidates of a node being its points 0, n, 2n, ... -- where every single one of them goes.
// No pass over the keys, no scan over the points.
struct CandCountF {
  const uint32_t* nstart;
  const uint8_t* nmode;
  uint32_t stride;
  __device__ uint32_t operator()(uint32_t j) const {
    return nmode[j] == MODE_SAMPLE ? (nstart[j + 1] - nstart[j] + stride - 1u) / stride : 0u;
  }
};
struct CandNodeG {
  const uint8_t* nmode;
  const uint32_t* snode_of;  // node -> index among the sampled nodes
  uint32_t num_nodes;
  uint32_t* cbase;           // [node]: first candidate of a sampled node
  uint32_t* cnstart;         // [sampled node] and one behind the last: the candidate set's node starts
  uint8_t* cnmode;           // [sampled node]: MODE_SAMPLE (the take-all decision was made on the full count)
  __device__ void operator()(uint32_t j, uint32_t excl, uint32_t cnt) const {
    cbase[j] = excl;
    if (nmode[j] == MODE_SAMPLE) {
      const uint32_t s = snode_of[j];
      cnstart[s] = excl;
      cnmode[s] = MODE_SAMPLE;
    }
    // (the table's end: sampled nodes behind this one there are none when j is the last node, and a take-all node counts 0)
    if (j == num_nodes - 1u) cnstart[snode_of[j] + (nmode[j] == MODE_SAMPLE ? 1u : 0u)] = excl + cnt;
  }
};
__global__ __launch_bounds__(256) void mdf_node_flag_kernel(const uint8_t* __restrict__ nmode, uint32_t nnodes, uint32_t* __restrict__ out) {
  const uint32_t j = blockIdx.x * 256 + threadIdx.x;
  if (j < nnodes) out[j] = nmode[j] == MODE_SAMPLE ? 1u : 0u;
}

// ----------------------------------------------------------------------------- candidates out, decisions back
// One thread per point of the level.  The node id and the node's start are read by every lane (4 bytes a point, the starts
// from cache); the key and the index only by the lanes that hold a candidate.  Candidate q of a node lands at the node's
// base + q: neighbouring candidates of a wavefront store to neighbouring slots.
struct MdfCand {
  const uint64_t* akey;
  const uint32_t* aidx;
  const uint32_t* nid;
  const uint32_t* nstart;
  const uint8_t* nmode;
  const uint32_t* cbase;
  const uint32_t* snode_of;
  uint32_t m, mc, stride;
  uint64_t* ckey;    // [mc] key
  uint32_t* cidx;    // [mc] position in the sorted arrays
  uint32_t* cplace;  // [mc] place in the level
  uint32_t* cnid;    // [mc] node of the candidate set
};
__device__ __forceinline__ bool mdf_slot(const MdfCand& a, uint32_t i, uint32_t* node, uint32_t* slot) {
  *node = a.nid[i];
  if (a.nmode[*node] != MODE_SAMPLE) return false;
  const uint32_t off = i - a.nstart[*node];
  // (strides are 2 and 4)
  if (off & (a.stride - 1u)) return false;
  *slot = a.cbase[*node] + off / a.stride;
  return *slot < a.mc;  // (always, with a consistent segmentation: never write beyond the arrays)
}
__global__ __launch_bounds__(256) void mdf_candidates_kernel(MdfCand a) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= a.m) return;
  uint32_t node, slot;
  if (!mdf_slot(a, i, &node, &slot)) return;
  a.ckey[slot] = a.akey[i];
  a.cidx[slot] = a.aidx ? a.aidx[i] : i;
  a.cplace[slot] = i;
  a.cnid[slot] = a.snode_of[node];
}
__global__ __launch_bounds__(256) void mdf_scatter_kernel(const uint8_t* __restrict__ ctaken, const uint32_t* __restrict__ cplace,
                                                          uint32_t mc, uint32_t m, uint8_t* __restrict__ taken) {
  const uint32_t j = blockIdx.x * 256 + threadIdx.x;
  if (j >= mc || !ctaken[j]) return;
  const uint32_t i = cplace[j];
  if (i < m) taken[i] = 1;
}

// ----------------------------------------------------------------------------- one level with a stride above one
// lb.taken is zero for the points of sampled nodes; num_nodes / sample_nodes: the level's counters.
int min_distance_fast_level(swz_ctx* c, const LevelPlan& plan, const ActiveSet& as, const SortedPoints& sp, const LevelBuffers& lb,
                            uint32_t stride, uint32_t num_nodes, uint32_t sample_nodes, uint32_t* rounds_out) {
  if (stride < 2u || (stride & (stride - 1u))) return c->fail(SWZ_ERR_INTERNAL, "MIN_DISTANCE_FAST: the stride of a strided level is a power of two");
  const uint32_t m = as.m;
  uint32_t *snode = nullptr, *cbase = nullptr, *cnstart = nullptr, *d_total = nullptr;
  uint8_t* cnmode = nullptr;
  uint32_t mc = 0;
  {
    ProfScope ps(c, "md_fast_candidates", (uint64_t)num_nodes * 21ull, 4);
    SWZ_TRY(c->get("mdf_snode", (size_t)num_nodes, &snode));
    SWZ_TRY(c->get("mdf_cbase", (size_t)num_nodes, &cbase));
    SWZ_TRY(c->get("mdf_nstart", (size_t)sample_nodes + 1, &cnstart));
    SWZ_TRY(c->get("mdf_nmode", (size_t)sample_nodes, &cnmode));
    SWZ_TRY(c->get("mdf_total", (size_t)1, &d_total));
    hipLaunchKernelGGL(mdf_node_flag_kernel, dim3(div_up(num_nodes, 256)), dim3(256), 0, c->stream, lb.nmode, num_nodes, snode);
    SWZ_LAUNCH_CHECK(c);
    SWZ_TRY(scan_exclusive_u32(c, snode, snode, num_nodes, nullptr, "mdf"));
    SWZ_TRY(fused_scan(c, CandCountF{lb.nstart, lb.nmode, stride}, CandNodeG{lb.nmode, snode, num_nodes, cbase, cnstart, cnmode}, num_nodes,
                       d_total, "mdf"));
    SWZ_TRY(read_u32(c, d_total, &mc));
  }
  // (every sampled node has a first point: at least one candidate each, and never more than the level has points)
  if (mc < sample_nodes || mc > m) return c->fail(SWZ_ERR_INTERNAL, "MIN_DISTANCE_FAST: candidate count inconsistent with the level's nodes");
  MdfCand a{as.akey, as.aidx, lb.nid, lb.nstart, lb.nmode, cbase, snode, m, mc, stride, nullptr, nullptr, nullptr, nullptr};
  uint8_t* ctaken = nullptr;
  SWZ_TRY(c->get("mdf_key", (size_t)mc, &a.ckey));
  SWZ_TRY(c->get("mdf_idx", (size_t)mc, &a.cidx));
  SWZ_TRY(c->get("mdf_place", (size_t)mc, &a.cplace));
  SWZ_TRY(c->get("mdf_nid", (size_t)mc, &a.cnid));
  SWZ_TRY(c->get("mdf_taken", (size_t)mc, &ctaken));
  {
    ProfScope ps(c, "md_fast_candidates", (uint64_t)m * 4ull + (uint64_t)mc * 32ull, 1);
    hipLaunchKernelGGL(mdf_candidates_kernel, dim3(div_up(m, 256)), dim3(256), 0, c->stream, a);
    SWZ_LAUNCH_CHECK(c);
    SWZ_HIP(c, hipMemsetAsync(ctaken, 0, mc, c->stream));
  }
  // The candidates as a level of their own: every node sampled, no files of earlier batches, nothing the incremental path of
  // a multi-batch tiler could trust (the merged range is strided anew by every visit).
  ActiveSet cas{a.ckey, a.cidx, mc};
  LevelBuffers clb;
  clb.nid = a.cnid;
  clb.nstart = cnstart;
  clb.nmode = cnmode;
  clb.taken = ctaken;
  clb.counters = lb.counters;  // (CTR_ERROR of the sweeps is read with the level's)
  SWZ_TRY(min_distance_level(c, plan, cas, sp, clb, sample_nodes, sample_nodes, mc, rounds_out));
  {
    ProfScope ps(c, "md_fast_scatter", (uint64_t)mc * 6ull, 1);
    hipLaunchKernelGGL(mdf_scatter_kernel, dim3(div_up(mc, 256)), dim3(256), 0, c->stream, ctaken, a.cplace, mc, m, lb.taken);
    SWZ_LAUNCH_CHECK(c);
  }
  return SWZ_OK;
}

}  // namespace swz
