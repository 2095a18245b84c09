// swz_shard.hip -- one batch spread over several GPUs: every shard runs a session (swz_session.h) on the points of its
// octants, in pieces, between which the driver (the caller, or swz_group.hip) passes what the shards owe each other.
// ACCURATE: the root node spans the shards, so a shard samples it with the lower shards' root samples in front of its
// own points (ghosts).  FAST: see swz_shard_fast_* below.
#include "swz_session.h"

namespace swz {

struct ShardState {
  TileSession t;
  uint32_t n_local = 0;
  bool open = false;
  // swz_shard_presort_device ran: the local points are indexed and sorted, `front` entries are free in front
  bool presorted = false;
  uint32_t front = 0;
  const double* xyz_local = nullptr;
  bool perm_local = false;  // perm of the local points counts from the first LOCAL point
  bool empty = false;       // the open batch has no local points
  bool fast = false;        // the open batch runs the FAST strategy (swz_shard_fast_*)
  uint32_t fast_candidates = 0;  // points of this shard's level-0 nodes: what the root is reconstructed from
};

static ShardState* shard_state(swz_ctx* c) {
  if (!c->shard) c->shard = new ShardState();
  return static_cast<ShardState*>(c->shard);
}
int shard_begin_empty(swz_ctx* c) {
  ShardState* s = shard_state(c);
  s->presorted = false;
  s->fast = false;
  s->t = TileSession{};
  s->n_local = 0;
  s->empty = true;
  s->open = true;
  return SWZ_OK;
}
void shard_free(swz_ctx* c) {
  delete static_cast<ShardState*>(c->shard);
  c->shard = nullptr;
}
// what a shard's session writes per sorted position
static int shard_outputs(swz_ctx* c, size_t count, TileDeviceOut* out) {
  SWZ_TRY(c->get("shard_keys", count, &out->keys));
  SWZ_TRY(c->get("shard_perm", count, &out->perm));
  SWZ_TRY(c->get("shard_level", count, &out->level));
  return SWZ_OK;
}

__global__ __launch_bounds__(256) void root_taken_count_kernel(const int8_t* __restrict__ level, uint32_t first,
                                                               uint32_t n, uint32_t* __restrict__ flags) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) flags[i] = (i >= first && level[i] == (int8_t)-1) ? 1u : 0u;
}
__global__ __launch_bounds__(256) void root_taken_gather_kernel(const int8_t* __restrict__ level, uint32_t first,
                                                                uint32_t n, const uint32_t* __restrict__ pos,
                                                                SortedPoints sp, double* __restrict__ out_xyz) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n || i < first || level[i] != (int8_t)-1) return;
  const uint64_t o = pos[i];
  store_sorted_point(sp, i, out_xyz, o);
}
__global__ __launch_bounds__(256) void shard_strip_kernel(const uint64_t* __restrict__ keys,
                                                          const uint32_t* __restrict__ perm,
                                                          const int8_t* __restrict__ level, uint32_t ghosts,
                                                          uint32_t perm_base, uint32_t n_local,
                                                          uint64_t* __restrict__ okeys, uint32_t* __restrict__ operm,
                                                          int8_t* __restrict__ olevel) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n_local) return;
  okeys[i] = keys[ghosts + i];
  operm[i] = perm[ghosts + i] - perm_base;
  olevel[i] = level[ghosts + i];
}

// Everything of swz_shard_begin_device that does not depend on the ghosts: index + sort + gather of the local
// points, with room for up to ghost_capacity ghosts in front of every array.  All shards can do this at the
// same time, so that only the root node itself is left in the chain that passes the ghosts from shard to shard.
int shard_presort_device(swz_ctx* c, const double* d_xyz_local, uint32_t n, const double bmin[3], const double bmax[3],
                         const swz_tile_params& p, uint32_t ghost_capacity) {
  if (p.strategy != SWZ_ACCURATE) return c->fail(SWZ_ERR_BAD_ARG, "this call runs the ACCURATE strategy of a sharded batch (FAST: swz_shard_fast_*)");
  if ((uint64_t)n + ghost_capacity > 0xFFFFFFFEull) return c->fail(SWZ_ERR_TOO_MANY_POINTS, "shard + ghosts exceed 2^32-2 points");
  ShardState* s = shard_state(c);
  s->open = false;
  s->presorted = false;
  s->fast = false;
  TileDeviceOut out{};
  SWZ_TRY(shard_outputs(c, (size_t)n + ghost_capacity, &out));
  out.keys += ghost_capacity;
  out.perm += ghost_capacity;
  out.level += ghost_capacity;
  SWZ_TRY(session_prepare(c, s->t, const_cast<double*>(d_xyz_local), n, bmin, bmax, p, out, ghost_capacity));
  s->n_local = n;
  s->front = ghost_capacity;
  s->xyz_local = d_xyz_local;
  s->perm_local = true;
  s->presorted = true;
  return SWZ_OK;
}

// ghosts lie in lower octants, so their keys are smaller than every local key: sorted ghosts ++ sorted locals
// is the sorted whole.  Writes the g ghosts into the free entries in front of the presorted arrays.
static int shard_attach_ghosts(swz_ctx* c, ShardState* s, const double* d_ghost_xyz, uint32_t g) {
  TileSession& t = s->t;
  if (g) {
    uint64_t* tmpk = nullptr;
    uint32_t* tmpv = nullptr;
    SWZ_TRY(c->get("ghost_keys", (size_t)g, &tmpk));
    SWZ_TRY(c->get("ghost_vals", (size_t)g, &tmpv));
    uint64_t* gk = t.keys - g;
    uint32_t* gp = t.perm - g;
    double* gx = const_cast<double*>(d_ghost_xyz);  // inside the bounds already: the clamp of the encode is a no-op
    SWZ_TRY(encode_device(c, gx, g, t.bmin, t.bmax, tmpk));
    SWZ_TRY(radix_sort_pairs(c, tmpk, tmpv, gk, gp, g, true));
    if (t.sp.X) SWZ_TRY(gather_positions(c, d_ghost_xyz, gp, g, const_cast<double*>(t.sp.X) - g, const_cast<double*>(t.sp.Y) - g,
                                         const_cast<double*>(t.sp.Z) - g));
    SWZ_HIP(c, hipMemsetAsync(t.level - g, 0x80, (size_t)g, c->stream));
    t.keys -= g;
    t.perm -= g;
    t.level -= g;
    if (t.sp.X) {
      t.sp.X -= g;
      t.sp.Y -= g;
      t.sp.Z -= g;
    }
    t.sp.perm = t.perm;  // (now starts with the ghosts' entries, which index the ghost array)
    t.sp.ghost_xyz = d_ghost_xyz;
    t.sp.ghosts = g;
    t.n += g;
    t.as = ActiveSet{t.keys, nullptr, t.n};
  }
  t.ghosts = g;
  return SWZ_OK;
}

int shard_begin_device(swz_ctx* c, const double* d_xyz_local, uint32_t n, const double bmin[3],
                       const double bmax[3], const swz_tile_params& p, uint64_t global_points,
                       const double* d_ghost_xyz, uint32_t ghosts, uint64_t* num_root_taken) {
  if (p.strategy != SWZ_ACCURATE) return c->fail(SWZ_ERR_BAD_ARG, "this call runs the ACCURATE strategy of a sharded batch (FAST: swz_shard_fast_*)");
  ShardState* s = shard_state(c);
  s->open = false;
  s->empty = false;
  s->fast = false;
  const uint32_t total = n + ghosts;
  const bool fast = s->presorted && s->xyz_local == d_xyz_local && s->n_local == n && ghosts <= s->front;
  s->presorted = false;
  if (fast) {
    SWZ_TRY(shard_attach_ghosts(c, s, d_ghost_xyz, ghosts));
  } else {
    s->perm_local = false;
    double* xyz = nullptr;
    if (ghosts == 0) {
      xyz = const_cast<double*>(d_xyz_local);  // already inside the bounds (it was encoded before the exchange)
    } else if (d_ghost_xyz + (size_t)ghosts * 3 == d_xyz_local) {
      xyz = const_cast<double*>(d_ghost_xyz);  // caller laid the ghosts out right in front of its points
    } else {
      SWZ_TRY(c->get("shard_xyz", (size_t)total * 3, &xyz));
      SWZ_HIP(c, hipMemcpyAsync(xyz, d_ghost_xyz, (size_t)ghosts * 24, hipMemcpyDeviceToDevice, c->stream));
      SWZ_HIP(c, hipMemcpyAsync(xyz + (size_t)ghosts * 3, d_xyz_local, (size_t)n * 24, hipMemcpyDeviceToDevice, c->stream));
    }
    TileDeviceOut out{};
    SWZ_TRY(shard_outputs(c, (size_t)total, &out));
    SWZ_TRY(session_prepare(c, s->t, xyz, total, bmin, bmax, p, out));
    s->t.ghosts = ghosts;
    s->n_local = n;
  }
  // the root node spans all shards: its take-all / sample decision uses the global point count
  const LevelPlan root_plan =
    make_plan(-1, p.sampler, p.max_points_per_node, p.spacing_at_root, p.max_depth, bmin, bmax, false, true);
  if ((p.sampler == SWZ_RANDOM_GRID || p.sampler == SWZ_GRID_CENTER) && root_plan.cand < 0 &&
      global_points > p.max_points_per_node)
    return c->fail(SWZ_ERR_BAD_ARG, "sharded root with candidate level -1 (spacing >= half the extent) is unsupported");
  SWZ_TRY(session_run_levels(c, s->t, -1, global_points > p.max_points_per_node ? 1 : 0));
  // how many LOCAL points the root took (their positions become the next shard's ghosts)
  const uint32_t nb = div_up(total, 256);
  SWZ_HIP(c, hipMemsetAsync(s->t.lb.counters, 0, CTR_COUNT * sizeof(uint32_t), c->stream));
  hipLaunchKernelGGL(root_taken_count_kernel, dim3(nb), dim3(256), 0, c->stream, s->t.level, ghosts, total,
                     s->t.lb.flags);
  SWZ_LAUNCH_CHECK(c);
  SWZ_TRY(scan_exclusive_u32(c, s->t.lb.flags, s->t.lb.flags, total, s->t.lb.counters + CTR_REMAINING, "shr"));
  uint32_t cnt = 0;
  SWZ_TRY(read_u32(c, s->t.lb.counters + CTR_REMAINING, &cnt));
  if (num_root_taken) *num_root_taken = cnt;
  s->open = true;
  return SWZ_OK;
}

int shard_root_taken_device(swz_ctx* c, double* d_xyz_out) {
  ShardState* s = shard_state(c);
  if (!s->open) return c->fail(SWZ_ERR_BAD_ARG, "no sharded batch is open");
  if (s->empty) return SWZ_OK;
  const uint32_t total = s->t.n;
  // lb.flags still holds the exclusive scan of the root-taken flags of swz_shard_begin
  hipLaunchKernelGGL(root_taken_gather_kernel, dim3(div_up(total, 256)), dim3(256), 0, c->stream, s->t.level,
                     s->t.ghosts, total, s->t.lb.flags, s->t.sp, d_xyz_out);
  SWZ_LAUNCH_CHECK(c);
  return SWZ_OK;
}

int shard_finish_device(swz_ctx* c, uint64_t* d_keys_out, uint32_t* d_perm_out, int8_t* d_level_out,
                        swz_tile_stats* stats) {
  ShardState* s = shard_state(c);
  if (!s->open) return c->fail(SWZ_ERR_BAD_ARG, "no sharded batch is open");
  s->open = false;
  if (s->empty) {
    s->empty = false;
    session_stats(s->t, stats);
    return SWZ_OK;
  }
  SWZ_TRY(session_run_levels(c, s->t, 20, -1));
  hipLaunchKernelGGL(shard_strip_kernel, dim3(div_up(s->n_local, 256)), dim3(256), 0, c->stream, s->t.keys, s->t.perm,
                     s->t.level, s->t.ghosts, s->perm_local ? 0u : s->t.ghosts, s->n_local, d_keys_out, d_perm_out, d_level_out);
  SWZ_LAUNCH_CHECK(c);
  session_stats(s->t, stats);
  return SWZ_OK;
}

// ---- FAST (TilingAlgorithmV3, the reference's default) on a sharded batch.  The start level comes from the distribution
// of the WHOLE batch (:1473-1535): every shard reports the counts of its part per 6-octant prefix, the driver sums them
// and tells every shard the level.  Start nodes lie at level >= 2, inside one shard's octants, so the levels from there
// down and the reconstruction of the skipped levels down to level 0 (:1717-1784) are local; the root is reconstructed
// from what the level-0 nodes of ALL shards hold -- in octant order, which is shard order --, so the driver collects
// those candidates (swz_shard_fast_root_candidates_device), samples them in one place (swz_sample_points_device with
// AlwaysAdhereToMinSpacing at node level -1) and hands every shard the flags of its part.
__global__ __launch_bounds__(256) void shard_fast_cand_kernel(const uint64_t* __restrict__ keys, uint32_t n, const uint32_t* __restrict__ pos,
                                                              const int8_t* __restrict__ level, const uint32_t* __restrict__ dup,
                                                              int start_node_level, uint32_t child_bit, SortedPoints sp,
                                                              uint64_t* __restrict__ okeys, double* __restrict__ oxyz) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  if (!recon_candidate(level, dup, i, start_node_level, child_bit)) return;
  const uint64_t o = pos[i];
  okeys[o] = keys[i];
  store_sorted_point(sp, i, oxyz, o);
}
__global__ __launch_bounds__(256) void shard_fast_mark_root_kernel(uint32_t n, const uint32_t* __restrict__ pos, const int8_t* __restrict__ level,
                                                                   uint32_t* __restrict__ dup, int start_node_level, uint32_t child_bit,
                                                                   const uint8_t* __restrict__ taken) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  if (recon_candidate(level, dup, i, start_node_level, child_bit) && taken[pos[i]]) dup[i] |= 1u;
}
__global__ __launch_bounds__(256) void shard_fast_strip_kernel(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ perm,
                                                               const int8_t* __restrict__ level, const uint32_t* __restrict__ dup, uint32_t n,
                                                               uint64_t* __restrict__ okeys, uint32_t* __restrict__ operm,
                                                               int8_t* __restrict__ olevel, uint32_t* __restrict__ odup) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  okeys[i] = keys[i];
  operm[i] = perm[i];
  olevel[i] = level[i];
  odup[i] = dup[i];
}

int shard_fast_begin_device(swz_ctx* c, const double* d_xyz_local, uint32_t n, const double bmin[3], const double bmax[3],
                            const swz_tile_params& p, uint32_t* counts_host) {
  if (p.strategy != SWZ_FAST) return c->fail(SWZ_ERR_BAD_ARG, "swz_shard_fast_begin_device: not the FAST strategy");
  ShardState* s = shard_state(c);
  s->open = false;
  s->presorted = false;
  s->fast = true;
  s->fast_candidates = 0;
  s->empty = n == 0;
  s->n_local = n;
  if (n == 0) {
    s->t = TileSession{};
    s->t.params = p;
    for (uint32_t b = 0; b < (1u << 18); ++b) counts_host[b] = 0;
    s->open = true;
    return SWZ_OK;
  }
  TileDeviceOut out{};
  SWZ_TRY(shard_outputs(c, (size_t)n, &out));
  SWZ_TRY(c->get("shard_dup", (size_t)n, &out.dup));
  SWZ_TRY(session_prepare(c, s->t, const_cast<double*>(d_xyz_local), n, bmin, bmax, p, out));
  s->perm_local = true;
  SWZ_TRY(fast_prefix_counts(c, s->t.keys, n, counts_host));
  s->open = true;
  return SWZ_OK;
}

// the levels from the start level down, the local reconstruction, and how many points this shard's level-0 nodes hold
int shard_fast_run_device(swz_ctx* c, int start_level, uint64_t* num_root_candidates) {
  ShardState* s = shard_state(c);
  if (!s->open || !s->fast) return c->fail(SWZ_ERR_BAD_ARG, "swz_shard_fast_run: no FAST sharded batch is open");
  if (start_level < 1 || start_level > 6) return c->fail(SWZ_ERR_BAD_ARG, "swz_shard_fast_run: start levels 1..6");
  *num_root_candidates = 0;
  TileSession& t = s->t;
  t.fast_start = start_level;
  if (s->empty) return SWZ_OK;
  t.next_level = start_level - 1;
  SWZ_TRY(session_run_levels(c, t, 20, -1));
  SWZ_TRY(session_fast_reconstruct(c, t, t.params, start_level, 1));
  // what the root's children hold (the selection of reconstruct level 0)
  const uint32_t child_bit = (1 == start_level) ? 0u : 2u;
  uint32_t* pos = nullptr;
  SWZ_TRY(c->get("shard_fast_pos", (size_t)t.n, &pos));
  SWZ_TRY(session_recon_ranks(c, t, start_level, child_bit, pos));
  uint32_t m = 0;
  SWZ_TRY(read_u32(c, t.lb.counters + CTR_REMAINING, &m));
  s->fast_candidates = m;
  *num_root_candidates = m;
  return SWZ_OK;
}

int shard_fast_root_candidates_device(swz_ctx* c, uint64_t* d_keys_out, double* d_xyz_out) {
  ShardState* s = shard_state(c);
  if (!s->open || !s->fast) return c->fail(SWZ_ERR_BAD_ARG, "swz_shard_fast_root_candidates_device: no FAST sharded batch is open");
  if (s->empty || !s->fast_candidates) return SWZ_OK;
  TileSession& t = s->t;
  uint32_t* pos = nullptr;
  SWZ_TRY(c->get("shard_fast_pos", (size_t)t.n, &pos));
  hipLaunchKernelGGL(shard_fast_cand_kernel, dim3(div_up(t.n, 256)), dim3(256), 0, c->stream, t.keys, t.n, pos, t.level, t.dup,
                     t.fast_start - 1, (1 == t.fast_start) ? 0u : 2u, t.sp, d_keys_out, d_xyz_out);
  SWZ_LAUNCH_CHECK(c);
  return SWZ_OK;
}

int shard_fast_set_root_device(swz_ctx* c, const uint8_t* d_taken) {
  ShardState* s = shard_state(c);
  if (!s->open || !s->fast) return c->fail(SWZ_ERR_BAD_ARG, "swz_shard_fast_set_root_device: no FAST sharded batch is open");
  if (s->empty || !s->fast_candidates) return SWZ_OK;
  TileSession& t = s->t;
  uint32_t* pos = nullptr;
  SWZ_TRY(c->get("shard_fast_pos", (size_t)t.n, &pos));
  hipLaunchKernelGGL(shard_fast_mark_root_kernel, dim3(div_up(t.n, 256)), dim3(256), 0, c->stream, t.n, pos, t.level, t.dup,
                     t.fast_start - 1, (1 == t.fast_start) ? 0u : 2u, d_taken);
  SWZ_LAUNCH_CHECK(c);
  return SWZ_OK;
}

int shard_fast_finish_device(swz_ctx* c, uint64_t* d_keys_out, uint32_t* d_perm_out, int8_t* d_level_out, uint32_t* d_dup_out,
                             swz_tile_stats* stats) {
  ShardState* s = shard_state(c);
  if (!s->open || !s->fast) return c->fail(SWZ_ERR_BAD_ARG, "swz_shard_fast_finish_device: no FAST sharded batch is open");
  s->open = false;
  s->fast = false;
  if (!s->empty) {
    hipLaunchKernelGGL(shard_fast_strip_kernel, dim3(div_up(s->n_local, 256)), dim3(256), 0, c->stream, s->t.keys, s->t.perm, s->t.level,
                       s->t.dup, s->n_local, d_keys_out, d_perm_out, d_level_out, d_dup_out);
    SWZ_LAUNCH_CHECK(c);
  }
  s->empty = false;
  session_stats(s->t, stats);
  return SWZ_OK;
}

}  // namespace swz
