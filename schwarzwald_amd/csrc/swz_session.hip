// swz_session.hip -- the driver of a single batch: index, sort, the level loop (ACCURATE), the start level and the
// reconstruction of the skipped levels (FAST), and swz_sample_points on one node's range.  A sharded batch runs the same
// session in pieces (swz_shard.hip); the multi-batch tiler has a loop of its own (swz_tiler.hip).
#include <algorithm>
#include <string>
#include <vector>

#include "swz_md.h"
#include "swz_session.h"

namespace swz {

// positions of the session's points into Morton order (once)
static int session_gather_positions(swz_ctx* c, TileSession& t) {
  if (t.sp.X) return SWZ_OK;
  double *X = nullptr, *Y = nullptr, *Z = nullptr;
  SWZ_TRY(c->get("sorted_x", (size_t)t.n + t.front, &X));
  SWZ_TRY(c->get("sorted_y", (size_t)t.n + t.front, &Y));
  SWZ_TRY(c->get("sorted_z", (size_t)t.n + t.front, &Z));
  SWZ_STAGE(c, "sort");
  const uint32_t g = t.sp.ghosts;
  if (g) {
    // ghosts are attached already (a sharded batch whose earlier levels were decided on keys): they lead the sorted
    // order and their perm entries index the ghost array.  They matter at the root level only -- later the caller's
    // ghost array may be gone, and nobody reads those entries any more.
    if (t.next_level <= -1) SWZ_TRY(gather_positions(c, t.sp.ghost_xyz, t.perm, g, X, Y, Z));
    SWZ_TRY(gather_positions(c, t.xyz_in, t.perm + g, t.n - g, X + g, Y + g, Z + g));
  } else {
    X += t.front;
    Y += t.front;
    Z += t.front;
    SWZ_TRY(gather_positions(c, t.xyz_in, t.perm, t.n, X, Y, Z));
  }
  SWZ_STAGE(c, "gather");
  t.sp.X = X;
  t.sp.Y = Y;
  t.sp.Z = Z;
  return SWZ_OK;
}
// a level that cannot be decided on keys needs them
static int session_need_positions(swz_ctx* c, TileSession& t, const LevelPlan& plan) {
  if (t.sp.X || level_decides_on_keys(c, plan, t.sp)) return SWZ_OK;
  return session_gather_positions(c, t);
}

int session_prepare(swz_ctx* c, TileSession& t, double* d_xyz, uint32_t n, const double bmin[3], const double bmax[3],
                    const swz_tile_params& p, const TileDeviceOut& out, uint32_t front) {
  t = TileSession{};
  t.n = n;
  for (int a = 0; a < 3; ++a) {
    t.bmin[a] = bmin[a];
    t.bmax[a] = bmax[a];
  }
  t.params = p;
  t.keys = out.keys;
  t.perm = out.perm;
  t.level = out.level;
  t.dup = out.dup;
  t.xyz_in = d_xyz;
  uint64_t* keys_b = nullptr;
  uint32_t* vals_b = nullptr;
  SWZ_TRY(c->get("sort_keys_b", (size_t)n, &keys_b));
  SWZ_TRY(c->get("sort_vals_b", (size_t)n, &vals_b));
  // (encoded into the sort's first pair: the sorted result lands in the output buffers)
  SWZ_TRY(encode_device(c, d_xyz, n, bmin, bmax, keys_b));
  SWZ_STAGE(c, "encode");
  SWZ_TRY(radix_sort_pairs(c, keys_b, vals_b, out.keys, out.perm, n, true));
  // The positions in Morton order (SoA).  RANDOM_GRID decides on the keys alone.  MIN_DISTANCE decides on the key
  // coordinates and looks up the pairs inside the quantisation band through the permutation (swz_mqsweep.hip): there
  // the gather is put off until a level asks for it (session_need_positions) -- for cubic bounds and exact mode that is
  // a level so deep that its spacing spans fewer than 64 key cells, which few clouds reach.  Sharded batches that
  // prepend ghosts (front > 0) look up two position arrays: the sorted positions in front are the ghosts
  // (shard_attach_ghosts; sorted_point_xyz).
  t.sp = SortedPoints{nullptr, nullptr, nullptr, d_xyz, out.perm};
  t.front = front;
  const LevelPlan top = make_plan(-1, p.sampler, p.max_points_per_node, p.spacing_at_root, p.max_depth, bmin, bmax, false, true);
  SWZ_TRY(session_need_positions(c, t, top));
  if (out.dup) SWZ_HIP(c, hipMemsetAsync(out.dup, 0, (size_t)n * 4, c->stream));
  SWZ_HIP(c, hipMemsetAsync(out.level, 0x80, (size_t)n, c->stream));  // -128 = not persisted yet
  SWZ_TRY(alloc_level_buffers(c, n + front, &t.lb));
  // survivors ping-pong between the sort's secondary buffers and one extra pair
  t.key_buf[0] = keys_b;
  t.idx_buf[0] = vals_b;
  t.as = ActiveSet{out.keys, nullptr, n};
  return SWZ_OK;
}

// Who defers its compaction is decided here and nowhere else.  A level leaves its survivors where they are -- the next
// level then runs on the same key / index arrays and gets the taken bytes as ActiveSet::gone -- when
//   * the caller allows chains at all (the single batch of swz_tile*, ACCURATE), the sampler is MIN_DISTANCE in exact
//     mode, nothing is sharded or forced, and SWZ_MD_DEFER is not 0;
//   * the key sweep with direct numbering sampled this level (level_step reports it);
//   * the next level is neither terminal nor re-rooted;
//   * the taken points stay below SWZ_MD_DEFER_MAX_GONE of the shared arrays (1/8: beyond that the dead bytes every sweep
//     steps over cost more than a quarter of the copy saved; reasoned, not measured).
// Whether the key sweep takes the NEXT level as well is known only once that level has been surveyed: if it does not, the
// level hands the arrays back untouched (LevelResult::needs_flush), the chain's one compaction runs and the level starts
// again on the compacted arrays.
int session_run_levels(swz_ctx* c, TileSession& t, int last_level, int first_mode, bool chains) {
  const uint64_t* pprefix = nullptr;
  uint32_t parents = 0;
  const bool chain_static = chains && first_mode < 0 && t.params.sampler == SWZ_MIN_DISTANCE &&
                            !(t.params.flags & SWZ_FLAG_MIN_DISTANCE_PROPERTY) && !t.sp.ghosts && !t.front && !c->shard &&
                            !c->md_shard_root && c->opt_on("SWZ_MD_DEFER", true);
  const bool prebuild = chain_static && c->opt_on("SWZ_MD_PREBUILD", true);
  c->mq_pre.valid = false;  // (tables built ahead never outlive the call that built them)
  LevelChain chain;
  chain.max_gone = c->opt_num("SWZ_MD_DEFER_MAX_GONE", 0.125);
  for (int level = t.next_level; (t.as.gone ? t.as.live : t.as.m) > 0 && level <= last_level; ++level) {
    if (level > 20) return c->fail(SWZ_ERR_INTERNAL, "level loop ran past level 20");
    if (!t.key_buf[t.which]) {
      SWZ_TRY(c->get("active_keys_2", (size_t)t.as.m, &t.key_buf[t.which]));
      SWZ_TRY(c->get("active_idx_2", (size_t)t.as.m, &t.idx_buf[t.which]));
    }
    LevelPlan plan = make_plan(level, t.params.sampler, t.params.max_points_per_node, t.params.spacing_at_root,
                               t.params.max_depth, t.bmin, t.bmax, false, true);
    plan.md_property = (t.params.flags & SWZ_FLAG_MIN_DISTANCE_PROPERTY) != 0;
    chain.may_defer = false;
    c->mq_pre.wanted = false;
    if (chain_static && level < 20) {
      const LevelPlan next = make_plan(level + 1, t.params.sampler, t.params.max_points_per_node, t.params.spacing_at_root,
                                       t.params.max_depth, t.bmin, t.bmax, false, true);
      chain.may_defer = !plan.terminal && !plan.reroot && !next.terminal && !next.reroot;
      // A level that may leave its survivors in place is followed by one on the same keys: should the key sweep take this
      // level, it builds that level's early tables under its own rounds (mq_prebuild_launch), for the grid guessed here from
      // the geometry and the points still open.  SWZ_MD_PREBUILD=0: never.
      if (chain.may_defer && prebuild) (void)md_guess_chained_level(c, next, t.sp, t.as.gone ? t.as.live : t.as.m, &c->mq_pre);
    }
    if (chain.may_defer || t.as.gone) plan.take_code = (uint8_t)(level + 2);
    // (the root of a sharded batch spans the shards: it is sampled exactly -- the lower shards' samples as ghosts, or all
    // shards sweeping together -- which has the property a fortiori; the flag decides the levels below)
    if (first_mode >= 0 && level == t.next_level) plan.md_property = false;
    if (first_mode >= 0 && level == t.next_level && !plan.terminal) {
      if (first_mode == 1) {
        plan.force_sample = true;
      } else {
        plan.max_points = ~0ull;
      }
    }
    SWZ_TRY(session_need_positions(c, t, plan));
    LevelResult r;
    t.as.parent_prefix = pprefix;
    t.as.parents = pprefix ? parents : 0u;
    const uint32_t found_tables = c->mq_pre.valid ? c->mq_pre.serial : 0u;
    const int step_status = level_step(c, plan, t.as, t.sp, t.lb, t.level, t.key_buf[t.which], t.idx_buf[t.which], &r, &chain);
    c->mq_pre.wanted = false;  // (a request no key sweep picked up ends with its level)
    SWZ_TRY(step_status);
    if (found_tables && c->mq_pre.valid && c->mq_pre.serial == found_tables && !r.needs_flush) {
      c->mq_pre.valid = false;  // tables built ahead for a level that went to no key sweep (take-all nodes, the block kernel after the flush)
      c->prof_count("mq_prebuild_dropped", 1);
    }
    if (r.needs_flush) {
      // the chain ends in front of this level: its one compaction, then the level again on the survivors
      if (!t.as.gone) return c->fail(SWZ_ERR_INTERNAL, "a level outside a chain asked for the chain's compaction");
      uint32_t remaining = 0;
      SWZ_TRY(level_flush_chain(c, t.as, t.lb, t.level, t.key_buf[t.which], t.idx_buf[t.which], &remaining));
      t.as = ActiveSet{t.key_buf[t.which], t.idx_buf[t.which], remaining};
      t.which ^= 1;
      --level;
      continue;
    }
    t.visited += t.as.gone ? t.as.live : t.as.m;
    t.nodes += r.num_nodes;
    t.rounds += r.md_rounds;
    t.max_level = level;
    ++t.nlevels;
    if (r.deferred) {  // the same arrays once more, with the taken bytes
      t.as.gone = t.lb.taken;
      t.as.gone_tiles = r.gone_tiles;
      t.as.live = r.remaining;
    } else {
      t.as = ActiveSet{t.key_buf[t.which], t.idx_buf[t.which], r.remaining};
      t.which ^= 1;
    }
    // (the nodes of this level for the next one's segmentation -- inside this call only: between two calls of a sharded
    // batch other work of the context may reuse the buffer)
    pprefix = r.node_prefix;
    parents = r.table_nodes;
    t.next_level = level + 1;
  }
  return SWZ_OK;
}

void session_stats(const TileSession& t, swz_tile_stats* stats) {
  if (!stats) return;
  stats->num_nodes = t.nodes;
  stats->points_visited = t.visited;
  stats->max_level = t.max_level;
  stats->fast_start_levels = t.fast_start;
  stats->num_levels = t.nlevels;
  stats->min_distance_rounds = t.rounds;
}

// ---- FAST (TilingAlgorithmV3) -------------------------------------------------------------------
// first index whose 6-octant prefix is >= bin, for every bin of the 8^6 grid (+ the end sentinel)
__global__ __launch_bounds__(256) void prefix_bounds_kernel(const uint64_t* __restrict__ keys, uint32_t n,
                                                            uint32_t* __restrict__ starts, uint32_t nbins) {
  const uint32_t b = blockIdx.x * 256 + threadIdx.x;
  if (b > nbins) return;
  if (b == nbins) {
    starts[b] = n;
    return;
  }
  const uint64_t target = (uint64_t)b << 45;  // 63 - 6*3
  uint32_t lo = 0, hi = n;
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (keys[mid] < target) lo = mid + 1; else hi = mid;
  }
  starts[b] = lo;
}

// estimate_start_node_level_in_octree -- TilingAlgorithms.cpp:1473-1535, from the 6-level prefix counts
static size_t estimate_start_level_host(const std::vector<uint32_t>& starts6, size_t concurrency) {
  constexpr uint32_t MIN_LEVEL = 3, MAX_LEVEL = 6;
  constexpr float MIN_SCORE = 1.f;
  for (uint32_t level = 0; level < MAX_LEVEL; ++level) {
    const uint32_t digits = level + 1;
    const uint32_t group = 1u << (3 * (6 - digits));  // 6-digit bins per range at this level
    size_t ranges = 0, large = 0;
    for (uint32_t b = 0; b < (1u << 18); b += group) {
      const uint32_t cnt = starts6[b + group] - starts6[b];
      if (cnt > 0) ++ranges;
      if (cnt >= 100000) ++large;
    }
    float score = 0.f;
    if (!(ranges <= concurrency / 2)) score = static_cast<float>(large) / static_cast<float>(concurrency);
    if (score >= MIN_SCORE) return std::max(level + 1, MIN_LEVEL);
  }
  return MAX_LEVEL;
}

// children's persisted points of the nodes being reconstructed (recon_candidate)
__global__ __launch_bounds__(256) void recon_select_kernel(const int8_t* __restrict__ level,
                                                           const uint32_t* __restrict__ dup, uint32_t n,
                                                           int start_node_level, uint32_t child_bit,
                                                           uint32_t* __restrict__ flags) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  flags[i] = recon_candidate(level, dup, i, start_node_level, child_bit) ? 1u : 0u;
}
__global__ __launch_bounds__(256) void recon_gather_kernel(const uint64_t* __restrict__ keys, uint32_t n,
                                                           const uint32_t* __restrict__ flags_in_scanned,
                                                           const int8_t* __restrict__ level,
                                                           const uint32_t* __restrict__ dup, int start_node_level,
                                                           uint32_t child_bit, uint64_t* __restrict__ okey,
                                                           uint32_t* __restrict__ oidx) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  if (recon_candidate(level, dup, i, start_node_level, child_bit)) {
    const uint32_t o = flags_in_scanned[i];
    okey[o] = keys[i];
    oidx[o] = i;
  }
}
__global__ __launch_bounds__(256) void recon_mark_kernel(const uint32_t* __restrict__ aidx, uint32_t m,
                                                         const uint8_t* __restrict__ taken, uint32_t bit,
                                                         uint32_t* __restrict__ dup) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i < m && taken[i]) dup[aidx[i]] |= bit;
}

// points per 6-octant prefix of a sorted batch (what the start-level estimate looks at), host array of 2^18 counts
int fast_prefix_counts(swz_ctx* c, const uint64_t* d_keys_sorted, uint32_t n, uint32_t* counts_host) {
  const uint32_t nbins = 1u << 18;
  uint32_t* d_starts = nullptr;
  SWZ_TRY(c->get("fast_starts", (size_t)nbins + 1, &d_starts));
  std::vector<uint32_t> starts(nbins + 1, 0);
  if (n) {
    hipLaunchKernelGGL(prefix_bounds_kernel, dim3(div_up(nbins + 1, 256)), dim3(256), 0, c->stream, d_keys_sorted, n, d_starts, nbins);
    SWZ_LAUNCH_CHECK(c);
    SWZ_HIP(c, hipMemcpyAsync(starts.data(), d_starts, (nbins + 1) * 4, hipMemcpyDeviceToHost, c->stream));
    SWZ_HIP(c, hipStreamSynchronize(c->stream));
  }
  for (uint32_t b = 0; b < nbins; ++b) counts_host[b] = starts[b + 1] - starts[b];
  return SWZ_OK;
}
// the estimate from counts that may be the sum over the shards of a batch (each below 2^32 in total)
int fast_start_level_from_counts(const uint64_t* counts, uint32_t concurrency) {
  std::vector<uint32_t> starts((1u << 18) + 1, 0);
  uint64_t run = 0;
  for (uint32_t b = 0; b < (1u << 18); ++b) {
    starts[b] = (uint32_t)std::min<uint64_t>(run, 0xFFFFFFFFull);
    run += counts[b];
  }
  starts[1u << 18] = (uint32_t)std::min<uint64_t>(run, 0xFFFFFFFFull);
  return (int)estimate_start_level_host(starts, concurrency);
}

int fast_start_level(swz_ctx* c, const uint64_t* d_keys_sorted, uint32_t n, uint32_t concurrency, int* start_level) {
  const uint32_t nbins = 1u << 18;
  uint32_t* d_starts = nullptr;
  SWZ_TRY(c->get("fast_starts", (size_t)nbins + 1, &d_starts));
  hipLaunchKernelGGL(prefix_bounds_kernel, dim3(div_up(nbins + 1, 256)), dim3(256), 0, c->stream, d_keys_sorted, n,
                     d_starts, nbins);
  SWZ_LAUNCH_CHECK(c);
  std::vector<uint32_t> starts(nbins + 1);
  SWZ_HIP(c, hipMemcpyAsync(starts.data(), d_starts, (nbins + 1) * 4, hipMemcpyDeviceToHost, c->stream));
  SWZ_HIP(c, hipStreamSynchronize(c->stream));
  *start_level = (int)estimate_start_level_host(starts, concurrency);
  return SWZ_OK;
}

// FAST: reconstruct the skipped levels S-1 .. lowest_lv, deepest first: a node with lv octants samples the points
// persisted by its (up to) 8 children with AlwaysAdhereToMinSpacing (reconstruct_single_node :1661-1715).
// lowest_lv = 0 includes the root; a shard of a sharded batch stops at 1 (the root's children lie on several shards).
int session_recon_ranks(swz_ctx* c, TileSession& t, int S, uint32_t child_bit, uint32_t* pos) {
  hipLaunchKernelGGL(recon_select_kernel, dim3(div_up(t.n, 256)), dim3(256), 0, c->stream, t.level, t.dup, t.n, S - 1, child_bit, pos);
  SWZ_LAUNCH_CHECK(c);
  SWZ_HIP(c, hipMemsetAsync(t.lb.counters, 0, CTR_COUNT * sizeof(uint32_t), c->stream));
  return scan_exclusive_u32(c, pos, pos, t.n, t.lb.counters + CTR_REMAINING, "rec");
}

int session_fast_reconstruct(swz_ctx* c, TileSession& t, const swz_tile_params& p, int S, int lowest_lv) {
  const uint32_t n = t.n;
  const double* bmin = t.bmin;
  const double* bmax = t.bmax;
  uint64_t* rkey = nullptr;
  uint32_t* ridx = nullptr;
  SWZ_TRY(c->get("recon_keys", (size_t)n, &rkey));
  SWZ_TRY(c->get("recon_idx", (size_t)n, &ridx));
  const uint32_t nb = div_up(n, 256);
  for (int lv = S - 1; lv >= lowest_lv; --lv) {
    const uint32_t child_bit = (lv + 1 == S) ? 0u : (1u << (lv + 1));
    SWZ_TRY(session_recon_ranks(c, t, S, child_bit, t.lb.flags));
    hipLaunchKernelGGL(recon_gather_kernel, dim3(nb), dim3(256), 0, c->stream, t.keys, n, t.lb.flags, t.level, t.dup,
                       S - 1, child_bit, rkey, ridx);
    SWZ_LAUNCH_CHECK(c);
    uint32_t m = 0;
    SWZ_TRY(read_u32(c, t.lb.counters + CTR_REMAINING, &m));
    if (m == 0) continue;
    LevelPlan plan = make_plan(lv - 1, p.sampler, p.max_points_per_node, p.spacing_at_root, p.max_depth, bmin,
                               bmax, true, false);
    plan.md_property = (p.flags & SWZ_FLAG_MIN_DISTANCE_PROPERTY) != 0;
    ActiveSet as{rkey, ridx, m};
    SWZ_TRY(session_need_positions(c, t, plan));
    LevelResult r;
    SWZ_TRY(level_step(c, plan, as, t.sp, t.lb, nullptr, nullptr, nullptr, &r));
    hipLaunchKernelGGL(recon_mark_kernel, dim3(div_up(m, 256)), dim3(256), 0, c->stream, ridx, m, t.lb.taken,
                       1u << lv, t.dup);
    SWZ_LAUNCH_CHECK(c);
    t.nodes += r.num_nodes;
    t.rounds += r.md_rounds;
  }
  return SWZ_OK;
}

int tile_device(swz_ctx* c, double* d_xyz, uint32_t n, const double bmin[3], const double bmax[3],
                const swz_tile_params& p, const TileDeviceOut& out_in, swz_tile_stats* stats) {
  TileDeviceOut out = out_in;
  if (p.strategy == SWZ_FAST && !out.dup) SWZ_TRY(c->get("fast_dup", (size_t)n, &out.dup));
  TileSession t;
  SWZ_TRY(session_prepare(c, t, d_xyz, n, bmin, bmax, p, out));
  if (p.strategy == SWZ_ACCURATE) {
    SWZ_TRY(session_run_levels(c, t, 20, -1, true));
    session_stats(t, stats);
    return SWZ_OK;
  }
  // ---- FAST: TilingAlgorithmV3 first iteration (:1250-1360) + finalize (:1717-1784)
  int S = 0;
  SWZ_TRY(fast_start_level(c, t.keys, n, p.fast_concurrency, &S));
  t.fast_start = S;
  // every point starts in the node made of its first S octants (split_indexed_points_into_subranges)
  t.next_level = S - 1;
  SWZ_TRY(session_run_levels(c, t, 20, -1));
  SWZ_TRY(session_fast_reconstruct(c, t, p, S, 0));
  session_stats(t, stats);
  return SWZ_OK;
}

__global__ __launch_bounds__(256) void count_taken_kernel(const uint8_t* __restrict__ taken, uint32_t n,
                                                          uint32_t* __restrict__ count) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  const bool t = (i < n) && taken[i];
  const uint64_t b = __ballot(t);
  if (lane_id() == 0 && b) atomicAdd(count, (uint32_t)__popcll(b));
}

// every key of the range must lie in the node: the reference takes the node's bounds from node_key
// (Sampling.h:441, 622), this implementation from the keys' own prefix -- the two agree exactly then
__global__ __launch_bounds__(256) void node_key_check_kernel(const uint64_t* __restrict__ keys, uint32_t n, uint32_t nsh,
                                                             uint64_t prefix, uint32_t* __restrict__ bad) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  const bool b = i < n && (keys[i] >> nsh) != prefix;
  const uint64_t m = __ballot(b);
  if (lane_id() == 0 && m) atomicAdd(bad, (uint32_t)__popcll(m));
}

int sample_points_device(swz_ctx* c, int sampler, uint64_t max_points, const uint64_t* d_keys, const uint32_t* d_idx,
                         uint32_t n, const double* d_xyz, uint64_t node_key, int32_t node_level,
                         const double rmin[3], const double rmax[3], float spacing, int behaviour, uint8_t* d_taken,
                         uint64_t* num_taken) {
  // RANDOM_GRID and GRID_CENTER never look at node_key: the whole range is "the node" (count, candidate level from
  // node_level; the reference's own test samples a range spanning all octants at node level 0,
  // test/TestOctreeIndexing.cpp:169-252).  MIN_DISTANCE and JITTERED take the node's box from node_key.
  const bool uses_node_key = greedy_sampler(sampler) || sampler == SWZ_JITTERED;
  if (node_level >= 0 && uses_node_key) {
    uint32_t* d_bad = nullptr;
    SWZ_TRY(c->get("lvl_counters", (size_t)CTR_COUNT, &d_bad));
    SWZ_HIP(c, hipMemsetAsync(d_bad, 0, sizeof(uint32_t), c->stream));
    const uint32_t nsh = level_shift(node_level);
    hipLaunchKernelGGL(node_key_check_kernel, dim3(div_up(n, 256)), dim3(256), 0, c->stream, d_keys, n, nsh,
                       node_key >> nsh, d_bad);
    SWZ_LAUNCH_CHECK(c);
    uint32_t bad = 0;
    SWZ_TRY(read_u32(c, d_bad, &bad));
    if (bad) return c->fail(SWZ_ERR_BAD_ARG, "swz_sample_points: " + std::to_string(bad) + " keys of the range do not lie in node_key's node");
  }
  double *X = nullptr, *Y = nullptr, *Z = nullptr;
  SWZ_TRY(c->get("sorted_x", (size_t)n, &X));
  SWZ_TRY(c->get("sorted_y", (size_t)n, &Y));
  SWZ_TRY(c->get("sorted_z", (size_t)n, &Z));
  SWZ_TRY(gather_positions(c, d_xyz, d_idx, n, X, Y, Z));
  LevelBuffers lb;
  SWZ_TRY(alloc_level_buffers(c, n, &lb));
  LevelPlan plan = make_plan(node_level, sampler, max_points, spacing, 100, rmin, rmax,
                             behaviour == SWZ_ALWAYS_ADHERE_TO_MIN_SPACING, false);
  if (!uses_node_key) plan.node_shift = 63;  // one node: the range
  ActiveSet as{d_keys, nullptr, n};
  SortedPoints sp{X, Y, Z, d_xyz, d_idx};
  LevelResult r;
  SWZ_TRY(level_step(c, plan, as, sp, lb, nullptr, nullptr, nullptr, &r));
  SWZ_HIP(c, hipMemcpyAsync(d_taken, lb.taken, n, hipMemcpyDeviceToDevice, c->stream));
  if (num_taken) {
    SWZ_HIP(c, hipMemsetAsync(lb.counters, 0, sizeof(uint32_t), c->stream));
    hipLaunchKernelGGL(count_taken_kernel, dim3(div_up(n, 256)), dim3(256), 0, c->stream, lb.taken, n, lb.counters);
    SWZ_LAUNCH_CHECK(c);
    uint32_t cnt = 0;
    SWZ_TRY(read_u32(c, lb.counters, &cnt));
    *num_taken = cnt;
  }
  return SWZ_OK;
}

}  // namespace swz
