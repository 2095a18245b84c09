// swz_mdkeys.hip -- MIN_DISTANCE frontier sweep on KEY COORDINATES: the exact greedy set without moving positions.
//
// Reference: PoissonDiskSampling::sample_points (core/tiling/Sampling.h:421-471) + SparseGrid::add
// (core/datastructures/SparseGrid.cpp:116-146) + GridCell::isDistant (GridCell.cpp:43-58); the result is the
// lexicographically-first maximal independent set in Morton order (see swz_mindist.hip for the derivation and the
// frontier rules (R) / (A), which are the same here).
//
// What is different from swz_mindist.hip:
//  * A Morton key IS the position, quantised to 2^-21 of the (cubic) bounds.  For two points with integer key
//    coordinates i, j the true distance in key cells lies within sqrt(3) of |i - j| (each coordinate is somewhere in its
//    cell), so "closer than the spacing?" is decided on the keys unless |i - j| falls into a band of +-1.75 cells around
//    the spacing (14 530 cells at the root for spacing = diagonal / 250).  Only those pairs are evaluated on the exact
//    positions, with the reference's arithmetic, through the sort's permutation.  Blocker scans need no exact answer at
//    all: "possibly closer" keeps a cell waiting, which is always allowed.  Nothing is gathered: a cell's points are a
//    run of the level's sorted keys (8 coalesced bytes per point instead of 24 gathered ones).
//  * A point that is known to be rejected (closer than the spacing to an accepted earlier point) gets a state byte, so a
//    cell tests each of its points against the accepted points of its neighbourhood once -- not again on every
//    activation -- and blocker scans skip dead points without testing them.
//  * ONE launch per round.  A cell's record (frontier, accepted points) is double buffered and stamped with the round
//    that wrote it: an activation reads, of every adjacent cell, the newer record written BEFORE this round (stable: its
//    owner writes the other one) and writes its own new record itself -- no second launch that publishes.  Sleeping and
//    waking without that launch: a cell that stalls writes {point it waits for, round} into the blocking cell's slot for
//    its direction and queues itself once more ("confirm": one round later the blocker's record of THIS round is stable
//    and says whether the point has been passed meanwhile).  A cell whose frontier moves claims the slots it has passed
//    with a compare-and-swap and queues their owners -- except slots stamped with the current round, whose owners
//    confirm themselves.  Whoever wins the compare-and-swap activates the sleeper, so a cell is never queued twice.
//
// Where what is: this file decides whether and how a level is taken and runs it, step by step (min_distance_keys_level);
// swz_mqbuild.hip builds the level's tables, swz_mqsweep.hip holds the activation and everything a round launches;
// swz_mdkeys.h is what the three share.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "swz_mdkeys.h"

namespace swz {

// ----------------------------------------------------------------------------- thresholds in key cells
KeyMetric key_metric(const swz_ctx* c, const LevelPlan& plan, const SortedPoints& sp) {
  KeyMetric k;
  if (!sp.xyz || !sp.perm) return k;
  if (!c->opt_on("SWZ_MD_KEYS", true)) return k;
  const double ex = plan.root.maxx - plan.root.minx, ey = plan.root.maxy - plan.root.miny, ez = plan.root.maxz - plan.root.minz;
  if (!(ex > 0.0) || ex != ey || ey != ez) return k;  // one key cell must be a cube (the Tiler's bounds are)
  const double cell = ex / 2097152.0;
  const double T = std::sqrt(plan.sq_spacing) / cell;
  // below that most near pairs fall into the band (levels >= 7 at spacing = diagonal / 250)
  const double tmin = c->opt_num("SWZ_MD_KEYS_MIN_CELLS", 64.0);
  if (!(T >= tmin) || !(T < 4.0e6)) return k;
  // A coordinate u = (p - min) * scale (calculate_morton_index, OctreeAlgorithms.h:64-87) has key coordinate
  // i = min(trunc(fl(u)), 2^21 - 1): u is within [i, i + 1] up to the rounding of fl (1e-9 cells).  Per axis
  // |du - di| <= 1 + 2e-9, so | |du| - |di| | <= sqrt(3) (1 + 2e-9) < 1.7321.  The squared integer distance is evaluated
  // in float (exact differences, three roundings: relative 3 * 2^-24, i.e. T * 2^-23 cells of distance near the
  // spacing).  Band: 1.75 + T * 2^-20 cells -- the reference's own rounding (1e-16 relative) disappears in the slack.
  double band = 1.75 + T * 0x1.0p-20;
  band += c->opt_num("SWZ_MD_KEYS_BAND", 0.0);  // tests: a wide band sends many / all pairs to the exact path
  const double lo = T - band, hi = T + band;
  float f_lo = 0.f;
  if (lo > 0.0) {
    f_lo = (float)(lo * lo);
    while ((double)f_lo > lo * lo) f_lo = std::nextafterf(f_lo, 0.f);
    f_lo = std::nextafterf(f_lo, 0.f);
  }
  float f_hi = (float)(hi * hi);
  while ((double)f_hi < hi * hi) f_hi = std::nextafterf(f_hi, INFINITY);
  f_hi = std::nextafterf(f_hi, INFINITY);
  k.T = T;
  k.f_lo = f_lo;
  k.f_hi = f_hi;
  k.ok = true;
  return k;
}

// (with ghosts in front -- a sharded batch --: ghost g keeps its index into the ghost array, local point p becomes
// ghosts + p: one id space, see SpArgs)
__global__ __launch_bounds__(256) void mq_point_ids_kernel(const uint32_t* __restrict__ aidx, const uint32_t* __restrict__ perm, uint32_t m,
                                                           uint32_t ghosts, uint32_t* __restrict__ ids) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= m) return;
  const uint32_t s = aidx ? aidx[i] : i;
  ids[i] = s < ghosts ? perm[s] : ghosts + perm[s];
}
int key_point_ids(swz_ctx* c, const ActiveSet& as, const SortedPoints& sp, const uint32_t** ids) {
  if (!as.aidx && !sp.ghosts) {
    *ids = sp.perm;
    return SWZ_OK;
  }
  uint32_t* d = nullptr;
  SWZ_TRY(c->get("md_qids", (size_t)as.m, &d));
  hipLaunchKernelGGL(mq_point_ids_kernel, dim3(div_up(as.m, 256)), dim3(256), 0, c->stream, as.aidx, sp.perm, as.m, sp.ghosts, d);
  SWZ_LAUNCH_CHECK(c);
  *ids = d;
  return SWZ_OK;
}

// ----------------------------------------------------------------------------- host
bool min_distance_level_uses_keys(const swz_ctx* c, const LevelPlan& plan, const SortedPoints& sp) {
  return key_metric(c, plan, sp).ok;  // (property mode decides on keys as well: swz_mdrounds.hip, or the exact set)
}

// ---- the steps of a level, in the order min_distance_keys_level (below) takes them
// What the kernels need to know of the level; over when the level cannot be decided on keys.
static int mq_fill_args(const swz_ctx* c, MqLevel& q) {
  const MdLevel& L = q.L;
  if (!L.km.ok) {
    q.over = true;
    return SWZ_OK;
  }
  q.sharded = q.shard_root != nullptr && q.shard_root->shards > 1;
  q.sfx = q.sharded ? "_sr" : "";
  MqArgs& a = q.a;
  a.akey = L.as.akey;
  a.aidx = L.as.aidx;
  a.m = L.as.m;
  a.nid = L.lb.nid;
  a.nmode = L.lb.nmode;
  a.nstart = L.lb.nstart;
  a.xyz = L.sp.xyz;
  a.perm = L.sp.perm;
  a.gxyz = L.sp.ghost_xyz;
  a.ng = L.sp.ghosts;
  a.taken = L.lb.taken;
  a.counters = L.lb.counters;
  a.snode_of = L.snode_of;
  a.cells_per_node = 1ull << (3 * q.cl);
  a.cpn_shift = 3u * (uint32_t)q.cl;
  a.cell_levels = (uint32_t)q.cl;
  a.peers.shards = q.sharded ? (uint32_t)q.shard_root->shards : 1u;
  a.peers.shard = q.sharded ? (uint32_t)q.shard_root->shard : 0u;
  a.cell_shift = L.plan.node_shift - 3u * (uint32_t)q.cl;
  a.cell_bits = a.cell_shift / 3u;
  a.f_lo = L.km.f_lo;
  a.f_hi = L.km.f_hi;
  a.sq_spacing = L.plan.sq_spacing;
  a.all_sampled = L.all_sampled ? 1u : 0u;
  a.no_dead_test = c->opt_on("SWZ_MD_NO_DEAD_TEST", false) ? 1u : 0u;
  a.stats = c->opt("SWZ_MD_STATS") ? 1u : 0u;
  // (measured at 1 B points: 2 cells per chain root / level 0 / level 1 78 / 69 / 96 -> 73 / 62 / 91 ms; longer chains make
  // launches as long as their longest chain and lose again)
  a.chain = std::min<uint32_t>(MQ_CHAIN, (uint32_t)std::max(1L, c->opt_int("SWZ_MD_CHAIN", 2)));
  if (a.cell_bits > 21u) q.over = true;
  return SWZ_OK;
}

// A cell r spacings wide ends with about 0.75 r^3 accepted points: records of 3 or 7 inline ones, the rest in the
// overflow.  (Small records win well beyond their capacity -- level 1 at 1 B points, cells two spacings wide with ~6
// accepted points each: 78 ms with records of 3, 84 with records of 7: less to stage, more wavefronts per CU.)
uint32_t key_sweep_record_granules(const swz_ctx* c, uint32_t cell_bits, double T) {
  const double r_cell = std::ldexp(1.0, (int)cell_bits) / T;
  const uint32_t rg = (0.75 * r_cell * r_cell * r_cell <= 12.0) ? 4u : 8u;
  return c->opt_int("SWZ_MD_KEYS_RG", rg) >= 8 ? 8u : 4u;
}

// Record size and how the cells are numbered; over when a level inside a chain would not get direct numbering.
static int mq_choose_records_and_numbering(const swz_ctx* c, MqLevel& q, bool* direct_out) {
  MqArgs& a = q.a;
  a.rg = key_sweep_record_granules(c, a.cell_bits, q.L.km.T);
  a.rg2_shift = a.rg == 4u ? 3u : 4u;
  // How the cells are numbered (MqArgs::direct).  By their place in the grid when most of the grid is occupied -- the
  // caller's estimate from THIS call's keys (from half of it on) -- and the per-cell arrays of the whole
  // grid fit what the device has left (plus what the arrays of the level before hold: they are reused).  The joint root
  // of a sharded batch keeps the compacted cells: its shards publish gridmap to each other.
  q.grid_entries = (uint64_t)q.L.sample_nodes * a.cells_per_node;
  const size_t per_cell = sizeof(uint2) + 32u * 4u + 2u * a.rg * sizeof(uint4) + 32u * 8u + sizeof(uint4) + 5u;
  uint64_t max_cells = 0x7FFFFFF0ull;
  if (const char* mc = c->opt("SWZ_MD_DIRECT_MAX_CELLS")) {
    max_cells = std::min<uint64_t>(max_cells, (uint64_t)std::max(0LL, atoll(mc)));
  } else {
    size_t free_b = 0, total_b = 0, held = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) free_b = 0;
    for (const auto& kv : c->bufs)
      if (!kv.second.host && kv.first.compare(0, 4, "md_q") == 0 &&
          !(kv.first.size() > 2 && kv.first.compare(kv.first.size() - 2, 2, "_b") == 0))  // (not the second set of tables built ahead: a level that builds its own never runs on it)
        held += kv.second.cap;
    max_cells = std::min<uint64_t>(max_cells, (uint64_t)((double)(free_b + held) * 0.9 / (double)per_cell));
  }
  const double occupancy = (double)q.L.occupied[q.cl] / (double)std::max<uint64_t>(1, q.grid_entries);
  bool direct = occupancy >= c->opt_num("SWZ_MD_DIRECT_MIN_OCCUPANCY", 0.5);
  if (const char* f = c->opt("SWZ_MD_DIRECT")) direct = atoi(f) != 0;  // tests: 1 whatever the occupancy, 0 never
  a.direct = (direct && !q.sharded && q.grid_entries <= max_cells) ? 1u : 0u;
  if (q.L.as.gone && !a.direct) {  // (a level inside a chain: with direct numbering or not at all)
    q.over = true;
    return SWZ_OK;
  }
  if (direct_out) *direct_out = a.direct != 0u;
  *q.used = true;
  return SWZ_OK;
}

// ---- the joint root of a sharded batch
// From the moment its views are published, a shard that leaves min_distance_keys_level early says so in its round word:
// the higher shards' face cells poll that word and would otherwise spin until their own limits.
struct MqWordGuard {
  swz_ctx* c;
  uint32_t* word = nullptr;  // armed with the shard's round word
  bool done = false;
  ~MqWordGuard() {
    if (word && !done) {
      mq_set_round_word(c->stream, word, MQ_ROUND_FAILED);
      (void)hipStreamSynchronize(c->stream);
    }
  }
};

// publish this shard's root level ...
static int mq_publish_view(swz_ctx* c, MqLevel& q) {
  MqArgs& a = q.a;
  const ActiveSet& as = q.L.as;
  MdPeerView& mine = q.shard_root->views[q.shard_root->shard];
  int my_status = SWZ_OK;
  if (q.cl < 1 || q.ncells >= (1u << MQ_PEER_SHIFT) || q.L.sample_nodes != 1) my_status = SWZ_ERR_INTERNAL;
  // (a tiler's root level -- the batch merged with the cached root file -- indexes its working arrays through aidx, a
  // buffer the next level reuses while higher shards may still look up exact positions here: a copy that stays)
  const uint32_t* aidx_sr = nullptr;
  if (as.aidx) {
    uint32_t* cp = nullptr;
    SWZ_TRY(c->get("md_qaidx_sr", (size_t)a.m, &cp));
    SWZ_HIP(c, hipMemcpyAsync(cp, as.aidx, (size_t)a.m * 4, hipMemcpyDeviceToDevice, c->stream));
    aidx_sr = cp;
  }
  SWZ_TRY(c->get("md_qround_sr", (size_t)32, &a.round_word));
  mq_set_round_word(c->stream, a.round_word, MQ_FIRST_ROUND);
  SWZ_LAUNCH_CHECK(c);
  SWZ_HIP(c, hipStreamSynchronize(c->stream));
  mine.rec = a.rec;
  mine.qpos = a.qpos;
  mine.state = a.state;
  mine.ovf = a.ovf;
  mine.gridmap = a.gridmap;
  mine.round_word = a.round_word;
  mine.perm = a.perm;
  mine.xyz = a.xyz;
  mine.aidx = aidx_sr;
  mine.ncells = q.ncells;
  mine.npoints = a.m;
  mine.rg = a.rg;
  mine.cell_shift = a.cell_shift;
  mine.status = my_status;
  mine.entered = 1;
  return SWZ_OK;
}

// ... meet the others, take the lower shards' views
static int mq_meet_peers(swz_ctx* c, MqLevel& q) {
  MqArgs& a = q.a;
  const MdShardRoot* sr = q.shard_root;
  sr->barrier(sr->barrier_arg);
  for (int p = 0; p < sr->shards; ++p) {
    const MdPeerView& v = sr->views[p];
    if (v.status != SWZ_OK || (v.ncells && (v.rg != a.rg || v.cell_shift != a.cell_shift)))
      return c->fail(SWZ_ERR_INTERNAL, "MIN_DISTANCE root of a sharded batch: shard " + std::to_string(p) +
                                         " cannot take part in the joint sweep (cell levels, cell count or record size differ)");
    if (p < sr->shard && v.ncells) {
      a.peers.rec[p] = v.rec;
      a.peers.qpos[p] = v.qpos;
      a.peers.state[p] = v.state;
      a.peers.ovf[p] = v.ovf;
      a.peers.gridmap[p] = v.gridmap;
      a.peers.round_word[p] = v.round_word;
      a.peers.perm[p] = v.perm;
      a.peers.xyz[p] = v.xyz;
      a.peers.aidx[p] = v.aidx;
    }
  }
  return SWZ_OK;
}

// scheduling: the same rules as the sweep on positions (swz_mindist.hip)
static void mq_schedule(const swz_ctx* c, MqLevel& q) {
  MqArgs& a = q.a;
  const uint32_t sample_nodes = q.L.sample_nodes;
  // the survey's number at cl: the points-weighted mean cell population
  const double typical_pop = q.L.pop[std::min(3, q.L.plan.cell_levels_geo - q.cl)];
  const bool many_small = q.occ_cells >= (4u << 20) && (double)q.L.sample_points / (double)q.occ_cells <= 128.0;
  a.patient = (uint32_t)c->opt_int("SWZ_MD_PATIENT", many_small ? 1 : 0);
  q.lazy = c->opt_on("SWZ_MD_LAZY", true);  // (on keys also for roots of thousands of points per cell: clustered root 99 -> 89 ms)
  a.lazy_frac = (float)c->opt_num("SWZ_MD_LAZY_FRAC", many_small ? 0.5 : 0.0);
  // (the build for large cells from a few hundred points per typical cell on: at 113 -- level 1 of the clustered cloud --
  // the small-cell build is still ahead, 48 against 55 ms; at 478 and 710 the large-cell one, 72 / 81 against 100+)
  q.big_cells = c->opt_on("SWZ_MD_BIG", typical_pop > 256.0);
  uint32_t groups = 1;
  if (sample_nodes >= 2 && !q.big_cells) groups = 2;
  groups = (uint32_t)std::max(1L, std::min(8L, c->opt_int("SWZ_MD_GROUPS", groups)));
  groups = std::min(groups, sample_nodes);
  if (q.sharded) groups = 1;
  q.groups = groups;
}

// the rounds: a level is done when a round starts with an empty queue (only running cells wake sleeping ones)
static int mq_run_rounds(swz_ctx* c, MqLevel& q) {
  const uint32_t groups = q.groups, m = q.a.m;
  const uint32_t sweep_grid = mq_sweep_grid(c, q);
  uint32_t batch = 32, batches_done = 0;
  const bool fixed_batch = c->opt("SWZ_MD_BATCH") != nullptr;
  if (fixed_batch) batch = std::max(1u, (uint32_t)c->opt_int("SWZ_MD_BATCH", 0));
  const auto wall0 = std::chrono::steady_clock::now();
  const double wall_limit = c->opt_num("SWZ_MD_TIME_LIMIT", 900.0);
  uint64_t max_rounds = 8ull * m + 1024;  // (the sweep on positions has its own, 4 m + 1024: swz_mindist.hip)
  if (q.sharded) {
    // A cell at the face of a lower shard looks again every round until that shard's sweep has got there, and a level only
    // ends with an empty queue: a shard of a few points beside a lower shard of 1e8 spends (cheap, nearly empty) rounds
    // for as long as the lower sweeps take.  Its limit therefore covers their work as well -- an empty round is ~10 us
    // against the >= 20 us of a working one, so their rounds count several times.
    uint64_t below = 0;
    for (int p = 0; p < q.shard_root->shard; ++p) below += q.shard_root->views[p].npoints;
    max_rounds += 64ull * below + 65536ull;
  }
  max_rounds = (uint64_t)c->opt_int("SWZ_MD_ROUND_LIMIT", (long)max_rounds);
  hipEvent_t fork = nullptr;
  if (groups > 1) {
    fork = c->take_event();
    SWZ_HIP(c, hipEventRecord(fork, c->stream));
    for (uint32_t g = 1; g < groups; ++g) SWZ_HIP(c, hipStreamWaitEvent(q.gs[g], fork, 0));
  }
  std::vector<uint32_t> gleft(groups, 1);
  uint32_t& round = q.round;
  bool running = true;
  while (running) {
    for (uint32_t b = 0; b < batch; ++b, ++round)
      for (uint32_t g = 0; g < groups; ++g) mq_launch_round(q, g, sweep_grid);
    SWZ_LAUNCH_CHECK(c);
    if (!fixed_batch && ++batches_done % 4u == 0u && batch < 128u) batch *= 2u;
    for (uint32_t g = 0; g < groups; ++g)  // what the last launched round started with
      SWZ_HIP(c, hipMemcpyAsync(&gleft[g], q.ga[g].qtotal + (round - 1u - MQ_FIRST_ROUND) % 3u, 4, hipMemcpyDeviceToHost, q.gs[g]));
    uint32_t peer_err = 0;
    if (q.sharded) SWZ_HIP(c, hipMemcpyAsync(&peer_err, q.ga[0].counters + CTR_ERROR, 4, hipMemcpyDeviceToHost, q.gs[0]));
    running = false;
    for (uint32_t g = 0; g < groups; ++g) {
      SWZ_HIP(c, hipStreamSynchronize(q.gs[g]));
      running |= gleft[g] != 0u;
    }
    if (peer_err) return c->fail(SWZ_ERR_INTERNAL, "MIN_DISTANCE root of a sharded batch: a lower shard's sweep failed (or a queue overflowed); this shard gives up as well");
    if (std::chrono::duration<double>(std::chrono::steady_clock::now() - wall0).count() > wall_limit) {
      char msg[200];
      snprintf(msg, sizeof(msg), "MIN_DISTANCE sweep on keys exceeded %.0f s: level %d, %u cells, %u rounds", wall_limit, q.L.plan.level,
               q.ncells, round);
      return c->fail(SWZ_ERR_INTERNAL, msg);
    }
    if (round > max_rounds) {
      char msg[160];
      snprintf(msg, sizeof(msg), "MIN_DISTANCE sweep on keys did not terminate: level %d, %u cells, %u rounds", q.L.plan.level, q.ncells, round);
      return c->fail(SWZ_ERR_INTERNAL, msg);
    }
  }
  if (fork) c->event_pool.push_back(fork);
  return mq_prebuild_join(c);  // (long done as a rule: what follows the rounds on the context's stream is ordered behind it)
}

// every way out of a level between the launch of the tables built ahead and the end of its rounds joins them
struct MqPrebuildGuard {
  swz_ctx* c;
  ~MqPrebuildGuard() {
    if (c->mq_pre.done) {
      (void)mq_prebuild_join(c);
      c->mq_pre.valid = false;
    }
  }
};

// SWZ_DEBUG: what the level starts with, and -- the event pair around the sweep -- how long it took
struct MqTrace {
  bool on = false;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
};
static void mq_trace_begin(swz_ctx* c, const MqLevel& q, MqTrace& t) {
  t.on = c->opt("SWZ_DEBUG") != nullptr;
  if (!t.on) return;
  const MqArgs& a = q.a;
  const MdLevel& L = q.L;
  fprintf(stderr, "[swz] MIN_DISTANCE level %d on keys: %u pts in %u nodes, %u cells%s (cell levels %d), spacing %.1f key cells, band "
                  "[%.0f, %.0f), records of %u, typical cell %.0f pts, lazy %d (%.2f) patient %u groups %u big %d dense cells %u\n",
          L.plan.level, L.sample_points, L.sample_nodes, q.ncells, a.direct ? " of the grid, numbered directly" : "", q.cl, L.km.T, (double)L.km.f_lo, (double)L.km.f_hi, a.rg - 1u,
          L.pop[std::min(3, L.plan.cell_levels_geo - q.cl)], (int)q.lazy, (double)a.lazy_frac, a.patient, q.groups, (int)q.big_cells, q.ndense);
  t.ev0 = c->take_event();
  t.ev1 = c->take_event();
  (void)hipEventRecord(t.ev0, c->stream);
}
static int mq_trace_end(swz_ctx* c, const MqLevel& q, MqTrace& t) {
  if (!t.on) return SWZ_OK;
  float ms = 0.f;
  (void)hipEventRecord(t.ev1, c->stream);
  (void)hipEventSynchronize(t.ev1);
  (void)hipEventElapsedTime(&ms, t.ev0, t.ev1);
  c->event_pool.push_back(t.ev0);
  c->event_pool.push_back(t.ev1);
  fprintf(stderr, "[swz] MIN_DISTANCE level %d on keys: sweep %.2f ms, %u rounds\n", q.L.plan.level, ms, q.round - MQ_FIRST_ROUND);
  for (uint32_t g = 0; g < q.groups; ++g) {
    uint32_t h[CTR_COUNT];
    SWZ_HIP(c, hipMemcpy(h, q.ga[g].counters, sizeof(h), hipMemcpyDeviceToHost));
    fprintf(stderr, "[swz]   group %u: %u full activations, %u confirms still asleep, %u confirms that lost the claim, %u stalls, %u scans\n", g,
            h[CTR_DBG_HIST], h[CTR_DBG_HIST + 1], h[CTR_DBG_HIST + 2], h[CTR_DBG_HIST + 3], h[CTR_DBG_HIST + 4]);
#ifdef SWZ_MQ_STATS
    {
      const double ns = std::max(1u, h[CTR_DBG_HIST + 15]) * 100.0;  // 100 MHz ticks -> us
      fprintf(stderr, "[swz]   timed %u full activations (us): first loads %.2f, records + window %.2f, list %.2f, first window (R) %.2f, "
                      "windows + candidates + scans %.2f, publish + wake %.2f, total %.2f\n", h[CTR_DBG_HIST + 15], h[CTR_DBG_HIST + 8] / ns,
              h[CTR_DBG_HIST + 9] / ns, h[CTR_DBG_HIST + 10] / ns, h[CTR_DBG_HIST + 11] / ns, h[CTR_DBG_HIST + 12] / ns, h[CTR_DBG_HIST + 13] / ns,
              h[CTR_DBG_HIST + 14] / ns);
    }
#endif
  }
  return SWZ_OK;
}

// a step; the level may end with it, without an error
#define MQ_STEP(call)            \
  do {                           \
    SWZ_TRY(call);               \
    if (q.over) return SWZ_OK;   \
  } while (0)

int min_distance_keys_level(swz_ctx* c, const MdLevel& L, int cl, uint32_t* rounds_out, bool* used, const MdShardRoot* shard_root,
                            bool* direct_out) {
  *used = false;
  if (direct_out) *direct_out = false;
  MqLevel q{L, cl, shard_root, used};
  MQ_STEP(mq_fill_args(c, q));
  ProfScope ps(c, "sample_min_distance", (uint64_t)L.sample_points * 33ull, 1);
  MQ_STEP(mq_choose_records_and_numbering(c, q, direct_out));
  MQ_STEP(mq_count_cells(c, q));
  SWZ_TRY(mq_alloc_arrays(c, q));
  SWZ_TRY(mq_build_cell_tables(c, q));
  MqWordGuard word_guard{c};
  if (q.sharded) {
    SWZ_TRY(mq_publish_view(c, q));
    word_guard.word = q.a.round_word;  // every return from here to the sweep's end writes MQ_ROUND_FAILED
    SWZ_TRY(mq_meet_peers(c, q));
  }
  mq_schedule(c, q);
  SWZ_TRY(mq_list_dense_cells(c, q));
  SWZ_TRY(mq_start_groups(c, q));
  MqPrebuildGuard prebuild_guard{c};
  SWZ_TRY(mq_prebuild_launch(c, q));
  MqTrace trace;
  mq_trace_begin(c, q, trace);
  SWZ_TRY(mq_run_rounds(c, q));
  if (q.sharded) {  // everything this shard has written is complete now
    mq_set_round_word(c->stream, q.a.round_word, MQ_ROUND_DONE);
    word_guard.done = true;
    SWZ_LAUNCH_CHECK(c);
  }
  SWZ_TRY(mq_verify(c, q));
  SWZ_TRY(mq_commit(c, q));
  if (rounds_out) *rounds_out += q.round - MQ_FIRST_ROUND;
  return mq_trace_end(c, q, trace);
}

}  // namespace swz
