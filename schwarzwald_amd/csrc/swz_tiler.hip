// swz_tiler.hip -- the multi-batch tiler (BASELINE config 5's single-GPU shape).
//
// The reference tiles a data set larger than internal_cache_size (executable/main.cpp:233-236, default 10 M points)
// batch by batch on ONE TilingAlgorithm object: every node a batch reaches re-reads the points earlier batches
// persisted under its name, re-keys them relative to the node (read_pnts_from_disk, core/tiling/TilingAlgorithms.cpp:
// 50-109), merges them with the new points (merge_node_data_sorted, core/tiling/Node.cpp:4-22: std::merge, new
// points first on equal keys), samples the union with AlwaysAdhereToMinSpacing (:272-275), REPLACES the node's file
// with the taken points (BinaryPersistence.h:46-57) and hands the rest -- new and displaced old points alike -- to
// the children.  Nodes no point of the batch reaches are not touched.
//
// Here the "files" are a device-resident node store: per octree level the (key, point id) entries of its nodes' files,
// each file contiguous and in file order, found through a node table (StoreLevel); positions (and attribute columns) of
// all points ever added live in pools indexed by point id (= running index over all batches).  A batch runs the same
// level-synchronous loop as a single batch (swz_session.hip); per level the files of the nodes the active set touches are
// copied out and merged in, and the level's taken points are appended as those nodes' new files -- carrying the key the
// reference computes when it reads a file back, so that the re-keying is paid once per stored entry, not per pull.  FAST (TilingAlgorithmV3) later iterations
// (:1362-1453, 1620-1659: per-thread chunks sorted, split at the start level, k-way merged, earlier chunk first on
// ties) are the stable sort of the batch; finalize (:1661-1784) rebuilds the skipped levels from the store.
//
// Staging (BASELINE config 5): swz_tiler_stage_batch copies the NEXT batch from pinned host memory straight into
// its final place in the pools with hipMemcpyAsync on a copy stream while the current batch is tiled.
//
// This file: the batch life cycle (prepare, run, close), FAST finalize, the store's node table and the C ABI.  The node
// store and the pools are in swz_tstore.hip, a level of a batch in swz_tlevel.hip, re-rooting in swz_treroot.hip; swz_tiler.h
// holds what they share.
#include <algorithm>
#include <chrono>
#include <cstring>
#include <vector>

#include "swz_tiler.h"

int tiler_guard(swz_tiler* t) {
  // (every call of the tiler's API starts a scratch epoch: what earlier calls asked for and nothing holds on to -- level
  // scratch, and the per-batch "tl_*" buffers once no batch is open -- may be freed when the device runs out of memory)
  if (!t->failed) {
    t->c->next_scratch_epoch();
    return SWZ_OK;
  }
  return t->c->fail(SWZ_ERR_TILER_FAILED, "swz_tiler: an earlier batch failed part-way (" + t->failed_why +
                                            "); the node store is incomplete -- destroy the tiler");
}
// st != SWZ_OK after the tiler started to change its state: remember it
static int tiler_poison(swz_tiler* t, int st) {
  if (st != SWZ_OK && !t->failed) {
    t->failed = true;
    t->failed_why = t->c->err;
    t->batch_open = false;
  }
  return st;
}
// the end of a call that ran a batch: waits for the stream, folds the profile, and remembers a failure of either
static int tiler_end_call(swz_tiler* t, int st) {
  swz_ctx* c = t->c;
  const hipError_t e = hipStreamSynchronize(c->stream);
  c->prof_collect();
  if (st != SWZ_OK) return tiler_poison(t, st);
  if (e != hipSuccess) return tiler_poison(t, c->hip_fail(e, "hipStreamSynchronize", __FILE__, __LINE__));
  return SWZ_OK;
}

namespace swz {

// ---------------------------------------------------------------------------------------------- kernels
__global__ __launch_bounds__(256) void tl_wgid_kernel(const uint32_t* __restrict__ perm, uint32_t n, uint32_t base,
                                                      uint32_t* __restrict__ wgid) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) wgid[i] = base + perm[i];
}

// index_points<21>(root bounds, ClampToBounds) on a COPY of the positions (reconstruct_single_node :1682-1688)
__global__ __launch_bounds__(256) void tl_reencode_kernel(const uint32_t* __restrict__ gid, uint32_t n,
                                                          const double* __restrict__ pool, Box b,
                                                          uint64_t* __restrict__ keys) {
  const uint32_t j = blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  const size_t g = gid[j];
  double x = pool[3 * g], y = pool[3 * g + 1], z = pool[3 * g + 2];
  const bool inside = (x >= b.minx && x <= b.maxx && y >= b.miny && y <= b.maxy && z >= b.minz && z <= b.maxz);
  if (!inside) {
    x = (b.minx < x) ? x : b.minx;
    x = (x < b.maxx) ? x : b.maxx;
    y = (b.miny < y) ? y : b.miny;
    y = (y < b.maxy) ? y : b.maxy;
    z = (b.minz < z) ? z : b.minz;
    z = (z < b.maxz) ? z : b.maxz;
  }
  keys[j] = morton_in_box(x, y, z, b);
}

struct TakeG {  // the node's new file content: taken points in the order of the merged range
  const uint64_t* mkey;
  const uint32_t* midx;
  const uint32_t* wgid;
  uint64_t* tkey;
  uint32_t* tgid;
  __device__ void operator()(uint32_t i, uint32_t excl, uint32_t t) const {
    if (!t) return;
    tkey[excl] = mkey[i];
    tgid[excl] = wgid[midx ? midx[i] : i];
  }
};

__global__ __launch_bounds__(256) void tl_fill_level_kernel(int8_t* __restrict__ out, uint32_t n, int8_t v) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) out[i] = v;
}

__global__ __launch_bounds__(256) void tl_rows_kernel(const uint32_t* __restrict__ gid, uint32_t n, const double* __restrict__ pool,
                                                      double* __restrict__ out) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const size_t g = gid[i];
  out[3 * (size_t)i] = pool[3 * g];
  out[3 * (size_t)i + 1] = pool[3 * g + 1];
  out[3 * (size_t)i + 2] = pool[3 * g + 2];
}

// ---------------------------------------------------------------------------------------------- host helpers
static void store_free(StoreLevel& s) { s = StoreLevel{}; }

static void zero_stats(swz_tile_stats* s) {
  if (!s) return;
  std::memset(s, 0, sizeof(*s));
  s->max_level = -1;
  s->fast_start_levels = -1;
}

static uint64_t stored_total(const swz_tiler* t) {
  uint64_t s = 0;
  for (int l = 0; l < 22; ++l) s += t->lv[l].cnt;
  return s;
}

// What TilingAlgorithmBase refuses before it touches anything: a batch after finalize, and under FAST a batch with fewer
// points than indexing threads, the empty one included (parallel::scatter throws, util/threading/Parallel.h:181-186).
// The entry points ask this BEFORE they reserve, copy or count anything, so that a refused batch leaves the tiler as
// it was (not poisoned, no point id used up).  A sharded batch is exempt: its driver checks the whole batch.
static int tiler_refuse_batch(swz_tiler* t, uint64_t n) {
  if (t->finalized) return t->c->fail(SWZ_ERR_BAD_ARG, "swz_tiler: batches cannot be added after finalize");
  if (t->p.strategy == SWZ_FAST && n < t->p.fast_concurrency && !t->shard_fast)
    return t->c->fail(SWZ_ERR_BAD_ARG, "FAST: a batch needs at least fast_concurrency points");
  return SWZ_OK;
}

int index_and_sort(swz_ctx* c, double* d_xyz, uint32_t n, const double bmin[3], const double bmax[3], uint64_t* keys_tmp,
                   uint32_t* vals_tmp, uint64_t* keys, uint32_t* perm) {
  SWZ_TRY(encode_device(c, d_xyz, n, bmin, bmax, keys_tmp));
  return radix_sort_pairs(c, keys_tmp, vals_tmp, keys, perm, n, true);
}
int add_base(swz_ctx* c, const uint32_t* perm, uint32_t n, uint32_t base, uint32_t* out) {
  hipLaunchKernelGGL(tl_wgid_kernel, dim3(div_up(n, 256)), dim3(256), 0, c->stream, perm, n, base, out);
  SWZ_LAUNCH_CHECK(c);
  return SWZ_OK;
}

// d_xyz: the batch inside the position pool (already there) or anywhere else on the device (copied in).
// Index + sort + positions into Morton order (K1, K2, gather), exactly like a single batch; leaves the batch open.
static int tiler_batch_prepare(swz_tiler* t, double* d_xyz, uint32_t n, uint32_t extra_pool) {
  swz_ctx* c = t->c;
  c->tiler_scratch_dead = false;  // (the batch's scratch lives until tiler_batch_close)
  if (t->batch_open) return c->fail(SWZ_ERR_BAD_ARG, "swz_tiler: the previous batch is still open (swz_tiler_shard_finish)");
  SWZ_TRY(tiler_refuse_batch(t, n));
  const uint32_t base = t->total;
  uint64_t* keys = nullptr;
  uint32_t* perm = nullptr;
  if (n) {
    double* slot = t->pool_xyz + (size_t)base * 3;
    const bool in_pool = d_xyz == slot;
    uint64_t* keys_b = nullptr;
    uint32_t* vals_b = nullptr;
    SWZ_TRY(c->get("tl_keys", (size_t)n, &keys));
    SWZ_TRY(c->get("tl_perm", (size_t)n, &perm));
    SWZ_TRY(c->get("sort_keys_b", (size_t)n, &keys_b));
    SWZ_TRY(c->get("sort_vals_b", (size_t)n, &vals_b));
    SWZ_TRY(index_and_sort(c, d_xyz, n, t->bmin, t->bmax, keys_b, vals_b, keys, perm));
    if (!in_pool)  // clamped positions (index_point clamps in place, OctreeAlgorithms.h:167-169) into the pool
      SWZ_HIP(c, hipMemcpyAsync(slot, d_xyz, (size_t)n * 24, hipMemcpyDefault, c->stream));
  }
  BatchWork& w = t->bw;
  w = BatchWork{};
  w.n = n;
  const uint64_t wcap64 = (uint64_t)n + stored_total(t) + extra_pool;
  if (wcap64 > 0xFFFF0000ull) return c->fail(SWZ_ERR_TOO_MANY_POINTS, "batch + stored points exceed 2^32-65536");
  w.wcap = (uint32_t)wcap64;
  SWZ_TRY(c->get("tl_wlevel", (size_t)w.wcap, &w.wlevel));
  SWZ_TRY(c->get("tl_wgid", (size_t)w.wcap, &w.wgid));
  if (n) SWZ_TRY(add_base(c, perm, n, base, w.wgid));  // (positions: on demand, work_need_positions)
  SWZ_HIP(c, hipMemsetAsync(w.wlevel, 0x80, (size_t)std::max<uint32_t>(w.wcap, 1u), c->stream));
  w.wused = n;
  t->next_level = -1;
  if (t->p.strategy == SWZ_FAST) {
    if (t->fast_start < 0 && !t->shard_fast) SWZ_TRY(fast_start_level(c, keys, n, t->p.fast_concurrency, &t->fast_start));
    t->next_level = t->fast_start - 1;  // (a sharded batch: set again once the driver has told the start level)
  }
  t->as = ActiveSet{keys, nullptr, n};
  t->acc_visited = t->acc_nodes = 0;
  t->acc_rounds = t->acc_levels = 0;
  t->acc_max_level = -1;
  t->batch_open = true;
  return SWZ_OK;
}

// the level loop from t->next_level to last_level (sr: the root level of a sharded batch)
static int tiler_batch_run(swz_tiler* t, int last_level, const ShardRoot* sr) {
  swz_ctx* c = t->c;
  BatchWork& w = t->bw;
  ActiveSet& as = t->as;
  as.parent_prefix = nullptr;  // (known inside one call only, see session_run_levels)
  as.parents = 0;
  for (int level = t->next_level; level <= last_level; ++level) {
    const bool shard_root = sr && sr->active && level == -1;
    if (as.m == 0 && !shard_root) break;
    if (level > 20) return c->fail(SWZ_ERR_INTERNAL, "level loop ran past level 20");
    LevelPlan plan = make_plan(level, t->p.sampler, t->p.max_points_per_node, t->p.spacing_at_root, t->p.max_depth,
                               t->bmin, t->bmax, false, true);
    plan.md_property = (t->p.flags & SWZ_FLAG_MIN_DISTANCE_PROPERTY) != 0 && !shard_root;  // (a sharded root is sampled exactly)
    if (plan.reroot && !plan.terminal && !greedy_sampler(t->p.sampler)) {
      RrTotals tot;
      SWZ_TRY(tiler_reroot_level(t, w, plan, as, tot));
      t->acc_visited += tot.visited;
      t->acc_nodes += tot.nodes;
      t->acc_max_level = std::max(t->acc_max_level, tot.max_level);
      ++t->acc_levels;
      as.m = 0;
      t->next_level = 21;
      return SWZ_OK;
    }
    LevelResult r;
    uint32_t merged = 0;
    SWZ_TRY(tiler_level(t, w, plan, as, &r, &merged, shard_root ? sr : nullptr));
    t->acc_visited += merged;
    t->acc_nodes += r.num_nodes;
    t->acc_rounds += r.md_rounds;
    if (merged) t->acc_max_level = level;
    ++t->acc_levels;
    t->next_level = level + 1;
  }
  return SWZ_OK;
}

static void tiler_batch_close(swz_tiler* t, swz_tile_stats* stats) {
  t->c->tiler_scratch_dead = true;
  t->total += t->bw.n;
  if (t->staged_total < t->total) t->staged_total = t->total;
  ++t->batches;
  t->batch_open = false;
  if (stats) {
    stats->num_nodes = t->acc_nodes;
    stats->points_visited = t->acc_visited;
    stats->max_level = t->acc_max_level;
    stats->fast_start_levels = t->fast_start;
    stats->num_levels = t->acc_levels;
    stats->min_distance_rounds = t->acc_rounds;
  }
}

static int tiler_add_batch(swz_tiler* t, double* d_xyz, uint32_t n, swz_tile_stats* stats) {
  zero_stats(stats);
  if (n == 0) {
    SWZ_TRY(tiler_refuse_batch(t, 0));
    ++t->batches;
    return SWZ_OK;
  }
  int st = tiler_batch_prepare(t, d_xyz, n, 0);
  if (st == SWZ_OK) st = tiler_batch_run(t, 20, nullptr);
  if (st != SWZ_OK) {
    t->batch_open = false;
    return st;
  }
  tiler_batch_close(t, stats);
  return SWZ_OK;
}

// TilingAlgorithmV3::finalize -> reconstruct_left_out_nodes (:1717-1784): every ancestor of a start node samples the
// points its children hold (children in octant order = the store order of the level below), re-indexed against the
// root bounds, with AlwaysAdhereToMinSpacing (reconstruct_single_node :1661-1715).
// While a call outside a batch holds "tl_*" buffers across level_step (whose MIN_DISTANCE levels open new scratch
// epochs and may run out of memory), the workspace must not count them as dead scratch: get() would free the very
// arrays the level is reading.
struct TilerScratchLive {
  swz_ctx* c;
  bool was;
  explicit TilerScratchLive(swz_ctx* ctx) : c(ctx), was(ctx->tiler_scratch_dead) { c->tiler_scratch_dead = false; }
  ~TilerScratchLive() { c->tiler_scratch_dead = was; }
};

static int tiler_finalize(swz_tiler* t, swz_tile_stats* stats, int lowest_children = 0) {
  swz_ctx* c = t->c;
  zero_stats(stats);
  TilerScratchLive live(c);
  if (t->finalized) return SWZ_OK;
  if (!t->staged_sizes.empty()) return c->fail(SWZ_ERR_BAD_ARG, "swz_tiler_finalize: staged batches have not been tiled");
  t->finalized = lowest_children == 0;  // (a shard stops below the root: swz_tiler_shard_fast_set_root ends the data set)
  if (t->p.strategy != SWZ_FAST || t->fast_start <= 0) return SWZ_OK;
  const int S = t->fast_start;
  uint64_t nodes = 0;
  uint32_t rounds = 0;
  uint32_t* counters = nullptr;
  SWZ_TRY(c->get("tl_counters", (size_t)4, &counters));
  for (int lv = S - 1; lv >= lowest_children; --lv) {  // children at node level lv, parents at lv - 1
    StoreLevel& src = t->lv[lv + 1];
    StoreLevel& dst = t->lv[lv];
    const uint32_t m = src.cnt;
    if (m == 0) continue;
    SWZ_TRY(store_linearize(t, src, lv + 1));
    uint64_t* keys = nullptr;
    uint32_t *gid = nullptr, *wgid = nullptr;
    double *wx = nullptr, *wy = nullptr, *wz = nullptr;
    SWZ_TRY(c->get("tl_keys", (size_t)m, &keys));
    SWZ_TRY(c->get("tl_perm", (size_t)m, &gid));
    SWZ_TRY(c->get("tl_wgid", (size_t)m, &wgid));
    LevelPlan plan = make_plan(lv - 1, t->p.sampler, t->p.max_points_per_node, t->p.spacing_at_root, t->p.max_depth,
                               t->bmin, t->bmax, true, false);
    plan.md_property = (t->p.flags & SWZ_FLAG_MIN_DISTANCE_PROPERTY) != 0;
    // Like the levels of a batch (tiler_level), the rebuilt levels are decided on key coordinates with the exact positions
    // looked up in the pool through the point ids (round 5: they gathered the positions and ran the sweep on positions --
    // 253 of the 1 073 ms of the default operating point's data set, 1 B points in 100 tile batches); positions in
    // Morton order only for what cannot be decided on keys.
    SortedPoints sp{nullptr, nullptr, nullptr, t->pool_xyz, wgid};
    const bool on_keys = level_decides_on_keys(c, plan, sp);
    if (!on_keys) {
      SWZ_TRY(c->get("tl_wx", (size_t)m, &wx));
      SWZ_TRY(c->get("tl_wy", (size_t)m, &wy));
      SWZ_TRY(c->get("tl_wz", (size_t)m, &wz));
      sp.X = wx;
      sp.Y = wy;
      sp.Z = wz;
    }
    SWZ_HIP(c, hipMemcpyAsync(gid, src.gid[src.cur], (size_t)m * 4, hipMemcpyDeviceToDevice, c->stream));
    hipLaunchKernelGGL(tl_reencode_kernel, dim3(div_up(m, 256)), dim3(256), 0, c->stream, gid, m, t->pool_xyz, root_box(t), keys);
    SWZ_LAUNCH_CHECK(c);
    // inside one PARENT the appended children must ascend (reconstruct_single_node does not sort a lossless store)
    SWZ_TRY(resort_if_inverted(t, keys, gid, m, store_shift(lv)));
    SWZ_TRY(fill_from_pool(c, gid, m, t->pool_xyz, wx, wy, wz, wgid));
    LevelBuffers lb;
    SWZ_TRY(alloc_level_buffers(c, m, &lb));
    ActiveSet as{keys, nullptr, m};
    LevelResult r;
    SWZ_TRY(level_step(c, plan, as, sp, lb, nullptr, nullptr, nullptr, &r));
    // count the taken points, then write them as the parents' files
    uint64_t* tkey = nullptr;
    uint32_t* tgid = nullptr;
    SWZ_TRY(c->get("tl_tkey", (size_t)m, &tkey));
    SWZ_TRY(c->get("tl_tgid", (size_t)m, &tgid));
    SWZ_TRY(fused_scan(c, TakenF{lb.taken}, TakeG{keys, nullptr, wgid, tkey, tgid}, m, counters + 2, "tl"));
    uint32_t nt = 0;
    SWZ_TRY(read_u32(c, counters + 2, &nt));
    SWZ_TRY(store_write_linear(c, dst, lv, tkey, tgid, nt));
    nodes += r.num_nodes;
    rounds += r.md_rounds;
  }
  SWZ_HIP(c, hipStreamSynchronize(c->stream));
  if (stats) {
    stats->num_nodes = nodes;
    stats->fast_start_levels = S;
    stats->min_distance_rounds = rounds;
  }
  return SWZ_OK;
}

// node table of the store: per level the runs of equal node prefix
static int tiler_node_table(swz_tiler* t, std::vector<int8_t>* nl, std::vector<uint64_t>* nk, std::vector<uint64_t>* no,
                            std::vector<uint64_t>* nc, uint64_t* num_nodes) {
  swz_ctx* c = t->c;
  uint64_t offset = 0, nn = 0;
  for (int l = 0; l < 22; ++l) {
    StoreLevel& s = t->lv[l];
    if (!s.cnt) continue;
    if (!nl && s.table_valid) {  // only the count is asked for
      nn += s.nn;
      offset += s.cnt;
      continue;
    }
    SWZ_TRY(store_linearize(t, s, l));
    const int level = l - 1;
    uint32_t* hp = nullptr;
    uint64_t* hk = nullptr;
    uint32_t heads = 0;
    SWZ_TRY(node_heads(c, s.key[s.cur], s.cnt, store_shift(l), &hp, &hk, &heads));
    if (nl) {
      std::vector<uint32_t> pos(heads);
      std::vector<uint64_t> key(heads);
      SWZ_HIP(c, hipMemcpyAsync(pos.data(), hp, (size_t)heads * 4, hipMemcpyDeviceToHost, c->stream));
      SWZ_HIP(c, hipMemcpyAsync(key.data(), hk, (size_t)heads * 8, hipMemcpyDeviceToHost, c->stream));
      SWZ_HIP(c, hipStreamSynchronize(c->stream));
      for (uint32_t k = 0; k < heads; ++k) {
        nl->push_back((int8_t)level);
        nk->push_back(key[k]);
        no->push_back(offset + pos[k]);
        nc->push_back((k + 1 < heads ? pos[k + 1] : s.cnt) - pos[k]);
      }
    }
    nn += heads;
    offset += s.cnt;
  }
  *num_nodes = nn;
  return SWZ_OK;
}

}  // namespace swz

using namespace swz;

// ================================================================================================== C ABI
extern "C" {

int swz_tiler_create(swz_ctx* c, const double bmin[3], const double bmax[3], const swz_tile_params* params,
                     uint64_t capacity_hint, swz_tiler** out) {
  if (!c || !out) return SWZ_ERR_BAD_ARG;
  *out = nullptr;
  SWZ_HIP(c, hipSetDevice(c->device));
  if (!bmin || !bmax || !params) return c->fail(SWZ_ERR_BAD_ARG, "swz_tiler_create: NULL argument");
  for (int a = 0; a < 3; ++a)
    if (!(bmax[a] > bmin[a])) return c->fail(SWZ_ERR_BAD_ARG, "bounds must have positive extent on every axis");
  SWZ_TRY(check_params(c, params));
  if (capacity_hint > 0xFFFF0000ull) return c->fail(SWZ_ERR_TOO_MANY_POINTS, "more than 2^32-65536 points per tiler");
  if (c->tiler_active) return c->fail(SWZ_ERR_BAD_ARG, "this context already has a tiler (one per context; use one context per data set)");
  swz_tiler* t = new swz_tiler();
  t->c = c;
  for (int a = 0; a < 3; ++a) {
    t->bmin[a] = bmin[a];
    t->bmax[a] = bmax[a];
  }
  t->p = *params;
  hipError_t e = hipStreamCreateWithFlags(&t->copy_stream, hipStreamNonBlocking);
  if (e != hipSuccess) {
    delete t;
    return c->fail(SWZ_ERR_HIP, std::string("hipStreamCreate(copy stream): ") + hipGetErrorString(e));
  }
  if (capacity_hint) {
    const int st = pool_reserve(t, (size_t)capacity_hint);
    if (st != SWZ_OK) {
      (void)hipStreamDestroy(t->copy_stream);
      delete t;
      return st;
    }
  }
  c->tiler_active = true;
  *out = t;
  return SWZ_OK;
}

int swz_tiler_destroy(swz_tiler* t) {
  if (!t) return SWZ_OK;
  (void)hipSetDevice(t->c->device);
  if (t->copy_stream) (void)hipStreamSynchronize(t->copy_stream);
  (void)hipStreamSynchronize(t->c->stream);
  for (hipEvent_t e : t->staged_events) (void)hipEventDestroy(e);
  for (int l = 0; l < 22; ++l) store_free(t->lv[l]);  // the memory stays in the context's workspace (swz_release_workspace)
  t->c->tiler_active = false;
  if (t->copy_stream) (void)hipStreamDestroy(t->copy_stream);
  delete t;
  return SWZ_OK;
}

int swz_tiler_add_batch_device(swz_tiler* t, double* d_xyz, uint64_t n, swz_tile_stats* stats) {
  if (!t) return SWZ_ERR_BAD_ARG;
  swz_ctx* c = t->c;
  SWZ_HIP(c, hipSetDevice(c->device));
  SWZ_TRY(tiler_guard(t));
  if (!t->staged_sizes.empty()) return c->fail(SWZ_ERR_BAD_ARG, "swz_tiler_add_batch_device: staged batches are pending");
  if (n && !d_xyz) return c->fail(SWZ_ERR_BAD_ARG, "swz_tiler_add_batch_device: NULL buffer");
  if ((uint64_t)t->total + n > 0xFFFF0000ull) return c->fail(SWZ_ERR_TOO_MANY_POINTS, "more than 2^32-65536 points per tiler");
  if (t->attr_mask) return c->fail(SWZ_ERR_BAD_ARG, "this tiler carries attribute columns: use swz_tiler_stage_batch");
  SWZ_TRY(tiler_refuse_batch(t, n));  // (a refusal up front changes nothing and does not poison)
  SWZ_TRY(pool_reserve(t, (size_t)t->total + n));
  const int st = tiler_add_batch(t, d_xyz, (uint32_t)n, stats);
  return tiler_end_call(t, st);
}

// ---- a tiler per GPU of a multi-GPU run: the shard owns the subtrees of its level-0 octants and ITS part of the root's
// file; the root node itself spans the shards (swz_shard_* for the single-batch form)
int swz_tiler_shard_begin_device(swz_tiler* t, double* d_xyz, uint64_t n, const swz_attribute_columns* d_attrs,
                                 const swz_tiler_shard_info* info, uint64_t* root_file_count_out) {
  if (!t) return SWZ_ERR_BAD_ARG;
  swz_ctx* c = t->c;
  SWZ_HIP(c, hipSetDevice(c->device));
  SWZ_TRY(tiler_guard(t));
  if (!info) return c->fail(SWZ_ERR_BAD_ARG, "swz_tiler_shard_begin_device: NULL shard info");
  if (const char* why = sharded_sampler_refusal(t->p.sampler)) return c->fail(SWZ_ERR_BAD_ARG, why);
  const bool fast = t->p.strategy == SWZ_FAST;
  if (!t->staged_sizes.empty()) return c->fail(SWZ_ERR_BAD_ARG, "swz_tiler_shard_begin_device: staged batches are pending");
  if ((n && !d_xyz) || (info->num_ghosts && !info->d_ghost_xyz)) return c->fail(SWZ_ERR_BAD_ARG, "swz_tiler_shard_begin_device: NULL buffer");
  if ((uint64_t)t->total + n > 0xFFFF0000ull || info->num_ghosts > 0x7FFFFFFFull)
    return c->fail(SWZ_ERR_TOO_MANY_POINTS, "more than 2^32-65536 points per tiler");
  uint32_t mask = 0;
  for (int a = 0; a < SWZ_ATTR_COUNT; ++a)
    if (d_attrs && d_attrs->column[a]) mask |= 1u << a;
  if (t->total == 0 && t->batches == 0) {
    t->attr_mask = mask;
    if (mask && t->pool_cap) {
      const size_t cap = t->pool_cap;
      t->pool_cap = 0;
      t->pool_xyz = nullptr;
      SWZ_TRY(pool_reserve(t, cap));
    }
  } else if (mask != t->attr_mask && n) {
    return c->fail(SWZ_ERR_BAD_ARG, "swz_tiler_shard_begin_device: every batch must carry the same attribute columns");
  }
  SWZ_TRY(pool_reserve(t, (size_t)t->total + n));
  for (int a = 0; a < SWZ_ATTR_COUNT && n; ++a) {
    if (!(t->attr_mask & (1u << a))) continue;
    const size_t rb = TILER_ATTR_BYTES[a];
    SWZ_HIP(c, hipMemcpyAsync((char*)t->pool_attr[a] + (size_t)t->total * rb, d_attrs->column[a], (size_t)n * rb,
                              hipMemcpyDefault, c->stream));
  }
  t->shard_fast = fast;
  int st = tiler_batch_prepare(t, d_xyz, (uint32_t)n, (uint32_t)info->num_ghosts);
  t->shard_fast = false;
  // FAST (TilingAlgorithmV3) skips the levels above its start nodes until the data set ends: no root step per batch
  if (st == SWZ_OK && info->global_new_points > 0 && !fast) {
    ShardRoot sr;
    sr.active = true;
    // tile_internal_node :272-275 with the counts of the WHOLE root: cached points force sampling, else count <= max takes all
    sr.sample = info->global_root_stored > 0 || info->global_new_points + info->global_root_stored > t->p.max_points_per_node;
    sr.ghost_xyz = info->d_ghost_xyz;
    sr.ghosts = sr.sample ? (uint32_t)info->num_ghosts : 0u;
    st = tiler_batch_run(t, -1, &sr);
  }
  SWZ_TRY(tiler_end_call(t, st));
  if (root_file_count_out) *root_file_count_out = t->lv[0].cnt;
  return SWZ_OK;
}

int swz_tiler_shard_finish(swz_tiler* t, swz_tile_stats* stats) {
  if (!t) return SWZ_ERR_BAD_ARG;
  swz_ctx* c = t->c;
  SWZ_HIP(c, hipSetDevice(c->device));
  SWZ_TRY(tiler_guard(t));
  zero_stats(stats);
  if (!t->batch_open) return c->fail(SWZ_ERR_BAD_ARG, "swz_tiler_shard_finish: no batch is open");
  if (t->p.strategy == SWZ_FAST) {
    if (t->fast_start < 1) return c->fail(SWZ_ERR_BAD_ARG, "swz_tiler_shard_finish: FAST needs swz_tiler_shard_set_start_level first");
    t->next_level = t->fast_start - 1;
  } else if (t->next_level < 0) {
    t->next_level = 0;  // the root was skipped (an empty batch)
  }
  const int st = tiler_batch_run(t, 20, nullptr);
  SWZ_TRY(tiler_end_call(t, st));
  tiler_batch_close(t, stats);
  return SWZ_OK;
}

// ---- FAST on a sharded data set.  The start level of TilingAlgorithmV3 comes from the distribution of the FIRST batch
// (TilingAlgorithms.cpp:1473-1535, kept afterwards :1230-1236): every shard reports the counts of its part per 6-octant
// prefix, the driver sums them and tells every shard the level.  Start nodes lie at level >= 2, inside one shard's
// octants, so batches need no root step; when the data set ends every shard rebuilds the skipped levels of its own
// octants down to level 0 and the root is rebuilt from the level-0 files of all shards by the driver.
int swz_tiler_shard_fast_histogram(swz_tiler* t, uint32_t* counts_out) {
  if (!t || !counts_out) return SWZ_ERR_BAD_ARG;
  swz_ctx* c = t->c;
  SWZ_HIP(c, hipSetDevice(c->device));
  SWZ_TRY(tiler_guard(t));
  if (!t->batch_open) return c->fail(SWZ_ERR_BAD_ARG, "swz_tiler_shard_fast_histogram: no batch is open");
  return tiler_poison(t, fast_prefix_counts(c, t->as.akey, t->as.m, counts_out));
}
int swz_fast_start_level_from_counts(const uint64_t* counts, uint32_t fast_concurrency, int32_t* start_level_out) {
  if (!counts || !start_level_out || !fast_concurrency) return SWZ_ERR_BAD_ARG;
  *start_level_out = fast_start_level_from_counts(counts, fast_concurrency);
  return SWZ_OK;
}
int swz_tiler_shard_set_start_level(swz_tiler* t, int32_t start_level) {
  if (!t) return SWZ_ERR_BAD_ARG;
  swz_ctx* c = t->c;
  SWZ_TRY(tiler_guard(t));
  if (t->p.strategy != SWZ_FAST || start_level < 1 || start_level > 6) return c->fail(SWZ_ERR_BAD_ARG, "swz_tiler_shard_set_start_level: FAST tilers, levels 1..6");
  if (t->fast_start >= 0 && t->fast_start != start_level) return c->fail(SWZ_ERR_BAD_ARG, "swz_tiler_shard_set_start_level: the start level is fixed by the first batch");
  t->fast_start = start_level;
  return SWZ_OK;
}
int swz_tiler_shard_fast_finalize_local(swz_tiler* t, swz_tile_stats* stats) {
  if (!t) return SWZ_ERR_BAD_ARG;
  swz_ctx* c = t->c;
  SWZ_HIP(c, hipSetDevice(c->device));
  SWZ_TRY(tiler_guard(t));
  if (t->p.strategy != SWZ_FAST) return c->fail(SWZ_ERR_BAD_ARG, "swz_tiler_shard_fast_finalize_local: not a FAST tiler");
  const int st = tiler_finalize(t, stats, 1);  // parents down to level 0; the root spans the shards
  c->prof_collect();
  return tiler_poison(t, st);
}
// d_taken: one flag per entry of this shard's level-0 files, in file order: the entry belongs to the rebuilt root
int swz_tiler_shard_fast_set_root(swz_tiler* t, const uint8_t* d_taken) {
  if (!t) return SWZ_ERR_BAD_ARG;
  swz_ctx* c = t->c;
  SWZ_HIP(c, hipSetDevice(c->device));
  SWZ_TRY(tiler_guard(t));
  if (t->p.strategy != SWZ_FAST || t->finalized) return c->fail(SWZ_ERR_BAD_ARG, "swz_tiler_shard_fast_set_root: an open FAST tiler is needed");
  StoreLevel& src = t->lv[1];
  StoreLevel& dst = t->lv[0];
  const uint32_t m = src.cnt;
  t->finalized = true;
  if (m == 0) return SWZ_OK;
  if (!d_taken) return c->fail(SWZ_ERR_BAD_ARG, "swz_tiler_shard_fast_set_root: NULL flags");
  TilerScratchLive live(c);
  auto body = [&]() -> int {
    SWZ_TRY(store_linearize(t, src, 1));
    uint64_t *keys = nullptr, *tkey = nullptr;
    uint32_t *tgid = nullptr, *counters = nullptr;
    SWZ_TRY(c->get("tl_keys", (size_t)m, &keys));
    SWZ_TRY(c->get("tl_tkey", (size_t)m, &tkey));
    SWZ_TRY(c->get("tl_tgid", (size_t)m, &tgid));
    SWZ_TRY(c->get("tl_counters", (size_t)4, &counters));
    hipLaunchKernelGGL(tl_reencode_kernel, dim3(div_up(m, 256)), dim3(256), 0, c->stream, src.gid[src.cur], m, t->pool_xyz, root_box(t), keys);
    SWZ_LAUNCH_CHECK(c);
    SWZ_TRY(fused_scan(c, TakenF{d_taken}, TakeG{keys, nullptr, src.gid[src.cur], tkey, tgid}, m, counters + 2, "tl"));
    uint32_t nt = 0;
    SWZ_TRY(read_u32(c, counters + 2, &nt));
    SWZ_TRY(store_write_linear(c, dst, 0, tkey, tgid, nt));
    SWZ_HIP(c, hipStreamSynchronize(c->stream));
    return SWZ_OK;
  };
  return tiler_poison(t, body());
}

int swz_tiler_poison(swz_tiler* t, const char* why) {
  if (!t) return SWZ_ERR_BAD_ARG;
  if (!t->failed) {
    t->failed = true;
    t->failed_why = why ? why : "poisoned by the caller";
    t->batch_open = false;
  }
  return SWZ_OK;
}

int swz_tiler_level_count(swz_tiler* t, int level, uint64_t* count_out) {
  if (!t || !count_out || level < -1 || level > 20) return SWZ_ERR_BAD_ARG;
  SWZ_TRY(tiler_guard(t));
  *count_out = t->lv[level + 1].cnt;
  return SWZ_OK;
}

int swz_tiler_level_positions_device(swz_tiler* t, int level, double* d_xyz_out) {
  if (!t || level < -1 || level > 20) return SWZ_ERR_BAD_ARG;
  swz_ctx* c = t->c;
  SWZ_HIP(c, hipSetDevice(c->device));
  SWZ_TRY(tiler_guard(t));
  StoreLevel& s = t->lv[level + 1];
  if (!s.cnt) return SWZ_OK;
  if (!d_xyz_out) return c->fail(SWZ_ERR_BAD_ARG, "swz_tiler_level_positions_device: NULL buffer");
  SWZ_TRY(store_linearize(t, s, level + 1));
  hipLaunchKernelGGL(tl_rows_kernel, dim3(div_up(s.cnt, 256)), dim3(256), 0, c->stream, s.gid[s.cur], s.cnt, t->pool_xyz, d_xyz_out);
  SWZ_LAUNCH_CHECK(c);
  SWZ_HIP(c, hipStreamSynchronize(c->stream));
  return SWZ_OK;
}

int swz_tiler_stage_batch(swz_tiler* t, const double* xyz_host, uint64_t n, const swz_attribute_columns* attrs_host) {
  if (!t) return SWZ_ERR_BAD_ARG;
  swz_ctx* c = t->c;
  SWZ_HIP(c, hipSetDevice(c->device));
  SWZ_TRY(tiler_guard(t));
  SWZ_TRY(tiler_refuse_batch(t, n));  // (nothing is copied or staged for a batch that tile_staged would refuse)
  if (t->staged_sizes.size() >= 2) return c->fail(SWZ_ERR_BAD_ARG, "swz_tiler_stage_batch: two batches are already staged");
  if (n && !xyz_host) return c->fail(SWZ_ERR_BAD_ARG, "swz_tiler_stage_batch: NULL buffer");
  if ((uint64_t)t->staged_total + n > 0xFFFF0000ull) return c->fail(SWZ_ERR_TOO_MANY_POINTS, "more than 2^32-65536 points per tiler");
  uint32_t mask = 0;
  for (int a = 0; a < SWZ_ATTR_COUNT; ++a)
    if (attrs_host && attrs_host->column[a]) mask |= 1u << a;
  if (t->staged_total == 0 && t->batches == 0) {
    t->attr_mask = mask;
    if (mask && t->pool_cap) {  // the pools were presized before the columns were known
      const size_t cap = t->pool_cap;
      t->pool_cap = 0;
      t->pool_xyz = nullptr;
      SWZ_TRY(pool_reserve(t, cap));
    }
  } else if (mask != t->attr_mask) {
    return c->fail(SWZ_ERR_BAD_ARG, "swz_tiler_stage_batch: every batch must carry the same attribute columns");
  }
  SWZ_TRY(pool_reserve(t, (size_t)t->staged_total + n));
  const size_t at = t->staged_total;
  if (n) {
    SWZ_HIP(c, hipMemcpyAsync(t->pool_xyz + at * 3, xyz_host, (size_t)n * 24, hipMemcpyDefault, t->copy_stream));
    t->staged_bytes += n * 24;
    for (int a = 0; a < SWZ_ATTR_COUNT; ++a) {
      if (!(mask & (1u << a))) continue;
      const size_t rb = TILER_ATTR_BYTES[a];
      SWZ_HIP(c, hipMemcpyAsync((char*)t->pool_attr[a] + at * rb, attrs_host->column[a], (size_t)n * rb,
                                hipMemcpyDefault, t->copy_stream));
      t->staged_bytes += n * rb;
    }
  }
  hipEvent_t ev = nullptr;
  SWZ_HIP(c, hipEventCreateWithFlags(&ev, hipEventDisableTiming));
  SWZ_HIP(c, hipEventRecord(ev, t->copy_stream));
  t->staged_events.push_back(ev);
  t->staged_sizes.push_back((uint32_t)n);
  t->staged_total += (uint32_t)n;
  return SWZ_OK;
}

int swz_tiler_tile_staged(swz_tiler* t, swz_tile_stats* stats) {
  if (!t) return SWZ_ERR_BAD_ARG;
  swz_ctx* c = t->c;
  SWZ_HIP(c, hipSetDevice(c->device));
  SWZ_TRY(tiler_guard(t));
  if (t->staged_sizes.empty()) return c->fail(SWZ_ERR_BAD_ARG, "swz_tiler_tile_staged: nothing is staged");
  const uint32_t n = t->staged_sizes.front();
  hipEvent_t ev = t->staged_events.front();
  t->staged_sizes.erase(t->staged_sizes.begin());
  t->staged_events.erase(t->staged_events.begin());
  // this batch needs its copy complete; the copy of the NEXT staged batch keeps running beside the kernels
  const auto t0 = std::chrono::steady_clock::now();
  SWZ_HIP(c, hipEventSynchronize(ev));
  t->staged_wait_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  const int st = tiler_add_batch(t, t->pool_xyz + (size_t)t->total * 3, n, stats);
  (void)hipEventDestroy(ev);
  // (a failure also leaves the pools one staged batch ahead of the ids the next batch would use)
  return tiler_end_call(t, st);
}

int swz_tiler_add_batch(swz_tiler* t, const double* xyz_host, uint64_t n, const swz_attribute_columns* attrs_host,
                        swz_tile_stats* stats) {
  if (!t) return SWZ_ERR_BAD_ARG;
  if (!t->staged_sizes.empty()) return t->c->fail(SWZ_ERR_BAD_ARG, "swz_tiler_add_batch: staged batches are pending");
  SWZ_TRY(swz_tiler_stage_batch(t, xyz_host, n, attrs_host));
  return swz_tiler_tile_staged(t, stats);
}

int swz_tiler_finalize(swz_tiler* t, swz_tile_stats* stats) {
  if (!t) return SWZ_ERR_BAD_ARG;
  SWZ_HIP(t->c, hipSetDevice(t->c->device));
  SWZ_TRY(tiler_guard(t));
  const int st = tiler_finalize(t, stats);
  t->c->prof_collect();
  return tiler_poison(t, st);
}

int swz_tiler_get_info(swz_tiler* t, swz_tiler_info* info) {
  if (!t || !info) return SWZ_ERR_BAD_ARG;
  SWZ_HIP(t->c, hipSetDevice(t->c->device));
  std::memset(info, 0, sizeof(*info));
  info->num_points = t->total;
  info->num_stored = stored_total(t);
  info->num_batches = t->batches;
  info->rekey_inversions = t->rekey_inversions;
  info->fast_start_levels = t->fast_start;
  info->staged_bytes = t->staged_bytes;
  info->staged_wait_ms = t->staged_wait_ms;
  uint64_t nn = 0;
  SWZ_TRY(tiler_node_table(t, nullptr, nullptr, nullptr, nullptr, &nn));
  info->num_nodes = nn;
  return SWZ_OK;
}

uint32_t swz_tiler_merge_tile(void) { return merge_tile(); }
uint32_t swz_tiler_merge_lds(void) { return merge_lds(); }
uint32_t swz_tiler_gather_lds(void) { return gather_lds(); }

int swz_tiler_path_counts(swz_tiler* t, uint64_t* out, uint32_t n) {
  if (!t || (n && !out)) return SWZ_ERR_BAD_ARG;
  for (uint32_t i = 0; i < n; ++i) out[i] = i < TP_COUNT ? t->paths[i] : 0ull;
  return SWZ_OK;
}

int swz_tiler_pool_residency(swz_tiler* t, uint64_t* device_bytes_out, uint64_t* host_bytes_out) {
  if (!t) return SWZ_ERR_BAD_ARG;
  uint64_t dev = 0, host = 0;
  auto add = [&](const std::string& name) {
    auto it = t->c->bufs.find(name);
    if (it == t->c->bufs.end()) return;
    (it->second.host ? host : dev) += it->second.cap;
  };
  add("tiler_pool_xyz");
  for (int a = 0; a < SWZ_ATTR_COUNT; ++a)
    if (t->attr_mask & (1u << a)) add("tiler_pool_attr" + std::to_string(a));
  if (device_bytes_out) *device_bytes_out = dev;
  if (host_bytes_out) *host_bytes_out = host;
  return SWZ_OK;
}

int swz_tiler_reserve(swz_tiler* t, uint64_t total_points) {
  if (!t) return SWZ_ERR_BAD_ARG;
  swz_ctx* c = t->c;
  SWZ_HIP(c, hipSetDevice(c->device));
  SWZ_TRY(tiler_guard(t));
  if (total_points > 0xFFFF0000ull) return c->fail(SWZ_ERR_TOO_MANY_POINTS, "more than 2^32-65536 points per tiler");
  if (total_points <= t->pool_cap && t->pool_xyz) return SWZ_OK;
  return pool_reserve(t, (size_t)total_points);
}

int swz_tiler_store_residency(swz_tiler* t, uint64_t* device_bytes_out, uint64_t* host_bytes_out) {
  if (!t) return SWZ_ERR_BAD_ARG;
  uint64_t dev = 0, host = 0;
  for (const auto& kv : t->c->bufs)
    if (kv.first.compare(0, 11, "tiler_store") == 0) (kv.second.host ? host : dev) += kv.second.cap;
  if (device_bytes_out) *device_bytes_out = dev;
  if (host_bytes_out) *host_bytes_out = host;
  return SWZ_OK;
}

int swz_tiler_node_table(swz_tiler* t, uint64_t max_nodes, int8_t* node_level_out, uint64_t* node_key_out,
                         uint64_t* node_offset_out, uint64_t* node_count_out, uint64_t* num_nodes_out) {
  if (!t || !num_nodes_out) return SWZ_ERR_BAD_ARG;
  swz_ctx* c = t->c;
  SWZ_HIP(c, hipSetDevice(c->device));
  SWZ_TRY(tiler_guard(t));
  std::vector<int8_t> nl;
  std::vector<uint64_t> nk, no, nc;
  uint64_t nn = 0;
  SWZ_TRY(tiler_node_table(t, &nl, &nk, &no, &nc, &nn));
  *num_nodes_out = nn;
  if (nn > max_nodes) return c->fail(SWZ_ERR_BAD_ARG, "max_nodes too small");
  if (!node_level_out || !node_key_out || !node_offset_out || !node_count_out)
    return c->fail(SWZ_ERR_BAD_ARG, "swz_tiler_node_table: NULL buffer");
  std::memcpy(node_level_out, nl.data(), nn);
  std::memcpy(node_key_out, nk.data(), nn * 8);
  std::memcpy(node_offset_out, no.data(), nn * 8);
  std::memcpy(node_count_out, nc.data(), nn * 8);
  return SWZ_OK;
}

int swz_tiler_export_device(swz_tiler* t, uint64_t* d_keys_out, uint32_t* d_ids_out, int8_t* d_level_out) {
  if (!t) return SWZ_ERR_BAD_ARG;
  swz_ctx* c = t->c;
  SWZ_HIP(c, hipSetDevice(c->device));
  SWZ_TRY(tiler_guard(t));
  size_t off = 0;
  for (int l = 0; l < 22; ++l) {
    StoreLevel& s = t->lv[l];
    if (!s.cnt) continue;
    SWZ_TRY(store_linearize(t, s, l));
    if (d_keys_out) SWZ_HIP(c, hipMemcpyAsync(d_keys_out + off, s.key[s.cur], (size_t)s.cnt * 8, hipMemcpyDeviceToDevice, c->stream));
    if (d_ids_out) SWZ_HIP(c, hipMemcpyAsync(d_ids_out + off, s.gid[s.cur], (size_t)s.cnt * 4, hipMemcpyDeviceToDevice, c->stream));
    if (d_level_out) {
      hipLaunchKernelGGL(tl_fill_level_kernel, dim3(div_up(s.cnt, 256)), dim3(256), 0, c->stream, d_level_out + off, s.cnt,
                         (int8_t)(l - 1));
      SWZ_LAUNCH_CHECK(c);
    }
    off += s.cnt;
  }
  SWZ_HIP(c, hipStreamSynchronize(c->stream));
  return SWZ_OK;
}

// One batch as node files (see the header): a tiler of its own for the batch, closed by the second call.
int swz_tile_nodes_begin_device(swz_ctx* c, double* d_xyz, uint64_t n, const double bmin[3], const double bmax[3],
                                const swz_tile_params* params, uint64_t* num_stored_out, uint64_t* num_nodes_out, swz_tile_stats* stats) {
  if (!c) return SWZ_ERR_BAD_ARG;
  if (!num_stored_out || !num_nodes_out) return c->fail(SWZ_ERR_BAD_ARG, "swz_tile_nodes_begin_device: NULL argument");
  if (c->nodes_tiler) return c->fail(SWZ_ERR_BAD_ARG, "swz_tile_nodes_begin_device: the call before has not been closed (swz_tile_nodes_end_device)");
  swz_tiler* t = nullptr;
  SWZ_TRY(swz_tiler_create(c, bmin, bmax, params, n, &t));
  swz_tile_stats batch{}, fin{};
  int st = swz_tiler_add_batch_device(t, d_xyz, n, &batch);
  if (st == SWZ_OK) st = swz_tiler_finalize(t, &fin);
  swz_tiler_info info{};
  if (st == SWZ_OK) st = swz_tiler_get_info(t, &info);
  if (st != SWZ_OK) {
    const std::string why = c->err;  // (destroying the tiler must not lose the reason)
    (void)swz_tiler_destroy(t);
    return c->fail(st, why);
  }
  if (stats) {
    *stats = batch;
    stats->num_nodes = (uint32_t)info.num_nodes;
    stats->points_visited += fin.points_visited;
    stats->num_levels += fin.num_levels;
    stats->min_distance_rounds += fin.min_distance_rounds;
    stats->max_level = std::max(batch.max_level, fin.max_level);
  }
  *num_stored_out = info.num_stored;
  *num_nodes_out = info.num_nodes;
  c->nodes_tiler = t;
  return SWZ_OK;
}

int swz_tile_nodes_end_device(swz_ctx* c, uint64_t* d_keys_out, uint32_t* d_ids_out, int8_t* d_level_out, uint64_t max_nodes,
                              int8_t* node_level_out, uint64_t* node_key_out, uint64_t* node_offset_out, uint64_t* node_count_out) {
  if (!c) return SWZ_ERR_BAD_ARG;
  swz_tiler* t = c->nodes_tiler;
  if (!t) return c->fail(SWZ_ERR_BAD_ARG, "swz_tile_nodes_end_device: no call is open (swz_tile_nodes_begin_device)");
  int st = SWZ_OK;
  if (d_keys_out || d_ids_out || d_level_out) st = swz_tiler_export_device(t, d_keys_out, d_ids_out, d_level_out);
  if (st == SWZ_OK && (max_nodes || node_level_out || node_key_out || node_offset_out || node_count_out)) {
    uint64_t nn = 0;
    st = swz_tiler_node_table(t, max_nodes, node_level_out, node_key_out, node_offset_out, node_count_out, &nn);
  }
  const std::string why = c->err;
  c->nodes_tiler = nullptr;
  (void)swz_tiler_destroy(t);
  return st == SWZ_OK ? SWZ_OK : c->fail(st, why);
}

int swz_tiler_pools_device(swz_tiler* t, const double** d_xyz_out, swz_attribute_columns* d_attrs_out) {
  if (!t) return SWZ_ERR_BAD_ARG;
  if (d_xyz_out) *d_xyz_out = t->pool_xyz;
  if (d_attrs_out)
    for (int a = 0; a < SWZ_ATTR_COUNT; ++a) d_attrs_out->column[a] = (t->attr_mask & (1u << a)) ? t->pool_attr[a] : nullptr;
  return SWZ_OK;
}

}  // extern "C"
