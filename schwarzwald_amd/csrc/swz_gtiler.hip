// swz_gtiler.hip -- a data set in several batches on a group (BASELINE config 5 from the C++ host): one swz_tiler per
// shard (swz_group_tiler_open), batches staged from pinned host memory into two device buffers per shard and tiled through
// swz_group_add_batch (swz_group.hip), a data set of LAS files read in one call, and finalize with FAST's root rebuilt on
// shard 0.  swz_group_add_las_files has no thread of its own: it runs las_input_stream (swz_tinput.h) over one lane per
// shard, which decodes every shard's slice of a batch into its stage buffer and hands the batch to swz_group_tile_staged.
#include <algorithm>

#include "swz_group.h"
#include "swz_srs.h"
#include "swz_tinput.h"

using namespace swz;

namespace {
// flag of the i-th sorted element back to the position its element had before the sort
__global__ __launch_bounds__(256) void grp_unsort_flags_kernel(const uint32_t* __restrict__ perm, const uint8_t* __restrict__ taken, uint32_t n,
                                                               uint8_t* __restrict__ flags) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) flags[perm[i]] = taken[i];
}
}  // namespace

extern "C" {

static void group_free_tilers(swz_group* g) {
  for (swz_tiler* t : g->ds.tiler)
    if (t) (void)swz_tiler_destroy(t);
  g->ds.tiler.clear();
  for (size_t r = 0; r < g->stage.copy_stream.size(); ++r) {
    (void)hipSetDevice(g->devices[r]);
    if (g->stage.copy_stream[r]) {
      (void)hipStreamSynchronize(g->stage.copy_stream[r]);
      (void)hipStreamDestroy(g->stage.copy_stream[r]);
    }
    for (StageSlot& s : g->stage.slot[r]) {
      if (s.done) (void)hipEventDestroy(s.done);
      if (s.xyz) (void)hipFree(s.xyz);
      for (int t = 0; t < SWZ_ATTR_COUNT; ++t)
        if (s.attr.column[t]) (void)hipFree(s.attr.column[t]);
    }
  }
  g->stage = swz_group::Stage{};
}

int swz_group_tiler_open(swz_group* g, const double bmin[3], const double bmax[3], const swz_tile_params* params,
                         uint64_t capacity_hint_per_shard) {
  if (!g || !bmin || !bmax || !params) return SWZ_ERR_BAD_ARG;
  if (!g->ds.tiler.empty()) {
    g->err = "swz_group_tiler_open: a data set is open already (swz_group_tiler_close)";
    return SWZ_ERR_BAD_ARG;
  }
  if (const char* why = sharded_sampler_refusal(params->sampler)) {
    g->err = why;
    return SWZ_ERR_BAD_ARG;
  }
  g->ds.fast_start = -1;
  g->ds.has_srs = false;
  g->call.hist.assign(g->n, std::vector<uint32_t>());
  for (int a = 0; a < 3; ++a) {
    g->ds.bmin[a] = bmin[a];
    g->ds.bmax[a] = bmax[a];
  }
  g->ds.params = *params;
  g->ds.tiler.assign(g->n, nullptr);
  for (int r = 0; r < g->n; ++r) {
    (void)hipSetDevice(g->devices[r]);
    const int st = swz_tiler_create(g->ctx[r], bmin, bmax, params, capacity_hint_per_shard, &g->ds.tiler[r]);
    if (st != SWZ_OK) {
      g->err = shard_says(r, swz_last_error(g->ctx[r]));
      group_free_tilers(g);
      return st;
    }
  }
  g->ds.root_stored.assign(g->n, 0);
  g->stage.copy_stream.assign(g->n, nullptr);
  g->stage.slot.assign(g->n, {});
  return SWZ_OK;
}

int swz_group_tiler_close(swz_group* g) {
  if (!g) return SWZ_ERR_BAD_ARG;
  group_free_tilers(g);
  g->ds.has_srs = false;
  return SWZ_OK;
}

int swz_group_set_source_srs(swz_group* g, const swz_srs* srs) {
  if (!g) return SWZ_ERR_BAD_ARG;
  auto refuse = [&](const std::string& why) {
    g->err = why;
    return (int)SWZ_ERR_BAD_ARG;
  };
  if (g->ds.tiler.empty()) return refuse("swz_group_set_source_srs: no data set is open (swz_group_tiler_open)");
  if (!g->stage.staged.empty()) return refuse("swz_group_set_source_srs: a batch is staged or open");
  for (const swz_tiler* t : g->ds.tiler)
    if (t->failed || t->finalized || !tiler_empty(t))
      return refuse("swz_group_set_source_srs: the data set holds points, or a batch is staged or open");
  if (srs && !srs_valid(srs)) return refuse("swz_group_set_source_srs: not a definition swz_srs_parse made");
  g->ds.has_srs = srs != nullptr;
  if (srs) g->ds.srs = *srs;
  return SWZ_OK;
}

swz_tiler* swz_group_tiler(swz_group* g, int shard) {
  return (g && shard >= 0 && shard < (int)g->ds.tiler.size()) ? g->ds.tiler[shard] : nullptr;
}

static bool stage_hip(swz_group* g, int r, hipError_t e, const char* what) {
  if (e == hipSuccess) return true;
  g->err = shard_says(r, std::string(what) + ": " + hipGetErrorString(e));
  return false;
}

// shard r's copy stream, the event of the slot and its device buffers for `rows` rows of the columns in `mask` (the device
// of shard r is current); false: g->err.  A buffer that grows is free: the batch it held has been tiled --
// swz_group_tile_staged returns after the shard's stream is idle.
static bool stage_reserve(swz_group* g, int slot, int r, uint64_t rows, uint32_t mask) {
  auto hip = [&](hipError_t e, const char* what) { return stage_hip(g, r, e, what); };
  StageSlot& s = g->stage.slot[r][slot];
  if (!g->stage.copy_stream[r] && !hip(hipStreamCreateWithFlags(&g->stage.copy_stream[r], hipStreamNonBlocking), "hipStreamCreate")) return false;
  if (!s.done && !hip(hipEventCreateWithFlags(&s.done, hipEventDisableTiming), "hipEventCreate")) return false;
  if (s.cap >= std::max<uint64_t>(rows, 1) && !(mask & ~g->stage.mask)) return true;
  const uint64_t cap = std::max<uint64_t>(rows + rows / 8, 1);
  if (s.xyz) (void)hipFree(s.xyz);
  s.xyz = nullptr;
  s.cap = 0;
  if (!hip(hipMalloc(&s.xyz, cap * 24), "hipMalloc(stage)")) return false;
  for (int t = 0; t < SWZ_ATTR_COUNT; ++t) {
    if (s.attr.column[t]) (void)hipFree(s.attr.column[t]);
    s.attr.column[t] = nullptr;
    if ((mask >> t) & 1u)
      if (!hip(hipMalloc(&s.attr.column[t], cap * swz_attribute_row_bytes(t)), "hipMalloc(stage column)")) return false;
  }
  s.cap = cap;
  return true;
}

// Staging: the batch is copied from pinned host memory into one of two device buffers per shard on the shard's copy
// stream, beside whatever its tiling stream is doing (the batch before).  At most two batches are staged.
int swz_group_stage_batch(swz_group* g, const double* const* xyz_host, const swz_attribute_columns* attrs_host, const uint64_t* n) {
  if (!g || !xyz_host || !n) return SWZ_ERR_BAD_ARG;
  if (g->ds.tiler.empty() || g->stage.staged.size() >= 2) {
    g->err = g->ds.tiler.empty() ? "swz_group_stage_batch: no data set is open" : "swz_group_stage_batch: two batches are staged already";
    return SWZ_ERR_BAD_ARG;
  }
  uint32_t mask = 0;
  if (const int st = common_columns(g, attrs_host, &mask)) return st;
  const int slot = g->stage.next_slot;
  swz_group::Staged sb;
  sb.slot = slot;
  sb.n.assign(n, n + g->n);
  for (int r = 0; r < g->n; ++r) {
    (void)hipSetDevice(g->devices[r]);
    auto hip = [&](hipError_t e, const char* what) { return stage_hip(g, r, e, what); };
    if (!stage_reserve(g, slot, r, n[r], mask)) return SWZ_ERR_HIP;
    const StageSlot& s = g->stage.slot[r][slot];
    hipStream_t cs = g->stage.copy_stream[r];
    if (n[r]) {
      if (!hip(hipMemcpyAsync(s.xyz, xyz_host[r], n[r] * 24, hipMemcpyHostToDevice, cs), "hipMemcpyAsync")) return SWZ_ERR_HIP;
      for (int t = 0; t < SWZ_ATTR_COUNT; ++t)
        if ((mask >> t) & 1u)
          if (!hip(hipMemcpyAsync(s.attr.column[t], attrs_host[r].column[t], n[r] * swz_attribute_row_bytes(t), hipMemcpyHostToDevice, cs),
                   "hipMemcpyAsync")) return SWZ_ERR_HIP;
    }
    if (!hip(hipEventRecord(s.done, cs), "hipEventRecord")) return SWZ_ERR_HIP;
  }
  g->stage.mask |= mask;
  g->stage.staged.push_back(sb);
  g->stage.next_slot ^= 1;
  return SWZ_OK;
}

int swz_group_tile_staged(swz_group* g, swz_tile_stats* stats) {
  if (!g) return SWZ_ERR_BAD_ARG;
  if (g->stage.staged.empty()) {
    g->err = "swz_group_tile_staged: nothing is staged";
    return SWZ_ERR_BAD_ARG;
  }
  const swz_group::Staged sb = g->stage.staged.front();
  g->stage.staged.erase(g->stage.staged.begin());
  std::vector<double*> xyz(g->n);
  std::vector<swz_attribute_columns> attrs(g->n);
  for (int r = 0; r < g->n; ++r) {
    (void)hipSetDevice(g->devices[r]);
    const StageSlot& s = g->stage.slot[r][sb.slot];
    // the shard's kernels wait for its copy on the device; the host goes on
    if (!stage_hip(g, r, hipStreamWaitEvent(g->ctx[r]->stream, s.done, 0), "hipStreamWaitEvent")) return SWZ_ERR_HIP;
    xyz[r] = s.xyz;
    attrs[r] = s.attr;
  }
  return swz_group_add_batch(g, xyz.data(), g->stage.mask ? attrs.data() : nullptr, sb.n.data(), stats);
}

// A data set of LAS files through the group in one call: swz_tiler_add_las_files's scan, refusals and cuts ONCE
// (swz_tinput.h), then per batch every shard reads, copies and decodes its slice of the batch's points -- consecutive
// slices in shard order -- into one of its two stage buffers, and the batch goes the way of swz_group_tile_staged.
int swz_group_add_las_files(swz_group* g, const char* const* paths, uint64_t num_files, const swz_input_params* params,
                            swz_input_stats* stats) {
  if (!g) return SWZ_ERR_BAD_ARG;
  const char* who = "swz_group_add_las_files";
  const auto t_wall = std::chrono::steady_clock::now();
  if (stats) *stats = swz_input_stats{};
  auto refuse = [&](int st, const std::string& why) {
    g->err = why;
    return st;
  };
  if (!params || (num_files && !paths)) return refuse(SWZ_ERR_BAD_ARG, "swz_group_add_las_files: NULL argument");
  if (g->ds.tiler.empty()) return refuse(SWZ_ERR_BAD_ARG, "swz_group_add_las_files: no data set is open (swz_group_tiler_open)");
  if (!g->stage.staged.empty()) return refuse(SWZ_ERR_BAD_ARG, "swz_group_add_las_files: a batch is staged or open");
  const int N = g->n;
  bool mask_fixed = false;
  uint32_t mask_now = 0;
  uint64_t points_now = 0;  // the worst case: one shard receives everything
  for (int r = 0; r < N; ++r) {
    const swz_tiler* t = g->ds.tiler[r];
    std::string why;
    if (const int st = tiler_refuses_input(t, who, &why))
      return refuse(st, shard_says(r, (st == SWZ_ERR_TILER_FAILED ? "the tiler has failed: " : "") + why));
    if (!tiler_empty(t) && !mask_fixed) {
      mask_fixed = true;
      mask_now = t->attr_mask;
    }
    points_now = std::max<uint64_t>(points_now, t->staged_total);
  }
  swz_ctx* c0 = g->ctx[0];
  (void)hipSetDevice(g->devices[0]);
  const swz_srs* const srs = g->ds.has_srs ? &g->ds.srs : nullptr;
  LasInputPlan plan;
  int st = las_input_plan(c0, who, paths, num_files, params, g->ds.bmin, g->ds.bmax, g->ds.params, mask_fixed, mask_now, points_now, srs, &plan);
  if (st != SWZ_OK) return refuse(st, swz_last_error(c0));

  // ---- per shard: its slices, two raw images, host and device, and the two stage buffers the slices are decoded into
  const bool two = plan.num_batches() > 1;
  std::vector<InputLane> lanes(N);
  for (int r = 0; r < N; ++r) {
    InputLane& lane = lanes[r];
    (void)hipSetDevice(g->devices[r]);
    lane.c = g->ctx[r];
    lane.cut(plan, r, N);
    if ((st = lane.ib.reserve(lane.c, std::max<uint64_t>(lane.image_max, 16), two)) != SWZ_OK) return refuse(st, shard_says(r, swz_last_error(lane.c)));
    for (int k = 0; k < (two ? 2 : 1); ++k)
      if (!stage_reserve(g, g->stage.next_slot ^ k, r, lane.rows_max, plan.mask)) return SWZ_ERR_HIP;
    lane.copy = g->stage.copy_stream[r];
  }
  g->stage.mask |= plan.mask;

  // ---- the stream: every batch into the stage buffers of the next slot, staged like a pinned batch
  InputStreamOps ops;
  ops.lane_name = "shard";
  ops.target = [&](int r) {
    const StageSlot& s = g->stage.slot[r][g->stage.next_slot];
    return InputTarget{s.xyz, s.attr, plan.mask};
  };
  ops.commit = [&](uint64_t j, std::string* why) -> int {
    swz_group::Staged sb;
    sb.slot = g->stage.next_slot;
    for (int r = 0; r < N; ++r) {
      (void)hipSetDevice(g->devices[r]);
      if (!stage_hip(g, r, hipEventRecord(g->stage.slot[r][sb.slot].done, g->stage.copy_stream[r]), "hipEventRecord")) {
        *why = g->err;
        return SWZ_ERR_HIP;
      }
      sb.n.push_back(lanes[r].batches[j].points);
    }
    g->stage.staged.push_back(sb);
    g->stage.next_slot ^= 1;
    return SWZ_OK;
  };
  ops.tile = [&](double* waited_ms, std::string* why) -> int {
    *waited_ms = 0;  // (the shards' streams wait for their copies on the device)
    const int rc = swz_group_tile_staged(g, nullptr);  // (a failure here has poisoned every tiler with its own text)
    if (rc != SWZ_OK) *why = g->err;
    return rc;
  };
  InputStreamResult res;
  las_input_stream(plan, srs, who, paths, lanes, ops, &res);
  g->stage.staged.clear();  // (a batch staged behind the one that failed is dropped)
  // (until the first batch is handed to swz_group_tile_staged the slices lie in the group's stage buffers: no tiler has seen them)
  if (res.status != SWZ_OK && res.tiled)
    for (int r = 0; r < N; ++r) (void)swz_tiler_poison(g->ds.tiler[r], res.why.c_str());
  if (stats) res.fill(stats, plan.ds.readable_files, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_wall).count());
  if (res.status != SWZ_OK) g->err = res.why;
  return res.status;
}

// a failure of shard r while the data set is finalized: nobody goes on
static int finalize_fail(swz_group* g, int r, int rc) {
  g->err = "shard " + std::to_string(r) + ": " + swz_last_error(g->ctx[r]);
  for (int s = 0; s < g->n; ++s) (void)swz_tiler_poison(g->ds.tiler[s], ("the group failed to finalize: " + g->err).c_str());
  return rc;
}

// The root of TilingAlgorithmV3::finalize (reconstruct_single_node, :1661-1715) samples what its eight children hold,
// and they lie on different shards: their files come together on shard 0 in shard order (= octant order: the order
// the reference appends them in), are indexed against the root bounds and sampled with AlwaysAdhereToMinSpacing there.
// *d_flags0: one flag per row, in the order the rows came in.
static int finalize_fast_root_on_shard0(swz_group* g, const std::vector<uint64_t>& cnt, const std::vector<uint64_t>& off, uint8_t** d_flags0) {
  const uint64_t total = off[g->n];
  swz_ctx* c0 = g->ctx[0];
  (void)hipSetDevice(g->devices[0]);
  double* all = nullptr;
  uint64_t *keys = nullptr, *skeys = nullptr;
  uint32_t* perm = nullptr;
  uint8_t* taken = nullptr;
  if (c0->get("grp_root_xyz", (size_t)total * 3, &all) != SWZ_OK || c0->get("grp_root_keys", (size_t)total, &keys) != SWZ_OK ||
      c0->get("grp_root_skeys", (size_t)total, &skeys) != SWZ_OK || c0->get("grp_root_perm", (size_t)total, &perm) != SWZ_OK ||
      c0->get("grp_root_taken", (size_t)total, &taken) != SWZ_OK || c0->get("grp_root_flags", (size_t)total, d_flags0) != SWZ_OK)
    return finalize_fail(g, 0, SWZ_ERR_HIP);
  std::vector<const void*> files(g->n, nullptr);
  for (int r = 0; r < g->n; ++r) {
    if (!cnt[r]) continue;
    (void)hipSetDevice(g->devices[r]);
    swz_ctx* c = g->ctx[r];
    double* mine = nullptr;
    if (c->get("grp_l0_xyz", (size_t)cnt[r] * 3, &mine) != SWZ_OK) return finalize_fail(g, r, SWZ_ERR_HIP);
    const int rc = swz_tiler_level_positions_device(g->ds.tiler[r], 0, mine);
    if (rc != SWZ_OK) return finalize_fail(g, r, rc);
    if (hipStreamSynchronize(c->stream) != hipSuccess) {
      c->err = "copy of the level-0 file to shard 0 failed";
      return finalize_fail(g, r, SWZ_ERR_HIP);
    }
    files[r] = mine;
  }
  (void)hipSetDevice(g->devices[0]);
  if (rows_to_shard0(g, cnt, off, {{all, files, 24}}) != hipSuccess) {
    c0->err = "copy of the level-0 files to shard 0 failed";
    return finalize_fail(g, 0, SWZ_ERR_HIP);
  }
  int rc = swz_morton_encode_device(c0, all, total, g->ds.bmin, g->ds.bmax, keys);
  if (rc == SWZ_OK) rc = swz_sort_by_key_device(c0, keys, total, perm, skeys);
  if (rc == SWZ_OK)
    rc = swz::sample_points_device(c0, g->ds.params.sampler, g->ds.params.max_points_per_node, skeys, perm, (uint32_t)total, all, 0, -1, g->ds.bmin,
                                   g->ds.bmax, g->ds.params.spacing_at_root, SWZ_ALWAYS_ADHERE_TO_MIN_SPACING, taken, nullptr);
  if (rc != SWZ_OK) return finalize_fail(g, 0, rc);
  hipLaunchKernelGGL(grp_unsort_flags_kernel, dim3((uint32_t)((total + 255) / 256)), dim3(256), 0, c0->stream, perm, taken, (uint32_t)total, *d_flags0);
  if (hipStreamSynchronize(c0->stream) != hipSuccess) {
    c0->err = "root reconstruction failed on the device";
    return finalize_fail(g, 0, SWZ_ERR_HIP);
  }
  return SWZ_OK;
}

int swz_group_finalize(swz_group* g, swz_tile_stats* stats) {
  if (!g) return SWZ_ERR_BAD_ARG;
  if (g->ds.tiler.empty() || !g->stage.staged.empty()) {
    g->err = g->ds.tiler.empty() ? "swz_group_finalize: no data set is open" : "swz_group_finalize: staged batches have not been tiled";
    return SWZ_ERR_BAD_ARG;
  }
  const bool fast = g->ds.params.strategy == SWZ_FAST && g->ds.fast_start > 0;
  for (int r = 0; r < g->n; ++r) {
    (void)hipSetDevice(g->devices[r]);
    swz_tile_stats st{};
    const int rc = fast ? swz_tiler_shard_fast_finalize_local(g->ds.tiler[r], &st) : swz_tiler_finalize(g->ds.tiler[r], &st);
    if (rc != SWZ_OK) return finalize_fail(g, r, rc);
    if (stats) stats[r] = st;
  }
  if (!fast) return SWZ_OK;
  // FAST: the root is rebuilt from the level-0 files of all shards on shard 0; every shard keeps the part of the root's
  // file that comes from its own points
  std::vector<uint64_t> cnt(g->n, 0), off(g->n + 1, 0);
  for (int r = 0; r < g->n; ++r) {
    (void)hipSetDevice(g->devices[r]);
    const int rc = swz_tiler_level_count(g->ds.tiler[r], 0, &cnt[r]);
    if (rc != SWZ_OK) return finalize_fail(g, r, rc);
    off[r + 1] = off[r] + cnt[r];
  }
  uint8_t* d_flags0 = nullptr;
  if (off[g->n] > 0xFFFF0000ull) {
    g->err = "more than 2^32-65536 points in the level-0 files";
    return SWZ_ERR_TOO_MANY_POINTS;
  }
  if (off[g->n]) {
    const int rc = finalize_fast_root_on_shard0(g, cnt, off, &d_flags0);
    if (rc != SWZ_OK) return rc;
  }
  for (int r = 0; r < g->n; ++r) {
    (void)hipSetDevice(g->devices[r]);
    swz_ctx* c = g->ctx[r];
    uint8_t* mine = (r == 0 && cnt[0]) ? d_flags0 : nullptr;
    if (cnt[r] && r != 0) {
      if (c->get("grp_l0_flags", (size_t)cnt[r], &mine) != SWZ_OK) return finalize_fail(g, r, SWZ_ERR_HIP);
      if (flags_to_shard(g, r, mine, d_flags0 + off[r], cnt[r]) != hipSuccess) {
        c->err = "copy of the root flags failed";
        return finalize_fail(g, r, SWZ_ERR_HIP);
      }
    }
    const int rc = swz_tiler_shard_fast_set_root(g->ds.tiler[r], mine);
    if (rc != SWZ_OK) return finalize_fail(g, r, rc);
  }
  return SWZ_OK;
}

}  // extern "C"
