// Shards that fail (swz_group_*, include/swz_gpu.h): a failing shard keeps walking through the group's barriers so that
// the others are not stranded, the call reports the first failure as "shard N: ...", and the group can be used again.
// Every case runs on one device with peer copies, on a 20 000-point uniform cloud in the unit cube with 2, 4 and 8
// shards, and prints "ok".  A shard that strands the others shows up as the caller's time limit.
// Exit code 0 = pass.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/swz_gpu.h"

static const size_t kN = 20000;
static const double kMin[3] = {0, 0, 0}, kMax[3] = {1, 1, 1};

#define CHECK(cond, ...)                   \
  do {                                     \
    if (!(cond)) {                         \
      std::fprintf(stderr, "FAIL: ");      \
      std::fprintf(stderr, __VA_ARGS__);   \
      std::fprintf(stderr, "\n");          \
      return false;                        \
    }                                      \
  } while (0)

static swz_tile_params params(int sampler, int strategy, uint32_t fast_concurrency) {
  swz_tile_params p{};
  p.sampler = sampler;
  p.max_points_per_node = 500;
  p.spacing_at_root = (float)(std::sqrt(3.0) / 60.0);
  p.max_depth = 100;
  p.strategy = strategy;
  p.fast_concurrency = fast_concurrency;
  return p;
}

// rows [first, first + count) of the cloud, in equal pieces on the shards' devices
struct Pieces {
  std::vector<double*> d_xyz;
  std::vector<uint64_t> cnt;
  bool upload(swz_group* g, const std::vector<double>& xyz, size_t first, size_t count) {
    const int shards = swz_group_num_shards(g);
    d_xyz.assign(shards, nullptr);
    cnt.assign(shards, 0);
    for (int s = 0; s < shards; ++s) {
      const size_t b0 = first + count * s / shards, b1 = first + count * (s + 1) / shards;
      cnt[s] = b1 - b0;
      swz_ctx* c = swz_group_ctx(g, s);
      CHECK(swz_device_alloc_on(c, std::max<uint64_t>(cnt[s], 1) * 24, (void**)&d_xyz[s]) == SWZ_OK, "device alloc");
      CHECK(!cnt[s] || swz_copy_to_device(c, d_xyz[s], xyz.data() + 3 * b0, cnt[s] * 24) == SWZ_OK, "upload");
    }
    return true;
  }
  ~Pieces() {
    for (double* p : d_xyz) swz_device_free(p);
  }
};

static bool new_group(int shards, swz_group** g) {
  std::vector<int> devices(shards, 0);
  CHECK(swz_group_create(shards, devices.data(), 0, g) == SWZ_OK, "swz_group_create: %s", swz_group_last_error(nullptr));
  return true;
}

// 1. swz_group_tile, FAST with fast_concurrency above the number of points: refused on every shard; the same group then
// tiles the cloud
static bool case_fast_refusal(int shards, const std::vector<double>& xyz) {
  swz_group* g = nullptr;
  if (!new_group(shards, &g)) return false;
  Pieces in;
  if (!in.upload(g, xyz, 0, kN)) return false;
  std::vector<swz_group_result> res(shards);
  swz_tile_params p = params(SWZ_RANDOM_GRID, SWZ_FAST, (uint32_t)kN + 1);
  const int st = swz_group_tile(g, in.d_xyz.data(), nullptr, in.cnt.data(), kMin, kMax, &p, res.data());
  CHECK(st == SWZ_ERR_BAD_ARG, "FAST below fast_concurrency: status %d, \"%s\"", st, swz_group_last_error(g));
  CHECK(std::strstr(swz_group_last_error(g), "fast_concurrency"), "the message does not name fast_concurrency: \"%s\"", swz_group_last_error(g));
  p.fast_concurrency = 8;
  CHECK(swz_group_tile(g, in.d_xyz.data(), nullptr, in.cnt.data(), kMin, kMax, &p, res.data()) == SWZ_OK, "the group after a refusal: %s",
        swz_group_last_error(g));
  uint64_t total = 0;
  for (int s = 0; s < shards; ++s) {
    const uint64_t m = res[s].num_points;
    total += m;
    std::vector<uint64_t> k(m);
    CHECK(!m || swz_copy_to_host(swz_group_ctx(g, s), k.data(), res[s].d_keys, m * 8) == SWZ_OK, "download");
    CHECK(std::is_sorted(k.begin(), k.end()), "keys of shard %d do not ascend", s);
  }
  CHECK(total == kN, "%llu points after the exchange, %zu went in", (unsigned long long)total, kN);
  swz_group_destroy(g);
  std::printf("FAST refusal in swz_group_tile, %d shards ok\n", shards);
  return true;
}

// 2. the same through a data set in batches: the refused batch poisons every shard's tiler; a fresh data set works
static bool case_fast_refusal_batch(int shards, const std::vector<double>& xyz) {
  swz_group* g = nullptr;
  if (!new_group(shards, &g)) return false;
  Pieces all, half[2];
  if (!all.upload(g, xyz, 0, kN) || !half[0].upload(g, xyz, 0, kN / 2) || !half[1].upload(g, xyz, kN / 2, kN - kN / 2)) return false;
  swz_tile_params p = params(SWZ_RANDOM_GRID, SWZ_FAST, (uint32_t)kN + 1);
  CHECK(swz_group_tiler_open(g, kMin, kMax, &p, 0) == SWZ_OK, "swz_group_tiler_open: %s", swz_group_last_error(g));
  int st = swz_group_add_batch(g, all.d_xyz.data(), nullptr, all.cnt.data(), nullptr);
  CHECK(st == SWZ_ERR_BAD_ARG, "FAST batch below fast_concurrency: status %d, \"%s\"", st, swz_group_last_error(g));
  CHECK(std::strstr(swz_group_last_error(g), "fast_concurrency"), "the message does not name fast_concurrency: \"%s\"", swz_group_last_error(g));
  st = swz_group_add_batch(g, all.d_xyz.data(), nullptr, all.cnt.data(), nullptr);
  CHECK(st == SWZ_ERR_TILER_FAILED, "a batch after the refused one: status %d, \"%s\"", st, swz_group_last_error(g));
  CHECK(swz_group_tiler_close(g) == SWZ_OK, "swz_group_tiler_close");
  p.fast_concurrency = 8;
  CHECK(swz_group_tiler_open(g, kMin, kMax, &p, 0) == SWZ_OK, "swz_group_tiler_open after a poisoned data set: %s", swz_group_last_error(g));
  for (int b = 0; b < 2; ++b)
    CHECK(swz_group_add_batch(g, half[b].d_xyz.data(), nullptr, half[b].cnt.data(), nullptr) == SWZ_OK, "batch %d of the fresh data set: %s", b,
          swz_group_last_error(g));
  CHECK(swz_group_finalize(g, nullptr) == SWZ_OK, "swz_group_finalize: %s", swz_group_last_error(g));
  CHECK(swz_group_tiler_close(g) == SWZ_OK, "swz_group_tiler_close");
  swz_group_destroy(g);
  std::printf("FAST refusal in swz_group_add_batch, %d shards ok\n", shards);
  return true;
}

static bool refused(swz_group* g, int st, const char* what) {
  CHECK(st == SWZ_ERR_BAD_ARG, "%s: status %d, \"%s\"", what, st, swz_group_last_error(g));
  CHECK(swz_group_last_error(g)[0] != 0, "%s: no message", what);
  return true;
}

// 3. what is refused before any shard thread starts
static bool case_refused_up_front(int shards, const std::vector<double>& xyz) {
  swz_group* g = nullptr;
  if (!new_group(shards, &g)) return false;
  Pieces in;
  if (!in.upload(g, xyz, 0, kN)) return false;
  swz_tile_params p = params(SWZ_GRID_CENTER, SWZ_ACCURATE, 8);
  // only shard 1 brings a GPS time column
  void* d_gps = nullptr;
  CHECK(swz_device_alloc_on(swz_group_ctx(g, 1), std::max<uint64_t>(in.cnt[1], 1) * 8, &d_gps) == SWZ_OK, "device alloc");
  std::vector<swz_attribute_columns> uneven(shards, swz_attribute_columns{});
  uneven[1].column[SWZ_ATTR_GPS_TIME] = d_gps;
  std::vector<swz_group_result> res(shards);
  if (!refused(g, swz_group_tile(g, in.d_xyz.data(), uneven.data(), in.cnt.data(), kMin, kMax, &p, res.data()), "swz_group_tile, uneven columns")) return false;
  // no data set open
  std::vector<const double*> h_xyz(shards, nullptr);
  std::vector<void*> pinned(shards, nullptr);
  for (int s = 0; s < shards; ++s) {
    CHECK(swz_host_alloc_pinned(std::max<uint64_t>(in.cnt[s], 1) * 24, &pinned[s]) == SWZ_OK, "pinned alloc");
    std::copy(xyz.begin() + 3 * (kN * s / shards), xyz.begin() + 3 * (kN * (s + 1) / shards), (double*)pinned[s]);
    h_xyz[s] = (const double*)pinned[s];
  }
  if (!refused(g, swz_group_add_batch(g, in.d_xyz.data(), nullptr, in.cnt.data(), nullptr), "swz_group_add_batch, no data set")) return false;
  if (!refused(g, swz_group_stage_batch(g, h_xyz.data(), nullptr, in.cnt.data()), "swz_group_stage_batch, no data set")) return false;
  if (!refused(g, swz_group_tile_staged(g, nullptr), "swz_group_tile_staged, no data set")) return false;
  if (!refused(g, swz_group_finalize(g, nullptr), "swz_group_finalize, no data set")) return false;
  // an open data set
  CHECK(swz_group_tiler_open(g, kMin, kMax, &p, 0) == SWZ_OK, "swz_group_tiler_open: %s", swz_group_last_error(g));
  if (!refused(g, swz_group_add_batch(g, in.d_xyz.data(), uneven.data(), in.cnt.data(), nullptr), "swz_group_add_batch, uneven columns")) return false;
  if (!refused(g, swz_group_tile_staged(g, nullptr), "swz_group_tile_staged, nothing staged")) return false;
  CHECK(swz_group_stage_batch(g, h_xyz.data(), nullptr, in.cnt.data()) == SWZ_OK, "swz_group_stage_batch: %s", swz_group_last_error(g));
  CHECK(swz_group_stage_batch(g, h_xyz.data(), nullptr, in.cnt.data()) == SWZ_OK, "swz_group_stage_batch (second): %s", swz_group_last_error(g));
  if (!refused(g, swz_group_stage_batch(g, h_xyz.data(), nullptr, in.cnt.data()), "a third swz_group_stage_batch")) return false;
  if (!refused(g, swz_group_finalize(g, nullptr), "swz_group_finalize with batches staged")) return false;
  CHECK(swz_group_tiler_close(g) == SWZ_OK, "swz_group_tiler_close");
  for (void* q : pinned) swz_host_free_pinned(q);
  swz_device_free(d_gps);
  swz_group_destroy(g);
  std::printf("refusals before any shard thread starts, %d shards ok\n", shards);
  return true;
}

// 4. shard 1 alone fails at the MIN_DISTANCE root of a batch (its position pool cannot grow: the library's switch for an
// allocation that fails, with spilling off).  The call must come back -- the root swept by all shards at once, where the
// group meets the others for the shard that never reached the sweep, and the root taken in turns, where the failed shard
// still takes its turn and passes it on -- and the data set is poisoned.
static bool case_one_shard_fails_at_the_root(int shards, bool joint, const std::vector<double>& xyz) {
  swz_group* g = nullptr;
  if (!new_group(shards, &g)) return false;
  Pieces in;
  if (!in.upload(g, xyz, 0, kN)) return false;
  swz_tile_params p = params(SWZ_MIN_DISTANCE, SWZ_ACCURATE, 8);
  if (!joint)
    for (int s = 0; s < shards; ++s) CHECK(swz_set_option(swz_group_ctx(g, s), "SWZ_GROUP_JOINT_ROOT", "0") == SWZ_OK, "swz_set_option");
  CHECK(swz_group_tiler_open(g, kMin, kMax, &p, 0) == SWZ_OK, "swz_group_tiler_open: %s", swz_group_last_error(g));
  CHECK(swz_set_option(swz_group_ctx(g, 1), "SWZ_TILER_SPILL", "off") == SWZ_OK, "swz_set_option");
  CHECK(swz_set_option(swz_group_ctx(g, 1), "SWZ_FAIL_ALLOC", "tiler_pool_xyz") == SWZ_OK, "swz_set_option");
  int st = swz_group_add_batch(g, in.d_xyz.data(), nullptr, in.cnt.data(), nullptr);
  const std::string msg = swz_group_last_error(g);
  CHECK(st != SWZ_OK, "the batch went through although shard 1 cannot store it");
  CHECK(msg.compare(0, 5, "shard") == 0, "the message does not begin with the shard: \"%s\"", msg.c_str());
  std::printf("  (status %d, \"%s\")\n", st, msg.c_str());
  st = swz_group_add_batch(g, in.d_xyz.data(), nullptr, in.cnt.data(), nullptr);
  CHECK(st == SWZ_ERR_TILER_FAILED, "a batch after the failed one: status %d, \"%s\"", st, swz_group_last_error(g));
  CHECK(swz_group_tiler_close(g) == SWZ_OK, "swz_group_tiler_close");
  swz_group_destroy(g);
  std::printf("one shard fails at the root %s, %d shards ok\n", joint ? "swept by all shards at once" : "taken in turns", shards);
  return true;
}

int main() {
  std::vector<double> xyz(kN * 3);
  uint64_t state = 0x9E3779B97F4A7C15ull;
  for (double& v : xyz) {
    state = state * 6364136223846793005ull + 1442695040888963407ull;
    v = (double)(state >> 11) / 9007199254740992.0;
  }
  for (int shards : {2, 4, 8}) {
    if (!case_fast_refusal(shards, xyz)) return 1;
    if (!case_fast_refusal_batch(shards, xyz)) return 1;
    if (!case_refused_up_front(shards, xyz)) return 1;
  }
  for (int shards : {2, 8})
    for (bool joint : {true, false})
      if (!case_one_shard_fails_at_the_root(shards, joint, xyz)) return 1;
  return 0;
}
