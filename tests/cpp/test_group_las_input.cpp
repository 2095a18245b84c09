// swz_group_add_las_files against swz_tiler_add_las_files of a single swz_tiler in this process: the program reads the
// same LAS files both ways, finalizes, writes both data sets (swz_tiler_write_output / swz_group_write_output, LAS and
// BIN) and prints "pair <single dir> <group dir>" for each; tests/test_cpp_group_las_input.py writes the files and compares
// every pair file by file, byte for byte.  Checked here: stats.points and stats.batches equal the single call's, the
// batches span files and a folded FAST tail is folded on both sides, and (mode acc) every refusal refuses, names what it
// should and leaves swz_tiler_get_info of every shard as it was -- the data set is added after them.
// Usage: test_group_las_input <work dir> <shards> <mode> <laz-flagged file> <file> ...   (all shards on device 0, peer copies)
// mode: acc   = ACCURATE MIN_DISTANCE, the refusals first
//       fast  = FAST RANDOM_GRID, fast_concurrency 5000: the tail of 4002 points joins the batch before it
//       shift = ACCURATE MIN_DISTANCE with shift_to_center, the group driven through ShardedTilingAlgorithmGPU
//       tail  = acc without the refusals, batch_points 13 333: the last batch holds 3 of the 40 002 points, so with 8 shards
//               most shards get an empty slice of a batch that is not empty
//       one   = acc without the refusals, batch_points 50 000: the whole data set is one batch, every shard holds one image
// Exit code 0 = pass.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/swz_gpu.h"
#include "../../schwarzwald_amd/host/swz_tiling.hpp"

#define REQUIRE(cond, what)                                                     \
  do {                                                                          \
    if (!(cond)) {                                                              \
      std::fprintf(stderr, "FAIL (%s:%d): %s\n", __FILE__, __LINE__, what);     \
      return false;                                                             \
    }                                                                           \
  } while (0)

static uint64_t kBatchPoints = 9000;  // (modes tail and one set their own)

static bool same_info(const swz_tiler_info& a, const swz_tiler_info& b) {
  return a.num_points == b.num_points && a.num_stored == b.num_stored && a.num_nodes == b.num_nodes && a.num_batches == b.num_batches &&
         a.rekey_inversions == b.rekey_inversions && a.fast_start_levels == b.fast_start_levels && a.staged_bytes == b.staged_bytes;
}

// the call must refuse with `status`, name `needle`, and leave every shard's tiler as it was
static bool refused(swz_group* g, const std::vector<const char*>& paths, const swz_input_params& ip, int status, const char* needle,
                    const char* what) {
  const int shards = swz_group_num_shards(g);
  std::vector<swz_tiler_info> before(shards), after(shards);
  for (int s = 0; s < shards; ++s) REQUIRE(swz_tiler_get_info(swz_group_tiler(g, s), &before[s]) == SWZ_OK, "swz_tiler_get_info");
  swz_input_stats st{};
  const int rc = swz_group_add_las_files(g, paths.data(), paths.size(), &ip, &st);
  if (rc != status || !std::strstr(swz_group_last_error(g), needle)) {
    std::fprintf(stderr, "FAIL: %s: status %d, wanted %d with \"%s\": %s\n", what, rc, status, needle, swz_group_last_error(g));
    return false;
  }
  REQUIRE(st.points == 0 && st.batches == 0, "a refused call reads nothing");
  for (int s = 0; s < shards; ++s) {
    REQUIRE(swz_tiler_get_info(swz_group_tiler(g, s), &after[s]) == SWZ_OK, "a refusal poisons no tiler");
    REQUIRE(same_info(before[s], after[s]), "a refusal leaves swz_tiler_get_info of every shard unchanged");
  }
  std::printf("refused: %s -- %s\n", what, swz_group_last_error(g));
  return true;
}

static bool run(const std::string& work, int shards, const std::string& mode, const char* laz, const std::vector<const char*>& paths) {
  const bool fast = mode == "fast", shift = mode == "shift", tail = mode == "tail", one = mode == "one";
  REQUIRE(fast || shift || tail || one || mode == "acc", "mode: acc | fast | shift | tail | one");
  if (tail) kBatchPoints = 13333;
  if (one) kBatchPoints = 50000;
  swz_ctx* c = nullptr;
  REQUIRE(swz_create(&c, 0) == SWZ_OK, "swz_create");
  swz_las_dataset ds{};
  REQUIRE(swz_las_scan_files(c, paths.data(), paths.size(), 0, nullptr, &ds) == SWZ_OK, swz_last_error(c));
  const double* mn = shift ? ds.origin_min : ds.cubic_min;
  const double* mx = shift ? ds.origin_max : ds.cubic_max;
  swz_tile_params p{};
  p.sampler = fast ? SWZ_RANDOM_GRID : SWZ_MIN_DISTANCE;
  p.max_points_per_node = 500;
  p.spacing_at_root = (float)((mx[0] - mn[0]) / 50.0);
  p.max_depth = 100;
  p.strategy = fast ? SWZ_FAST : SWZ_ACCURATE;
  p.fast_concurrency = fast ? 5000 : 8;
  swz_input_params ip{};
  ip.batch_points = kBatchPoints;
  ip.attribute_mask = ~0u;
  ip.shift_to_center = shift ? 1 : 0;

  // ---- the yardstick: one tiler, one call
  swz_tiler* single = nullptr;
  swz_input_stats want{};
  REQUIRE(swz_tiler_create(c, mn, mx, &p, 0, &single) == SWZ_OK, swz_last_error(c));
  REQUIRE(swz_tiler_add_las_files(single, paths.data(), paths.size(), &ip, &want) == SWZ_OK, swz_last_error(c));
  REQUIRE(swz_tiler_finalize(single, nullptr) == SWZ_OK, swz_last_error(c));
  REQUIRE(want.points == ds.total_points && (one || want.points > (tail ? 3 : 4) * kBatchPoints), "the data set spans several batches");
  if (tail) REQUIRE(want.points % kBatchPoints == 3 && shards == 8, "the last batch has fewer points than the group has shards");
  if (one) REQUIRE(want.batches == 1 && kBatchPoints >= want.points, "the whole data set is one batch");
  const uint64_t cut_batches = (ds.total_points + kBatchPoints - 1) / kBatchPoints;
  REQUIRE(want.batches == (fast ? cut_batches - 1 : cut_batches), "FAST folds the short tail into the batch before it, ACCURATE keeps it");

  const uint32_t out_mask = ds.attribute_mask;
  std::vector<int> devices(shards, 0);
  auto write_single = [&](int format, const std::string& dir, swz_output_params* o) {
    *o = swz_output_params{};
    o->format = format;
    o->attribute_mask = out_mask;
    o->rgb_mapping = SWZ_PNTS_RGB_FROM_COLOR;
    o->chunk_points = 4096;
    return swz_tiler_write_output(single, dir.c_str(), o, nullptr) == SWZ_OK;
  };
  int pairs = 0;
  swz_input_stats got{};
  if (shift) {  // through the methods of the host adapter
    struct NoSink : swz_host::PointsSink {
      void persist_points(const uint32_t*, const uint32_t*, const double*, const swz_host::AABB&, const std::string&) override {}
    } sink;
    swz_host::TilerMetaParameters meta;
    meta.spacing_at_root = p.spacing_at_root;
    meta.max_depth = p.max_depth;
    swz_host::SamplingStrategy strategy{SWZ_MIN_DISTANCE, 500};
    const swz_host::AABB box{{mn[0], mn[1], mn[2]}, {mx[0], mx[1], mx[2]}};
    try {
      swz_host::ShardedTilingAlgorithmGPU algo(strategy, sink, meta, devices, 0);
      algo.open_tiler(box, SWZ_ACCURATE);
      std::vector<std::string> names(paths.begin(), paths.end());
      got = algo.add_las_files(names, ip);
      for (int format : {SWZ_OUT_LAS, SWZ_OUT_BIN}) {
        const std::string leg = format == SWZ_OUT_LAS ? "las" : "bin", a = work + "/single_" + leg, b = work + "/group_" + leg;
        swz_output_params o{};
        REQUIRE(write_single(format, a, &o), swz_last_error(c));
        algo.write_output(b, o);
        std::printf("pair %s %s\n", a.c_str(), b.c_str());
        ++pairs;
      }
    } catch (const std::exception& ex) {
      std::fprintf(stderr, "FAIL: the adapter threw: %s\n", ex.what());
      return false;
    }
  } else {
    swz_group* g = nullptr;
    REQUIRE(swz_group_create(shards, devices.data(), 0, &g) == SWZ_OK, "swz_group_create");
    REQUIRE(swz_group_add_las_files(g, paths.data(), paths.size(), &ip, nullptr) == SWZ_ERR_BAD_ARG, "the call before swz_group_tiler_open is refused");
    REQUIRE(swz_group_tiler_open(g, mn, mx, &p, 0) == SWZ_OK, swz_group_last_error(g));
    if (mode == "acc") {
      std::vector<const char*> with_laz(paths);
      with_laz.insert(with_laz.begin() + 2, laz);
      if (!refused(g, with_laz, ip, SWZ_ERR_BAD_ARG, laz, "a LAZ-flagged file, named")) return false;
      // a box that does not contain the data set: shifted to the centre it lies round the origin, the group's box does not
      swz_input_params bad = ip;
      bad.shift_to_center = 1;
      if (!refused(g, paths, bad, SWZ_ERR_BAD_ARG, "does not contain", "a box that does not contain the data set")) return false;
      bad = ip;
      bad.attribute_mask = ds.attribute_mask | (1u << SWZ_ATTR_NORMAL);
      if (!refused(g, paths, bad, SWZ_ERR_BAD_ARG, "normals", "SWZ_ATTR_NORMAL in the mask")) return false;
    }
    if (swz_group_add_las_files(g, paths.data(), paths.size(), &ip, &got) != SWZ_OK) {
      std::fprintf(stderr, "FAIL: swz_group_add_las_files: %s\n", swz_group_last_error(g));
      return false;
    }
    uint64_t on_shards = 0;
    for (int s = 0; s < shards; ++s) {
      swz_tiler_info info{};
      REQUIRE(swz_tiler_get_info(swz_group_tiler(g, s), &info) == SWZ_OK, "swz_tiler_get_info");
      REQUIRE(info.num_batches == want.batches, "every shard has seen every batch");
      on_shards += info.num_points;
    }
    REQUIRE(on_shards == want.points, "the shards hold the data set's points");
    REQUIRE(swz_group_finalize(g, nullptr) == SWZ_OK, swz_group_last_error(g));
    for (int format : {SWZ_OUT_LAS, SWZ_OUT_BIN}) {
      const std::string leg = format == SWZ_OUT_LAS ? "las" : "bin", a = work + "/single_" + leg, b = work + "/group_" + leg;
      swz_output_params o{};
      REQUIRE(write_single(format, a, &o), swz_last_error(c));
      if (swz_group_write_output(g, b.c_str(), &o, nullptr, nullptr) != SWZ_OK) {
        std::fprintf(stderr, "FAIL: swz_group_write_output: %s\n", swz_group_last_error(g));
        return false;
      }
      std::printf("pair %s %s\n", a.c_str(), b.c_str());
      ++pairs;
    }
    REQUIRE(swz_group_tiler_close(g) == SWZ_OK && swz_group_destroy(g) == SWZ_OK, "close");
  }
  std::printf("single: %llu points in %llu batches, %llu bytes; group: %llu points in %llu batches, %llu bytes\n", (unsigned long long)want.points,
              (unsigned long long)want.batches, (unsigned long long)want.bytes_read, (unsigned long long)got.points, (unsigned long long)got.batches,
              (unsigned long long)got.bytes_read);
  std::printf("group stats ms: wall %.3f read %.3f copy %.3f decode %.3f tile %.3f wait %.3f\n", got.wall_ms, got.read_ms, got.copy_ms,
              got.decode_ms, got.tile_ms, got.wait_ms);
  REQUIRE(got.points == want.points && got.batches == want.batches, "stats.points and stats.batches equal the single call's");
  REQUIRE(got.bytes_read == want.bytes_read && got.files == want.files, "stats.bytes_read and stats.files equal the single call's");
  REQUIRE(swz_tiler_destroy(single) == SWZ_OK, "swz_tiler_destroy");
  swz_destroy(c);
  std::printf("pairs %d\n", pairs);
  return true;
}

int main(int argc, char** argv) {
  if (argc < 6) {
    std::fprintf(stderr, "usage: test_group_las_input <work dir> <shards> <mode> <laz-flagged file> <file> ...\n");
    return 2;
  }
  std::vector<const char*> paths(argv + 5, argv + argc);
  return run(argv[1], std::atoi(argv[2]), argv[3], argv[4], paths) ? 0 : 1;
}
