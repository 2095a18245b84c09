// swz_group_set_source_srs + swz_group_add_las_files against swz_tiler_set_source_srs + swz_tiler_add_las_files of a single
// swz_tiler in this process: both read the same LAS files in a source projection, shifted to the centre of the data set's ECEF
// box (swz_las_scan_files_srs), finalize and write their data sets as BIN; the program prints "pair <single dir> <group dir>"
// and tests/test_cpp_group_srs.py compares the pair file by file, byte for byte -- the merged node table (the files' names and
// lengths) and every position.  Checked here: the set before swz_group_tiler_open and after the first batch is refused, a
// root box in the source CRS is refused with "does not contain" and touches no shard, swz_group_tiler_close forgets the
// projection (the source CRS's own box then takes the files as they are).
// Usage: test_group_srs <work dir> <shards> <mode> <definition> <file> ...   (all shards on device 0, peer copies)
// mode: abi     = the C calls
//       adapter = ShardedTilingAlgorithmGPU::add_las_files(paths, params, &SourceProjection)
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

static const uint64_t kBatchPoints = 9000;

static bool untouched(swz_group* g) {
  for (int s = 0; s < swz_group_num_shards(g); ++s) {
    swz_tiler_info info{};
    REQUIRE(swz_tiler_get_info(swz_group_tiler(g, s), &info) == SWZ_OK, "a refusal poisons no tiler");
    REQUIRE(info.num_points == 0 && info.num_batches == 0, "a refusal leaves every shard without points");
  }
  return true;
}

static bool run(const std::string& work, int shards, const std::string& mode, const char* definition, const std::vector<const char*>& paths) {
  const bool adapter = mode == "adapter";
  REQUIRE(adapter || mode == "abi", "mode: abi | adapter");
  swz_ctx* c = nullptr;
  REQUIRE(swz_create(&c, 0) == SWZ_OK, "swz_create");
  swz_srs srs{};
  REQUIRE(swz_srs_parse(c, definition, &srs) == SWZ_OK, swz_last_error(c));
  swz_las_dataset ds{}, plain{};
  REQUIRE(swz_las_scan_files_srs(c, paths.data(), paths.size(), 0, &srs, nullptr, &ds) == SWZ_OK, swz_last_error(c));
  REQUIRE(swz_las_scan_files(c, paths.data(), paths.size(), 0, nullptr, &plain) == SWZ_OK, swz_last_error(c));
  const double* mn = ds.origin_min;
  const double* mx = ds.origin_max;
  swz_tile_params p{};
  p.sampler = SWZ_MIN_DISTANCE;
  p.max_points_per_node = 300;
  p.spacing_at_root = (float)((mx[0] - mn[0]) / 50.0);
  p.max_depth = 100;
  p.strategy = SWZ_ACCURATE;
  p.fast_concurrency = 8;
  swz_input_params ip{};
  ip.batch_points = kBatchPoints;
  ip.attribute_mask = ~0u;
  ip.shift_to_center = 1;

  // ---- the yardstick (tiler A): one tiler, one call
  swz_tiler* single = nullptr;
  swz_input_stats want{}, got{};
  REQUIRE(swz_tiler_create(c, mn, mx, &p, 0, &single) == SWZ_OK, swz_last_error(c));
  REQUIRE(swz_tiler_set_source_srs(single, &srs) == SWZ_OK, swz_last_error(c));
  REQUIRE(swz_tiler_add_las_files(single, paths.data(), paths.size(), &ip, &want) == SWZ_OK, swz_last_error(c));
  REQUIRE(swz_tiler_finalize(single, nullptr) == SWZ_OK, swz_last_error(c));
  REQUIRE(want.points == ds.total_points && want.batches >= 3, "the data set spans several batches");

  std::vector<int> devices(shards, 0);
  swz_output_params o{};
  o.format = SWZ_OUT_BIN;
  o.attribute_mask = ds.attribute_mask;
  o.rgb_mapping = SWZ_PNTS_RGB_FROM_COLOR;
  o.chunk_points = 4096;
  const std::string a = work + "/single_bin", b = work + "/group_bin";
  REQUIRE(swz_tiler_write_output(single, a.c_str(), &o, nullptr) == SWZ_OK, swz_last_error(c));

  if (adapter) {
    struct NoSink : swz_host::PointsSink {
      void persist_points(const uint32_t*, const uint32_t*, const double*, const swz_host::AABB&, const std::string&) override {}
    } sink;
    swz_host::TilerMetaParameters meta;
    meta.spacing_at_root = p.spacing_at_root;
    meta.max_depth = p.max_depth;
    swz_host::SamplingStrategy strategy{SWZ_MIN_DISTANCE, 300};
    const swz_host::AABB box{{mn[0], mn[1], mn[2]}, {mx[0], mx[1], mx[2]}};
    try {
      const swz_host::SourceProjection projection{definition};
      swz_host::ShardedTilingAlgorithmGPU algo(strategy, sink, meta, devices, 0);
      algo.open_tiler(box, SWZ_ACCURATE);
      std::vector<std::string> names(paths.begin(), paths.end());
      got = algo.add_las_files(names, ip, &projection);
      bool threw = false;
      try {  // the projection can only come with the first points
        (void)algo.add_las_files(names, ip, &projection);
      } catch (const std::exception& ex) {
        threw = std::strstr(ex.what(), "swz_group_set_source_srs") != nullptr;
      }
      REQUIRE(threw, "a projection given after the first batch throws, naming swz_group_set_source_srs");
      std::printf("refused: a projection after the first batch (adapter)\n");
      algo.write_output(b, o);
    } catch (const std::exception& ex) {
      std::fprintf(stderr, "FAIL: the adapter threw: %s\n", ex.what());
      return false;
    }
  } else {
    swz_group* g = nullptr;
    REQUIRE(swz_group_create(shards, devices.data(), 0, &g) == SWZ_OK, "swz_group_create");
    REQUIRE(swz_group_set_source_srs(g, &srs) == SWZ_ERR_BAD_ARG && std::strstr(swz_group_last_error(g), "no data set is open"),
            "the set before swz_group_tiler_open is refused");
    std::printf("refused: set before open -- %s\n", swz_group_last_error(g));
    // a root box that is the source CRS's: refused by the existing message, no shard touched; the close forgets the projection
    REQUIRE(swz_group_tiler_open(g, plain.cubic_min, plain.cubic_max, &p, 0) == SWZ_OK, swz_group_last_error(g));
    REQUIRE(swz_group_set_source_srs(g, &srs) == SWZ_OK, swz_group_last_error(g));
    swz_input_stats st{};
    int rc = swz_group_add_las_files(g, paths.data(), paths.size(), &ip, &st);
    REQUIRE(rc == SWZ_ERR_BAD_ARG && std::strstr(swz_group_last_error(g), "does not contain"), swz_group_last_error(g));
    REQUIRE(st.points == 0 && untouched(g), "a refused call reads nothing");
    std::printf("refused: the source CRS's box with a projection -- %s\n", swz_group_last_error(g));
    REQUIRE(swz_group_tiler_close(g) == SWZ_OK, "close");
    // the close forgot the projection: the source CRS's cubic box, unshifted, now takes the files as they are
    REQUIRE(swz_group_tiler_open(g, plain.cubic_min, plain.cubic_max, &p, 0) == SWZ_OK, swz_group_last_error(g));
    swz_input_params as_is = ip;
    as_is.shift_to_center = 0;
    REQUIRE(swz_group_add_las_files(g, paths.data(), paths.size(), &as_is, &st) == SWZ_OK, swz_group_last_error(g));
    REQUIRE(st.points == ds.total_points, "without the projection the data set is read in its own CRS");
    REQUIRE(swz_group_tiler_close(g) == SWZ_OK, "close");
    REQUIRE(swz_group_tiler_open(g, mn, mx, &p, 0) == SWZ_OK, swz_group_last_error(g));
    REQUIRE(swz_group_set_source_srs(g, &srs) == SWZ_OK && swz_group_set_source_srs(g, nullptr) == SWZ_OK, "set and clear");
    swz_srs garbage{};
    garbage.kind = 7;
    REQUIRE(swz_group_set_source_srs(g, &garbage) == SWZ_ERR_BAD_ARG, "a struct swz_srs_parse did not make is refused");
    REQUIRE(swz_group_set_source_srs(g, &srs) == SWZ_OK, swz_group_last_error(g));
    if (swz_group_add_las_files(g, paths.data(), paths.size(), &ip, &got) != SWZ_OK) {
      std::fprintf(stderr, "FAIL: swz_group_add_las_files: %s\n", swz_group_last_error(g));
      return false;
    }
    REQUIRE(swz_group_set_source_srs(g, &srs) == SWZ_ERR_BAD_ARG && std::strstr(swz_group_last_error(g), "holds points"),
            "the set after the first batch is refused");
    std::printf("refused: set after the first batch -- %s\n", swz_group_last_error(g));
    REQUIRE(swz_group_set_source_srs(g, nullptr) == SWZ_ERR_BAD_ARG, "... and so is the clear");
    uint64_t on_shards = 0;
    for (int s = 0; s < shards; ++s) {
      swz_tiler_info info{};
      REQUIRE(swz_tiler_get_info(swz_group_tiler(g, s), &info) == SWZ_OK, "swz_tiler_get_info");
      REQUIRE(info.num_batches == want.batches, "every shard has seen every batch");
      on_shards += info.num_points;
    }
    REQUIRE(on_shards == want.points, "the shards hold the data set's points");
    REQUIRE(swz_group_finalize(g, nullptr) == SWZ_OK, swz_group_last_error(g));
    if (swz_group_write_output(g, b.c_str(), &o, nullptr, nullptr) != SWZ_OK) {
      std::fprintf(stderr, "FAIL: swz_group_write_output: %s\n", swz_group_last_error(g));
      return false;
    }
    REQUIRE(swz_group_tiler_close(g) == SWZ_OK && swz_group_destroy(g) == SWZ_OK, "close");
  }
  std::printf("pair %s %s\n", a.c_str(), b.c_str());
  REQUIRE(got.points == want.points && got.batches == want.batches && got.bytes_read == want.bytes_read, "the stats equal the single call's");
  REQUIRE(swz_tiler_destroy(single) == SWZ_OK, "swz_tiler_destroy");
  swz_destroy(c);
  return true;
}

int main(int argc, char** argv) {
  if (argc < 6) {
    std::fprintf(stderr, "usage: test_group_srs <work dir> <shards> <mode> <definition> <file> ...\n");
    return 2;
  }
  std::vector<const char*> paths(argv + 5, argv + argc);
  return run(argv[1], std::atoi(argv[2]), argv[3], argv[4], paths) ? 0 : 1;
}
