// swz_group_write_output against swz_tiler_write_output of a single swz_tiler fed the same batches in this process: the
// program tiles a data set both ways, writes both directories and prints "pair <single dir> <group dir>" for each;
// tests/test_cpp_group_output.py compares every pair file by file, byte for byte.  What can be checked here is checked
// here: no two points share a Morton key (so that the order inside a file is defined by the keys alone), every shard of
// the 8-shard run holds a part of the root, the edge data sets look as described, every refusal refuses, leaves no
// directory behind and leaves the group usable.
// Usage: test_group_output <work dir> <shards> [part]     (all shards on device 0, peer copies)
// part (8 shards): acc_md | acc_rg | fast_rg_<format> | edges; none = everything.  The FAST leg is one part per format: below
// 100 000 points per range FAST starts at level 6 (estimate_start_node_level_in_octree), which gives this data set 76 115
// nodes, most of one point -- two seconds of file creation per directory on either side.
// Exit code 0 = pass.
#include <sys/stat.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>
#include <string>
#include <vector>

#include "../../include/swz_gpu.h"
#include "../../schwarzwald_amd/host/swz_tiling.hpp"

static int g_pairs = 0;
static const auto g_t0 = std::chrono::steady_clock::now();
static void stamp(const char* what) {  // where the time of a run goes, for whoever has to shorten it
  std::printf("time %8.0f ms  %s\n", std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - g_t0).count(), what);
}

#define REQUIRE(cond, what)                                                     \
  do {                                                                          \
    if (!(cond)) {                                                              \
      std::fprintf(stderr, "FAIL (%s:%d): %s\n", __FILE__, __LINE__, what);     \
      return false;                                                             \
    }                                                                           \
  } while (0)

struct Data {
  size_t n = 0;
  std::vector<double> xyz, gps;
  std::vector<uint8_t> rgb, cls;
  std::vector<uint16_t> intensity;
  swz_attribute_columns columns(size_t first) {
    swz_attribute_columns c{};
    c.column[SWZ_ATTR_RGB] = rgb.data() + 3 * first;
    c.column[SWZ_ATTR_INTENSITY] = intensity.data() + first;
    c.column[SWZ_ATTR_CLASSIFICATION] = cls.data() + first;
    c.column[SWZ_ATTR_GPS_TIME] = gps.data() + first;
    return c;
  }
};
static const uint32_t kMask = (1u << SWZ_ATTR_RGB) | (1u << SWZ_ATTR_INTENSITY) | (1u << SWZ_ATTR_CLASSIFICATION) | (1u << SWZ_ATTR_GPS_TIME);

// seeded uniform doubles in [0, scale)^3 plus one dense clump (a sixth of the points)
static Data make_data(size_t n, uint64_t seed, double scale) {
  Data d;
  d.n = n;
  d.xyz.resize(3 * n);
  d.gps.resize(n);
  d.rgb.resize(3 * n);
  d.cls.resize(n);
  d.intensity.resize(n);
  std::mt19937_64 rng(seed);
  std::uniform_real_distribution<double> u(0.0, 1.0);
  const double clump[3] = {0.31, 0.62, 0.17};
  for (size_t i = 0; i < n; ++i) {
    const bool in_clump = i % 6 == 5;
    for (int a = 0; a < 3; ++a) d.xyz[3 * i + a] = scale * (in_clump ? clump[a] + 0.02 * u(rng) : u(rng));
    d.gps[i] = 1000.0 + 0.25 * (double)i;
    d.rgb[3 * i] = (uint8_t)i, d.rgb[3 * i + 1] = (uint8_t)(i >> 8), d.rgb[3 * i + 2] = (uint8_t)(i * 7);
    d.cls[i] = (uint8_t)(i % 19);
    d.intensity[i] = (uint16_t)(i * 31 + 5);
  }
  return d;
}

static bool keys_distinct(swz_ctx* c, const Data& d, const double mn[3], const double mx[3]) {
  std::vector<double> copy(d.xyz);
  std::vector<uint64_t> keys(d.n);
  REQUIRE(swz_morton_encode(c, copy.data(), d.n, mn, mx, keys.data()) == SWZ_OK, swz_last_error(c));
  std::sort(keys.begin(), keys.end());
  REQUIRE(std::adjacent_find(keys.begin(), keys.end()) == keys.end(), "two points share a Morton key: file order would not be defined by the keys");
  return true;
}

static bool exists(const std::string& path) {
  struct stat st;
  return stat(path.c_str(), &st) == 0;
}

static swz_tile_params tile_params(int sampler, int strategy, float spacing) {
  swz_tile_params p{};
  p.sampler = sampler;
  p.max_points_per_node = 500;
  p.spacing_at_root = spacing;
  p.max_depth = 100;
  p.strategy = strategy;
  p.fast_concurrency = 8;
  return p;
}

// the yardstick: one tiler, the batches one after the other, finalize
static bool tile_single(swz_ctx* c, Data& d, int batches, const double mn[3], const double mx[3], const swz_tile_params& p, swz_tiler** out) {
  REQUIRE(swz_tiler_create(c, mn, mx, &p, 0, out) == SWZ_OK, swz_last_error(c));
  for (int b = 0; b < batches; ++b) {
    const size_t b0 = d.n * b / batches, b1 = d.n * (b + 1) / batches;
    std::vector<double> copy(d.xyz.begin() + 3 * b0, d.xyz.begin() + 3 * b1);  // (the call clamps in place)
    const swz_attribute_columns cols = d.columns(b0);
    REQUIRE(swz_tiler_add_batch(*out, copy.data(), b1 - b0, &cols, nullptr) == SWZ_OK, swz_last_error(c));
  }
  REQUIRE(swz_tiler_finalize(*out, nullptr) == SWZ_OK, swz_last_error(c));
  stamp("single tiled");
  return true;
}

// one batch of the group: the rows lie on the shards in uneven pieces, the second piece empty (as tests/cpp/test_group.cpp)
static bool group_batch(swz_group* g, Data& d, size_t b0, size_t bn) {
  const int shards = swz_group_num_shards(g);
  std::vector<size_t> bc(shards + 1, 0);
  for (int s = 1; s <= shards; ++s) bc[s] = (s == 2 && shards > 2) ? bc[1] : std::min(bn, (size_t)((double)bn * s * s / ((double)shards * shards)));
  bc[shards] = bn;
  std::vector<double*> d_xyz(shards, nullptr);
  std::vector<swz_attribute_columns> d_attrs(shards);
  std::vector<uint64_t> cnt(shards);
  bool ok = true;
  for (int s = 0; s < shards && ok; ++s) {
    cnt[s] = bc[s + 1] - bc[s];
    d_attrs[s] = swz_attribute_columns{};
    const uint64_t rows = std::max<uint64_t>(cnt[s], 1);
    swz_ctx* c = swz_group_ctx(g, s);
    const swz_attribute_columns host = d.columns(b0 + bc[s]);
    ok = swz_device_alloc_on(c, rows * 24, (void**)&d_xyz[s]) == SWZ_OK;
    if (ok && cnt[s]) ok = swz_copy_to_device(c, d_xyz[s], d.xyz.data() + 3 * (b0 + bc[s]), cnt[s] * 24) == SWZ_OK;
    for (int a = 0; a < SWZ_ATTR_COUNT && ok; ++a) {
      if (!host.column[a]) continue;
      const uint32_t rb = swz_attribute_row_bytes(a);
      ok = swz_device_alloc_on(c, rows * rb, &d_attrs[s].column[a]) == SWZ_OK;
      if (ok && cnt[s]) ok = swz_copy_to_device(c, d_attrs[s].column[a], host.column[a], cnt[s] * rb) == SWZ_OK;
    }
  }
  REQUIRE(ok, "upload of a batch");
  const int st = swz_group_add_batch(g, d_xyz.data(), d_attrs.data(), cnt.data(), nullptr);
  for (int s = 0; s < shards; ++s) {
    swz_device_free(d_xyz[s]);
    for (int a = 0; a < SWZ_ATTR_COUNT; ++a) swz_device_free(d_attrs[s].column[a]);
  }
  REQUIRE(st == SWZ_OK, swz_group_last_error(g));
  return true;
}

static bool tile_group(swz_group* g, Data& d, int batches, const double mn[3], const double mx[3], const swz_tile_params& p) {
  REQUIRE(swz_group_tiler_open(g, mn, mx, &p, 0) == SWZ_OK, swz_group_last_error(g));
  for (int b = 0; b < batches; ++b) {
    const size_t b0 = d.n * b / batches, b1 = d.n * (b + 1) / batches;
    if (!group_batch(g, d, b0, b1 - b0)) return false;
  }
  REQUIRE(swz_group_finalize(g, nullptr) == SWZ_OK, swz_group_last_error(g));
  stamp("group tiled");
  return true;
}

static swz_output_params out_params(int format, uint64_t chunk_points, const swz_ept_json* ept = nullptr) {
  swz_output_params o{};
  o.format = format;
  o.attribute_mask = kMask;
  o.rgb_mapping = SWZ_PNTS_RGB_FROM_COLOR;
  o.chunk_points = chunk_points;
  o.ept = ept;
  return o;
}

// writes both directories and announces the pair; the group's statistics must describe the merged table
static bool write_pair(const std::string& work, const std::string& leg, swz_tiler* single, swz_group* g, const swz_output_params& o) {
  const std::string a = work + "/single_" + leg, b = work + "/group_" + leg;
  swz_output_stats want{}, total{};
  std::vector<swz_output_stats> per(swz_group_num_shards(g));
  REQUIRE(swz_tiler_write_output(single, a.c_str(), &o, &want) == SWZ_OK, "swz_tiler_write_output");
  if (swz_group_write_output(g, b.c_str(), &o, per.data(), &total) != SWZ_OK) {
    std::fprintf(stderr, "FAIL: swz_group_write_output (%s): %s\n", leg.c_str(), swz_group_last_error(g));
    return false;
  }
  REQUIRE(total.nodes == want.nodes && total.stored_points == want.stored_points, "total: nodes and stored points of the merged table");
  REQUIRE(total.bytes_written == want.bytes_written, "total: the bytes of all shards are the single tiler's");
  uint64_t bytes = 0;
  for (const swz_output_stats& s : per) bytes += s.bytes_written;
  REQUIRE(bytes == total.bytes_written, "total: bytes summed over the shards");
  std::printf("pair %s %s\n", a.c_str(), b.c_str());
  char line[256];
  std::snprintf(line, sizeof(line), "%s: %llu nodes, single %.0f ms (pack %.0f copy %.0f write %.0f), group %.0f ms (pack %.0f copy %.0f write %.0f)", leg.c_str(),
                (unsigned long long)want.nodes, want.wall_ms, want.pack_ms, want.copy_ms, want.write_ms, total.wall_ms, total.pack_ms, total.copy_ms, total.write_ms);
  stamp(line);
  ++g_pairs;
  return true;
}

static const char* kFormat[5] = {"bin", "binz", "3dtiles", "las", "ept"};

static swz_ept_json ept_for(const double mn[3], const double mx[3], uint64_t points) {
  swz_ept_json e{};
  for (int a = 0; a < 3; ++a) {
    e.bounds_min[a] = e.conforming_min[a] = mn[a];
    e.bounds_max[a] = e.conforming_max[a] = mx[a];
  }
  e.points = points;
  e.attribute_mask = kMask;
  e.span = 128;
  e.srs_authority = "EPSG";
  e.srs_horizontal = "25832";
  e.srs_wkt = "";
  e.version = "1.0.0";
  return e;
}

static bool refused(swz_group* g, const std::string& dir, const swz_output_params& o, const char* what) {
  const int st = swz_group_write_output(g, dir.c_str(), &o, nullptr, nullptr);
  if (st != SWZ_ERR_BAD_ARG || exists(dir)) {
    std::fprintf(stderr, "FAIL: %s: status %d (%s), directory %s\n", what, st, swz_group_last_error(g), exists(dir) ? "exists" : "absent");
    return false;
  }
  std::printf("refused: %s -- %s\n", what, swz_group_last_error(g));
  return true;
}

static bool run(const std::string& work, int shards, const std::string& part) {
  auto wanted = [&](const std::string& name) { return part.empty() || part == name; };
  const double mn[3] = {0, 0, 0}, mx[3] = {1, 1, 1};
  const float spacing = 0.1f;  // the root samples (60 000 points > 500) and keeps a few hundred points of every octant
  swz_ctx* c = nullptr;
  REQUIRE(swz_create(&c, 0) == SWZ_OK, "swz_create");
  std::vector<int> devices(shards, 0);
  swz_group* g = nullptr;
  REQUIRE(swz_group_create(shards, devices.data(), 0, &g) == SWZ_OK, "swz_group_create");
  Data d = make_data(60000, 11, 1.0);
  if (!keys_distinct(c, d, mn, mx)) return false;
  const swz_ept_json ept = ept_for(mn, mx, d.n);

  struct Leg {
    const char* name;
    int sampler, strategy;
  };
  std::vector<Leg> legs = {{"acc_md", SWZ_MIN_DISTANCE, SWZ_ACCURATE}};
  if (shards == 8) {
    legs.push_back({"acc_rg", SWZ_RANDOM_GRID, SWZ_ACCURATE});
    legs.push_back({"fast_rg", SWZ_RANDOM_GRID, SWZ_FAST});
  }
  for (const Leg& leg : legs) {
    if (shards == 8 && !part.empty() && part.compare(0, std::strlen(leg.name), leg.name) != 0) continue;
    const swz_tile_params p = tile_params(leg.sampler, leg.strategy, spacing);
    swz_tiler* single = nullptr;
    if (!tile_single(c, d, 3, mn, mx, p, &single) || !tile_group(g, d, 3, mn, mx, p)) return false;
    if (shards == 8)
      for (int s = 0; s < shards; ++s) {
        uint64_t part = 0;
        REQUIRE(swz_tiler_level_count(swz_group_tiler(g, s), -1, &part) == SWZ_OK && part > 0, "every shard of the 8-shard run holds a part of the root");
      }
    // the merged table is the single tiler's
    swz_tiler_info info{};
    REQUIRE(swz_tiler_get_info(single, &info) == SWZ_OK, "swz_tiler_get_info");
    std::vector<int8_t> l1(info.num_nodes), l2(info.num_nodes);
    std::vector<uint64_t> k1(info.num_nodes), o1(info.num_nodes), c1(info.num_nodes), k2(info.num_nodes), c2(info.num_nodes);
    std::vector<int32_t> owner(info.num_nodes);
    uint64_t n1 = 0, n2 = 0;
    REQUIRE(swz_tiler_node_table(single, info.num_nodes, l1.data(), k1.data(), o1.data(), c1.data(), &n1) == SWZ_OK, "swz_tiler_node_table");
    REQUIRE(swz_group_node_table(g, info.num_nodes, l2.data(), k2.data(), c2.data(), owner.data(), &n2) == SWZ_OK, swz_group_last_error(g));
    REQUIRE(n1 == n2 && l1 == l2 && k1 == k2 && c1 == c2, "swz_group_node_table differs from the single tiler's table");
    for (uint64_t k = 0; k < n2; ++k)
      REQUIRE(l2[k] < 0 ? owner[k] == -1 : owner[k] == (int)(k2[k] >> 60) * shards / 8, "a node's owner is the shard of its level-0 octant");
    if (shards == 8) {
      for (int f = 0; f < 5; ++f) {
        const std::string name = std::string(leg.name) + "_" + kFormat[f];
        if (leg.strategy == SWZ_FAST && !wanted(name)) continue;
        if (!write_pair(work, name, single, g, out_params(f, 4096, f == SWZ_OUT_ENTWINE_LAS ? &ept : nullptr))) return false;
      }
      // chunk_points 0 (one chunk per shard) once
      if (leg.sampler == SWZ_MIN_DISTANCE && !write_pair(work, std::string(leg.name) + "_bin_chunk0", single, g, out_params(SWZ_OUT_BIN, 0))) return false;
    } else {
      if (!write_pair(work, std::string(leg.name) + "_3dtiles", single, g, out_params(SWZ_OUT_3DTILES, 4096))) return false;
      if (!write_pair(work, std::string(leg.name) + "_ept", single, g, out_params(SWZ_OUT_ENTWINE_LAS, 4096, &ept))) return false;
    }

    if (shards == 8 && leg.sampler == SWZ_MIN_DISTANCE) {
      // ---- 3DTILES with the grey value of the intensity as colour and a UTM-sized offset
      swz_output_params o = out_params(SWZ_OUT_3DTILES, 4096);
      o.rgb_mapping = SWZ_PNTS_RGB_FROM_INTENSITY_LOG;
      o.global_offset[0] = 432100.25, o.global_offset[1] = 5412345.5, o.global_offset[2] = 310.125;
      if (!write_pair(work, "acc_md_3dtiles_log_utm", single, g, o)) return false;

      // ---- refusals: each before anything is created, and after each a valid call gives the single tiler's directory
      const std::string dir = work + "/refused";
      int valid = 0;
      auto then_valid = [&]() { return write_pair(work, "acc_md_bin_after_refusal" + std::to_string(valid++), single, g, out_params(SWZ_OUT_BIN, 4096)); };
      swz_output_params bad = out_params(7, 4096);
      if (!refused(g, dir, bad, "an unknown format") || !then_valid()) return false;
      bad = out_params(SWZ_OUT_BIN, 4096);
      bad.attribute_mask |= 1u << SWZ_ATTR_USER_DATA;
      if (!refused(g, dir, bad, "a mask naming a column the batches did not carry") || !then_valid()) return false;
      bad = out_params(SWZ_OUT_3DTILES, 4096);
      bad.attribute_mask = 1u << SWZ_ATTR_RGB;
      bad.rgb_mapping = SWZ_PNTS_RGB_FROM_INTENSITY_LINEAR;
      if (!refused(g, dir, bad, "an rgb_mapping without intensities") || !then_valid()) return false;
      bad = out_params(SWZ_OUT_3DTILES, 4096);
      bad.global_offset[1] = std::numeric_limits<double>::infinity();
      if (!refused(g, dir, bad, "a global_offset that is not finite") || !then_valid()) return false;
      {
        const std::string file = work + "/a_regular_file";
        FILE* f = std::fopen(file.c_str(), "wb");
        REQUIRE(f != nullptr, "cannot create a file in the work directory");
        std::fclose(f);
        for (int fmt : {SWZ_OUT_BIN, SWZ_OUT_ENTWINE_LAS})
          if (!refused(g, file + "/sub", out_params(fmt, 4096), "a dir whose parent is a regular file") || !then_valid()) return false;
      }
      {  // a batch staged on the group
        std::vector<const double*> h(shards, d.xyz.data());
        std::vector<swz_attribute_columns> ha(shards, d.columns(0));
        std::vector<uint64_t> cnt(shards, 16);
        // (staging only copies; a staged batch cannot be taken back, so the valid call that follows this refusal and the next
        // one is the one after the data set has been closed and tiled again)
        REQUIRE(swz_group_stage_batch(g, h.data(), ha.data(), cnt.data()) == SWZ_OK, swz_group_last_error(g));
        if (!refused(g, dir, out_params(SWZ_OUT_BIN, 4096), "the call while a batch is staged")) return false;
      }
    }
    REQUIRE(swz_group_tiler_close(g) == SWZ_OK, "swz_group_tiler_close");
    if (shards == 8 && leg.sampler == SWZ_MIN_DISTANCE) {
      if (!refused(g, work + "/refused", out_params(SWZ_OUT_BIN, 4096), "the call before swz_group_tiler_open")) return false;
      // ... and the group is usable: the same data set again, the same directory
      if (!tile_group(g, d, 3, mn, mx, p)) return false;
      if (!write_pair(work, "acc_md_las_after_reopen", single, g, out_params(SWZ_OUT_LAS, 4096))) return false;
      REQUIRE(swz_group_tiler_close(g) == SWZ_OK, "swz_group_tiler_close");
    }
    REQUIRE(swz_tiler_destroy(single) == SWZ_OK, "swz_tiler_destroy");
  }

  if (shards == 8 && wanted("edges")) {
    const swz_tile_params p = tile_params(SWZ_MIN_DISTANCE, SWZ_ACCURATE, spacing);
    {  // ---- a data set inside octant 0: seven shards have no node and no part of the root
      Data e = make_data(30000, 12, 0.49);
      if (!keys_distinct(c, e, mn, mx)) return false;
      swz_tiler* single = nullptr;
      if (!tile_single(c, e, 3, mn, mx, p, &single) || !tile_group(g, e, 3, mn, mx, p)) return false;
      for (int s = 1; s < shards; ++s) {
        swz_tiler_info info{};
        REQUIRE(swz_tiler_get_info(swz_group_tiler(g, s), &info) == SWZ_OK && info.num_nodes == 0, "octant 0 only: shards 1..7 hold no node");
      }
      for (int f : {SWZ_OUT_BIN, SWZ_OUT_3DTILES, SWZ_OUT_ENTWINE_LAS})
        if (!write_pair(work, std::string("octant0_") + kFormat[f], single, g, out_params(f, 4096, f == SWZ_OUT_ENTWINE_LAS ? &ept : nullptr))) return false;
      REQUIRE(swz_group_tiler_close(g) == SWZ_OK && swz_tiler_destroy(single) == SWZ_OK, "close");
    }
    {  // ---- 300 points: the root takes them all, its file is the only one and its parts lie on several shards
      Data e = make_data(300, 13, 1.0);
      if (!keys_distinct(c, e, mn, mx)) return false;
      swz_tiler* single = nullptr;
      if (!tile_single(c, e, 1, mn, mx, p, &single) || !tile_group(g, e, 1, mn, mx, p)) return false;
      uint64_t nn = 0;
      int holders = 0;
      REQUIRE(swz_group_node_table(g, 0, nullptr, nullptr, nullptr, nullptr, &nn) == SWZ_OK && nn == 1, "300 points: the root is the only node");
      for (int s = 0; s < shards; ++s) {
        uint64_t part = 0;
        REQUIRE(swz_tiler_level_count(swz_group_tiler(g, s), -1, &part) == SWZ_OK, "swz_tiler_level_count");
        holders += part > 0;
      }
      REQUIRE(holders >= 4, "300 points: the parts of the root are spread over the shards");
      for (int f = 0; f < 5; ++f)
        if (!write_pair(work, std::string("takeall_") + kFormat[f], single, g, out_params(f, 4096, f == SWZ_OUT_ENTWINE_LAS ? &ept : nullptr))) return false;
      REQUIRE(swz_group_tiler_close(g) == SWZ_OK && swz_tiler_destroy(single) == SWZ_OK, "close");
    }
    {  // ---- through the methods of the host adapter instead of the C ABI
      struct NoSink : swz_host::PointsSink {
        void persist_points(const uint32_t*, const uint32_t*, const double*, const swz_host::AABB&, const std::string&) override {}
      } sink;
      swz_host::TilerMetaParameters meta;
      meta.spacing_at_root = spacing;
      swz_host::SamplingStrategy strategy{SWZ_MIN_DISTANCE, 500};
      const swz_host::AABB box{{0, 0, 0}, {1, 1, 1}};
      swz_tiler* single = nullptr;
      if (!tile_single(c, d, 3, mn, mx, p, &single)) return false;
      try {
        swz_host::ShardedTilingAlgorithmGPU algo(strategy, sink, meta, devices, 0);
        algo.open_tiler(box, SWZ_ACCURATE);
        for (int b = 0; b < 3; ++b) {
          const size_t b0 = d.n * b / 3, b1 = d.n * (b + 1) / 3;
          const swz_attribute_columns cols = d.columns(b0);
          algo.add_batch(d.xyz.data() + 3 * b0, &cols, b1 - b0);
        }
        const std::string a = work + "/single_adapter_ept", b = work + "/group_adapter_ept";
        const swz_output_params o = out_params(SWZ_OUT_ENTWINE_LAS, 4096, &ept);
        REQUIRE(swz_tiler_write_output(single, a.c_str(), &o, nullptr) == SWZ_OK, "swz_tiler_write_output");
        const swz_output_stats total = algo.write_output(b, o);
        REQUIRE(total.stored_points == d.n, "the adapter's write_output returns the totals");
        std::printf("pair %s %s\n", a.c_str(), b.c_str());
        ++g_pairs;
      } catch (const std::exception& ex) {
        std::fprintf(stderr, "FAIL: the adapter threw: %s\n", ex.what());
        return false;
      }
      REQUIRE(swz_tiler_destroy(single) == SWZ_OK, "swz_tiler_destroy");
    }
  }
  REQUIRE(swz_group_destroy(g) == SWZ_OK, "swz_group_destroy");
  swz_destroy(c);
  std::printf("pairs %d\n", g_pairs);
  return true;
}

int main(int argc, char** argv) {
  if (argc < 3) {
    std::fprintf(stderr, "usage: test_group_output <work dir> <shards> [part]\n");
    return 2;
  }
  return run(argv[1], std::atoi(argv[2]), argc > 3 ? argv[3] : "") ? 0 : 1;
}
