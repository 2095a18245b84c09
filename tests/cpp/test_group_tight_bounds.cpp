// SWZ_OUT_TIGHT_BOUNDS on a group: swz_group_write_output with the flag against swz_tiler_write_output with the flag of a
// single swz_tiler fed the same batches in this process, and swz_group_node_boxes against swz_tiler_node_boxes.  The data is a
// thin, tilted sheet in the unit box (6 000 points, two batches, 64 points per node): its upper-x upper-y quarter lies in the
// upper half only, so one level-0 octant is empty and its shard holds nothing but a part of the root.  The program prints
// "pair <single dir> <group dir>" per format; tests/test_cpp_group_tight_bounds.py compares every pair file by file, byte for
// byte.  Checked here: no two points share a Morton key (the order inside a file is then defined by the keys alone), the
// merged table is the single tiler's, the boxes are equal with ==, the root's box is the min / max over the parts of all
// shards, and the boxes differ from the octree cubes (the flag did something).
// All shards are on device 0: this has never run on more than one device.
// Usage: test_group_tight_bounds <work dir> <shards>.  Exit code 0 = pass.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <vector>

#include "../../include/swz_gpu.h"
#include "../../schwarzwald_amd/host/swz_tiling.hpp"

#define REQUIRE(cond, what)                                                 \
  do {                                                                      \
    if (!(cond)) {                                                          \
      std::fprintf(stderr, "FAIL (%s:%d): %s\n", __FILE__, __LINE__, what); \
      return false;                                                         \
    }                                                                       \
  } while (0)

struct Data {
  size_t n = 0;
  std::vector<double> xyz;
  std::vector<uint8_t> rgb;
  std::vector<uint16_t> intensity;
  swz_attribute_columns columns(size_t first) {
    swz_attribute_columns c{};
    c.column[SWZ_ATTR_RGB] = rgb.data() + 3 * first;
    c.column[SWZ_ATTR_INTENSITY] = intensity.data() + first;
    return c;
  }
};
static const uint32_t kMask = (1u << SWZ_ATTR_RGB) | (1u << SWZ_ATTR_INTENSITY);

static Data make_sheet(size_t n, uint64_t seed) {
  Data d;
  d.n = n;
  d.xyz.resize(3 * n);
  d.rgb.resize(3 * n);
  d.intensity.resize(n);
  std::mt19937_64 rng(seed);
  std::uniform_real_distribution<double> u(0.0, 1.0);
  for (size_t i = 0; i < n; ++i) {
    const double x = u(rng), y = u(rng);
    d.xyz[3 * i] = x, d.xyz[3 * i + 1] = y;
    d.xyz[3 * i + 2] = 0.25 + 0.45 * x + 0.2 * y + 0.004 * (u(rng) - 0.5);
    d.rgb[3 * i] = (uint8_t)i, d.rgb[3 * i + 1] = (uint8_t)(i >> 8), d.rgb[3 * i + 2] = (uint8_t)(i * 7);
    d.intensity[i] = (uint16_t)(i * 31 + 5);
  }
  return d;
}

static bool tile_single(swz_ctx* c, Data& d, int batches, const double mn[3], const double mx[3], const swz_tile_params& p, swz_tiler** out) {
  REQUIRE(swz_tiler_create(c, mn, mx, &p, 0, out) == SWZ_OK, swz_last_error(c));
  for (int b = 0; b < batches; ++b) {
    const size_t b0 = d.n * b / batches, b1 = d.n * (b + 1) / batches;
    std::vector<double> copy(d.xyz.begin() + 3 * b0, d.xyz.begin() + 3 * b1);  // (the call clamps in place)
    const swz_attribute_columns cols = d.columns(b0);
    REQUIRE(swz_tiler_add_batch(*out, copy.data(), b1 - b0, &cols, nullptr) == SWZ_OK, swz_last_error(c));
  }
  REQUIRE(swz_tiler_finalize(*out, nullptr) == SWZ_OK, swz_last_error(c));
  return true;
}

// one batch of the group: the rows lie on the shards in uneven pieces, the second piece empty (as tests/cpp/test_group_output.cpp)
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

static bool write_pair(const std::string& work, const std::string& leg, swz_tiler* single, swz_group* g, const swz_output_params& o) {
  const std::string a = work + "/single_" + leg, b = work + "/group_" + leg;
  swz_output_stats want{}, total{};
  REQUIRE(swz_tiler_write_output(single, a.c_str(), &o, &want) == SWZ_OK, "swz_tiler_write_output");
  if (swz_group_write_output(g, b.c_str(), &o, nullptr, &total) != SWZ_OK) {
    std::fprintf(stderr, "FAIL: swz_group_write_output (%s): %s\n", leg.c_str(), swz_group_last_error(g));
    return false;
  }
  REQUIRE(total.nodes == want.nodes && total.stored_points == want.stored_points && total.bytes_written == want.bytes_written,
          "total: nodes, stored points and bytes of the merged table");
  std::printf("pair %s %s\n", a.c_str(), b.c_str());
  return true;
}

static bool run(const std::string& work, int shards) {
  const double mn[3] = {0, 0, 0}, mx[3] = {1, 1, 1};
  swz_ctx* c = nullptr;
  REQUIRE(swz_create(&c, 0) == SWZ_OK, "swz_create");
  std::vector<int> devices(shards, 0);
  swz_group* g = nullptr;
  REQUIRE(swz_group_create(shards, devices.data(), 0, &g) == SWZ_OK, "swz_group_create");
  Data d = make_sheet(6000, 23);
  {
    std::vector<double> copy(d.xyz);
    std::vector<uint64_t> keys(d.n);
    REQUIRE(swz_morton_encode(c, copy.data(), d.n, mn, mx, keys.data()) == SWZ_OK, swz_last_error(c));
    std::sort(keys.begin(), keys.end());
    REQUIRE(std::adjacent_find(keys.begin(), keys.end()) == keys.end(), "two points share a Morton key: file order would not be defined by the keys");
  }
  swz_tile_params p{};
  p.sampler = SWZ_MIN_DISTANCE;
  p.max_points_per_node = 64;
  p.spacing_at_root = 0.1f;
  p.max_depth = 100;
  p.strategy = SWZ_ACCURATE;
  p.fast_concurrency = 8;
  swz_tiler* single = nullptr;
  if (!tile_single(c, d, 2, mn, mx, p, &single)) return false;
  REQUIRE(swz_group_tiler_open(g, mn, mx, &p, 0) == SWZ_OK, swz_group_last_error(g));
  for (int b = 0; b < 2; ++b)
    if (!group_batch(g, d, d.n * b / 2, d.n * (b + 1) / 2 - d.n * b / 2)) return false;
  REQUIRE(swz_group_finalize(g, nullptr) == SWZ_OK, swz_group_last_error(g));

  // ---- the tables are aligned: the merged table is the single tiler's, node by node
  swz_tiler_info info{};
  REQUIRE(swz_tiler_get_info(single, &info) == SWZ_OK, "swz_tiler_get_info");
  const uint64_t cap = info.num_nodes;
  std::vector<int8_t> l1(cap), l2(cap);
  std::vector<uint64_t> k1(cap), o1(cap), c1(cap), k2(cap), c2(cap);
  std::vector<int32_t> owner(cap);
  uint64_t n1 = 0, n2 = 0;
  REQUIRE(swz_tiler_node_table(single, cap, l1.data(), k1.data(), o1.data(), c1.data(), &n1) == SWZ_OK, "swz_tiler_node_table");
  REQUIRE(swz_group_node_table(g, cap, l2.data(), k2.data(), c2.data(), owner.data(), &n2) == SWZ_OK, swz_group_last_error(g));
  REQUIRE(n1 == n2 && l1 == l2 && k1 == k2 && c1 == c2, "swz_group_node_table differs from the single tiler's table");
  int max_level = -1, shards_with_nodes = 0;
  for (uint64_t k = 0; k < n1; ++k) max_level = std::max(max_level, (int)l1[k]);
  for (int s = 0; s < shards; ++s) shards_with_nodes += std::count(owner.begin(), owner.begin() + n2, s) > 0;
  REQUIRE(max_level >= 2 && n1 >= 50 && l1[0] == -1 && c1[0] > 0, "the tree has a root with points and at least three levels");
  if (shards == 8) REQUIRE(shards_with_nodes >= 4 && shards_with_nodes < 8, "the sheet leaves a shard with nothing but its part of the root");

  // ---- the boxes
  std::vector<double> lo1(3 * cap), hi1(3 * cap), lo2(3 * cap), hi2(3 * cap);
  uint64_t b1 = 0, b2 = 0;
  REQUIRE(swz_tiler_node_boxes(single, cap, lo1.data(), hi1.data(), &b1) == SWZ_OK, swz_last_error(c));
  REQUIRE(swz_group_node_boxes(g, cap, lo2.data(), hi2.data(), &b2) == SWZ_OK, swz_group_last_error(g));
  REQUIRE(b1 == n1 && b2 == n1, "one box per node of the table");
  uint64_t inside_cube = 0;
  for (uint64_t k = 0; k < n1; ++k) {
    double cmn[3], cmx[3];
    REQUIRE(swz_node_bounds(l1[k], k1[k], mn, mx, cmn, cmx) == SWZ_OK, "swz_node_bounds");
    for (int a = 0; a < 3; ++a) {
      if (lo1[3 * k + a] != lo2[3 * k + a] || hi1[3 * k + a] != hi2[3 * k + a]) {
        std::fprintf(stderr, "FAIL: node %llu (level %d) axis %d: single [%.17g, %.17g], group [%.17g, %.17g]\n", (unsigned long long)k, (int)l1[k], a,
                     lo1[3 * k + a], hi1[3 * k + a], lo2[3 * k + a], hi2[3 * k + a]);
        return false;
      }
      REQUIRE(lo1[3 * k + a] <= hi1[3 * k + a], "a node with points has a box");
    }
    inside_cube += (hi1[3 * k + 2] - lo1[3 * k + 2]) < 0.75 * (cmx[2] - cmn[2]);
  }
  REQUIRE(inside_cube * 2 > n1, "the boxes of a sheet are flatter than the cubes");
  // the root's box is the min / max over the parts the shards hold of it
  {
    double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    int parts = 0;
    for (int s = 0; s < shards; ++s) {
      swz_tiler* t = swz_group_tiler(g, s);
      swz_tiler_info si{};
      REQUIRE(swz_tiler_get_info(t, &si) == SWZ_OK, "swz_tiler_get_info(shard)");
      const uint64_t m = std::max<uint64_t>(si.num_nodes, 1);
      std::vector<int8_t> sl(m);
      std::vector<uint64_t> sk(m), so(m), sc(m);
      std::vector<double> slo(3 * m), shi(3 * m);
      uint64_t got = 0, gotb = 0;
      REQUIRE(swz_tiler_node_table(t, m, sl.data(), sk.data(), so.data(), sc.data(), &got) == SWZ_OK, "swz_tiler_node_table(shard)");
      REQUIRE(swz_tiler_node_boxes(t, m, slo.data(), shi.data(), &gotb) == SWZ_OK && gotb == got, "swz_tiler_node_boxes(shard)");
      for (uint64_t k = 0; k < got; ++k) {
        if (sl[k] >= 0 || sc[k] == 0) continue;
        ++parts;
        for (int a = 0; a < 3; ++a) lo[a] = std::min(lo[a], slo[3 * k + a]), hi[a] = std::max(hi[a], shi[3 * k + a]);
      }
    }
    REQUIRE(parts >= (shards > 1 ? 2 : 1), "the root lies on more than one shard");
    for (int a = 0; a < 3; ++a) REQUIRE(lo[a] == lo2[a] && hi[a] == hi2[a], "the root's box is the min / max of the shards' parts");
  }
  std::printf("boxes %llu\n", (unsigned long long)n1);

  // ---- the directories
  swz_ept_json ept{};
  for (int a = 0; a < 3; ++a) ept.bounds_min[a] = ept.conforming_min[a] = mn[a], ept.bounds_max[a] = ept.conforming_max[a] = mx[a];
  ept.points = d.n;
  ept.attribute_mask = kMask;
  ept.span = 128;
  ept.srs_authority = "EPSG", ept.srs_horizontal = "25832", ept.srs_wkt = "", ept.version = "1.0.0";
  swz_output_params o{};
  o.format = SWZ_OUT_3DTILES;
  o.attribute_mask = kMask;
  o.flags = SWZ_OUT_TIGHT_BOUNDS;
  o.chunk_points = 512;
  o.global_offset[0] = 1000.5, o.global_offset[1] = -20.25, o.global_offset[2] = 3.0;
  if (!write_pair(work, "3dtiles", single, g, o)) return false;
  o.format = SWZ_OUT_ENTWINE_LAS;
  o.ept = &ept;
  if (!write_pair(work, "ept", single, g, o)) return false;
  // the flag is refused for BIN once, before anything is created, and the group goes on
  o.format = SWZ_OUT_BIN;
  o.ept = nullptr;
  const std::string refused = work + "/refused";
  REQUIRE(swz_group_write_output(g, refused.c_str(), &o, nullptr, nullptr) == SWZ_ERR_BAD_ARG, "the flag with BIN is refused");
  REQUIRE(std::string(swz_group_last_error(g)).find("OUT_TIGHT_BOUNDS") != std::string::npos, "the refusal names the flag");
  o.format = SWZ_OUT_LAS;
  if (!write_pair(work, "las", single, g, o)) return false;
  std::printf("pairs 3\n");

  REQUIRE(swz_group_tiler_close(g) == SWZ_OK, swz_group_last_error(g));
  swz_tiler_destroy(single);
  swz_group_destroy(g);
  swz_destroy(c);
  return true;
}

int main(int argc, char** argv) {
  if (argc < 3) {
    std::fprintf(stderr, "usage: %s <work dir> <shards>\n", argv[0]);
    return 2;
  }
  return run(argv[1], std::atoi(argv[2])) ? 0 : 1;
}
