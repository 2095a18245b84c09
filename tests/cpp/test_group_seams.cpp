// One cloud, one parameter set, one shard count through swz_group_tile (include/swz_gpu.h): the driver of
// tests/test_shard_seams.py.  It reads the cloud from a file, cuts it into uneven pieces in input order (the second piece
// empty when there are more than two shards), lets the library exchange and tile, checks what can be checked row by row
// (keys ascend, every row on the shard that owns its octant, the GPS-time column -- the input index -- travelled with its
// point) and writes one record per received row.  It holds no oracle: the comparison is numpy's.
// Usage: test_group_seams CLOUD N OUT MINX MINY MINZ MAXX MAXY MAXZ SPACING_BITS MAX_POINTS SAMPLER STRATEGY FAST_CONCURRENCY
//                         FLAGS SHARDS [NAME=VALUE ...]
//   CLOUD: N x 3 little-endian doubles.  Bounds: anything strtod reads (hex floats are exact).  SPACING_BITS: the bit
//   pattern of the float spacing_at_root.  NAME=VALUE: swz_set_option on every shard's context.
//   OUT: per row { u64 key; u32 input index; u32 dup mask; i32 level; u32 shard }.
// stdout: "joint_root_possible 0|1", then per shard "shard S points M stamps <exchange done> <root begun> <root done>
// <levels done>" (swz_group_shard_timing, ms), then "done".  Exit code 0 = the run and the row checks passed; 3 = swz_group_tile
// failed (its code and message on stderr).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/swz_gpu.h"

static int fail(const char* msg, const char* detail = "") {
  std::fprintf(stderr, "FAIL: %s %s\n", msg, detail);
  return 1;
}

struct Record {
  uint64_t key;
  uint32_t index;
  uint32_t dup;
  int32_t level;
  uint32_t shard;
};
static_assert(sizeof(Record) == 24, "the record layout tests/test_shard_seams.py reads");

int main(int argc, char** argv) {
  if (argc < 17) return fail("usage: test_group_seams CLOUD N OUT 6 x BOUNDS SPACING_BITS MAX_POINTS SAMPLER STRATEGY FAST_CONCURRENCY FLAGS SHARDS [NAME=VALUE ...]");
  const char* cloud = argv[1];
  const size_t n = (size_t)std::strtoull(argv[2], nullptr, 10);
  const char* out_path = argv[3];
  double mn[3], mx[3];
  for (int d = 0; d < 3; ++d) mn[d] = std::strtod(argv[4 + d], nullptr), mx[d] = std::strtod(argv[7 + d], nullptr);
  const uint32_t spacing_bits = (uint32_t)std::strtoul(argv[10], nullptr, 0);
  float spacing;
  std::memcpy(&spacing, &spacing_bits, 4);
  swz_tile_params p{};
  p.spacing_at_root = spacing;
  p.max_points_per_node = std::strtoull(argv[11], nullptr, 10);
  p.sampler = std::atoi(argv[12]);
  p.strategy = std::atoi(argv[13]);
  p.fast_concurrency = (uint32_t)std::atoi(argv[14]);
  p.flags = (uint32_t)std::strtoul(argv[15], nullptr, 0);
  p.max_depth = 100;
  const int shards = std::atoi(argv[16]);
  if (n == 0 || n > 0xFFFF0000ull || (shards != 1 && shards != 2 && shards != 4 && shards != 8)) return fail("bad point or shard count");

  std::vector<double> xyz(n * 3);
  {
    std::FILE* f = std::fopen(cloud, "rb");
    if (!f) return fail("cannot open the cloud", cloud);
    const size_t got = std::fread(xyz.data(), 24, n, f);
    std::fclose(f);
    if (got != n) return fail("the cloud is shorter than N points", cloud);
  }
  std::vector<double> gps(n);
  for (size_t i = 0; i < n; ++i) gps[i] = (double)i;

  std::vector<int> devices(shards, 0);
  swz_group* g = nullptr;
  if (swz_group_create(shards, devices.data(), 0, &g) != SWZ_OK) return fail("swz_group_create", swz_group_last_error(nullptr));
  for (int a = 17; a < argc; ++a) {
    const char* eq = std::strchr(argv[a], '=');
    if (!eq) return fail("an option must read NAME=VALUE:", argv[a]);
    const std::string name(argv[a], (size_t)(eq - argv[a]));
    for (int s = 0; s < shards; ++s)
      if (swz_set_option(swz_group_ctx(g, s), name.c_str(), eq + 1) != SWZ_OK) return fail("swz_set_option", argv[a]);
  }
  std::printf("joint_root_possible %d\n", swz_shard_joint_root_possible(swz_group_ctx(g, 0), &p, mn, mx));

  // uneven pieces in input order; the second piece is empty
  std::vector<size_t> cut(shards + 1, 0);
  for (int s = 1; s <= shards; ++s) cut[s] = (s == 2 && shards > 2) ? cut[1] : std::min(n, (size_t)((double)n * s * s / ((double)shards * shards)));
  cut[shards] = n;
  std::vector<double*> d_xyz(shards, nullptr);
  std::vector<swz_attribute_columns> d_attrs(shards);
  std::vector<uint64_t> cnt(shards, 0);
  for (int s = 0; s < shards; ++s) {
    cnt[s] = cut[s + 1] - cut[s];
    d_attrs[s] = swz_attribute_columns{};
    const uint64_t rows = std::max<uint64_t>(cnt[s], 1);
    swz_ctx* c = swz_group_ctx(g, s);
    if (swz_device_alloc_on(c, rows * 24, (void**)&d_xyz[s]) != SWZ_OK || swz_device_alloc_on(c, rows * 8, &d_attrs[s].column[SWZ_ATTR_GPS_TIME]) != SWZ_OK)
      return fail("device alloc");
    if (!cnt[s]) continue;
    if (swz_copy_to_device(c, d_xyz[s], xyz.data() + 3 * cut[s], cnt[s] * 24) != SWZ_OK ||
        swz_copy_to_device(c, d_attrs[s].column[SWZ_ATTR_GPS_TIME], gps.data() + cut[s], cnt[s] * 8) != SWZ_OK)
      return fail("upload");
  }

  std::vector<swz_group_result> res(shards);
  const int rc = swz_group_tile(g, d_xyz.data(), d_attrs.data(), cnt.data(), mn, mx, &p, res.data());
  if (rc != SWZ_OK) {
    std::fprintf(stderr, "swz_group_tile failed: code %d: %s\n", rc, swz_group_last_error(g));
    return 3;
  }

  std::vector<Record> records;
  records.reserve(n);
  for (int s = 0; s < shards; ++s) {
    const uint64_t m = res[s].num_points;
    double t[4] = {0, 0, 0, 0};
    if (swz_group_shard_timing(g, s, t) != SWZ_OK) return fail("swz_group_shard_timing");
    std::printf("shard %d points %llu stamps %.6f %.6f %.6f %.6f\n", s, (unsigned long long)m, t[0], t[1], t[2], t[3]);
    if (!m) continue;
    std::vector<double> px(m * 3), got_gps(m);
    std::vector<uint64_t> k(m);
    std::vector<uint32_t> perm(m), dup(m, 0u);
    std::vector<int8_t> lv(m);
    swz_ctx* c = swz_group_ctx(g, s);
    if (!res[s].attrs.column[SWZ_ATTR_GPS_TIME]) return fail("the GPS-time column is missing in the result");
    if (swz_copy_to_host(c, got_gps.data(), res[s].attrs.column[SWZ_ATTR_GPS_TIME], m * 8) || swz_copy_to_host(c, px.data(), res[s].d_xyz, m * 24) ||
        swz_copy_to_host(c, k.data(), res[s].d_keys, m * 8) || swz_copy_to_host(c, perm.data(), res[s].d_perm, m * 4) ||
        swz_copy_to_host(c, lv.data(), res[s].d_level, m))
      return fail("download");
    if ((p.strategy == SWZ_FAST) != (res[s].d_dup != nullptr)) return fail("d_dup must be set for FAST and only then");
    if (res[s].d_dup && swz_copy_to_host(c, dup.data(), res[s].d_dup, m * 4)) return fail("download of the dup mask");
    for (uint64_t i = 0; i < m; ++i) {
      if (i && k[i] < k[i - 1]) return fail("keys of a shard do not ascend");
      if ((int)(k[i] >> 60) * shards / 8 != s) return fail("point on a shard that does not own its octant");
      const uint32_t q = perm[i];
      if (q >= m) return fail("perm out of range");
      const double src_d = got_gps[q];
      if (!(src_d >= 0.0) || src_d >= (double)n) return fail("GPS time column holds no input index");
      const size_t src = (size_t)src_d;
      if (xyz[3 * src] != px[3 * q] || xyz[3 * src + 1] != px[3 * q + 1] || xyz[3 * src + 2] != px[3 * q + 2])
        return fail("GPS time column did not travel with its point");
      records.push_back(Record{k[i], (uint32_t)src, dup[i], (int32_t)lv[i], (uint32_t)s});
    }
  }
  {
    std::FILE* f = std::fopen(out_path, "wb");
    if (!f) return fail("cannot write", out_path);
    const size_t put = records.empty() ? 0 : std::fwrite(records.data(), sizeof(Record), records.size(), f);
    if (std::fclose(f) != 0 || put != records.size()) return fail("short write", out_path);
  }
  for (int s = 0; s < shards; ++s) {
    swz_device_free(d_xyz[s]);
    swz_device_free(d_attrs[s].column[SWZ_ATTR_GPS_TIME]);
  }
  swz_group_destroy(g);
  std::printf("done\n");
  return 0;
}
