// Drives swz_host::query_dataset_filtered and swz_host::Filter (schwarzwald_amd/host/swz_tiling.hpp).
// Usage: test_query_filter <dir>
//   Three batches with intensity and classification go through tile_batch; write_output writes <dir>/bin (BIN, with
//   write_properties).  query_dataset_filtered returns, in small chunks, the points of an L-shaped outline along two faces of
//   the root whose classification is 2 or 9 and whose intensity lies in [1000, 40000.5] -- only the intensity is asked back.
//   The rows go to <dir>/f_xyz.f64, f_intensity.u16 and f_nodes.u32.  A filter the library refuses must surface as the
//   adapter's exception with the library's text.
// tests/test_cpp_query_filter.py compares the dumped rows with numpy over every node file.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../schwarzwald_amd/host/swz_tiling.hpp"

using namespace swz_host;

static uint64_t g_state = 0x13198A2E03707344ull;
static uint64_t next_u64() {  // splitmix64
  uint64_t z = (g_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
static double next_unit() { return (double)(next_u64() >> 11) * (1.0 / 9007199254740992.0); }

static bool dump(const std::string& path, const void* data, size_t bytes) {
  FILE* f = std::fopen(path.c_str(), "wb");
  if (!f) return false;
  const bool ok = std::fwrite(data, 1, bytes, f) == bytes;
  return std::fclose(f) == 0 && ok;
}

struct NoSink : PointsSink {
  void persist_points(const uint32_t*, const uint32_t*, const double*, const AABB&, const std::string&) override {}
};

static const double OUTLINE[12] = {0.0, 0.0, 1.0, 0.0, 1.0, 0.25, 0.25, 0.25, 0.25, 1.0, 0.0, 1.0};

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  const std::string dir = argv[1];
  const AABB bounds{{0, 0, 0}, {1, 1, 1}};
  try {
    const size_t batch = 3000, batches = 3, n = batch * batches;
    std::vector<double> xyz(3 * n);
    std::vector<uint16_t> intensity(n);
    std::vector<uint8_t> classification(n);
    for (auto& v : xyz) v = next_unit();
    for (auto& v : intensity) v = (uint16_t)next_u64();
    for (auto& v : classification) v = (uint8_t)(next_u64() % 12);
    NoSink sink;
    TilerMetaParameters meta;
    meta.spacing_at_root = (float)(std::sqrt(3.0) / 16.0);
    meta.max_points_per_node = 200;
    TilingAlgorithmGPU tiler(make_sampling_strategy_from_name("GRID_CENTER", 200), sink, meta);
    for (size_t b = 0; b < batches; ++b) {
      swz_attribute_columns cols{};
      cols.column[SWZ_ATTR_INTENSITY] = intensity.data() + b * batch;
      cols.column[SWZ_ATTR_CLASSIFICATION] = classification.data() + b * batch;
      tiler.tile_batch(xyz.data() + 3 * b * batch, cols, batch, bounds);
    }
    swz_output_params p{};
    p.attribute_mask = (1u << SWZ_ATTR_INTENSITY) | (1u << SWZ_ATTR_CLASSIFICATION);
    p.format = SWZ_OUT_BIN;
    (void)tiler.write_output(dir + "/bin", p);
    tiler.write_properties(dir + "/bin");

    Context ctx;
    swz_query_params qp{};
    for (int a = 0; a < 3; ++a) qp.box_max[a] = 1.0;
    qp.max_depth = -1;
    qp.attribute_mask = 1u << SWZ_ATTR_INTENSITY;  // the classification is read for the filter only
    qp.chunk_points = 1000;

    swz_region outline{};
    outline.kind = SWZ_REGION_POLYGON;
    outline.count = 6;
    outline.values = OUTLINE;
    Filter filter;
    filter.any_of(SWZ_ATTR_CLASSIFICATION, {2, 9}).range(SWZ_ATTR_INTENSITY, 1000.0, 40000.5);
    const QueryResult region = query_dataset_region(ctx, dir + "/bin", qp, &outline, false, true);
    const QueryResult f = query_dataset_filtered(ctx, dir + "/bin", qp, &outline, filter.get(), false, true);
    if (f.count == 0 || f.count != f.stats.points_out || f.stats.chunks < 2 || f.stats.nodes_read != region.stats.nodes_read ||
        f.stats.points_read != region.stats.points_read || f.count >= region.count || f.nodes.size() != f.count ||
        !f.columns[SWZ_ATTR_CLASSIFICATION].empty() || f.columns[SWZ_ATTR_INTENSITY].size() != 2 * f.count)
      return 4;
    // without a filter: the region query
    const QueryResult same = query_dataset_filtered(ctx, dir + "/bin", qp, &outline, nullptr, false, true);
    if (same.count != region.count || same.positions != region.positions || same.nodes != region.nodes) return 4;
    if (!dump(dir + "/outline.f64", OUTLINE, sizeof OUTLINE) || !dump(dir + "/f_xyz.f64", f.positions.data(), f.positions.size() * 8) ||
        !dump(dir + "/f_intensity.u16", f.columns[SWZ_ATTR_INTENSITY].data(), f.columns[SWZ_ATTR_INTENSITY].size()) ||
        !dump(dir + "/f_nodes.u32", f.nodes.data(), f.nodes.size() * 4))
      return 6;

    std::string refusal, missing;
    try {
      Filter bad;
      bad.range(SWZ_ATTR_INTENSITY, 0.0, 1.0).any_of(SWZ_ATTR_INTENSITY, {1});
      (void)query_dataset_filtered(ctx, dir + "/bin", qp, &outline, bad.get());
    } catch (const std::runtime_error& e) {
      refusal = e.what();
    }
    if (refusal.find("clause 1: a SET on SWZ_ATTR_INTENSITY") == std::string::npos) {
      std::fprintf(stderr, "FAIL: the refusal reads \"%s\"\n", refusal.c_str());
      return 5;
    }
    try {
      Filter absent;
      absent.range(SWZ_ATTR_GPS_TIME, 0.0, 1.0);
      (void)query_dataset_filtered(ctx, dir + "/bin", qp, &outline, absent.get());
    } catch (const std::runtime_error& e) {
      missing = e.what();
    }
    if (missing.find("swz_dataset_query_filtered: the filter names SWZ_ATTR_GPS_TIME") == std::string::npos) {
      std::fprintf(stderr, "FAIL: the refusal reads \"%s\"\n", missing.c_str());
      return 5;
    }
    std::printf("refused: %s\n", refusal.c_str());
    std::printf("refused: %s\n", missing.c_str());
    std::printf("filtered query ok: %llu of the region's %llu points, %llu nodes read\n", (unsigned long long)f.count,
                (unsigned long long)region.count, (unsigned long long)f.stats.nodes_read);
    return 0;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "FAIL: %s\n", e.what());
    return 1;
  }
}
