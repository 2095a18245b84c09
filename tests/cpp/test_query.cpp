// Drives swz_host::query_dataset (schwarzwald_amd/host/swz_tiling.hpp).  Usage: test_query <dir>
//   Three batches with attribute columns go through tile_batch; write_output writes <dir>/bin (BIN, with write_properties);
//   query_dataset returns the octant [0, 0.5]^3 of it in small chunks, which goes to <dir>/xyz.f64, <dir>/intensity.u16,
//   <dir>/gps.f64 and <dir>/nodes.u32.  A query with box_min > box_max must surface as the adapter's exception with the
//   library's text.
// tests/test_cpp_query.py compares the dumped rows with numpy over every node file.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../schwarzwald_amd/host/swz_tiling.hpp"

using namespace swz_host;

static uint64_t g_state = 0x452821E638D01377ull;
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

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  const std::string dir = argv[1];
  const AABB bounds{{0, 0, 0}, {1, 1, 1}};
  try {
    const size_t batch = 3000, batches = 3, n = batch * batches;
    std::vector<double> xyz(3 * n), gps(n);
    std::vector<uint8_t> rgb(3 * n);
    std::vector<uint16_t> intensity(n);
    for (auto& v : xyz) v = next_unit();
    for (auto& v : rgb) v = (uint8_t)next_u64();
    for (auto& v : intensity) v = (uint16_t)next_u64();
    for (auto& v : gps) v = next_unit() * 1e9;
    NoSink sink;
    TilerMetaParameters meta;
    meta.spacing_at_root = (float)(std::sqrt(3.0) / 16.0);
    meta.max_points_per_node = 200;
    TilingAlgorithmGPU tiler(make_sampling_strategy_from_name("GRID_CENTER", 200), sink, meta);
    for (size_t b = 0; b < batches; ++b) {
      swz_attribute_columns cols{};
      cols.column[SWZ_ATTR_RGB] = rgb.data() + 3 * b * batch;
      cols.column[SWZ_ATTR_INTENSITY] = intensity.data() + b * batch;
      cols.column[SWZ_ATTR_GPS_TIME] = gps.data() + b * batch;
      tiler.tile_batch(xyz.data() + 3 * b * batch, cols, batch, bounds);
    }
    swz_output_params p{};
    p.attribute_mask = (1u << SWZ_ATTR_RGB) | (1u << SWZ_ATTR_INTENSITY) | (1u << SWZ_ATTR_GPS_TIME);
    p.format = SWZ_OUT_BIN;
    const swz_output_stats bin = tiler.write_output(dir + "/bin", p);
    tiler.write_properties(dir + "/bin");

    Context ctx;
    swz_query_params qp{};
    for (int a = 0; a < 3; ++a) qp.box_max[a] = 0.5;
    qp.max_depth = -1;
    qp.attribute_mask = (1u << SWZ_ATTR_INTENSITY) | (1u << SWZ_ATTR_GPS_TIME);
    qp.chunk_points = 1000;
    const QueryResult r = query_dataset(ctx, dir + "/bin", qp, false, true);
    if (r.count == 0 || r.count != r.stats.points_out || r.stats.chunks < 2 || r.stats.nodes_read > r.stats.nodes_scanned ||
        r.stats.points_read > bin.stored_points || !r.columns[SWZ_ATTR_RGB].empty() || r.nodes.size() != r.count)
      return 4;
    if (!dump(dir + "/xyz.f64", r.positions.data(), r.positions.size() * 8) ||
        !dump(dir + "/intensity.u16", r.columns[SWZ_ATTR_INTENSITY].data(), r.columns[SWZ_ATTR_INTENSITY].size()) ||
        !dump(dir + "/gps.f64", r.columns[SWZ_ATTR_GPS_TIME].data(), r.columns[SWZ_ATTR_GPS_TIME].size()) ||
        !dump(dir + "/nodes.u32", r.nodes.data(), r.nodes.size() * 4))
      return 6;

    std::string refusal;
    try {
      qp.box_min[1] = 0.75;
      (void)query_dataset(ctx, dir + "/bin", qp);
    } catch (const std::runtime_error& e) {
      refusal = e.what();
    }
    if (refusal.find("swz_dataset_query_nodes: box_min > box_max") == std::string::npos) {
      std::fprintf(stderr, "FAIL: the refusal reads \"%s\"\n", refusal.c_str());
      return 5;
    }
    std::printf("refused: %s\n", refusal.c_str());
    std::printf("query ok: %llu points of %llu read, %llu of %llu nodes, %llu chunks\n", (unsigned long long)r.count,
                (unsigned long long)r.stats.points_read, (unsigned long long)r.stats.nodes_read,
                (unsigned long long)r.stats.nodes_scanned, (unsigned long long)r.stats.chunks);
    return 0;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "FAIL: %s\n", e.what());
    return 1;
  }
}
