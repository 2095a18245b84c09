// Drives swz_host::summarize_dataset and swz_host::query_dataset_filtered_nodes (schwarzwald_amd/host/swz_tiling.hpp).
// Usage: test_query_summaries <dir>
//   Three batches whose intensity grows with x and whose classification is 2 below z = 0.35 go through tile_batch; write_output
//   writes <dir>/bin (BIN, with write_properties).  The points of one intensity band that are ground are queried, the data
//   set is summarised, and the query runs again: the same rows, fewer nodes read -- those query_dataset_filtered_nodes flags.
//   The rows of the second query go to <dir>/s_xyz.f64, s_intensity.u16 and s_nodes.u32.
// tests/test_cpp_query_summaries.py compares the dumped rows with numpy over every node file.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../schwarzwald_amd/host/swz_tiling.hpp"

using namespace swz_host;

static uint64_t g_state = 0x243F6A8885A308D3ull;
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
    std::vector<double> xyz(3 * n);
    std::vector<uint16_t> intensity(n);
    std::vector<uint8_t> classification(n);
    for (auto& v : xyz) v = next_unit();
    for (size_t i = 0; i < n; ++i) {
      intensity[i] = (uint16_t)std::floor(xyz[3 * i] * 50000.0);
      classification[i] = xyz[3 * i + 2] < 0.35 ? 2 : (uint8_t)(3 + next_u64() % 4);
    }
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
    qp.attribute_mask = 1u << SWZ_ATTR_INTENSITY;
    qp.chunk_points = 1000;
    Filter filter;
    filter.range(SWZ_ATTR_INTENSITY, 10000.0, 14999.0).any_of(SWZ_ATTR_CLASSIFICATION, {2});

    const FilteredNodes all = query_dataset_filtered_nodes(ctx, dir + "/bin", qp, nullptr, filter.get());
    const QueryResult before = query_dataset_filtered(ctx, dir + "/bin", qp, nullptr, filter.get(), false, true);
    const swz_summarize_stats st = summarize_dataset(ctx, dir + "/bin", false, 1000);
    const FilteredNodes some = query_dataset_filtered_nodes(ctx, dir + "/bin", qp, nullptr, filter.get());
    const QueryResult after = query_dataset_filtered(ctx, dir + "/bin", qp, nullptr, filter.get(), false, true);

    uint64_t all_read = 0, some_read = 0;
    for (uint8_t r : all.read) all_read += r;
    for (uint8_t r : some.read) some_read += r;
    if (all_read != all.read.size() || all.key != some.key || all.count != some.count || some_read == 0 || some_read >= all_read ||
        some.points_bound >= all.points_bound)
      return 4;
    if (st.nodes != all.read.size() || st.points != n || st.chunks < 2) return 4;
    if (before.count == 0 || before.count != after.count || before.positions != after.positions || before.nodes != after.nodes ||
        before.columns[SWZ_ATTR_INTENSITY] != after.columns[SWZ_ATTR_INTENSITY])
      return 5;
    if (before.stats.nodes_read != all_read || after.stats.nodes_read != some_read || after.stats.points_read != some.points_bound ||
        after.stats.bytes_read >= before.stats.bytes_read)
      return 5;
    if (!dump(dir + "/s_xyz.f64", after.positions.data(), after.positions.size() * 8) ||
        !dump(dir + "/s_intensity.u16", after.columns[SWZ_ATTR_INTENSITY].data(), after.columns[SWZ_ATTR_INTENSITY].size()) ||
        !dump(dir + "/s_nodes.u32", after.nodes.data(), after.nodes.size() * 4))
      return 6;
    std::printf("summaries ok: %llu points, %llu of %llu nodes read\n", (unsigned long long)after.count, (unsigned long long)some_read,
                (unsigned long long)all_read);
    return 0;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "FAIL: %s\n", e.what());
    return 1;
  }
}
