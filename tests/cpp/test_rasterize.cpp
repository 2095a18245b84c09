// Drives swz_host::rasterize_dataset (schwarzwald_amd/host/swz_tiling.hpp).
// Usage: test_rasterize <dir>
//   Three batches with intensity and classification go through tile_batch; write_output writes <dir>/bin (BIN, with
//   write_properties).  rasterize_dataset rasters, in small chunks, a 9 x 5 grid over a sub-box: z of the box alone, z of an
//   L-shaped outline whose classification is 2 or 9, and the intensity of the same selection.  Every table must be the bytes
//   of a direct call of swz_dataset_rasterize, and its decode swz_raster_finish's.  The cells go to <dir>/z_box.cells,
//   z_sel.cells and i_sel.cells, the means to *.mean.  A grid the library refuses must surface as the adapter's exception with
//   the library's text.
// tests/test_cpp_rasterize.py compares the dumped tables with numpy over every node file.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <utility>
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

static const double OUTLINE[12] = {0.0, 0.0, 1.0, 0.0, 1.0, 0.25, 0.25, 0.25, 0.25, 1.0, 0.0, 1.0};

// the adapter's result against the C call it wraps
static bool same_as_c(Context& ctx, const std::string& dir, const swz_query_params& qp, const swz_region* region, const swz_filter* filter,
                      const swz_raster_grid& grid, const RasterResult& r) {
  const size_t n = (size_t)grid.nx * grid.ny;
  std::vector<swz_raster_cell> cells(n);
  swz_raster_frame frame{};
  swz_query_stats stats{};
  if (swz_dataset_rasterize(ctx.get(), dir.c_str(), &qp, region, filter, &grid, cells.data(), &frame, &stats) != SWZ_OK) return false;
  if (r.cells.size() != n || std::memcmp(cells.data(), r.cells.data(), n * sizeof(swz_raster_cell)) != 0) return false;
  if (std::memcmp(&frame, &r.frame, sizeof frame) != 0 || stats.points_out != r.stats.points_out || stats.nodes_read != r.stats.nodes_read) return false;
  std::vector<uint64_t> count(n);
  std::vector<double> lo(n), hi(n), mean(n);
  if (swz_raster_finish(&frame, cells.data(), count.data(), lo.data(), hi.data(), mean.data()) != SWZ_OK) return false;
  uint64_t total = 0;
  for (size_t i = 0; i < n; ++i) total += count[i];
  return count == r.count && std::memcmp(lo.data(), r.min.data(), 8 * n) == 0 && std::memcmp(hi.data(), r.max.data(), 8 * n) == 0 &&
         std::memcmp(mean.data(), r.mean.data(), 8 * n) == 0 && total == r.stats.points_out;
}

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
    const double lo[3] = {0.0, 0.0, 0.125}, hi[3] = {0.875, 1.0, 0.75};
    for (int a = 0; a < 3; ++a) {
      qp.box_min[a] = lo[a];
      qp.box_max[a] = hi[a];
    }
    qp.max_depth = -1;
    qp.chunk_points = 1000;
    swz_raster_grid grid{};
    grid.nx = 9;
    grid.ny = 5;
    grid.value = SWZ_RASTER_VALUE_Z;
    swz_region outline{};
    outline.kind = SWZ_REGION_POLYGON;
    outline.count = 6;
    outline.values = OUTLINE;
    Filter filter;
    filter.any_of(SWZ_ATTR_CLASSIFICATION, {2, 9});

    const RasterResult z_box = rasterize_dataset(ctx, dir + "/bin", qp, nullptr, nullptr, grid);
    const RasterResult z_sel = rasterize_dataset(ctx, dir + "/bin", qp, &outline, filter.get(), grid);
    swz_raster_grid by_intensity = grid;
    by_intensity.value = SWZ_ATTR_INTENSITY;
    const RasterResult i_sel = rasterize_dataset(ctx, dir + "/bin", qp, &outline, filter.get(), by_intensity);
    if (z_box.stats.points_out == 0 || z_box.stats.chunks < 2 || z_sel.stats.points_out == 0 || z_sel.stats.points_out >= z_box.stats.points_out ||
        i_sel.stats.points_out != z_sel.stats.points_out || z_box.cells.size() != 45 || i_sel.frame.scale != 1.0)
      return 4;
    if (!same_as_c(ctx, dir + "/bin", qp, nullptr, nullptr, grid, z_box) || !same_as_c(ctx, dir + "/bin", qp, &outline, filter.get(), grid, z_sel) ||
        !same_as_c(ctx, dir + "/bin", qp, &outline, filter.get(), by_intensity, i_sel))
      return 4;
    const std::pair<const char*, const RasterResult*> named[3] = {{"z_box", &z_box}, {"z_sel", &z_sel}, {"i_sel", &i_sel}};
    if (!dump(dir + "/outline.f64", OUTLINE, sizeof OUTLINE) || !dump(dir + "/box.f64", qp.box_min, 48)) return 6;
    for (const auto& nr : named)
      if (!dump(dir + "/" + nr.first + ".cells", nr.second->cells.data(), nr.second->cells.size() * sizeof(swz_raster_cell)) ||
          !dump(dir + "/" + nr.first + ".mean", nr.second->mean.data(), nr.second->mean.size() * 8))
        return 6;

    std::string refusal, missing;
    try {
      swz_raster_grid bad = grid;
      bad.value = SWZ_ATTR_GPS_TIME;
      (void)rasterize_dataset(ctx, dir + "/bin", qp, nullptr, nullptr, bad);
    } catch (const std::runtime_error& e) {
      refusal = e.what();
    }
    if (refusal.find("swz_raster_frame_of: SWZ_ATTR_GPS_TIME is not a value the raster takes") == std::string::npos) {
      std::fprintf(stderr, "FAIL: the refusal reads \"%s\"\n", refusal.c_str());
      return 5;
    }
    try {
      swz_raster_grid absent = grid;
      absent.value = SWZ_ATTR_USER_DATA;
      (void)rasterize_dataset(ctx, dir + "/bin", qp, nullptr, nullptr, absent);
    } catch (const std::runtime_error& e) {
      missing = e.what();
    }
    if (missing.find("swz_dataset_rasterize: the value is SWZ_ATTR_USER_DATA, which the source does not hold") == std::string::npos) {
      std::fprintf(stderr, "FAIL: the refusal reads \"%s\"\n", missing.c_str());
      return 5;
    }
    std::printf("refused: %s\n", refusal.c_str());
    std::printf("refused: %s\n", missing.c_str());
    std::printf("raster ok: %llu rows of the box, %llu of the selection, %llu nodes read\n", (unsigned long long)z_box.stats.points_out,
                (unsigned long long)z_sel.stats.points_out, (unsigned long long)z_box.stats.nodes_read);
    return 0;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "FAIL: %s\n", e.what());
    return 1;
  }
}
