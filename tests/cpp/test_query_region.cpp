// Drives swz_host::query_dataset_region and swz_host::frustum_planes (schwarzwald_amd/host/swz_tiling.hpp).
// Usage: test_query_region <dir>
//   Three batches with attribute columns go through tile_batch; write_output writes <dir>/bin (BIN, with write_properties).
//   query_dataset_region returns, in small chunks, (1) the points of an L-shaped outline along two faces of the root and
//   (2) the points of the frustum of a fixed camera, whose matrix goes to <dir>/matrix.f64 and whose planes, as
//   frustum_planes returns them, to <dir>/planes.f64.  The rows go to <dir>/<name>_xyz.f64, _intensity.u16 and _nodes.u32.
//   A region without vertices must surface as the adapter's exception with the library's text.
// tests/test_cpp_query_region.py compares the dumped rows with numpy over every node file.
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

static bool dump_result(const std::string& stem, const QueryResult& r) {
  return dump(stem + "_xyz.f64", r.positions.data(), r.positions.size() * 8) &&
         dump(stem + "_intensity.u16", r.columns[SWZ_ATTR_INTENSITY].data(), r.columns[SWZ_ATTR_INTENSITY].size()) &&
         dump(stem + "_nodes.u32", r.nodes.data(), r.nodes.size() * 4);
}

struct NoSink : PointsSink {
  void persist_points(const uint32_t*, const uint32_t*, const double*, const AABB&, const std::string&) override {}
};

// a camera above one corner of the unit cube looking into it (row-major, clip = m (x, y, z, 1))
static const double MATRIX[16] = {1.3918452239017374, -1.7011441625465678, 0.0,                 0.15464946932241516,
                                  1.1376283962480003, 0.9307868696574547,  2.321221576182789,   -1.7305741058075645,
                                  0.698977447285233,  0.5718906386879179,  -0.5718906386879178, 1.1275149385476704,
                                  0.6538821281055405, 0.5349944684499877,  -0.5349944684499875, 1.2483204263833043};
static const double OUTLINE[12] = {0.0, 0.0, 1.0, 0.0, 1.0, 0.25, 0.25, 0.25, 0.25, 1.0, 0.0, 1.0};

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  const std::string dir = argv[1];
  const AABB bounds{{0, 0, 0}, {1, 1, 1}};
  try {
    const size_t batch = 3000, batches = 3, n = batch * batches;
    std::vector<double> xyz(3 * n);
    std::vector<uint16_t> intensity(n);
    for (auto& v : xyz) v = next_unit();
    for (auto& v : intensity) v = (uint16_t)next_u64();
    NoSink sink;
    TilerMetaParameters meta;
    meta.spacing_at_root = (float)(std::sqrt(3.0) / 16.0);
    meta.max_points_per_node = 200;
    TilingAlgorithmGPU tiler(make_sampling_strategy_from_name("GRID_CENTER", 200), sink, meta);
    for (size_t b = 0; b < batches; ++b) {
      swz_attribute_columns cols{};
      cols.column[SWZ_ATTR_INTENSITY] = intensity.data() + b * batch;
      tiler.tile_batch(xyz.data() + 3 * b * batch, cols, batch, bounds);
    }
    swz_output_params p{};
    p.attribute_mask = 1u << SWZ_ATTR_INTENSITY;
    p.format = SWZ_OUT_BIN;
    (void)tiler.write_output(dir + "/bin", p);
    tiler.write_properties(dir + "/bin");

    Context ctx;
    swz_query_params qp{};
    for (int a = 0; a < 3; ++a) qp.box_max[a] = 1.0;
    qp.max_depth = -1;
    qp.attribute_mask = 1u << SWZ_ATTR_INTENSITY;
    qp.chunk_points = 1000;

    swz_region outline{};
    outline.kind = SWZ_REGION_POLYGON;
    outline.count = 6;
    outline.values = OUTLINE;
    const QueryResult whole = query_dataset(ctx, dir + "/bin", qp);
    const QueryResult l = query_dataset_region(ctx, dir + "/bin", qp, &outline, false, true);
    if (l.count == 0 || l.count != l.stats.points_out || l.stats.chunks < 2 || l.stats.nodes_read >= whole.stats.nodes_read ||
        l.count >= whole.count || l.nodes.size() != l.count)
      return 4;

    const std::array<double, 24> planes = frustum_planes(MATRIX);
    swz_region frustum{};
    frustum.kind = SWZ_REGION_PLANES;
    frustum.count = 6;
    frustum.values = planes.data();
    const QueryResult f = query_dataset_region(ctx, dir + "/bin", qp, &frustum, false, true);
    if (f.count == 0 || f.count >= whole.count || f.count != f.stats.points_out || f.nodes.size() != f.count) return 4;
    if (!dump(dir + "/matrix.f64", MATRIX, sizeof MATRIX) || !dump(dir + "/planes.f64", planes.data(), sizeof(double) * 24) ||
        !dump(dir + "/outline.f64", OUTLINE, sizeof OUTLINE) || !dump_result(dir + "/l", l) || !dump_result(dir + "/frustum", f))
      return 6;

    std::string refusal;
    try {
      outline.count = 2;
      (void)query_dataset_region(ctx, dir + "/bin", qp, &outline);
    } catch (const std::runtime_error& e) {
      refusal = e.what();
    }
    if (refusal.find("swz_dataset_query_region_nodes: a polygon region holds 3 to 1024 vertices") == std::string::npos) {
      std::fprintf(stderr, "FAIL: the refusal reads \"%s\"\n", refusal.c_str());
      return 5;
    }
    std::printf("refused: %s\n", refusal.c_str());
    std::printf("region query ok: outline %llu points of %llu nodes, frustum %llu points of %llu nodes, box %llu points of %llu nodes\n",
                (unsigned long long)l.count, (unsigned long long)l.stats.nodes_read, (unsigned long long)f.count,
                (unsigned long long)f.stats.nodes_read, (unsigned long long)whole.count, (unsigned long long)whole.stats.nodes_read);
    return 0;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "FAIL: %s\n", e.what());
    return 1;
  }
}
