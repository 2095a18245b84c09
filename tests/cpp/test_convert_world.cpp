// Drives swz_host::convert_dataset_world (schwarzwald_amd/host/swz_tiling.hpp).  Usage: test_convert_world <dir>
//   Three batches in UTM 32N coordinates with attribute columns go through tile_batch; write_output writes <dir>/bin (BIN, with
//   write_properties); the adapter converts it into <dir>/world_adapter and the C call, with the same parameters, into
//   <dir>/world_c.  A target other than 3DTILES and a conversion onto the source itself must surface as the adapter's exception
//   with the library's text.
// tests/test_cpp_convert_world.py compares the two directories byte for byte.
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

struct NoSink : PointsSink {
  void persist_points(const uint32_t*, const uint32_t*, const double*, const AABB&, const std::string&) override {}
};

static std::string refusal_of(Context& ctx, const std::string& src, const std::string& dst, const swz_convert_params& cp,
                              const SourceProjection* projection) {
  try {
    (void)convert_dataset_world(ctx, src, dst, cp, projection);
  } catch (const std::runtime_error& e) {
    return e.what();
  }
  return "";
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  const std::string dir = argv[1];
  const double origin[3] = {500000.0, 5400000.0, 200.0}, side = 512.0;
  const AABB bounds{{origin[0], origin[1], origin[2]}, {origin[0] + side, origin[1] + side, origin[2] + side}};
  try {
    const size_t batch = 2000, batches = 3, n = batch * batches;
    std::vector<double> xyz(3 * n);
    std::vector<uint8_t> rgb(3 * n);
    std::vector<uint16_t> intensity(n);
    for (size_t i = 0; i < 3 * n; ++i) xyz[i] = origin[i % 3] + std::floor(next_unit() * side * 1000.0) / 1000.0;
    for (auto& v : rgb) v = (uint8_t)next_u64();
    for (auto& v : intensity) v = (uint16_t)next_u64();
    NoSink sink;
    TilerMetaParameters meta;
    meta.spacing_at_root = (float)(side * std::sqrt(3.0) / 16.0);
    meta.max_points_per_node = 200;
    TilingAlgorithmGPU tiler(make_sampling_strategy_from_name("GRID_CENTER", 200), sink, meta);
    for (size_t b = 0; b < batches; ++b) {
      swz_attribute_columns cols{};
      cols.column[SWZ_ATTR_RGB] = rgb.data() + 3 * b * batch;
      cols.column[SWZ_ATTR_INTENSITY] = intensity.data() + b * batch;
      tiler.tile_batch(xyz.data() + 3 * b * batch, cols, batch, bounds);
    }
    swz_output_params p{};
    p.attribute_mask = (1u << SWZ_ATTR_RGB) | (1u << SWZ_ATTR_INTENSITY);
    p.format = SWZ_OUT_BIN;
    const swz_output_stats bin = tiler.write_output(dir + "/bin", p);
    tiler.write_properties(dir + "/bin");

    Context ctx;
    const SourceProjection utm32{"+proj=utm +zone=32 +datum=WGS84"};
    swz_convert_params cp{};
    cp.out = p;
    cp.out.format = SWZ_OUT_3DTILES;
    cp.out.chunk_points = 1000;
    cp.out.flags = SWZ_OUT_TIGHT_BOUNDS;
    cp.max_depth = -1;
    const swz_convert_stats st = convert_dataset_world(ctx, dir + "/bin", dir + "/world_adapter", cp, &utm32);
    if (st.nodes != bin.nodes || st.points != bin.stored_points || st.chunks < 2) return 4;
    swz_convert_stats st_c{};
    const std::string src = dir + "/bin", dst = dir + "/world_c";
    if (swz_convert_dataset_world(ctx.get(), src.c_str(), dst.c_str(), &cp, utm32.srs(), &st_c) != SWZ_OK) {
      std::fprintf(stderr, "FAIL: the C call: %s\n", swz_last_error(ctx.get()));
      return 6;
    }
    if (st_c.nodes != st.nodes || st_c.points != st.points || st_c.chunks != st.chunks || st_c.bytes_written != st.bytes_written) return 7;

    swz_convert_params las = cp;
    las.out.format = SWZ_OUT_LAS;
    las.out.flags = 0;
    const std::string r1 = refusal_of(ctx, dir + "/bin", dir + "/refused", las, &utm32);
    const std::string r2 = refusal_of(ctx, dir + "/bin", dir + "/bin", cp, nullptr);
    if (r1.find("swz_convert_dataset_world: only 3DTILES") == std::string::npos ||
        r2.find("swz_convert_dataset_world: dst_dir is src_dir") == std::string::npos) {
      std::fprintf(stderr, "FAIL: the refusals read \"%s\" and \"%s\"\n", r1.c_str(), r2.c_str());
      return 5;
    }
    std::printf("refused: %s\nrefused: %s\n", r1.c_str(), r2.c_str());
    std::printf("convert world ok: %llu nodes, %llu points, %llu chunks\n", (unsigned long long)st.nodes, (unsigned long long)st.points,
                (unsigned long long)st.chunks);
    return 0;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "FAIL: %s\n", e.what());
    return 1;
  }
}
