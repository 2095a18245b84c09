// Drives LASSink and EntwineSink (schwarzwald_amd/host/swz_tiling.hpp).  Usage: test_las_sink <dir> [--gpu]
//   without --gpu (no device needed): a few hand-made nodes go through persist_rows of a LASSink (<dir>/las), of an
//     EntwineSink with an explicit finish() (<dir>/ept) and through persist_points of an EntwineSink whose hierarchy is left
//     to the destructor (<dir>/plain); an empty range is accepted by both and writes nothing;
//   with --gpu: TilingAlgorithmGPU tiles one batch into an EntwineSink (<dir>/gpu).
// The inputs are dumped under <dir>/input; tests/test_cpp_las.py builds the expected directories from them.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../schwarzwald_amd/host/swz_tiling.hpp"

using namespace swz_host;

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static uint64_t next_u64() {  // splitmix64
  uint64_t z = (g_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
static double next_unit() { return (double)(next_u64() >> 11) * (1.0 / 9007199254740992.0); }

static bool dump(const std::string& path, const void* p, size_t bytes) {
  FILE* f = std::fopen(path.c_str(), "wb");
  if (!f) return false;
  const bool ok = std::fwrite(p, 1, bytes, f) == bytes;
  return std::fclose(f) == 0 && ok;
}

static AABB node_box(const std::string& name, AABB b) {
  for (size_t l = 1; l < name.size(); ++l) b = get_octant_bounds(static_cast<uint8_t>(name[l] - '0'), b);
  return b;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  const std::string dir = argv[1];
  const bool gpu = argc > 2 && std::strcmp(argv[2], "--gpu") == 0;
  const AABB bounds{{0, 0, 0}, {1, 1, 1}};
  const float spacing = (float)(std::sqrt(3.0) / 16.0);
  try {
    if (!gpu) {
      const char* names[] = {"r", "r3", "r30", "r301", "r3011", "r5"};
      const size_t counts[] = {5, 1, 2, 3, 300, 7};
      size_t total = 0;
      for (size_t c : counts) total += c;
      std::vector<double> xyz(3 * total), gps(total);
      std::vector<uint8_t> rgb(3 * total);
      std::vector<uint16_t> intensity(total);
      for (auto& v : xyz) v = next_unit();
      for (auto& v : rgb) v = (uint8_t)next_u64();
      for (auto& v : intensity) v = (uint16_t)next_u64();
      for (auto& v : gps) v = next_unit() * 1e6;
      if (!dump(dir + "/input/xyz.f64", xyz.data(), xyz.size() * 8) || !dump(dir + "/input/rgb.u8", rgb.data(), rgb.size()) ||
          !dump(dir + "/input/intensity.u16", intensity.data(), intensity.size() * 2) ||
          !dump(dir + "/input/gps.f64", gps.data(), gps.size() * 8))
        return 3;
      LASSink las(dir + "/las");
      EntwineSink ept(dir + "/ept");
      {
        EntwineSink plain(dir + "/plain");
        size_t at = 0;
        std::vector<uint32_t> ids(total);
        for (int k = 0; k < 6; ++k) {
          swz_attribute_columns cols{};
          cols.column[SWZ_ATTR_RGB] = rgb.data() + 3 * at;
          cols.column[SWZ_ATTR_INTENSITY] = intensity.data() + at;
          cols.column[SWZ_ATTR_GPS_TIME] = gps.data() + at;
          const AABB b = node_box(names[k], bounds);
          las.persist_rows(counts[k], xyz.data() + 3 * at, cols, b, names[k]);
          ept.persist_rows(counts[k], xyz.data() + 3 * at, cols, b, names[k]);
          plain.persist_points(ids.data() + at, ids.data() + at + counts[k], xyz.data() + 3 * at, b, names[k]);
          at += counts[k];
        }
        // an empty range: neither sink throws, neither writes
        las.persist_rows(0, xyz.data(), swz_attribute_columns{}, bounds, "r7");
        plain.persist_rows(0, xyz.data(), swz_attribute_columns{}, bounds, "r7");
        if (plain.num_nodes() != 6) return 4;
      }  // ~plain writes its hierarchy
      bool refused = false;
      try {
        ept.persist_rows(1, xyz.data(), swz_attribute_columns{}, bounds, "x12");
      } catch (const std::runtime_error&) {
        refused = true;
      }
      if (!refused || ept.num_nodes() != 6) return 5;
      ept.finish();
      std::printf("sink ok: 3 directories of 6 nodes\n");
      return 0;
    }
    const size_t n = 20000;
    std::vector<double> xyz(3 * n);
    for (auto& v : xyz) v = next_unit();
    if (!dump(dir + "/input/xyz_gpu.f64", xyz.data(), xyz.size() * 8)) return 3;
    EntwineSink sink(dir + "/gpu");
    TilerMetaParameters meta;
    meta.spacing_at_root = spacing;
    meta.max_points_per_node = 500;
    TilingAlgorithmGPU tiler(make_sampling_strategy_from_name("GRID_CENTER", 500), sink, meta);
    tiler.tile_batch(xyz.data(), n, bounds);
    const size_t persisted = tiler.finalize(bounds);
    if (persisted != sink.num_nodes()) return 6;
    sink.finish();
    std::printf("sink ok: %zu nodes\n", persisted);
    return 0;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "FAIL: %s\n", e.what());
    return 1;
  }
}
