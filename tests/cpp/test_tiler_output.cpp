// Drives TilingAlgorithmGPU::write_output (schwarzwald_amd/host/swz_tiling.hpp).  Usage: test_tiler_output <dir>
//   Three batches with attribute columns (RGB, intensity, classification, GPS time) go through tile_batch; write_output
//   writes <dir>/tiles (3DTILES) and <dir>/ept (ENTWINE_LAS, in small chunks); then the old path -- finalize() into a sink
//   that records what persist_points receives -- dumps every node's name, ids and positions under <dir>/sink.
// The inputs are dumped under <dir>/input; tests/test_cpp_tiler_output.py reads the files back and compares.
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

static bool dump(const std::string& path, const void* p, size_t bytes) {
  FILE* f = std::fopen(path.c_str(), "wb");
  if (!f) return false;
  const bool ok = std::fwrite(p, 1, bytes, f) == bytes;
  return std::fclose(f) == 0 && ok;
}

struct RecordingSink : PointsSink {
  std::string names;  // one per line: name, count
  std::vector<uint32_t> ids;
  std::vector<double> positions;
  size_t nodes = 0;
  void persist_points(const uint32_t* ids_begin, const uint32_t* ids_end, const double* pos, const AABB&, const std::string& node_name) override {
    const size_t count = static_cast<size_t>(ids_end - ids_begin);
    names += node_name + " " + std::to_string(count) + "\n";
    ids.insert(ids.end(), ids_begin, ids_end);
    positions.insert(positions.end(), pos, pos + 3 * count);
    ++nodes;
  }
};

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  const std::string dir = argv[1];
  const AABB bounds{{0, 0, 0}, {1, 1, 1}};
  const float spacing = (float)(std::sqrt(3.0) / 16.0);
  try {
    const size_t batch = 3000, batches = 3, n = batch * batches;
    std::vector<double> xyz(3 * n), gps(n);
    std::vector<uint8_t> rgb(3 * n), cls(n);
    std::vector<uint16_t> intensity(n);
    for (auto& v : xyz) v = next_unit();
    for (auto& v : rgb) v = (uint8_t)next_u64();
    for (auto& v : intensity) v = (uint16_t)next_u64();
    for (auto& v : cls) v = (uint8_t)(next_u64() & 31u);
    for (auto& v : gps) v = next_unit() * 1e9;
    if (!dump(dir + "/input/xyz.f64", xyz.data(), xyz.size() * 8) || !dump(dir + "/input/rgb.u8", rgb.data(), rgb.size()) ||
        !dump(dir + "/input/intensity.u16", intensity.data(), intensity.size() * 2) ||
        !dump(dir + "/input/classification.u8", cls.data(), cls.size()) || !dump(dir + "/input/gps_time.f64", gps.data(), gps.size() * 8))
      return 3;
    RecordingSink sink;
    TilerMetaParameters meta;
    meta.spacing_at_root = spacing;
    meta.max_points_per_node = 200;
    TilingAlgorithmGPU tiler(make_sampling_strategy_from_name("GRID_CENTER", 200), sink, meta);
    for (size_t b = 0; b < batches; ++b) {
      swz_attribute_columns cols{};
      cols.column[SWZ_ATTR_RGB] = rgb.data() + 3 * b * batch;
      cols.column[SWZ_ATTR_INTENSITY] = intensity.data() + b * batch;
      cols.column[SWZ_ATTR_CLASSIFICATION] = cls.data() + b * batch;
      cols.column[SWZ_ATTR_GPS_TIME] = gps.data() + b * batch;
      tiler.tile_batch(xyz.data() + 3 * b * batch, cols, batch, bounds);
    }
    swz_output_params p{};
    p.format = SWZ_OUT_3DTILES;
    p.attribute_mask = (1u << SWZ_ATTR_RGB) | (1u << SWZ_ATTR_INTENSITY) | (1u << SWZ_ATTR_CLASSIFICATION) | (1u << SWZ_ATTR_GPS_TIME);
    p.rgb_mapping = SWZ_PNTS_RGB_FROM_COLOR;
    p.global_offset[0] = 4.5e6;
    p.global_offset[1] = -1.25e5;
    p.global_offset[2] = 300.0;
    const swz_output_stats tiles = tiler.write_output(dir + "/tiles", p);
    p.format = SWZ_OUT_ENTWINE_LAS;
    p.chunk_points = 1000;
    const swz_output_stats ept = tiler.write_output(dir + "/ept", p);
    if (tiles.nodes != ept.nodes || tiles.chunks != 1 || ept.chunks < 2) return 4;
    bool refused = false;
    try {
      swz_attribute_columns none{};
      tiler.tile_batch(xyz.data(), none, batch, bounds);
    } catch (const std::runtime_error&) {
      refused = true;  // no batch after write_output has finalized the tiler
    }
    if (!refused) return 5;
    const size_t persisted = tiler.finalize(bounds);  // the old path, afterwards: the same files, as ids and positions
    if (persisted != sink.nodes || persisted != tiles.nodes) return 6;
    if (!dump(dir + "/sink/nodes.txt", sink.names.data(), sink.names.size()) ||
        !dump(dir + "/sink/ids.u32", sink.ids.data(), sink.ids.size() * 4) ||
        !dump(dir + "/sink/positions.f64", sink.positions.data(), sink.positions.size() * 8))
      return 3;
    std::printf("output ok: %zu nodes, %llu stored points\n", persisted, (unsigned long long)tiles.stored_points);
    return 0;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "FAIL: %s\n", e.what());
    return 1;
  }
}
