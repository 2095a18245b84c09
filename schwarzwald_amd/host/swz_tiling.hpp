// swz_tiling.hpp -- host-side C++17 mirror of the reference's tiler/sampling interface on top of the
// C ABI (include/swz_gpu.h).  Header only, no dependency besides the C++ standard library and
// libswz_gpu.so.  Names, argument meaning and error behaviour follow the reference seams so that the
// adapter a maintainer writes inside Schwarzwald is a thin forwarding layer:
//
//   reference (schwarzwald/core/...)                         here (namespace swz_host)
//   ------------------------------------------------------   -----------------------------------------
//   Vector3<double>, AABB            math/Vector3.h, AABB.h   Vector3d, AABB
//   MortonIndex64                    MortonIndex.h:80-169     MortonIndex64 (uint64_t) + helpers
//   IndexedPoint64                   tiling/Sampling.h:147    IndexedPoint64 {point_index, morton_index}
//   OutlierPointsBehaviour           OctreeAlgorithms.h:20    OutlierPointsBehaviour
//   index_points<21>                 OctreeAlgorithms.h:181   index_points
//   Range::sort                      containers/Range.h:62    sort_indexed_points
//   SamplingStrategy + factory       Sampling.h:761-791       SamplingStrategy, make_sampling_strategy_from_name
//   SamplingBehaviour                Sampling.h:170-181       SamplingBehaviour
//   sample_points                    Sampling.h:799-821       sample_points (returns the partition point)
//   TilerMetaParameters              process/Tiler.h:64-75    TilerMetaParameters
//   PointsPersistence::persist_points io/PointsPersistence.h  PointsSink::persist_points
//   TilingAlgorithmBase              TilingAlgorithms.h:70    TilingAlgorithmGPU::tile_batch / add_las_files / finalize / write_output / write_properties
//   get_octant_bounds                OctreeAlgorithms.cpp:3   get_octant_bounds
//
// Errors: every failing ABI call becomes std::runtime_error carrying swz_last_error(), the way the
// reference reports tiler failures (executable/main.cpp:599-602).
#pragma once

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdint>
#include <initializer_list>
#include <map>
#include <memory>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "../../include/swz_gpu.h"

namespace swz_host {

struct Vector3d {
  double x = 0, y = 0, z = 0;
};
struct AABB {
  Vector3d min, max;
  Vector3d extent() const { return {max.x - min.x, max.y - min.y, max.z - min.z}; }
};

using MortonIndex64 = uint64_t;
constexpr unsigned MortonIndex64Levels = 21;

struct IndexedPoint64 {
  uint32_t point_index;  // stands for PointBuffer::PointReference: row of the position array
  MortonIndex64 morton_index;
};

enum class OutlierPointsBehaviour { ClampToBounds, Abort };
enum class SamplingBehaviour { TakeAllWhenCountBelowMaxPoints, AlwaysAdhereToMinSpacing };
enum class TilingStrategy { Accurate, Fast };

struct SamplingStrategy {
  int kind;  // SWZ_RANDOM_GRID ...
  size_t max_points_per_node;
  // SWZ_MIN_DISTANCE_FAST (AdaptivePoissonDiskSampling): the share of a node's points that is examined, per node level.  The
  // library samples with the command line's densities and no others (swz_min_distance_fast_stride); this is their record.
  float (*density_per_level)(int32_t) = nullptr;
};
// the densities TilerProcess::make_sampling_strategy attaches (TilerProcess.cpp:502-508): 0.25f, 0.5f, then 1.f
inline float min_distance_fast_density(int32_t node_level) { return 1.f / static_cast<float>(swz_min_distance_fast_stride(node_level)); }
// make_sampling_strategy_from_name -- core/tiling/Sampling.h:774-791 (no MIN_DISTANCE_FAST: like the reference's, this
// factory has no densities to build the adaptive sampler with; see make_sampling_strategy)
inline SamplingStrategy make_sampling_strategy_from_name(const std::string& name, size_t max_points_per_node) {
  if (name == "RANDOM_GRID") return {SWZ_RANDOM_GRID, max_points_per_node};
  if (name == "GRID_CENTER") return {SWZ_GRID_CENTER, max_points_per_node};
  if (name == "MIN_DISTANCE") return {SWZ_MIN_DISTANCE, max_points_per_node};
  if (name == "JITTERED") return {SWZ_JITTERED, max_points_per_node};
  throw std::runtime_error{"Unrecognized sampling strategy name \"" + name + "\""};
}
// TilerProcess::make_sampling_strategy -- core/process/TilerProcess.cpp:491-516: the five --sampling names
inline SamplingStrategy make_sampling_strategy(const std::string& name, size_t max_points_per_node) {
  if (name == "MIN_DISTANCE_FAST") return {SWZ_MIN_DISTANCE_FAST, max_points_per_node, &min_distance_fast_density};
  if (name == "RANDOM_GRID" || name == "GRID_CENTER" || name == "MIN_DISTANCE" || name == "JITTERED")
    return make_sampling_strategy_from_name(name, max_points_per_node);
  throw std::invalid_argument{"Unrecognized sampling strategy " + name};
}

struct TilerMetaParameters {  // core/process/Tiler.h:64-75
  float spacing_at_root = 0.f;
  uint32_t max_depth = 100;
  size_t max_points_per_node = 20000;
  TilingStrategy tiling_strategy = TilingStrategy::Accurate;
  uint32_t num_indexing_threads = 8;  // FAST: decides the start level
};

// get_octant_bounds -- core/tiling/OctreeAlgorithms.cpp:3-18
inline AABB get_octant_bounds(uint8_t octant, const AABB& parent) {
  const Vector3d e = parent.extent();
  const double min_z = (octant & 1) ? (parent.min.z + e.z / 2) : parent.min.z;
  const double min_y = ((octant >> 1) & 1) ? (parent.min.y + e.y / 2) : parent.min.y;
  const double min_x = ((octant >> 2) & 1) ? (parent.min.x + e.x / 2) : parent.min.x;
  return {{min_x, min_y, min_z}, {min_x + e.x / 2, min_y + e.y / 2, min_z + e.z / 2}};
}
inline uint8_t get_octant_at_level(MortonIndex64 key, uint32_t level) {
  return static_cast<uint8_t>((key >> ((MortonIndex64Levels - level - 1) * 3)) & 0b111);
}

// One swz_ctx, owned.  Not thread-safe (one call in flight per context).
// SRSTransformHelper's two calls (core/util/Transformation.h) over the library's own map of a source projection
// (swz_srs_parse: UTM zones, +proj=tmerc, longlat; no PROJ).  The constructor throws the reference's "Source projection ...
// not recognized!" (Proj4Transform, Transformation.cpp:74-85) for a definition the library refuses; why() says which token.
class SourceProjection {
public:
  explicit SourceProjection(const std::string& definition) {
    char why[512] = {0};
    if (swz_srs_parse_why(definition.c_str(), &_srs, why, sizeof(why)) != SWZ_OK)
      throw std::runtime_error{"Source projection " + definition + " not recognized! (" + why + ")"};
  }
  const swz_srs* srs() const { return &_srs; }
  // target: SWZ_SRS_ECEF (the reference's TargetSRS::CesiumWorld) or SWZ_SRS_WGS84; in place
  void transformPositionsTo(int target, Vector3d* positions, size_t count) const {
    static_assert(sizeof(Vector3d) == 24, "positions are rows of three doubles");
    if (swz_srs_transform(&_srs, target, reinterpret_cast<double*>(positions), count) != SWZ_OK)
      throw std::runtime_error{"SourceProjection: unknown target"};
  }
  void transformAABBsTo(int target, AABB* boxes, size_t count) const {
    for (size_t i = 0; i < count; ++i) {
      const double mn[3] = {boxes[i].min.x, boxes[i].min.y, boxes[i].min.z}, mx[3] = {boxes[i].max.x, boxes[i].max.y, boxes[i].max.z};
      double lo[3], hi[3];
      if (swz_srs_transform_box(&_srs, target, mn, mx, lo, hi) != SWZ_OK) throw std::runtime_error{"SourceProjection: unknown target"};
      boxes[i].min = {lo[0], lo[1], lo[2]};
      boxes[i].max = {hi[0], hi[1], hi[2]};
    }
  }

private:
  swz_srs _srs{};
};

class Context {
public:
  explicit Context(int device = 0) {
    if (swz_create(&_ctx, device) != SWZ_OK) throw std::runtime_error{swz_last_error(nullptr)};
  }
  ~Context() { swz_destroy(_ctx); }
  Context(const Context&) = delete;
  Context& operator=(const Context&) = delete;
  swz_ctx* get() const { return _ctx; }
  void check(int status) const {
    if (status != SWZ_OK) throw std::runtime_error{swz_last_error(_ctx)};
  }

private:
  swz_ctx* _ctx = nullptr;
};

// ConverterProcess::run (core/process/ConverterProcess.cpp) in one call: the written data set in src_dir (BIN, BINZ, LAS or
// ENTWINE_LAS node files; root box and spacing from its properties.json or ept.json unless params gives them) converted into
// dst_dir in the format of params.out, node files unpacked and packed on the device (swz_convert_dataset).  lossy_source (or
// SWZ_CONVERT_LOSSY_SOURCE in params.source_flags) admits a 3DTILES source, whose .pnts files hold float positions, RGB and
// intensity only (the reference's converter reads them through Cesium3DTilesPersistence).  A refusal -- a .pnts source
// without the switch, dst_dir equal to src_dir, a mask outside the source's, no root box -- throws with the library's text.
inline swz_convert_stats convert_dataset(Context& ctx, const std::string& src_dir, const std::string& dst_dir,
                                         const swz_convert_params& params, bool lossy_source = false) {
  swz_convert_params p = params;
  if (lossy_source) p.source_flags |= SWZ_CONVERT_LOSSY_SOURCE;
  swz_convert_stats stats{};
  ctx.check(swz_convert_dataset(ctx.get(), src_dir.c_str(), dst_dir.c_str(), &p, &stats));
  return stats;
}

// The conversion the reference's --converter mode exists for (convert_to_pnts_file, ConverterProcess.cpp:505-530;
// ConverterArguments::source_projection): src_dir converted into 3D Tiles in the world frame -- positions mapped to ECEF on the
// device, every .pnts file relative to its node's own origin, tile volumes as oriented boxes (swz_convert_dataset_world).
// projection == nullptr is the reference's IdentityTransform.  params.out.format must be SWZ_OUT_3DTILES and
// params.out.global_offset zero; lossy_source as in convert_dataset; a refusal throws with the library's text.
inline swz_convert_stats convert_dataset_world(Context& ctx, const std::string& src_dir, const std::string& dst_dir,
                                               const swz_convert_params& params, const SourceProjection* projection = nullptr,
                                               bool lossy_source = false) {
  swz_convert_params p = params;
  if (lossy_source) p.source_flags |= SWZ_CONVERT_LOSSY_SOURCE;
  swz_convert_stats stats{};
  ctx.check(swz_convert_dataset_world(ctx.get(), src_dir.c_str(), dst_dir.c_str(), &p, projection ? projection->srs() : nullptr,
                                      &stats));
  return stats;
}

// The points of a written data set inside a closed box, of the nodes down to params.max_depth (swz_dataset_query): the kept
// nodes' files are streamed and unpacked as convert_dataset does, the rows of the box selected on the device into arrays of
// swz_dataset_query_nodes' points_bound rows, and the result copied to the host -- positions (3 doubles per point), the
// columns of params.attribute_mask (~0u: all the source holds) as raw rows, and with want_nodes per point the index of its
// node in swz_dataset_query_nodes' table.  The order is the node table's, then the file's.  lossy_source as in
// convert_dataset.  A refusal -- a bad box, a .pnts source without the switch, no root box -- throws with the library's text.
struct QueryResult {
  uint64_t count = 0;
  std::vector<double> positions;
  std::vector<uint8_t> columns[SWZ_ATTR_COUNT];  // empty: not asked for, or not in the source
  std::vector<uint32_t> nodes;
  swz_query_stats stats{};
};
// A swz_filter put together clause by clause: Filter().range(SWZ_ATTR_GPS_TIME, lo, hi).any_of(SWZ_ATTR_CLASSIFICATION, {2, 9})
// .none_of(SWZ_ATTR_CLASSIFICATION, {7, 18}).  range: lo <= value <= hi as doubles, closed (infinities open an end; a NaN value
// fails); any_of / none_of: the value is (not) one of these, on the one-byte columns -- a value is stored as its byte, so scan
// angle rank -1 is bit 255.  A row passes iff it passes every clause.  Only what cannot be stored throws here (a ninth clause, a
// value outside a byte); the library refuses the rest (include/swz_gpu.h), through query_dataset_filtered.
class Filter {
public:
  Filter& range(int attribute, double lo, double hi) {
    swz_filter_clause& c = next(attribute, SWZ_FILTER_RANGE);
    c.lo = lo;
    c.hi = hi;
    return *this;
  }
  Filter& any_of(int attribute, std::initializer_list<int> values) { return set(attribute, SWZ_FILTER_SET, values); }
  Filter& none_of(int attribute, std::initializer_list<int> values) { return set(attribute, SWZ_FILTER_SET | SWZ_FILTER_NOT, values); }
  const swz_filter* get() const { return &_f; }

private:
  swz_filter_clause& next(int attribute, uint32_t kind) {
    if (_f.count >= SWZ_FILTER_MAX_CLAUSES) throw std::runtime_error{"Filter: a filter holds 8 clauses at the most"};
    swz_filter_clause& c = _f.clause[_f.count++];
    c.attribute = attribute;
    c.kind = kind;
    return c;
  }
  Filter& set(int attribute, uint32_t kind, std::initializer_list<int> values) {
    for (int v : values)
      if (v < -128 || v > 255) throw std::runtime_error{"Filter: a set holds the values of one byte"};
    swz_filter_clause& c = next(attribute, kind);
    for (int v : values) c.set[(v & 255) >> 6] |= 1ull << (v & 63);
    return *this;
  }
  swz_filter _f{};
};

// query_dataset_region for the rows that also pass a filter over the attribute columns (swz_dataset_query_filtered); filter ==
// nullptr is query_dataset_region.  The columns of params.attribute_mask come back; the columns the filter names are read for
// it whether the mask holds them or not.  nodes index swz_dataset_query_region_nodes' table; after summarize_dataset (below) the
// node files the filter cannot reach are not read, which changes the stats and nothing else.
// A filter the library refuses throws with swz_filter_check's text before a file is read.
inline QueryResult query_dataset_filtered(Context& ctx, const std::string& dir, const swz_query_params& params, const swz_region* region,
                                          const swz_filter* filter, bool lossy_source = false, bool want_nodes = false) {
  static const uint32_t widths[SWZ_ATTR_COUNT] = {3, 12, 2, 1, 1, 8, 1, 1, 2, 1, 1, 1};
  if (filter) {
    char why[512];
    if (swz_filter_check(filter, why, sizeof why) != SWZ_OK) throw std::runtime_error{why};
  }
  swz_query_params p = params;
  if (lossy_source) p.source_flags |= SWZ_CONVERT_LOSSY_SOURCE;
  uint64_t kept = 0, bound = 0;
  if (region) ctx.check(swz_dataset_query_region_nodes(ctx.get(), dir.c_str(), &p, region, 0, nullptr, nullptr, nullptr, &kept, &bound));
  else ctx.check(swz_dataset_query_nodes(ctx.get(), dir.c_str(), &p, 0, nullptr, nullptr, nullptr, &kept, &bound));
  if (p.attribute_mask == ~0u) {
    swz_dataset_info info{};
    uint64_t scanned = 0;
    ctx.check(swz_dataset_scan(ctx.get(), dir.c_str(), p.max_depth, &info, 0, nullptr, nullptr, nullptr, &scanned));
    p.attribute_mask = info.attribute_mask;
  }
  struct Device {  // freed however the call ends
    std::vector<void*> ptrs;
    ~Device() {
      for (void* d : ptrs) (void)swz_device_free(d);
    }
  } device;
  auto alloc = [&](uint64_t bytes) {
    void* d = nullptr;
    ctx.check(swz_device_alloc_on(ctx.get(), bytes ? bytes : 1, &d));
    device.ptrs.push_back(d);
    return d;
  };
  QueryResult out;
  double* d_xyz = static_cast<double*>(alloc(24 * bound));
  swz_attribute_columns d_cols{};
  for (int a = 0; a < SWZ_ATTR_COUNT; ++a)
    if ((p.attribute_mask >> a) & 1u) d_cols.column[a] = alloc(widths[a] * bound);
  uint32_t* d_nodes = want_nodes ? static_cast<uint32_t*>(alloc(4 * bound)) : nullptr;
  if (filter)
    ctx.check(swz_dataset_query_filtered(ctx.get(), dir.c_str(), &p, region, filter, bound, d_xyz, &d_cols, d_nodes, &out.count, &out.stats));
  else if (region) ctx.check(swz_dataset_query_region(ctx.get(), dir.c_str(), &p, region, bound, d_xyz, &d_cols, d_nodes, &out.count, &out.stats));
  else ctx.check(swz_dataset_query(ctx.get(), dir.c_str(), &p, bound, d_xyz, &d_cols, d_nodes, &out.count, &out.stats));
  out.positions.resize(3 * out.count);
  if (out.count) ctx.check(swz_copy_to_host(ctx.get(), out.positions.data(), d_xyz, 24 * out.count));
  for (int a = 0; a < SWZ_ATTR_COUNT; ++a) {
    if (!d_cols.column[a]) continue;
    out.columns[a].resize(widths[a] * out.count);
    if (out.count) ctx.check(swz_copy_to_host(ctx.get(), out.columns[a].data(), d_cols.column[a], widths[a] * out.count));
  }
  if (want_nodes) {
    out.nodes.resize(out.count);
    if (out.count) ctx.check(swz_copy_to_host(ctx.get(), out.nodes.data(), d_nodes, 4 * out.count));
  }
  return out;
}
// The rows query_dataset_filtered selects, rastered on the device instead of returned (swz_dataset_rasterize): per cell of
// grid.nx x grid.ny cells over the x-y rectangle of params' box the count and the min, max and mean of grid.value -- the row's
// z (SWZ_RASTER_VALUE_Z) or a scalar attribute of one or two bytes.  Only the table comes back: cells as the device left them
// (integer sums and order-preserving codes, bit-exact whatever the chunking), decoded by swz_raster_finish into count, min, max
// and mean; element iy * nx + ix, iy ascending with y; an empty cell has count 0, min +inf, max -inf, mean NaN.
// params.attribute_mask is ignored (0 or ~0u).  region and filter may be nullptr.  A grid or a filter the library refuses
// throws with its text before a file is read.
struct RasterResult {
  swz_raster_frame frame{};
  std::vector<swz_raster_cell> cells;
  std::vector<uint64_t> count;
  std::vector<double> min, max, mean;
  swz_query_stats stats{};
};
inline RasterResult rasterize_dataset(Context& ctx, const std::string& dir, const swz_query_params& params, const swz_region* region,
                                      const swz_filter* filter, const swz_raster_grid& grid, bool lossy_source = false) {
  char why[512];
  if (filter && swz_filter_check(filter, why, sizeof why) != SWZ_OK) throw std::runtime_error{why};
  RasterResult out;
  if (swz_raster_frame_of(params.box_min, params.box_max, &grid, &out.frame, why, sizeof why) != SWZ_OK) throw std::runtime_error{why};
  swz_query_params p = params;
  if (lossy_source) p.source_flags |= SWZ_CONVERT_LOSSY_SOURCE;
  const size_t n = (size_t)grid.nx * grid.ny;
  out.cells.resize(n);
  ctx.check(swz_dataset_rasterize(ctx.get(), dir.c_str(), &p, region, filter, &grid, out.cells.data(), &out.frame, &out.stats));
  out.count.resize(n);
  out.min.resize(n);
  out.max.resize(n);
  out.mean.resize(n);
  ctx.check(swz_raster_finish(&out.frame, out.cells.data(), out.count.data(), out.min.data(), out.max.data(), out.mean.data()));
  return out;
}
// Per-node attribute summaries (swz_dataset_summarize): every node file of dir is streamed once, the scalar columns are
// summarised per node on the device and dir/node-summaries.swz is written.  Afterwards query_dataset_filtered skips the node
// files the filter cannot reach -- the same rows, fewer nodes read.  Run it again after the data set changed: a summary that
// does not describe the files is refused as stale.  lossy_source as in convert_dataset.
inline swz_summarize_stats summarize_dataset(Context& ctx, const std::string& dir, bool lossy_source = false, uint64_t chunk_points = 0) {
  swz_summarize_stats stats{};
  ctx.check(swz_dataset_summarize(ctx.get(), dir.c_str(), lossy_source ? SWZ_CONVERT_LOSSY_SOURCE : 0u, chunk_points, &stats));
  return stats;
}
// The nodes a filtered query reads (swz_dataset_query_filtered_nodes): the table of the region query, unchanged, and per node
// whether the summaries of dir let the filter reach it (all of them without node-summaries.swz or without a filter).
struct FilteredNodes {
  std::vector<int8_t> level;
  std::vector<uint64_t> key, count;
  std::vector<uint8_t> read;
  uint64_t points_bound = 0;  // the sum of the counts of the nodes that are read
};
inline FilteredNodes query_dataset_filtered_nodes(Context& ctx, const std::string& dir, const swz_query_params& params, const swz_region* region,
                                                  const swz_filter* filter, bool lossy_source = false) {
  swz_query_params p = params;
  if (lossy_source) p.source_flags |= SWZ_CONVERT_LOSSY_SOURCE;
  FilteredNodes out;
  uint64_t num = 0;
  ctx.check(swz_dataset_query_filtered_nodes(ctx.get(), dir.c_str(), &p, region, filter, 0, nullptr, nullptr, nullptr, nullptr, &num, &out.points_bound));
  out.level.resize(num);
  out.key.resize(num);
  out.count.resize(num);
  out.read.resize(num);
  if (num)
    ctx.check(swz_dataset_query_filtered_nodes(ctx.get(), dir.c_str(), &p, region, filter, num, out.level.data(), out.key.data(), out.count.data(),
                                               out.read.data(), &num, &out.points_bound));
  return out;
}
// query_dataset for the box cut by a region (swz_dataset_query_region): planes (a frustum: frustum_planes) or a polygon in
// x-y; region == nullptr is the box alone.  Everything else is query_dataset's; nodes index swz_dataset_query_region_nodes'
// table.
inline QueryResult query_dataset_region(Context& ctx, const std::string& dir, const swz_query_params& params, const swz_region* region,
                                        bool lossy_source = false, bool want_nodes = false) {
  return query_dataset_filtered(ctx, dir, params, region, nullptr, lossy_source, want_nodes);
}
inline QueryResult query_dataset(Context& ctx, const std::string& dir, const swz_query_params& params, bool lossy_source = false,
                                 bool want_nodes = false) {
  return query_dataset_region(ctx, dir, params, nullptr, lossy_source, want_nodes);
}

// The six inward planes of a row-major 4 x 4 view-projection matrix m (clip = m (x, y, z, 1), clip volume -w <= x, y, z <= w),
// as rows (a, b, c, d) for a swz_region of SWZ_REGION_PLANES: the sums and differences of m's rows with its last row -- left,
// right, bottom, top, near, far --, every row divided by the length of its normal.  The doubles returned are the planes the
// query takes; nothing is promised about how exactly they follow the matrix.
inline std::array<double, 24> frustum_planes(const double m[16]) {
  std::array<double, 24> out{};
  for (int k = 0; k < 6; ++k) {
    const double sign = (k & 1) ? -1.0 : 1.0;
    double row[4];
    for (int j = 0; j < 4; ++j) row[j] = m[12 + j] + sign * m[4 * (k / 2) + j];
    const double len = std::sqrt(row[0] * row[0] + row[1] * row[1] + row[2] * row[2]);
    for (int j = 0; j < 4; ++j) out[4 * k + j] = row[j] / len;
  }
  return out;
}

// index_points<21> -- OctreeAlgorithms.h:181-197.  positions: n x 3 doubles (PointBuffer::positions().data());
// outliers are clamped in place, like index_point does.
inline void index_points(Context& ctx, double* positions, size_t n, IndexedPoint64* indexed_points_begin,
                         const AABB& bounds, OutlierPointsBehaviour behaviour) {
  if (behaviour != OutlierPointsBehaviour::ClampToBounds)
    throw std::runtime_error{"only OutlierPointsBehaviour::ClampToBounds is implemented (the tiler never uses Abort)"};
  std::vector<uint64_t> keys(n);
  const double mn[3] = {bounds.min.x, bounds.min.y, bounds.min.z}, mx[3] = {bounds.max.x, bounds.max.y, bounds.max.z};
  ctx.check(swz_morton_encode(ctx.get(), positions, n, mn, mx, keys.data()));
  for (size_t i = 0; i < n; ++i) indexed_points_begin[i] = {static_cast<uint32_t>(i), keys[i]};
}

// Range<IndexedPointsIter>::sort -- containers/Range.h:62-66; ties keep their input order
inline void sort_indexed_points(Context& ctx, IndexedPoint64* begin, IndexedPoint64* end) {
  const size_t n = static_cast<size_t>(end - begin);
  std::vector<uint64_t> keys(n);
  for (size_t i = 0; i < n; ++i) keys[i] = begin[i].morton_index;
  std::vector<uint32_t> perm(n);
  ctx.check(swz_sort_by_key(ctx.get(), keys.data(), n, perm.data(), nullptr));
  std::vector<IndexedPoint64> tmp(begin, end);
  for (size_t i = 0; i < n; ++i) begin[i] = tmp[perm[i]];
}

// sample_points -- Sampling.h:799-821: stable partition of [begin, end) into [taken | rest], returns the
// partition point.  positions: the PointBuffer's position array the point indices refer to.
inline IndexedPoint64* sample_points(Context& ctx, const SamplingStrategy& strategy, IndexedPoint64* begin,
                                     IndexedPoint64* end, MortonIndex64 node_key, int32_t node_level,
                                     const AABB& root_bounds, float spacing_at_root, SamplingBehaviour behaviour,
                                     const double* positions, size_t num_positions) {
  const size_t n = static_cast<size_t>(end - begin);
  std::vector<uint64_t> keys(n);
  std::vector<uint32_t> idx(n);
  for (size_t i = 0; i < n; ++i) {
    keys[i] = begin[i].morton_index;
    idx[i] = begin[i].point_index;
  }
  std::vector<uint8_t> taken(n);
  uint64_t num_taken = 0;
  const double mn[3] = {root_bounds.min.x, root_bounds.min.y, root_bounds.min.z};
  const double mx[3] = {root_bounds.max.x, root_bounds.max.y, root_bounds.max.z};
  ctx.check(swz_sample_points(ctx.get(), strategy.kind, strategy.max_points_per_node, keys.data(), idx.data(), n,
                              positions, num_positions, node_key, node_level, mn, mx, spacing_at_root,
                              behaviour == SamplingBehaviour::AlwaysAdhereToMinSpacing
                                ? SWZ_ALWAYS_ADHERE_TO_MIN_SPACING
                                : SWZ_TAKE_ALL_WHEN_COUNT_BELOW_MAX_POINTS,
                              taken.data(), &num_taken));
  std::vector<IndexedPoint64> tmp(begin, end);
  IndexedPoint64* front = begin;
  IndexedPoint64* back = begin + num_taken;
  for (size_t i = 0; i < n; ++i) *(taken[i] ? front++ : back++) = tmp[i];
  return begin + num_taken;
}

// What the adapter needs from PointsPersistence (core/io/PointsPersistence.h:23-53).
struct PointsSink {
  virtual ~PointsSink() = default;
  // The complete content of one node file, in file (Morton) order.  ids are point ids: the running index of the
  // point over ALL batches in input order (batch 0 holds ids 0..n0-1, batch 1 the next n1, ...); positions are
  // the node's count x 3 clamped positions, gathered on the device (what persist_points reads through the
  // PointReferences, core/tiling/TilingAlgorithms.cpp:232-236, 316-322).
  virtual void persist_points(const uint32_t* ids_begin, const uint32_t* ids_end, const double* positions,
                              const AABB& node_bounds, const std::string& node_name) = 0;
  // Sharded batches (ShardedTilingAlgorithmGPU): the attribute columns travelled with the points between the
  // GPUs, so a node's file arrives as rows instead of ids: count positions plus every attribute column present
  // (host memory, count rows each, in file order).
  virtual void persist_rows(size_t /*count*/, const double* /*positions*/, const swz_attribute_columns& /*attributes*/,
                            const AABB& /*node_bounds*/, const std::string& /*node_name*/) {
    throw std::runtime_error{"PointsSink::persist_rows is not implemented by this sink"};
  }
};

// Cesium3DTilesPersistence (core/io/Cesium3DTilesPersistence.cpp:53-210), the reference's default persistence, as a sink:
// every node becomes "<work_dir>/<name>.pnts" (swz_pnts_write_node_rows: positions narrowed to float and not shifted,
// RTC_CENTER = global_offset; RGB and intensity when the rows carry them), the sink remembers the names it wrote, and
// write_tilesets() -- called by the destructor if nobody did, like the reference's -- writes the tileset JSON files of
// those nodes and their ancestors (swz_tileset_build + swz_tileset_write).  rgb_mapping: --calculate-rgb-from
// (SWZ_PNTS_RGB_FROM_*): with a mapping RGB is the grey value of the intensity, written only if the rows have intensities.
// persist_points receives ids and positions only, so its files hold POSITION alone.
class Cesium3DTilesSink : public PointsSink {
public:
  Cesium3DTilesSink(std::string work_dir, const AABB& root_bounds, float spacing_at_root, Vector3d global_offset = {},
                    int rgb_mapping = SWZ_PNTS_RGB_FROM_COLOR)
    : _work_dir(std::move(work_dir)), _root_bounds(root_bounds), _spacing_at_root(spacing_at_root),
      _offset{global_offset.x, global_offset.y, global_offset.z}, _rgb_mapping(rgb_mapping) {}
  ~Cesium3DTilesSink() override {
    if (!_tilesets_written) {
      try {
        write_tilesets();
      } catch (...) {  // a destructor reports nothing; call write_tilesets() to see the error
      }
    }
  }
  Cesium3DTilesSink(const Cesium3DTilesSink&) = delete;
  Cesium3DTilesSink& operator=(const Cesium3DTilesSink&) = delete;

  void persist_points(const uint32_t* ids_begin, const uint32_t* ids_end, const double* positions, const AABB& node_bounds,
                      const std::string& node_name) override {
    persist_rows(static_cast<size_t>(ids_end - ids_begin), positions, swz_attribute_columns{}, node_bounds, node_name);
  }
  void persist_rows(size_t count, const double* positions, const swz_attribute_columns& attributes, const AABB&,
                    const std::string& node_name) override {
    if (count == 0) throw std::runtime_error{"persist_points requires a non-empty range"};  // Cesium3DTilesPersistence.cpp:58-60
    const bool has_intensity = attributes.column[SWZ_ATTR_INTENSITY] != nullptr;
    const bool mapped = _rgb_mapping != SWZ_PNTS_RGB_FROM_COLOR;
    uint32_t mask = has_intensity ? SWZ_PNTS_INTENSITY : 0u;
    if (mapped ? has_intensity : attributes.column[SWZ_ATTR_RGB] != nullptr) mask |= SWZ_PNTS_RGB;
    const std::string path = _work_dir + "/" + node_name + ".pnts";
    if (swz_pnts_write_node_rows(nullptr, path.c_str(), count, positions, &attributes, mask,
                                 (mapped && has_intensity) ? _rgb_mapping : SWZ_PNTS_RGB_FROM_COLOR, _offset) != SWZ_OK)
      throw std::runtime_error{"Could not write .pnts file \"" + path + "\""};
    _node_names.push_back(node_name);
  }

  // the names of the nodes written so far, in the order they arrived
  const std::vector<std::string>& node_names() const { return _node_names; }

  void write_tilesets() {
    _tilesets_written = true;
    if (_node_names.empty()) return;
    std::vector<int8_t> level(_node_names.size());
    std::vector<uint64_t> key(_node_names.size());
    for (size_t j = 0; j < _node_names.size(); ++j) {  // "r" + octant digits
      const std::string& name = _node_names[j];
      if (name.empty() || name[0] != 'r' || name.size() > MortonIndex64Levels + 1)
        throw std::runtime_error{"not a node name: \"" + name + "\""};
      level[j] = static_cast<int8_t>(static_cast<int>(name.size()) - 2);
      for (size_t l = 1; l < name.size(); ++l) {
        if (name[l] < '0' || name[l] > '7') throw std::runtime_error{"not a node name: \"" + name + "\""};
        key[j] |= static_cast<uint64_t>(name[l] - '0') << ((MortonIndex64Levels - l) * 3);
      }
    }
    const double mn[3] = {_root_bounds.min.x, _root_bounds.min.y, _root_bounds.min.z};
    const double mx[3] = {_root_bounds.max.x, _root_bounds.max.y, _root_bounds.max.z};
    uint64_t num = 0;
    if (swz_tileset_build(level.size(), level.data(), key.data(), mn, mx, _spacing_at_root, _offset, 0, nullptr, &num) != SWZ_OK)
      throw std::runtime_error{"swz_tileset_build failed"};
    std::vector<swz_tileset_node> tiles(num);
    if (swz_tileset_build(level.size(), level.data(), key.data(), mn, mx, _spacing_at_root, _offset, num, tiles.data(), &num) != SWZ_OK ||
        swz_tileset_write(nullptr, tiles.data(), num, _work_dir.c_str()) != SWZ_OK)
      throw std::runtime_error{"Error writing tileset JSON to \"" + _work_dir + "\""};
  }

private:
  std::string _work_dir;
  AABB _root_bounds;
  float _spacing_at_root;
  double _offset[3];
  int _rgb_mapping;
  std::vector<std::string> _node_names;
  bool _tilesets_written = false;
};

// "r" + octant digits (TilingAlgorithms.cpp:139) -> (node level, Morton key); throws for anything else
inline void node_from_potree_name(const std::string& name, int8_t* level, uint64_t* key) {
  if (name.empty() || name[0] != 'r' || name.size() > MortonIndex64Levels + 1)
    throw std::runtime_error{"not a node name: \"" + name + "\""};
  *level = static_cast<int8_t>(static_cast<int>(name.size()) - 2);
  *key = 0;
  for (size_t l = 1; l < name.size(); ++l) {
    if (name[l] < '0' || name[l] > '7') throw std::runtime_error{"not a node name: \"" + name + "\""};
    *key |= static_cast<uint64_t>(name[l] - '0') << ((MortonIndex64Levels - l) * 3);
  }
}

// LASPersistence (core/io/LASPersistence.cpp:69-271) as a sink: every node becomes "<work_dir>/<name>.las", a LAS 1.2 file
// whose offsets and box are node_bounds and whose scale is compute_las_scale_from_bounds of them (swz_las_write_node_rows).
// The records carry every attribute column the rows have; persist_points receives ids and positions only, so its files are
// point format 0 with zero attributes.  An empty range: the reference writes a file of a header and no records, this sink
// writes nothing and does not throw.
class LASSink : public PointsSink {
public:
  explicit LASSink(std::string work_dir) : _work_dir(std::move(work_dir)) {}

  void persist_points(const uint32_t* ids_begin, const uint32_t* ids_end, const double* positions, const AABB& node_bounds,
                      const std::string& node_name) override {
    persist_rows(static_cast<size_t>(ids_end - ids_begin), positions, swz_attribute_columns{}, node_bounds, node_name);
  }
  void persist_rows(size_t count, const double* positions, const swz_attribute_columns& attributes, const AABB& node_bounds,
                    const std::string& node_name) override {
    write_las(_work_dir + "/" + node_name + ".las", count, positions, attributes, node_bounds);
  }

protected:
  static void write_las(const std::string& path, size_t count, const double* positions, const swz_attribute_columns& attributes,
                        const AABB& b) {
    if (count == 0) return;
    uint32_t mask = 0;
    for (int a = 0; a < SWZ_ATTR_COUNT; ++a)
      if (attributes.column[a]) mask |= 1u << a;
    const double mn[3] = {b.min.x, b.min.y, b.min.z}, mx[3] = {b.max.x, b.max.y, b.max.z};
    if (swz_las_write_node_rows(nullptr, path.c_str(), count, positions, &attributes, mask, mn, mx, swz_las_scale_from_bounds(mn, mx)) !=
        SWZ_OK)
      throw std::runtime_error{"Could not write LAS file \"" + path + "\""};
  }
  std::string _work_dir;
};

// EntwinePersistence (core/io/EntwinePersistence.cpp:271-333) as a sink: the constructor creates ept-data, ept-hierarchy and
// ept-sources under work_dir; every non-empty node becomes "ept-data/<D-X-Y-Z>.las" (the Potree name converted) through the
// LAS writer and its count is recorded; finish() -- called by the destructor if nobody did, where the reference writes them
// -- writes the ept-hierarchy files (swz_ept_hierarchy_write).  An empty range returns silently, like the reference.
// ept.json is the caller's (swz_ept_json_write), as it is the reference's tiler process's.
class EntwineSink : public LASSink {
public:
  explicit EntwineSink(std::string work_dir) : LASSink(std::move(work_dir)) {
    if (swz_ept_create_dirs(nullptr, _work_dir.c_str()) != SWZ_OK)
      throw std::runtime_error{"Could not create the ept directories under \"" + _work_dir + "\""};
  }
  ~EntwineSink() override {
    if (!_finished) {
      try {
        finish();
      } catch (...) {  // a destructor reports nothing; call finish() to see the error
      }
    }
  }
  EntwineSink(const EntwineSink&) = delete;
  EntwineSink& operator=(const EntwineSink&) = delete;

  void persist_rows(size_t count, const double* positions, const swz_attribute_columns& attributes, const AABB& node_bounds,
                    const std::string& node_name) override {
    if (count == 0) return;  // EntwinePersistence.cpp:297-298
    int8_t level = 0;
    uint64_t key = 0;
    node_from_potree_name(node_name, &level, &key);
    char name[72];
    if (swz_node_name_entwine(level, key, name) != SWZ_OK) throw std::runtime_error{"not a node name: \"" + node_name + "\""};
    write_las(_work_dir + "/ept-data/" + name + ".las", count, positions, attributes, node_bounds);
    _counts[{level, key}] = count;  // a node persisted again replaces its file and its count
  }

  // number of nodes recorded so far
  size_t num_nodes() const { return _counts.size(); }

  void finish() {
    _finished = true;
    std::vector<int8_t> level;
    std::vector<uint64_t> key, count;
    for (const auto& kv : _counts) {
      level.push_back(kv.first.first);
      key.push_back(kv.first.second);
      count.push_back(kv.second);
    }
    if (swz_ept_hierarchy_write(nullptr, _work_dir.c_str(), level.size(), level.data(), key.data(), count.data()) != SWZ_OK)
      throw std::runtime_error{"Could not write hierarchy file under \"" + _work_dir + "\""};
  }

private:
  std::map<std::pair<int8_t, uint64_t>, uint64_t> _counts;
  bool _finished = false;
};

// The shape of TilingAlgorithmBase (core/tiling/TilingAlgorithms.h:70-116): one object per Tiler, fed one batch at
// a time (Tiler.cpp:509-510), finalize() once at the end.  tile_batch() is what the single task emitted by
// build_execution_graph() runs.  Unlike the reference, which rewrites the files of every node a batch reaches
// (and re-reads them for the next batch, TilingAlgorithms.cpp:50-109), the node files live in device memory
// between the batches (swz_tiler) and each is handed to the persistence ONCE, by finalize(): same final files,
// no intermediate ones.
class TilingAlgorithmGPU {
public:
  TilingAlgorithmGPU(SamplingStrategy sampling_strategy, PointsSink& persistence, TilerMetaParameters meta,
                     int device = 0)
    : _ctx(device), _sampling_strategy(sampling_strategy), _persistence(persistence), _meta(meta) {}
  ~TilingAlgorithmGPU() { swz_tiler_destroy(_tiler); }
  TilingAlgorithmGPU(const TilingAlgorithmGPU&) = delete;
  TilingAlgorithmGPU& operator=(const TilingAlgorithmGPU&) = delete;

  // positions: n x 3 doubles of this batch (host memory; pinned memory makes the copy asynchronous);
  // bounds: the octree's (cubic) root bounds, the same for every batch
  swz_tile_stats tile_batch(const double* positions, size_t n, const AABB& bounds) { return tile_batch(positions, nullptr, n, bounds); }
  // ... with the batch's attribute columns (host memory, n rows each; the same set for every batch): they go into the
  // tiler's pools and come out in the files of write_output()
  swz_tile_stats tile_batch(const double* positions, const swz_attribute_columns& attributes, size_t n, const AABB& bounds) {
    return tile_batch(positions, &attributes, n, bounds);
  }

  // The node files and the format's metadata under `dir`, written by the library in one call (swz_tiler_write_output): packed
  // on the device straight from the pools, with the attribute columns of params.attribute_mask, chunk by chunk while the
  // chunk before is being written -- what replaces the hand-off of every node to a PointsSink.  Finalizes the tiler if
  // finalize() has not; the persistence given to the constructor is not involved.
  swz_output_stats write_output(const std::string& dir, const swz_output_params& params) {
    if (!_tiler) throw std::runtime_error{"TilingAlgorithmGPU: write_output before the first batch"};
    finalize_tiler();
    swz_output_stats stats{};
    _ctx.check(swz_tiler_write_output(_tiler, dir.c_str(), &params, &stats));
    return stats;
  }

  // dir/properties.json (write_properties_json, TilerProcess.cpp:76-151): the root box, spacing_at_root and the points added --
  // what convert_dataset, and the reference's converter, find the root of a BIN, BINZ, LAS or 3DTILES data set with.
  void write_properties(const std::string& dir) {
    if (!_tiler) throw std::runtime_error{"TilingAlgorithmGPU: write_properties before the first batch"};
    _ctx.check(swz_tiler_write_properties(_tiler, dir.c_str()));
  }

  // The boxes of the nodes' POINTS (3 doubles per node, in the order of the node table; a node without points: +inf / -inf),
  // reduced on the device from the pools (swz_tiler_node_boxes) -- what write_output() writes into the metadata when
  // params.flags carries SWZ_OUT_TIGHT_BOUNDS, instead of the octree cubes.  Finalizes the tiler if finalize() has not.
  struct NodeBoxes {
    std::vector<double> min, max;
  };
  NodeBoxes node_boxes() {
    if (!_tiler) throw std::runtime_error{"TilingAlgorithmGPU: node_boxes before the first batch"};
    finalize_tiler();
    swz_tiler_info info{};
    _ctx.check(swz_tiler_get_info(_tiler, &info));
    const uint64_t cap = info.num_nodes ? info.num_nodes : 1;
    NodeBoxes boxes{std::vector<double>(3 * cap), std::vector<double>(3 * cap)};
    uint64_t got = 0;
    _ctx.check(swz_tiler_node_boxes(_tiler, cap, boxes.min.data(), boxes.max.data(), &got));
    boxes.min.resize(3 * got);
    boxes.max.resize(3 * got);
    return boxes;
  }

  // A data set of uncompressed LAS files, read by the library in one call (swz_tiler_add_las_files): headers scanned, files
  // cut into batches of params.batch_points points, raw records read by reader threads, copied and decoded on the device
  // straight into the tiler's pools, every batch tiled while the next is read -- what replaces MultiReaderPointSource and
  // the tile_batch loop for files that need neither a PROJ transformation nor LASzip.  bounds: the octree's root bounds,
  // the data set's cubic box (swz_las_scan_files), or that box at the origin with params.shift_to_center.
  // projection (may be null): the files are in that source projection and are tiled in ECEF; bounds is then a box of
  // swz_las_scan_files_srs.  It can only come with the call that brings the first points.
  swz_input_stats add_las_files(const std::vector<std::string>& paths, const AABB& bounds, const swz_input_params& params,
                                const SourceProjection* projection = nullptr) {
    if (_finalized || _tiler_finalized) throw std::runtime_error{"TilingAlgorithmGPU: add_las_files after finalize"};
    open_tiler(bounds);
    if (projection) _ctx.check(swz_tiler_set_source_srs(_tiler, projection->srs()));
    std::vector<const char*> names;
    for (const std::string& p : paths) names.push_back(p.c_str());
    swz_input_stats stats{};
    _ctx.check(swz_tiler_add_las_files(_tiler, names.data(), names.size(), &params, &stats));
    return stats;
  }

private:
  void open_tiler(const AABB& bounds) {
    if (_tiler) return;
    swz_tile_params p{};
    p.sampler = _sampling_strategy.kind;
    p.max_points_per_node = _sampling_strategy.max_points_per_node;
    p.spacing_at_root = _meta.spacing_at_root;
    p.max_depth = _meta.max_depth;
    p.strategy = _meta.tiling_strategy == TilingStrategy::Fast ? SWZ_FAST : SWZ_ACCURATE;
    p.fast_concurrency = _meta.num_indexing_threads;
    const double mn[3] = {bounds.min.x, bounds.min.y, bounds.min.z}, mx[3] = {bounds.max.x, bounds.max.y, bounds.max.z};
    _ctx.check(swz_tiler_create(_ctx.get(), mn, mx, &p, 0, &_tiler));
    _bounds = bounds;
  }
  void finalize_tiler() {
    if (_tiler_finalized) return;
    swz_tile_stats stats{};
    _ctx.check(swz_tiler_finalize(_tiler, &stats));
    _tiler_finalized = true;
  }
  swz_tile_stats tile_batch(const double* positions, const swz_attribute_columns* attributes, size_t n, const AABB& bounds) {
    if (_finalized || _tiler_finalized) throw std::runtime_error{"TilingAlgorithmGPU: tile_batch after finalize"};
    open_tiler(bounds);
    swz_tile_stats stats{};
    _ctx.check(swz_tiler_add_batch(_tiler, positions, n, attributes, &stats));
    return stats;
  }

public:

  // TilingAlgorithmBase::finalize (FAST: reconstruct_left_out_nodes), then every node file goes to the persistence.
  // Returns the number of nodes persisted.
  size_t finalize(const AABB&) {
    if (!_tiler || _finalized) return 0;
    _finalized = true;
    finalize_tiler();
    swz_tiler_info info{};
    _ctx.check(swz_tiler_get_info(_tiler, &info));
    const uint64_t ns = info.num_stored, nn = info.num_nodes;
    if (ns == 0) return 0;
    // The ids of all files in node order (4 bytes per stored point), then the files in CHUNKS of whole nodes: positions
    // gathered by id on the device, copied, handed to the persistence -- host and device hold ns * 4 + chunk * 24 bytes
    // instead of all ns * 28 at once, and the persistence starts writing while later chunks are still on the device.
    DeviceBuffer ids_buf(ns * 4);
    uint32_t* d_ids = static_cast<uint32_t*>(ids_buf.ptr);
    _ctx.check(swz_tiler_export_device(_tiler, nullptr, d_ids, nullptr));
    const double* pool = nullptr;
    _ctx.check(swz_tiler_pools_device(_tiler, &pool, nullptr));
    std::vector<uint32_t> ids(ns);
    _ctx.check(swz_copy_to_host(_ctx.get(), ids.data(), d_ids, ns * 4));
    std::vector<int8_t> nl(nn);
    std::vector<uint64_t> nk(nn), no(nn), nc(nn);
    uint64_t got = 0;
    _ctx.check(swz_tiler_node_table(_tiler, nn, nl.data(), nk.data(), no.data(), nc.data(), &got));
    uint64_t largest = 0;
    for (uint64_t j = 0; j < got; ++j) largest = std::max<uint64_t>(largest, nc[j]);
    const uint64_t chunk_cap = std::max<uint64_t>(std::max<uint64_t>(_export_chunk_points, 1), largest);
    DeviceBuffer xyz_buf(std::min(chunk_cap, ns) * 24);
    std::vector<double> xyz(std::min(chunk_cap, ns) * 3);
    for (uint64_t j0 = 0; j0 < got;) {
      uint64_t j1 = j0, cnt = 0;  // nodes [j0, j1): consecutive files, stored back to back from no[j0] on
      while (j1 < got && cnt + nc[j1] <= chunk_cap) cnt += nc[j1++];
      if (cnt) {
        _ctx.check(swz_gather_payload_device(_ctx.get(), d_ids + no[j0], nullptr, cnt, pool, nullptr, static_cast<double*>(xyz_buf.ptr),
                                             nullptr));
        _ctx.check(swz_copy_to_host(_ctx.get(), xyz.data(), xyz_buf.ptr, cnt * 24));
      }
      for (uint64_t j = j0; j < j1; ++j) {
        std::string name = "r";  // node names: "r" + octant digits, TilingAlgorithms.cpp:139
        AABB b = _bounds;
        for (int l = 0; l <= nl[j]; ++l) {
          const uint8_t o = get_octant_at_level(nk[j], static_cast<uint32_t>(l));
          name.push_back(static_cast<char>('0' + o));
          b = get_octant_bounds(o, b);
        }
        _persistence.persist_points(ids.data() + no[j], ids.data() + no[j] + nc[j], xyz.data() + 3 * (no[j] - no[j0]), b, name);
      }
      j0 = j1;
    }
    return static_cast<size_t>(got);
  }

  swz_tiler_info info() {
    swz_tiler_info i{};
    if (_tiler) _ctx.check(swz_tiler_get_info(_tiler, &i));
    return i;
  }
  // stored points per export chunk of finalize() (whole node files; at least the largest file)
  void set_export_chunk_points(uint64_t n) { _export_chunk_points = n; }
  // swz_set_option on the tiler's own context (value NULL removes the switch): the spill and budget options of the
  // pools (SWZ_TILER_SPILL, SWZ_TILER_DEVICE_BUDGET_MB) are read when a pool grows, so set them before the first batch
  void set_option(const char* name, const char* value) { _ctx.check(swz_set_option(_ctx.get(), name, value)); }

private:
  struct DeviceBuffer {  // device scratch through the ABI (no HIP headers needed by the host code)
    void* ptr = nullptr;
    explicit DeviceBuffer(uint64_t bytes) {
      if (swz_device_alloc(bytes, &ptr) != SWZ_OK) throw std::runtime_error{"swz_device_alloc failed"};
    }
    ~DeviceBuffer() { swz_device_free(ptr); }
  };

  Context _ctx;
  SamplingStrategy _sampling_strategy;
  PointsSink& _persistence;
  TilerMetaParameters _meta;
  swz_tiler* _tiler = nullptr;
  AABB _bounds;
  bool _finalized = false;        // finalize() has handed the files to the persistence
  bool _tiler_finalized = false;  // swz_tiler_finalize has run (finalize() or write_output())
  uint64_t _export_chunk_points = 16u << 20;
};

// One batch over several GPUs from this one process (swz_group_*): the batch is cut into equal pieces in input
// order, one per GPU, the library exchanges the points (and their attribute columns) by level-0 octant, tiles, and
// every shard hands the files of its subtrees to the persistence; the root node's file is the concatenation of the
// shards' parts in shard order (= Morton order).  transport: 0 peer copies, 1 RCCL.
class ShardedTilingAlgorithmGPU {
public:
  ShardedTilingAlgorithmGPU(SamplingStrategy sampling_strategy, PointsSink& persistence, TilerMetaParameters meta,
                            const std::vector<int>& devices, int transport = 0)
    : _sampling_strategy(sampling_strategy), _persistence(persistence), _meta(meta), _shards(static_cast<int>(devices.size())) {
    if (swz_group_create(_shards, devices.data(), transport, &_group) != SWZ_OK)
      throw std::runtime_error{std::string("swz_group_create: ") + swz_group_last_error(nullptr)};
  }
  ~ShardedTilingAlgorithmGPU() { swz_group_destroy(_group); }
  ShardedTilingAlgorithmGPU(const ShardedTilingAlgorithmGPU&) = delete;
  ShardedTilingAlgorithmGPU& operator=(const ShardedTilingAlgorithmGPU&) = delete;

  // positions: n x 3 doubles, attributes: host columns of n rows (may be NULL).  Returns the number of node files.
  size_t tile_batch(const double* positions, const swz_attribute_columns* attributes, size_t n, const AABB& bounds) {
    swz_tile_params p{};
    p.sampler = _sampling_strategy.kind;
    p.max_points_per_node = _sampling_strategy.max_points_per_node;
    p.spacing_at_root = _meta.spacing_at_root;
    p.max_depth = _meta.max_depth;
    p.strategy = SWZ_ACCURATE;
    const double mn[3] = {bounds.min.x, bounds.min.y, bounds.min.z}, mx[3] = {bounds.max.x, bounds.max.y, bounds.max.z};
    std::vector<std::vector<Scratch>> owned(_shards);
    std::vector<double*> d_xyz(_shards, nullptr);
    std::vector<swz_attribute_columns> d_attrs(_shards);
    std::vector<uint64_t> cnt(_shards, 0);
    for (int s = 0; s < _shards; ++s) {
      const size_t lo = n * s / _shards, hi = n * (s + 1) / _shards;
      cnt[s] = hi - lo;
      swz_ctx* c = swz_group_ctx(_group, s);
      d_attrs[s] = swz_attribute_columns{};
      d_xyz[s] = static_cast<double*>(upload(owned[s], c, positions + 3 * lo, cnt[s] * 24));
      for (int t = 0; t < SWZ_ATTR_COUNT; ++t)
        if (attributes && attributes->column[t]) {
          const uint32_t rb = swz_attribute_row_bytes(t);
          d_attrs[s].column[t] = upload(owned[s], c, static_cast<const char*>(attributes->column[t]) + lo * rb, cnt[s] * rb);
        }
    }
    std::vector<swz_group_result> res(_shards);
    if (swz_group_tile(_group, d_xyz.data(), attributes ? d_attrs.data() : nullptr, cnt.data(), mn, mx, &p, res.data()) != SWZ_OK)
      throw std::runtime_error{std::string("swz_group_tile: ") + swz_group_last_error(_group)};

    // node files: per shard on its device, the root's parts joined afterwards
    size_t files = 0;
    std::vector<double> root_xyz;
    std::vector<std::vector<char>> root_attr(SWZ_ATTR_COUNT);
    for (int s = 0; s < _shards; ++s) {
      const uint64_t m = res[s].num_points;
      if (!m) continue;
      swz_ctx* c = swz_group_ctx(_group, s);
      std::vector<Scratch> tmp;
      uint32_t* d_order = static_cast<uint32_t*>(alloc(tmp, c, m * 4));
      std::vector<int8_t> nl(m);
      std::vector<uint64_t> nk(m), no(m), nc(m);
      uint64_t nn = 0;
      check(c, swz_build_node_lists_device(c, res[s].d_keys, res[s].d_level, m, d_order, m, nl.data(), nk.data(), no.data(), nc.data(), &nn));
      double* d_rows = static_cast<double*>(alloc(tmp, c, m * 24));
      swz_attribute_columns d_out{}, h_out{};
      std::vector<std::vector<char>> host_cols(SWZ_ATTR_COUNT);
      for (int t = 0; t < SWZ_ATTR_COUNT; ++t)
        if (res[s].attrs.column[t]) d_out.column[t] = alloc(tmp, c, m * swz_attribute_row_bytes(t));
      check(c, swz_gather_payload_device(c, res[s].d_perm, d_order, m, res[s].d_xyz, &res[s].attrs, d_rows, &d_out));
      std::vector<double> rows(m * 3);
      check(c, swz_copy_to_host(c, rows.data(), d_rows, m * 24));
      for (int t = 0; t < SWZ_ATTR_COUNT; ++t)
        if (d_out.column[t]) {
          host_cols[t].resize(m * swz_attribute_row_bytes(t));
          check(c, swz_copy_to_host(c, host_cols[t].data(), d_out.column[t], host_cols[t].size()));
        }
      for (uint64_t j = 0; j < nn; ++j) {
        if (nl[j] < 0) {  // this shard's part of the root
          root_xyz.insert(root_xyz.end(), rows.begin() + 3 * no[j], rows.begin() + 3 * (no[j] + nc[j]));
          for (int t = 0; t < SWZ_ATTR_COUNT; ++t)
            if (d_out.column[t]) {
              const uint32_t rb = swz_attribute_row_bytes(t);
              root_attr[t].insert(root_attr[t].end(), host_cols[t].begin() + no[j] * rb, host_cols[t].begin() + (no[j] + nc[j]) * rb);
            }
          continue;
        }
        std::string name = "r";
        AABB b = bounds;
        for (int l = 0; l <= nl[j]; ++l) {
          const uint8_t o = get_octant_at_level(nk[j], static_cast<uint32_t>(l));
          name.push_back(static_cast<char>('0' + o));
          b = get_octant_bounds(o, b);
        }
        for (int t = 0; t < SWZ_ATTR_COUNT; ++t)
          h_out.column[t] = d_out.column[t] ? host_cols[t].data() + no[j] * swz_attribute_row_bytes(t) : nullptr;
        _persistence.persist_rows(nc[j], rows.data() + 3 * no[j], h_out, b, name);
        ++files;
      }
    }
    if (!root_xyz.empty()) {
      swz_attribute_columns h_out{};
      for (int t = 0; t < SWZ_ATTR_COUNT; ++t) h_out.column[t] = root_attr[t].empty() ? nullptr : root_attr[t].data();
      _persistence.persist_rows(root_xyz.size() / 3, root_xyz.data(), h_out, bounds, "r");
      ++files;
    }
    return files;
  }

  // ---- a data set in several batches on the group's tilers (swz_group_tiler_open ... swz_group_write_output): what
  // TilingAlgorithmGPU's tile_batch / write_output are on one GPU.  The persistence is not involved.
  // bounds: the octree's (cubic) root bounds; strategy: SWZ_ACCURATE or SWZ_FAST (fast_concurrency = num_indexing_threads)
  void open_tiler(const AABB& bounds, int strategy = SWZ_ACCURATE) {
    swz_tile_params p{};
    p.sampler = _sampling_strategy.kind;
    p.max_points_per_node = _sampling_strategy.max_points_per_node;
    p.spacing_at_root = _meta.spacing_at_root;
    p.max_depth = _meta.max_depth;
    p.strategy = strategy;
    p.fast_concurrency = _meta.num_indexing_threads;
    const double mn[3] = {bounds.min.x, bounds.min.y, bounds.min.z}, mx[3] = {bounds.max.x, bounds.max.y, bounds.max.z};
    group_check(swz_group_tiler_open(_group, mn, mx, &p, 0), "swz_group_tiler_open");
    _tiler_finalized = false;
  }
  // host rows cut into equal consecutive pieces, one per shard, as tile_batch does; attributes may be NULL
  void add_batch(const double* positions, const swz_attribute_columns* attributes, size_t n) {
    if (_tiler_finalized) throw std::runtime_error{"ShardedTilingAlgorithmGPU: add_batch after finalize_tiler"};
    std::vector<std::vector<Scratch>> owned(_shards);
    std::vector<double*> d_xyz(_shards, nullptr);
    std::vector<swz_attribute_columns> d_attrs(_shards);
    std::vector<uint64_t> cnt(_shards, 0);
    for (int s = 0; s < _shards; ++s) {
      const size_t lo = n * s / _shards, hi = n * (s + 1) / _shards;
      cnt[s] = hi - lo;
      swz_ctx* c = swz_group_ctx(_group, s);
      d_attrs[s] = swz_attribute_columns{};
      d_xyz[s] = static_cast<double*>(upload(owned[s], c, positions + 3 * lo, cnt[s] * 24));
      for (int t = 0; t < SWZ_ATTR_COUNT; ++t)
        if (attributes && attributes->column[t]) {
          const uint32_t rb = swz_attribute_row_bytes(t);
          d_attrs[s].column[t] = upload(owned[s], c, static_cast<const char*>(attributes->column[t]) + lo * rb, cnt[s] * rb);
        }
    }
    group_check(swz_group_add_batch(_group, d_xyz.data(), attributes ? d_attrs.data() : nullptr, cnt.data(), nullptr), "swz_group_add_batch");
  }
  // A data set of uncompressed LAS files, read by the library in one call (swz_group_add_las_files) into the tilers that
  // open_tiler() opened; as TilingAlgorithmGPU::add_las_files it does not finalize
  swz_input_stats add_las_files(const std::vector<std::string>& paths, const swz_input_params& params,
                                const SourceProjection* projection = nullptr) {
    if (_tiler_finalized) throw std::runtime_error{"ShardedTilingAlgorithmGPU: add_las_files after finalize_tiler"};
    if (projection) group_check(swz_group_set_source_srs(_group, projection->srs()), "swz_group_set_source_srs");
    std::vector<const char*> names;
    for (const std::string& p : paths) names.push_back(p.c_str());
    swz_input_stats stats{};
    group_check(swz_group_add_las_files(_group, names.data(), names.size(), &params, &stats), "swz_group_add_las_files");
    return stats;
  }
  void finalize_tiler() {
    if (_tiler_finalized) return;
    group_check(swz_group_finalize(_group, nullptr), "swz_group_finalize");
    _tiler_finalized = true;
  }
  // the data set's directory, written by the library in one call (swz_group_write_output); finalizes if finalize_tiler() has not
  swz_output_stats write_output(const std::string& dir, const swz_output_params& params) {
    finalize_tiler();
    swz_output_stats total{};
    group_check(swz_group_write_output(_group, dir.c_str(), &params, nullptr, &total), "swz_group_write_output");
    return total;
  }
  // the boxes of the nodes' points in the order of swz_group_node_table (swz_group_node_boxes); see TilingAlgorithmGPU::node_boxes
  TilingAlgorithmGPU::NodeBoxes node_boxes() {
    finalize_tiler();
    uint64_t nn = 0;
    group_check(swz_group_node_table(_group, 0, nullptr, nullptr, nullptr, nullptr, &nn), "swz_group_node_table");
    const uint64_t cap = nn ? nn : 1;
    TilingAlgorithmGPU::NodeBoxes boxes{std::vector<double>(3 * cap), std::vector<double>(3 * cap)};
    group_check(swz_group_node_boxes(_group, cap, boxes.min.data(), boxes.max.data(), &nn), "swz_group_node_boxes");
    boxes.min.resize(3 * nn);
    boxes.max.resize(3 * nn);
    return boxes;
  }

private:
  void group_check(int status, const char* call) const {
    if (status != SWZ_OK) throw std::runtime_error{std::string(call) + ": " + swz_group_last_error(_group)};
  }
  bool _tiler_finalized = false;
  struct Scratch {
    void* ptr = nullptr;
    Scratch() = default;
    Scratch(Scratch&& o) noexcept : ptr(o.ptr) { o.ptr = nullptr; }
    Scratch(const Scratch&) = delete;
    ~Scratch() { swz_device_free(ptr); }
  };
  static void* alloc(std::vector<Scratch>& owner, swz_ctx* c, uint64_t bytes) {
    Scratch s;
    if (swz_device_alloc_on(c, bytes ? bytes : 1, &s.ptr) != SWZ_OK) throw std::runtime_error{"swz_device_alloc_on failed"};
    void* p = s.ptr;
    owner.push_back(std::move(s));
    return p;
  }
  static void check(swz_ctx* c, int status) {
    if (status != SWZ_OK) throw std::runtime_error{std::string("swz: ") + swz_last_error(c)};
  }
  static void* upload(std::vector<Scratch>& owner, swz_ctx* c, const void* src, uint64_t bytes) {
    void* d = alloc(owner, c, bytes);
    if (bytes) check(c, swz_copy_to_device(c, d, src, bytes));
    return d;
  }

  SamplingStrategy _sampling_strategy;
  PointsSink& _persistence;
  TilerMetaParameters _meta;
  int _shards;
  swz_group* _group = nullptr;
};

}  // namespace swz_host
