// swz_query.hip -- a written data set queried by box and depth (swz_dataset_query_nodes, swz_dataset_query) or by a region,
// the box cut by planes or by a polygon in x-y (swz_dataset_query_region_nodes, swz_dataset_query_region).  The source is
// opened as the converter opens it (source_open, swz_source.hip), the nodes whose widened boxes miss the query box or cannot
// hold a row of the region drop out of the table (host only), and the rest is streamed chunk by chunk with the converter's SourceStream: every chunk's
// chunk-local positions and columns go through the selection kernel (swz_select.hip) into the caller's arrays at the running
// offset.  The readers of chunk j + 1 run while chunk j is selected.  With a filter (swz_dataset_query_filtered) the stream
// unpacks the caller's columns and the filter's, and the selection reads the latter.  Where the directory holds
// node-summaries.swz (swz_dataset_summarize, below, writes it with the kernel of swz_summary.hip) the nodes that no row of
// which can pass a clause are neither read nor chunked (filter_reads: the node rule of a filter).
#include <chrono>
#include <cmath>
#include <cstddef>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "swz_convert.h"
#include "swz_hostio.h"
#include "swz_select.h"
#include "swz_summary.h"
#include "swz_toutput.h"

static_assert(sizeof(swz_query_params) == 72 && offsetof(swz_query_params, max_depth) == 48 && offsetof(swz_query_params, chunk_points) == 64 &&
                sizeof(swz_query_stats) == 88 && offsetof(swz_query_stats, read_ms) == 48,
              "the structs of the query as include/swz_gpu.h and the bindings lay them out");

namespace swz {

static double ms_since(std::chrono::steady_clock::time_point t0) {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// per selected row of a chunk its node: the last node of the chunk whose first row is not behind the row (nodes without
// points share their first row with the node behind them); node_index: the chunk's nodes as indices of the query's table
__global__ __launch_bounds__(256) void query_row_nodes_kernel(const uint32_t* __restrict__ rows, uint32_t cnt, const uint32_t* __restrict__ node_first,
                                                              uint32_t nodes, const uint32_t* __restrict__ node_index,
                                                              uint32_t* __restrict__ node_out) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= cnt) return;
  const uint32_t r = rows[i];
  uint32_t lo = 0, hi = nodes;  // node_first[lo] <= r < node_first[hi] (node_first[nodes]: the chunk's rows)
  while (hi - lo > 1u) {
    const uint32_t mid = (lo + hi) >> 1;
    if (node_first[mid] <= r) lo = mid;
    else hi = mid;
  }
  node_out[i] = node_index[lo];
}

// ---- the node rule of a region, on the node's widened box [lo, hi] (every room term of the box rule already in it)

// Planes.  The kernel evaluates f^(p) = ((a*x + b*y) + c*z) + d in four rounded operations.  With u = 2^-53 a term passes
// through four roundings at the most (a*x: its product and three sums), so |f^(p) - f(p)| <= g4 S(p) with g4 = 4u / (1 - 4u)
// and S(p) = |a||x| + |b||y| + |c||z| + |d| (the usual bound of a recursive sum).  Over the box, f(p) <= F = f(corner), the
// corner the coefficients' signs choose, and S(p) <= S = |a| max|x| + ... + |d|.  The host evaluates F^ at that corner the
// same way, |F^ - F| <= g4 S.  Hence f^(p) <= F^ + 2 g4 S for every p of the box, and 2 g4 < 8u = 4 eps; the rule takes
// 8 eps S (the rounding of S and of the product itself lies far inside the spare factor) and the smallest normal double for
// products that underflow.  A node is dropped iff F^ + that bound < 0 for some plane.
static bool planes_miss(const RegionHost& r, const double lo[3], const double hi[3]) {
  const double eps = std::numeric_limits<double>::epsilon();
  for (uint32_t k = 0; k < r.count; ++k) {
    const double* p = &r.v[4 * k];
    double at[3], s = std::fabs(p[3]);
    for (int a = 0; a < 3; ++a) {
      at[a] = p[a] >= 0.0 ? hi[a] : lo[a];
      s += std::fabs(p[a]) * std::max(std::fabs(lo[a]), std::fabs(hi[a]));
    }
    const double f = ((p[0] * at[0] + p[1] * at[1]) + p[2] * at[2]) + p[3];
    if (f + (8.0 * eps * s + std::numeric_limits<double>::min()) < 0.0) return true;
  }
  return false;
}

// does the segment touch the closed rectangle?  Separating axes: x, y and the segment's normal (the four corners strictly on
// one side of its line).  The side is the sign of a cross product computed in double; a value within its own rounding
// (8 eps of the sum of its two products' magnitudes) counts as touching.
static bool segment_touches(double x0, double y0, double x1, double y1, const double lo[2], const double hi[2]) {
  if (std::max(x0, x1) < lo[0] || std::min(x0, x1) > hi[0] || std::max(y0, y1) < lo[1] || std::min(y0, y1) > hi[1]) return false;
  const double eps = std::numeric_limits<double>::epsilon();
  const double dx = x1 - x0, dy = y1 - y0;
  int above = 0, below = 0;
  for (int corner = 0; corner < 4; ++corner) {
    const double cx = (corner & 1) ? hi[0] : lo[0], cy = (corner & 2) ? hi[1] : lo[1];
    const double m0 = dx * (cy - y0), m1 = (cx - x0) * dy;
    const double t = m0 - m1, tol = 8.0 * eps * (std::fabs(m0) + std::fabs(m1));
    if (t > tol) ++above;
    else if (t < -tol) ++below;
  }
  return !(above == 4 || below == 4);
}

// Polygon.  Where no edge touches a rectangle the exact parity is one value over all of it, the centre's.  The kernel's
// parity of a row differs from the exact one only if an edge whose y range holds the row has the wrong sign of t there; t is
// off by at most 3 eps (|x1 - x0||py - y0| + |px - x0||y1 - y0|) and |py - y0| <= |y1 - y0| for such an edge, so the row lies
// within 3 eps (|x1 - x0| + |px - x0|) of the edge along x: less than 12 eps of the largest |x| in play.  The rectangle is
// therefore widened once more, by 32 eps of the largest coordinate of the rectangle and the outline on either axis; then no
// edge touching it means every row of the node gets the centre's parity, by the formula as by the exact rule.
static bool polygon_misses(const RegionHost& r, const double lo[3], const double hi[3]) {
  const double eps = std::numeric_limits<double>::epsilon();
  double big = 0;
  for (int a = 0; a < 2; ++a) big = std::max(big, std::max(std::fabs(lo[a]), std::fabs(hi[a])));
  for (double v : r.v) big = std::max(big, std::fabs(v));
  const double more = 32.0 * eps * big;
  const double wlo[2] = {lo[0] - more, lo[1] - more}, whi[2] = {hi[0] + more, hi[1] + more};
  const uint32_t m = r.count;
  for (uint32_t i = 0; i < m; ++i) {
    const uint32_t j = (i + 1) % m;
    if (segment_touches(r.v[2 * i], r.v[2 * i + 1], r.v[2 * j], r.v[2 * j + 1], wlo, whi)) return false;
  }
  return !region_polygon_inside(r, lo[0] + 0.5 * (hi[0] - lo[0]), lo[1] + 0.5 * (hi[1] - lo[1]));
}

// The table a query reads: `kept` holds the nodes of the (depth-limited) scan whose widened boxes meet the query box and can
// hold a row of the region, in the scan's order; *scanned: the nodes of the scan; *region_out: the region, checked;
// *filter_attrs: the mask of the columns the filter (NULL: none) reads.  No node drops out for a filter here: filter_reads.
static int query_plan(swz_ctx* c, const char* who, const char* dir, const swz_query_params* q, const swz_region* region, const swz_filter* filter,
                      DatasetScan* kept, uint64_t* scanned, RegionHost* region_out, uint32_t* filter_attrs) {
  auto refuse = [&](const std::string& what) { return fail(c, SWZ_ERR_BAD_ARG, std::string(who) + ": " + what); };
  if (!dir || !q) return refuse("NULL argument");
  if (!finite3(q->box_min) || !finite3(q->box_max)) return refuse("a bound of the box is not finite");
  for (int a = 0; a < 3; ++a)
    if (q->box_min[a] > q->box_max[a]) return refuse("box_min > box_max");
  if (q->source_flags & ~(uint32_t)SWZ_CONVERT_LOSSY_SOURCE) return refuse("an unknown bit in source_flags");
  if (q->reserved) return refuse("reserved must be 0");
  SWZ_TRY(region_check(c, who, region, region_out));  // (before any file is read)
  SWZ_TRY(filter_check(c, who, filter, filter_attrs));
  const uint32_t fattrs = *filter_attrs;
  const RegionHost& rh = *region_out;
  DatasetScan scan;
  double rtc[3];
  SWZ_TRY(source_open(c, who, dir, q->max_depth, q->source_flags, &scan, rtc));
  // the filter's columns: known from the scan (and, for .pnts, from what the format carries), before a node file is opened
  for (int a = 0; a < SWZ_ATTR_COUNT; ++a) {
    if (!((fattrs >> a) & 1u)) continue;
    if (scan.info.format == SWZ_OUT_3DTILES && a != SWZ_ATTR_INTENSITY)
      return refuse(std::string("the filter names ") + attribute_name(a) + ", which .pnts files do not carry (a 3DTILES source holds RGB and intensity)");
    if (!((scan.info.attribute_mask >> a) & 1u)) {
      char hex[16];
      snprintf(hex, sizeof(hex), "0x%x", scan.info.attribute_mask);
      return refuse(std::string("the filter names ") + attribute_name(a) + ", which the source does not hold (its attribute mask is " + hex + ")");
    }
  }
  if (scan.info.root_source == SWZ_DATASET_ROOT_ABSENT)
    return refuse("no root box: the source has neither properties.json nor ept.json");
  const double* rmin = scan.info.root_min;
  const double* rmax = scan.info.root_max;
  if (!finite3(rmin) || !finite3(rmax)) return refuse("the root box of the source is not finite");
  const int format = scan.info.format;
  const bool las = format == SWZ_OUT_LAS || format == SWZ_OUT_ENTWINE_LAS;
  const bool pnts = format == SWZ_OUT_3DTILES;
  const uint64_t nn = scan.count.size();
  *scanned = nn;
  *kept = DatasetScan{};
  kept->info = scan.info;
  kept->info.points = 0;
  for (uint64_t k = 0; k < nn; ++k) {
    double lo[3], hi[3];
    if (swz_node_bounds(scan.level[k], scan.key[k], rmin, rmax, lo, hi) != SWZ_OK) return refuse("no box for the node " + scan.path[k]);
    bool meets = true;
    double wlo[3], whi[3];  // the widened box, for the region's rule
    for (int a = 0; a < 3; ++a) {
      // a point lies in the node of its KEY: two key cells cover the rounding of the cell edges against the halved boxes,
      // four ulps of the largest bound the rounding of the bounds themselves
      const double big = std::max(std::max(std::fabs(rmin[a]), std::fabs(rmax[a])), std::max(std::fabs(lo[a]), std::fabs(hi[a])));
      double room = std::ldexp(std::fabs(rmax[a] - rmin[a]), -20) + 4 * std::numeric_limits<double>::epsilon() * big;
      if (las) room += std::fabs(scan.layout[k].scale[a]);  // stored on the scale's grid: half a step off at the most
      if (pnts) {  // stored as floats relative to RTC_CENTER
        lo[a] -= rtc[a];
        hi[a] -= rtc[a];
        room += std::ldexp(std::max(std::fabs(lo[a]), std::fabs(hi[a])), -23) + 4 * std::numeric_limits<double>::epsilon() * std::fabs(rtc[a]);
      }
      if (!(lo[a] - room <= q->box_max[a] && q->box_min[a] <= hi[a] + room)) meets = false;
      wlo[a] = lo[a] - room;
      whi[a] = hi[a] + room;
    }
    if (!meets) continue;
    if (rh.kind == SWZ_REGION_PLANES && planes_miss(rh, wlo, whi)) continue;
    if (rh.kind == SWZ_REGION_POLYGON && polygon_misses(rh, wlo, whi)) continue;
    kept->level.push_back(scan.level[k]);
    kept->key.push_back(scan.key[k]);
    kept->count.push_back(scan.count[k]);
    kept->path.push_back(scan.path[k]);
    kept->layout.push_back(scan.layout[k]);
    kept->data_at.push_back(scan.data_at[k]);
    if (pnts) kept->file_bytes.push_back(scan.file_bytes[k]);
    kept->info.points += scan.count[k];
  }
  kept->info.num_nodes = kept->count.size();
  return SWZ_OK;
}

// ---- the node rule of a filter, on the summaries of node-summaries.swz

// has the node no row that could pass the clause?  Judged from the entry of the clause's attribute alone.
static bool clause_unreachable(const swz_filter_clause& cl, const swz_attr_summary& e) {
  const bool negate = (cl.kind & SWZ_FILTER_NOT) != 0u;
  if (ATTR_BYTES[cl.attribute] == 1) {  // exact: P is the set of byte values the clause's test accepts
    const bool set = (cl.kind & 0xFFu) == SWZ_FILTER_SET, is_signed = cl.attribute == SWZ_ATTR_SCAN_ANGLE_RANK;
    for (int b = 0; b < 256; ++b) {
      if (!((e.set[b >> 6] >> (b & 63)) & 1ull)) continue;
      const double v = is_signed ? (double)(int8_t)(uint8_t)b : (double)b;
      const bool pass = set ? ((cl.set[b >> 6] >> (b & 63)) & 1ull) != 0 : (cl.lo <= v && v <= cl.hi);
      if (pass != negate) return false;
    }
    return true;
  }
  if (!negate) return e.hi < cl.lo || e.lo > cl.hi;  // (a node without non-NaN values: hi = -inf)
  return !(e.flags & SWZ_SUMMARY_HAS_NAN) && cl.lo <= e.lo && e.hi <= cl.hi;  // every value inside the range, and no NaN passes
}

// read->at(k) = 0 for the nodes of `kept` the filter cannot reach; all 1 without a filter or without a sidecar in dir.  A
// sidecar that does not describe the scan is refused.
static int filter_reads(swz_ctx* c, const char* who, const char* dir, const DatasetScan& kept, const swz_filter* filter,
                        std::vector<uint8_t>* read) {
  const uint64_t nn = kept.count.size();
  read->assign(nn, 1);
  if (!filter || !filter->count) return SWZ_OK;
  Sidecar side;
  std::string why;
  if (sidecar_read(dir, &side, &why) != SWZ_OK)
    return fail(c, SWZ_ERR_BAD_ARG, std::string(who) + ": " + why + " -- run swz_dataset_summarize again");
  if (!side.present) return SWZ_OK;
  auto stale = [&](const std::string& what) {
    return fail(c, SWZ_ERR_BAD_ARG, std::string(who) + ": node-summaries.swz is stale: " + what + " -- run swz_dataset_summarize again");
  };
  if (side.format != kept.info.format)
    return stale("the data set's format is " + std::to_string(kept.info.format) + ", the summary's " + std::to_string(side.format));
  uint64_t at = 0;  // both tables ascend by (level, Morton index)
  const uint64_t sn = side.key.size();
  for (uint64_t k = 0; k < nn; ++k) {
    const int8_t level = kept.level[k];
    const uint64_t key = kept.key[k];
    while (at < sn && (side.level[at] != level ? side.level[at] < level : side.key[at] < key)) ++at;
    char name[24] = "?";
    (void)swz_node_name(level, key, name);
    if (at == sn || side.level[at] != level || side.key[at] != key) return stale(std::string("node ") + name + " is not in the summary");
    if (side.count[at] != kept.count[k])
      return stale(std::string("node ") + name + " holds " + std::to_string(kept.count[k]) + " points, the summary " + std::to_string(side.count[at]));
    for (uint32_t q = 0; q < filter->count && (*read)[k]; ++q) {
      const swz_filter_clause& cl = filter->clause[q];
      if (!((side.mask >> cl.attribute) & 1u)) continue;  // not summarised: the clause drops nothing
      const uint32_t j = (uint32_t)__builtin_popcount(side.mask & ((1u << cl.attribute) - 1u));
      if (clause_unreachable(cl, side.entries[at * side.cols + j])) (*read)[k] = 0;
    }
  }
  return SWZ_OK;
}

struct CopyStream {
  hipStream_t s = nullptr;
  ~CopyStream() {
    if (s) (void)hipStreamDestroy(s);
  }
};

static int query(swz_ctx* c, const char* who, const char* dir, const swz_query_params* q, const swz_region* region, const swz_filter* filter,
                 uint64_t capacity, double* d_xyz_out, const swz_attribute_columns* d_out, uint32_t* d_node_out, uint64_t* count_out,
                 swz_query_stats* stats) {
  auto refuse = [&](const std::string& what) { return c->fail(SWZ_ERR_BAD_ARG, std::string(who) + ": " + what); };
  const auto t_wall = std::chrono::steady_clock::now();
  if (stats) *stats = swz_query_stats{};
  if (!count_out) return refuse("NULL argument");
  *count_out = 0;
  DatasetScan kept;
  uint64_t scanned = 0;
  RegionHost region_host;
  uint32_t fattrs = 0;  // the columns the filter reads: unpacked for it, handed to the caller only if the mask names them too
  SWZ_TRY(query_plan(c, who, dir, q, region, filter, &kept, &scanned, &region_host, &fattrs));
  const bool count_only = !d_xyz_out && capacity == 0;
  if (!d_xyz_out && !count_only) return refuse("NULL d_xyz_out with a capacity (count only: NULL and capacity 0)");
  uint32_t mask = q->attribute_mask == ~0u ? kept.info.attribute_mask : q->attribute_mask;
  if (mask & ~kept.info.attribute_mask) return refuse("the attribute_mask names a column the source does not hold");
  if (count_only) mask = 0;  // positions decide
  for (int a = 0; a < SWZ_ATTR_COUNT; ++a)
    if (((mask >> a) & 1u) && (!d_out || !d_out->column[a])) return refuse("a bit of the mask without an output column");
  SWZ_HIP(c, hipSetDevice(c->device));

  // ---- the nodes that are read: all of the kept table, or those the filter can reach by the directory's summaries; `index`
  // holds their places in the kept table, which d_node_out keeps indexing
  std::vector<uint32_t> index;
  {
    std::vector<uint8_t> read;
    SWZ_TRY(filter_reads(c, who, dir, kept, filter, &read));
    const uint64_t all = kept.count.size();
    for (uint64_t k = 0; k < all; ++k)
      if (read[k]) index.push_back((uint32_t)k);
    if (index.size() < all) {
      DatasetScan reads;
      reads.info = kept.info;
      reads.info.points = 0;
      const bool pnts = kept.info.format == SWZ_OUT_3DTILES;
      for (uint32_t k : index) {
        reads.level.push_back(kept.level[k]);
        reads.key.push_back(kept.key[k]);
        reads.count.push_back(kept.count[k]);
        reads.path.push_back(kept.path[k]);
        reads.layout.push_back(kept.layout[k]);
        reads.data_at.push_back(kept.data_at[k]);
        if (pnts) reads.file_bytes.push_back(kept.file_bytes[k]);
        reads.info.points += kept.count[k];
      }
      reads.info.num_nodes = reads.count.size();
      kept = std::move(reads);
    }
  }
  // ---- the chunks: whole nodes of that table, as the converter cuts its source
  const uint64_t nn = kept.count.size();
  std::vector<uint64_t> first;
  {
    const uint64_t chunk_points = output_chunk_points(c, q->chunk_points);
    uint64_t num_chunks = 0;
    (void)swz_output_chunks(nn, kept.count.data(), chunk_points, 0, nullptr, &num_chunks);
    first.assign(num_chunks + 1, 0);
    (void)swz_output_chunks(nn, kept.count.data(), chunk_points, num_chunks, first.data(), &num_chunks);
  }
  OutputWorkspace ow{c};  // the chunk-local arrays ("out_*") are the call's part of the workspace
  CopyStream copy;
  SourceStream source;
  source.plan(c, who, &kept, &first, mask | fattrs);
  uint64_t total = 0, chunks = 0;
  double select_ms = 0;
  int status = SWZ_OK;
  if (source.rows_max) {
    uint64_t nodes_max = 0;
    for (uint64_t j = 0; j < source.num_chunks; ++j) nodes_max = std::max(nodes_max, first[j + 1] - first[j]);
    uint32_t *d_rows = nullptr, *d_first = nullptr;
    if (d_node_out && !count_only) {
      SWZ_TRY(c->get("out_q_rows", (size_t)source.rows_max, &d_rows));
      SWZ_TRY(c->get("out_q_first", 2 * (size_t)nodes_max + 1, &d_first));  // the first rows, then the nodes' indices
    }
    std::vector<uint32_t> node_first;
    RegionDev region_dev;  // a polygon's vertices go up once, not per chunk
    SWZ_TRY(region_upload(c, region_host, &region_dev));
    const Selection sel{q->box_min, q->box_max, nullptr, &region_dev, filter};
    SWZ_HIP(c, hipStreamCreateWithFlags(&copy.s, hipStreamNonBlocking));
    SWZ_TRY(source.start(copy.s));
    for (uint64_t j = 0; j < source.num_chunks; ++j) {
      SWZ_TRY(source.next(j));  // (a read error: the stream stops here, the file is named)
      ++chunks;
      const uint64_t rows = source.rows(j);
      const auto t_select = std::chrono::steady_clock::now();
      swz_attribute_columns at{};
      for (int a = 0; a < SWZ_ATTR_COUNT; ++a)
        if ((mask >> a) & 1u) at.column[a] = static_cast<uint8_t*>(d_out->column[a]) + total * ATTR_BYTES[a];
      const uint64_t room = count_only ? 0 : capacity - total;
      uint64_t cnt = 0;
      // (a chunk selects its rows at the most: the capacity the kernel's checks see ends with the chunk-local row array)
      status = region_select(c, who, source.xyz, rows, &source.cols, mask, sel, std::min(room, rows),
                             count_only ? nullptr : d_xyz_out + 3 * total, &at, d_rows, &cnt);
      if (status != SWZ_OK) {
        if (!count_only && cnt > room) {  // the stream stops after this chunk's count
          *count_out = total + cnt;
          return refuse("capacity " + std::to_string(capacity) + " is less than the " + std::to_string(total + cnt) +
                        " rows selected up to chunk " + std::to_string(j));
        }
        return status;
      }
      if (d_rows && cnt) {
        const uint64_t k0 = first[j], k1 = first[j + 1];
        const uint64_t nk = k1 - k0;
        node_first.assign(2 * nk + 1, 0);
        for (uint64_t k = k0; k < k1; ++k) {
          node_first[k - k0 + 1] = node_first[k - k0] + (uint32_t)kept.count[k];
          node_first[nk + 1 + (k - k0)] = index[k];
        }
        SWZ_HIP(c, hipMemcpyAsync(d_first, node_first.data(), node_first.size() * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
        hipLaunchKernelGGL(query_row_nodes_kernel, dim3(div_up(cnt, 256)), dim3(256), 0, c->stream, d_rows, (uint32_t)cnt, d_first,
                           (uint32_t)nk, d_first + nk + 1, d_node_out + total);
        SWZ_LAUNCH_CHECK(c);
        SWZ_HIP(c, hipStreamSynchronize(c->stream));  // (node_first is the next chunk's)
      }
      total += cnt;
      select_ms += ms_since(t_select);
    }
  }
  *count_out = total;
  if (stats) {
    stats->nodes_scanned = scanned;
    stats->nodes_read = nn;
    stats->points_read = kept.info.points;
    stats->points_out = total;
    stats->bytes_read = source.bytes_read;
    stats->chunks = chunks;
    stats->read_ms = source.read_ms;
    stats->unpack_ms = source.unpack_ms;
    stats->select_ms = select_ms;
    stats->copy_ms = source.copy_ms;
    stats->wall_ms = ms_since(t_wall);
  }
  return SWZ_OK;
}

// swz_dataset_summarize: every node of the source through the query's stream, the summaries kernel on every chunk, the sidecar
static int summarize(swz_ctx* c, const char* who, const char* dir, uint32_t source_flags, uint64_t chunk_points_in, swz_summarize_stats* stats) {
  auto refuse = [&](const std::string& what) { return c->fail(SWZ_ERR_BAD_ARG, std::string(who) + ": " + what); };
  const auto t_wall = std::chrono::steady_clock::now();
  if (stats) *stats = swz_summarize_stats{};
  if (!dir) return refuse("NULL argument");
  if (source_flags & ~(uint32_t)SWZ_CONVERT_LOSSY_SOURCE) return refuse("an unknown bit in source_flags");
  DatasetScan scan;
  SWZ_TRY(source_open(c, who, dir, -1, source_flags, &scan, nullptr));
  uint32_t mask = scan.info.attribute_mask & (uint32_t)SWZ_SUMMARY_SCALARS;
  if (scan.info.format == SWZ_OUT_3DTILES) mask &= 1u << SWZ_ATTR_INTENSITY;  // all a .pnts file carries beside RGB
  const uint32_t cols = (uint32_t)__builtin_popcount(mask);
  const uint64_t nn = scan.count.size();
  std::vector<swz_attr_summary> entries((size_t)(nn * cols), summary_empty());
  uint64_t chunks = 0;
  double summary_ms = 0;
  OutputWorkspace ow{c};
  CopyStream copy;
  SourceStream source;
  std::vector<uint64_t> first;
  if (cols) {
    const uint64_t chunk_points = output_chunk_points(c, chunk_points_in);
    uint64_t num_chunks = 0;
    (void)swz_output_chunks(nn, scan.count.data(), chunk_points, 0, nullptr, &num_chunks);
    first.assign(num_chunks + 1, 0);
    (void)swz_output_chunks(nn, scan.count.data(), chunk_points, num_chunks, first.data(), &num_chunks);
    SWZ_HIP(c, hipSetDevice(c->device));
    source.plan(c, who, &scan, &first, mask);
    if (source.rows_max) {
      SWZ_HIP(c, hipStreamCreateWithFlags(&copy.s, hipStreamNonBlocking));
      SWZ_TRY(source.start(copy.s));
      std::vector<uint64_t> offset;
      for (uint64_t j = 0; j < source.num_chunks; ++j) {
        SWZ_TRY(source.next(j));
        ++chunks;
        const auto t_summary = std::chrono::steady_clock::now();
        const uint64_t k0 = first[j], k1 = first[j + 1];
        offset.assign(k1 - k0, 0);
        for (uint64_t k = k0 + 1; k < k1; ++k) offset[k - k0] = offset[k - k0 - 1] + scan.count[k - 1];
        SWZ_TRY(node_summaries(c, who, source.rows(j), &source.cols, mask, k1 - k0, offset.data(), scan.count.data() + k0,
                               entries.data() + k0 * cols));
        summary_ms += ms_since(t_summary);
      }
    }
  }
  std::string why;
  const int st = sidecar_write(dir, scan.info.format, mask, nn, scan.level.data(), scan.key.data(), scan.count.data(), entries.data(), &why);
  if (st != SWZ_OK) return c->fail(st, std::string(who) + ": " + why);
  if (stats) {
    stats->nodes = nn;
    stats->points = scan.info.points;
    stats->bytes_read = source.bytes_read;
    stats->chunks = chunks;
    stats->read_ms = source.read_ms;
    stats->unpack_ms = source.unpack_ms;
    stats->summary_ms = summary_ms;
    stats->copy_ms = source.copy_ms;
    stats->wall_ms = ms_since(t_wall);
  }
  return SWZ_OK;
}

}  // namespace swz

using namespace swz;

extern "C" {

// swz_dataset_query_nodes and swz_dataset_query_region_nodes, and their _why forms on a context that only holds the text
// ... and swz_dataset_query_filtered_nodes, which also says which nodes of the table the filter lets the query read
static int query_nodes(swz_ctx* c, const std::string& who, const char* dir, const swz_query_params* params, const swz_region* region,
                       uint64_t max_nodes, int8_t* level_out, uint64_t* key_out, uint64_t* count_out, uint64_t* num_out,
                       uint64_t* points_bound_out, const swz_filter* filter = nullptr, uint8_t* read_out = nullptr) {
  swz_ctx text;  // (a NULL context: only the status comes back; no device is touched either way)
  if (!c) c = &text;
  if (!num_out) return c->fail(SWZ_ERR_BAD_ARG, who + ": NULL argument");
  DatasetScan kept;
  uint64_t scanned = 0;
  RegionHost region_host;
  uint32_t fattrs = 0;
  SWZ_TRY(query_plan(c, who.c_str(), dir, params, region, filter, &kept, &scanned, &region_host, &fattrs));
  const uint64_t nn = kept.count.size();
  std::vector<uint8_t> read;
  SWZ_TRY(filter_reads(c, who.c_str(), dir, kept, filter, &read));
  uint64_t bound = 0;
  for (uint64_t k = 0; k < nn; ++k)
    if (read[k]) bound += kept.count[k];
  *num_out = nn;
  if (points_bound_out) *points_bound_out = bound;
  if (!level_out && !key_out && !count_out && !read_out) return SWZ_OK;
  if (nn > max_nodes) return c->fail(SWZ_ERR_BAD_ARG, who + ": max_nodes too small");
  for (uint64_t k = 0; k < nn; ++k) {
    if (level_out) level_out[k] = kept.level[k];
    if (key_out) key_out[k] = kept.key[k];
    if (count_out) count_out[k] = kept.count[k];
    if (read_out) read_out[k] = read[k];
  }
  return SWZ_OK;
}

int swz_dataset_query_nodes(swz_ctx* c, const char* dir, const swz_query_params* params, uint64_t max_nodes, int8_t* level_out,
                            uint64_t* key_out, uint64_t* count_out, uint64_t* num_out, uint64_t* points_bound_out) {
  return query_nodes(c, "swz_dataset_query_nodes", dir, params, nullptr, max_nodes, level_out, key_out, count_out, num_out, points_bound_out);
}

int swz_dataset_query_region_nodes(swz_ctx* c, const char* dir, const swz_query_params* params, const swz_region* region, uint64_t max_nodes,
                                   int8_t* level_out, uint64_t* key_out, uint64_t* count_out, uint64_t* num_out, uint64_t* points_bound_out) {
  return query_nodes(c, "swz_dataset_query_region_nodes", dir, params, region, max_nodes, level_out, key_out, count_out, num_out,
                     points_bound_out);
}

int swz_dataset_query_nodes_why(const char* dir, const swz_query_params* params, uint64_t max_nodes, int8_t* level_out, uint64_t* key_out,
                                uint64_t* count_out, uint64_t* num_out, uint64_t* points_bound_out, char* why_out, uint64_t why_bytes) {
  swz_ctx text;
  const int st = query_nodes(&text, "swz_dataset_query_nodes", dir, params, nullptr, max_nodes, level_out, key_out, count_out, num_out,
                             points_bound_out);
  return why_text(st, text, why_out, why_bytes);
}

int swz_dataset_query_region_nodes_why(const char* dir, const swz_query_params* params, const swz_region* region, uint64_t max_nodes,
                                       int8_t* level_out, uint64_t* key_out, uint64_t* count_out, uint64_t* num_out,
                                       uint64_t* points_bound_out, char* why_out, uint64_t why_bytes) {
  swz_ctx text;
  const int st = query_nodes(&text, "swz_dataset_query_region_nodes", dir, params, region, max_nodes, level_out, key_out, count_out, num_out,
                             points_bound_out);
  return why_text(st, text, why_out, why_bytes);
}

int swz_dataset_query_filtered_nodes(swz_ctx* c, const char* dir, const swz_query_params* params, const swz_region* region,
                                     const swz_filter* filter, uint64_t max_nodes, int8_t* level_out, uint64_t* key_out,
                                     uint64_t* count_out, uint8_t* read_out, uint64_t* num_out, uint64_t* points_bound_out) {
  return query_nodes(c, "swz_dataset_query_filtered_nodes", dir, params, region, max_nodes, level_out, key_out, count_out, num_out,
                     points_bound_out, filter, read_out);
}

int swz_dataset_query_filtered_nodes_why(const char* dir, const swz_query_params* params, const swz_region* region,
                                         const swz_filter* filter, uint64_t max_nodes, int8_t* level_out, uint64_t* key_out,
                                         uint64_t* count_out, uint8_t* read_out, uint64_t* num_out, uint64_t* points_bound_out,
                                         char* why_out, uint64_t why_bytes) {
  swz_ctx text;
  const int st = query_nodes(&text, "swz_dataset_query_filtered_nodes", dir, params, region, max_nodes, level_out, key_out, count_out,
                             num_out, points_bound_out, filter, read_out);
  return why_text(st, text, why_out, why_bytes);
}

int swz_dataset_summarize(swz_ctx* c, const char* dir, uint32_t source_flags, uint64_t chunk_points, swz_summarize_stats* stats) {
  if (!c) return SWZ_ERR_BAD_ARG;
  return summarize(c, "swz_dataset_summarize", dir, source_flags, chunk_points, stats);
}

int swz_dataset_query(swz_ctx* c, const char* dir, const swz_query_params* params, uint64_t capacity, double* d_xyz_out,
                      const swz_attribute_columns* d_out, uint32_t* d_node_out, uint64_t* count_out, swz_query_stats* stats) {
  if (!c) return SWZ_ERR_BAD_ARG;
  return query(c, "swz_dataset_query", dir, params, nullptr, nullptr, capacity, d_xyz_out, d_out, d_node_out, count_out, stats);
}

int swz_dataset_query_region(swz_ctx* c, const char* dir, const swz_query_params* params, const swz_region* region, uint64_t capacity,
                             double* d_xyz_out, const swz_attribute_columns* d_out, uint32_t* d_node_out, uint64_t* count_out,
                             swz_query_stats* stats) {
  if (!c) return SWZ_ERR_BAD_ARG;
  return query(c, "swz_dataset_query_region", dir, params, region, nullptr, capacity, d_xyz_out, d_out, d_node_out, count_out, stats);
}

int swz_dataset_query_filtered(swz_ctx* c, const char* dir, const swz_query_params* params, const swz_region* region,
                               const swz_filter* filter, uint64_t capacity, double* d_xyz_out, const swz_attribute_columns* d_out,
                               uint32_t* d_node_out, uint64_t* count_out, swz_query_stats* stats) {
  if (!c) return SWZ_ERR_BAD_ARG;
  return query(c, "swz_dataset_query_filtered", dir, params, region, filter, capacity, d_xyz_out, d_out, d_node_out, count_out, stats);
}

}  // extern "C"
