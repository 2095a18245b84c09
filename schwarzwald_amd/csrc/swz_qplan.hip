// swz_qplan.hip -- which nodes of a written data set a query reads (host only: no kernel, no device): the scan cut down to
// the nodes whose widened boxes meet the query box and can hold a row of the region (query_plan, with the rounding proofs
// of the rules for planes and polygons), the nodes among them that a filter can reach by the directory's node-summaries.swz
// (filter_reads), and the entries that hand that table out without reading a point: swz_dataset_query_nodes,
// swz_dataset_query_region_nodes, swz_dataset_query_filtered_nodes and their _why forms.  The streaming query
// (swz_query.hip) reads the nodes this file leaves.
#include <cmath>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "swz_convert.h"
#include "swz_hostio.h"
#include "swz_qplan.h"
#include "swz_select.h"
#include "swz_summary.h"

namespace swz {

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

int query_plan(swz_ctx* c, const char* who, const char* dir, const swz_query_params* q, const swz_region* region, const swz_filter* filter,
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
  std::vector<uint32_t> keep;
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
    keep.push_back((uint32_t)k);
  }
  *kept = scan.subset(keep);
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

int filter_reads(swz_ctx* c, const char* who, const char* dir, const DatasetScan& kept, const swz_filter* filter,
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

}  // extern "C"
