// The free functions of the C++ host adapter (schwarzwald_amd/host/swz_tiling.hpp) -- index_points,
// sort_indexed_points, sample_points, get_octant_bounds / get_octant_at_level and the sampler factory -- called the
// way a Schwarzwald maintainer would call them and compared with the CPU oracle (oracle/oracle.h) and with closed
// forms.  Everything is an integer, a name or the bit pattern of a double: every comparison is ==.
//
//   test_adapter_seams                runs every case on the GPU
//   test_adapter_seams --oracle-only  builds every input, runs the oracle side and the pure-host checks and asserts
//                                     that each input really holds its hard case; creates no swz_host::Context
//
// One "<case> ok: ..." line per case (the same lines in both modes), "FAIL: ..." and exit code 1 at the first failure.
#include <array>
#include <cstdarg>
#include <limits>

#include "../../oracle/oracle.h"
#include "../../schwarzwald_amd/host/swz_tiling.hpp"
#include "seam_util.hpp"

using namespace swz_host;
using seam::Box;
using seam::Rng;
using seam::bits;

static bool g_oracle_only = false;
static Context* g_ctx = nullptr;
static int g_ok = 0;
static const char* mode() { return g_oracle_only ? "oracle only" : "gpu == oracle"; }

static void ok(const std::string& name, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  std::vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  std::printf("%s ok: %s [%s]\n", name.c_str(), buf, mode());
  std::fflush(stdout);
  ++g_ok;
}

static AABB aabb(const Box& b) { return AABB{{b.mn[0], b.mn[1], b.mn[2]}, {b.mx[0], b.mx[1], b.mx[2]}}; }

static uint64_t compact3(uint64_t v) {  // every third bit of v, from bit 0
  uint64_t out = 0;
  for (int bit = 0; bit < 21; ++bit) out |= ((v >> (3 * bit)) & 1ull) << bit;
  return out;
}
static uint64_t cell_of_key(uint64_t key, int axis) { return compact3(key >> (2 - axis)); }  // x: bit 2, y: 1, z: 0

// ------------------------------------------------------------------------------------------ index_points
static uint64_t axis_cell(const Box& b, int axis, double v) {  // v inside the bounds
  double p[3] = {b.mn[0], b.mn[1], b.mn[2]};
  p[axis] = v;
  return cell_of_key(orc_calculate_morton_index(p, b.mn, b.mx, 21), axis);
}

// the two neighbouring doubles between which the oracle's cell on `axis` changes from k - 1 to k
static void find_edge(const Box& b, int axis, uint64_t k, double* lo, double* hi) {
  const double inf = std::numeric_limits<double>::infinity();
  double x = b.mn[axis] + (double)k * (b.ext(axis) / 2097152.0);
  int steps = 0;
  if (axis_cell(b, axis, x) >= k) {
    while (axis_cell(b, axis, x) >= k && ++steps < 4096) x = std::nextafter(x, -inf);
    *lo = x;
    *hi = std::nextafter(x, inf);
  } else {
    while (axis_cell(b, axis, x) < k && ++steps < 4096) x = std::nextafter(x, inf);
    *hi = x;
    *lo = std::nextafter(x, -inf);
  }
  CHECK(axis_cell(b, axis, *lo) == k - 1 && axis_cell(b, axis, *hi) == k, "no cell edge found near k = %llu on axis %d",
        (unsigned long long)k, axis);
}

struct EdgeGroup {  // the special points that sit around the lower edge of cell k on one axis
  int axis;
  uint64_t k;
  size_t first, count;
};
struct Specials {
  std::vector<std::array<double, 3>> pts;
  std::vector<EdgeGroup> edges;
  size_t first_nonfinite = 0;  // nine points: per axis +inf, -inf, NaN on that axis; then one all-NaN point
};

static Specials special_points(const Box& b) {
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  Specials s;
  const std::array<double, 3> mid = {b.mn[0] + 0.37 * b.ext(0), b.mn[1] + 0.61 * b.ext(1), b.mn[2] + 0.43 * b.ext(2)};
  for (int a = 0; a < 3; ++a) {  // beyond each of the six faces
    auto p = mid;
    p[a] = b.mn[a] - 0.3 * b.ext(a);
    s.pts.push_back(p);
    p[a] = b.mx[a] + 0.3 * b.ext(a);
    s.pts.push_back(p);
  }
  s.pts.push_back({b.mn[0] - 1e300, b.mn[1] - 1.0, b.mn[2] - 1e-9});  // beyond three faces at once
  s.pts.push_back({b.mx[0] + 1e300, b.mx[1] + 1.0, b.mx[2] + 1e-9});
  s.pts.push_back({b.mn[0], b.mn[1], b.mn[2]});  // exactly on min, exactly on max
  s.pts.push_back({b.mx[0], b.mx[1], b.mx[2]});
  for (int a = 0; a < 3; ++a) {
    auto p = mid;
    p[a] = b.mn[a];
    s.pts.push_back(p);
    p[a] = b.mx[a];
    s.pts.push_back(p);
    p[a] = -0.0;
    s.pts.push_back(p);
  }
  s.pts.push_back({-0.0, -0.0, -0.0});
  const uint64_t ks[5] = {0, 1, 1ull << 20, (1ull << 21) - 1, 1ull << 21};
  for (uint64_t k : ks) {  // the same k on all three axes: the value, the double below, the double above
    std::array<double, 3> v, lo, hi;
    for (int a = 0; a < 3; ++a) {
      v[a] = b.mn[a] + (double)k * (b.ext(a) / 2097152.0);
      lo[a] = std::nextafter(v[a], -inf);
      hi[a] = std::nextafter(v[a], inf);
    }
    s.pts.push_back(v);
    s.pts.push_back(lo);
    s.pts.push_back(hi);
  }
  for (int a = 0; a < 3; ++a)
    for (uint64_t k : ks) {
      const double v = b.mn[a] + (double)k * (b.ext(a) / 2097152.0);
      std::vector<double> vals = {v, std::nextafter(v, -inf), std::nextafter(v, inf)};
      if (k != 0 && k != (1ull << 21)) {  // and the two doubles that the oracle's arithmetic separates
        double lo, hi;
        find_edge(b, a, k, &lo, &hi);
        vals.push_back(lo);
        vals.push_back(hi);
        s.edges.push_back({a, k, s.pts.size(), vals.size()});
      }
      for (double x : vals) {
        auto p = mid;
        p[a] = x;
        s.pts.push_back(p);
      }
    }
  s.first_nonfinite = s.pts.size();
  for (int a = 0; a < 3; ++a)
    for (double x : {inf, -inf, nan}) {
      auto p = mid;
      p[a] = x;
      s.pts.push_back(p);
    }
  s.pts.push_back({nan, nan, nan});
  return s;
}

static void case_index_points(const char* bname, const Box& b, size_t n) {
  const std::string name = std::string("index_points ") + bname + " n=" + std::to_string(n);
  const Specials sp = special_points(b);
  CHECK(sp.pts.size() <= 255, "%zu special points", sp.pts.size());
  Rng r(1000 + n);
  std::vector<double> in(3 * n);
  for (size_t i = 0; i < n; ++i)
    for (int a = 0; a < 3; ++a)
      in[3 * i + a] = i < sp.pts.size() ? sp.pts[i][a] : b.mn[a] + (r.uniform() * 1.5 - 0.25) * b.ext(a);
  const bool full = n >= sp.pts.size();  // n = 0 and n = 1 are launch edges only (n = 1 is one outlier)

  std::vector<double> want_xyz = in;
  std::vector<uint64_t> want_keys(n);
  orc_index_points(want_xyz.data(), n, b.mn, b.mx, 21, want_keys.data());

  // ---- the input holds what it claims (required, whatever the library does)
  size_t outliers = 0;
  if (full) {
    int beyond[6] = {0, 0, 0, 0, 0, 0};
    for (size_t i = 0; i < n; ++i) {
      bool out = false;
      for (int a = 0; a < 3; ++a) {
        if (in[3 * i + a] < b.mn[a]) ++beyond[2 * a], out = true;
        if (in[3 * i + a] > b.mx[a]) ++beyond[2 * a + 1], out = true;
      }
      outliers += out;
    }
    for (int f = 0; f < 6; ++f) CHECK(beyond[f] > 0, "no outlier beyond face %d", f);
    for (const EdgeGroup& e : sp.edges) {
      bool below = false, at = false;
      for (size_t i = e.first; i < e.first + e.count; ++i) {
        const uint64_t c = cell_of_key(want_keys[i], e.axis);
        below |= c == e.k - 1;
        at |= c == e.k;
      }
      CHECK(below && at, "the points around cell %llu on axis %d do not fall into both neighbouring cells",
            (unsigned long long)e.k, e.axis);
    }
    // the oracle's answer for +inf, -inf and NaN is well defined: the clamp maps them to max, min and min
    for (int a = 0; a < 3; ++a) {
      const size_t i = sp.first_nonfinite + 3 * a;
      CHECK(bits(want_xyz[3 * i + a]) == bits(b.mx[a]), "+inf on axis %d", a);
      CHECK(bits(want_xyz[3 * (i + 1) + a]) == bits(b.mn[a]), "-inf on axis %d", a);
      CHECK(bits(want_xyz[3 * (i + 2) + a]) == bits(b.mn[a]), "NaN on axis %d", a);
      CHECK(cell_of_key(want_keys[i], a) == (1u << 21) - 1 && cell_of_key(want_keys[i + 1], a) == 0 &&
              cell_of_key(want_keys[i + 2], a) == 0, "keys of the non-finite points on axis %d", a);
    }
    CHECK(want_keys[sp.first_nonfinite + 9] == 0, "the all-NaN point");
    for (double v : want_xyz) CHECK(std::isfinite(v), "a clamped position is not finite");
  } else if (n == 1) {
    CHECK(in[0] < b.mn[0], "the single point is an outlier");
  }

  if (!g_oracle_only) {
    const size_t G = 8;  // guard elements on either side of both arrays
    const IndexedPoint64 guard{0xDEADBEEFu, 0xA5A5A5A5A5A5A5A5ull};
    std::vector<IndexedPoint64> out(n + 2 * G, guard);
    std::vector<double> xyz(3 * (n + 2 * G), -12345.678);
    std::copy(in.begin(), in.end(), xyz.begin() + 3 * G);
    index_points(*g_ctx, xyz.data() + 3 * G, n, out.data() + G, aabb(b), OutlierPointsBehaviour::ClampToBounds);
    for (size_t i = 0; i < n; ++i) {
      CHECK(out[G + i].morton_index == want_keys[i], "key of point %zu: %llx, oracle %llx", i,
            (unsigned long long)out[G + i].morton_index, (unsigned long long)want_keys[i]);
      CHECK(out[G + i].point_index == i, "point_index of element %zu", i);
      for (int a = 0; a < 3; ++a)
        CHECK(bits(xyz[3 * (G + i) + a]) == bits(want_xyz[3 * i + a]), "clamped position of point %zu axis %d", i, a);
    }
    for (size_t g = 0; g < G; ++g) {
      CHECK(out[g].point_index == guard.point_index && out[g].morton_index == guard.morton_index, "written before the output");
      CHECK(out[G + n + g].point_index == guard.point_index && out[G + n + g].morton_index == guard.morton_index,
            "written behind the output");
    }
    for (size_t g = 0; g < 3 * G; ++g)
      CHECK(xyz[g] == -12345.678 && xyz[3 * (G + n) + g] == -12345.678, "written outside the positions");
  }
  ok(name, "%zu outliers, %zu cell edges, non-finite points %s", outliers, full ? sp.edges.size() : (size_t)0,
     full ? "clamped" : "absent");
}

static void case_index_lattice() {
  // point (cell + 0.5) in [0, 2^21]^3: octant digit l of the key is bit (20 - l) of x, y, z as 4x + 2y + z
  const Box b = seam::cube_box(2097152.0);
  const size_t n = 5000;
  Rng r(3);
  std::vector<uint64_t> cells(3 * n), closed(n);
  std::vector<double> in(3 * n);
  for (size_t i = 0; i < 3 * n; ++i) {
    cells[i] = r.below(1ull << 21);
    in[i] = (double)cells[i] + 0.5;
  }
  cells[0] = cells[1] = cells[2] = 0;  // the corners of the lattice
  cells[3] = cells[4] = cells[5] = (1ull << 21) - 1;
  for (int a = 0; a < 6; ++a) in[a] = (double)cells[a] + 0.5;
  for (size_t i = 0; i < n; ++i) {
    uint64_t k = 0;
    for (int bit = 0; bit < 21; ++bit)
      k |= ((cells[3 * i + 2] >> bit) & 1ull) << (3 * bit) | ((cells[3 * i + 1] >> bit) & 1ull) << (3 * bit + 1) |
           ((cells[3 * i] >> bit) & 1ull) << (3 * bit + 2);
    closed[i] = k;
  }
  std::vector<double> o_xyz = in;
  std::vector<uint64_t> o_keys(n);
  orc_index_points(o_xyz.data(), n, b.mn, b.mx, 21, o_keys.data());
  for (size_t i = 0; i < n; ++i) CHECK(o_keys[i] == closed[i], "oracle key of lattice point %zu", i);
  CHECK(closed[1] == 0x7FFFFFFFFFFFFFFFull, "the far corner has every bit set");
  if (!g_oracle_only) {
    std::vector<double> xyz = in;
    std::vector<IndexedPoint64> out(n);
    index_points(*g_ctx, xyz.data(), n, out.data(), aabb(b), OutlierPointsBehaviour::ClampToBounds);
    for (size_t i = 0; i < n; ++i) CHECK(out[i].morton_index == closed[i] && out[i].point_index == i, "lattice point %zu", i);
    CHECK(std::memcmp(xyz.data(), in.data(), 24 * n) == 0, "positions inside the bounds were changed");
  }
  ok("index_points lattice", "%zu keys built bit by bit", n);
}

static void case_index_abort() {
  // OutlierPointsBehaviour::Abort is not offered: the call throws before anything runs
  const Box b = seam::odd_box();
  double p[3] = {b.mn[0] - 1.0, b.mn[1] + 1.0, b.mn[2] + 1.0}, q[3] = {p[0], p[1], p[2]};
  uint64_t key = 0;
  orc_index_points(q, 1, b.mn, b.mx, 21, &key);
  CHECK(bits(q[0]) == bits(b.mn[0]), "the point is an outlier for the oracle");
  if (!g_oracle_only) {
    IndexedPoint64 out{77, 77};
    bool threw = false;
    try {
      index_points(*g_ctx, p, 1, &out, aabb(b), OutlierPointsBehaviour::Abort);
    } catch (const std::runtime_error&) {
      threw = true;
    }
    CHECK(threw, "Abort did not throw");
    CHECK(out.point_index == 77 && out.morton_index == 77 && p[0] == b.mn[0] - 1.0, "Abort wrote something");
  }
  ok("index_points Abort", "throws, nothing written");
}

// ------------------------------------------------------------------------------------------ sort_indexed_points
static void case_sort(const char* kind, size_t n) {
  const std::string name = std::string("sort_indexed_points ") + kind + " n=" + std::to_string(n);
  Rng r(77 + n);
  std::vector<IndexedPoint64> in(n);
  for (size_t i = 0; i < n; ++i) {
    uint64_t k;
    if (kind[0] == 'r') k = r.next() >> 1;                       // random 63-bit keys
    else if (kind[0] == 't') k = r.below(50) << 40;              // few distinct keys, long tie runs
    else k = 0x1234567812345678ull;                              // all equal
    in[i] = {(uint32_t)i, k};
  }
  if (kind[0] == 't')
    for (size_t i = 0; i < n; ++i) {
      if (i % 7 == 0) in[i].morton_index = 0;
      if (i % 13 == 1) in[i].morton_index = (1ull << 63) - 1;
    }
  for (size_t i = n; i > 1; --i) std::swap(in[i - 1].point_index, in[r.below(i)].point_index);  // payload: a permutation
  if (n == 2 && in[0].point_index == 0) std::swap(in[0].point_index, in[1].point_index);
  if (n >= 2) {
    bool iota = true;
    for (size_t i = 0; i < n; ++i) iota &= in[i].point_index == i;
    CHECK(!iota, "the payload is 0..n-1");
  }
  std::vector<uint64_t> keys(n);
  for (size_t i = 0; i < n; ++i) keys[i] = in[i].morton_index;
  std::vector<uint32_t> perm(n);
  orc_sort_by_key(keys.data(), n, perm.data());
  size_t longest = n ? 1 : 0, run = 1;
  for (size_t i = 1; i < n; ++i) {
    CHECK(keys[perm[i - 1]] <= keys[perm[i]], "oracle order");
    run = keys[perm[i - 1]] == keys[perm[i]] ? run + 1 : 1;
    longest = std::max(longest, run);
  }
  if (kind[0] != 'r' && n >= 4095) CHECK(longest >= n / 60, "no long run of equal keys (%zu)", longest);
  if (!g_oracle_only) {
    const IndexedPoint64 guard{0xDEADBEEFu, 0xA5A5A5A5A5A5A5A5ull};
    std::vector<IndexedPoint64> got(n + 2, guard);
    std::copy(in.begin(), in.end(), got.begin() + 1);
    sort_indexed_points(*g_ctx, got.data() + 1, got.data() + 1 + n);
    for (size_t i = 0; i < n; ++i)
      CHECK(got[1 + i].morton_index == in[perm[i]].morton_index && got[1 + i].point_index == in[perm[i]].point_index,
            "element %zu: the payload did not travel with its key, or ties lost their input order", i);
    CHECK(got[0].point_index == guard.point_index && got[n + 1].point_index == guard.point_index, "written outside the range");
  }
  ok(name, "longest run of equal keys %zu", longest);
}

// ------------------------------------------------------------------------------------------ sample_points
struct SortedCloud {
  Box b;
  std::vector<double> pos;  // clamped; holds more rows than the ranges refer to
  std::vector<uint64_t> keys;
  std::vector<uint32_t> idx;  // the sort permutation
};

static SortedCloud sorted_cloud(const Box& b, std::vector<double> xyz, size_t extra_rows, uint64_t seed) {
  SortedCloud s;
  s.b = b;
  const size_t n = xyz.size() / 3;
  std::vector<uint64_t> k(n);
  orc_index_points(xyz.data(), n, b.mn, b.mx, 21, k.data());
  std::vector<uint32_t> perm(n);
  orc_sort_by_key(k.data(), n, perm.data());
  s.keys.resize(n);
  for (size_t i = 0; i < n; ++i) s.keys[i] = k[perm[i]];
  s.idx = perm;
  s.pos = std::move(xyz);
  Rng r(seed);
  for (size_t i = 0; i < 3 * extra_rows; ++i) s.pos.push_back(b.mn[i % 3] + r.uniform() * b.ext((int)(i % 3)));
  return s;
}

// the most populated node of `level` in the sorted keys: [lo, hi) and its key
static void busiest_node(const SortedCloud& s, int level, size_t* lo, size_t* hi, uint64_t* node_key) {
  const int shift = (20 - level) * 3;
  size_t best = 0, i = 0;
  const size_t n = s.keys.size();
  while (i < n) {
    size_t j = i;
    while (j < n && (s.keys[j] >> shift) == (s.keys[i] >> shift)) ++j;
    if (j - i > best) best = j - i, *lo = i, *hi = j, *node_key = (s.keys[i] >> shift) << shift;
    i = j;
  }
}

static const char* SAMPLER_NAMES[4] = {"RANDOM_GRID", "GRID_CENTER", "MIN_DISTANCE", "JITTERED"};

// returns the number the oracle took
static int64_t run_sample(const SortedCloud& s, int sampler, uint64_t max_points, size_t lo, size_t hi, uint64_t node_key,
                          int32_t node_level, float spacing, int behaviour) {
  const size_t n = hi - lo;
  std::vector<uint64_t> ok_(s.keys.begin() + lo, s.keys.begin() + hi);
  std::vector<uint32_t> oi(s.idx.begin() + lo, s.idx.begin() + hi);
  // (non-NULL pointers for the empty range too)
  ok_.reserve(1);
  oi.reserve(1);
  const int64_t taken = orc_sample_points(sampler, max_points, ok_.data(), oi.data(), n, s.pos.data(), node_key, node_level, 21,
                                          s.b.mn, s.b.mx, spacing, behaviour);
  CHECK(taken >= 0 && (uint64_t)taken <= n, "oracle status %lld", (long long)taken);
  if (!g_oracle_only) {
    const IndexedPoint64 guard{0xDEADBEEFu, 0xA5A5A5A5A5A5A5A5ull};
    std::vector<IndexedPoint64> range(n + 2, guard);
    for (size_t i = 0; i < n; ++i) range[1 + i] = {s.idx[lo + i], s.keys[lo + i]};
    IndexedPoint64* begin = range.data() + 1;
    IndexedPoint64* p = sample_points(*g_ctx, make_sampling_strategy_from_name(SAMPLER_NAMES[sampler], max_points), begin, begin + n,
                                      node_key, node_level, aabb(s.b), spacing,
                                      behaviour == ORC_ALWAYS_ADHERE ? SamplingBehaviour::AlwaysAdhereToMinSpacing
                                                                     : SamplingBehaviour::TakeAllWhenCountBelowMaxPoints,
                                      s.pos.data(), s.pos.size() / 3);
    CHECK(p - begin == taken, "partition point %lld, oracle %lld", (long long)(p - begin), (long long)taken);
    for (size_t i = 0; i < n; ++i)
      CHECK(begin[i].morton_index == ok_[i] && begin[i].point_index == oi[i], "element %zu of the %s half differs", i,
            i < (size_t)taken ? "taken" : "remaining");
    CHECK(range[0].point_index == guard.point_index && range[n + 1].point_index == guard.point_index, "written outside the range");
  }
  return taken;
}

static void cases_sample(const char* cname, const SortedCloud& s) {
  const size_t n = s.keys.size();
  CHECK(s.pos.size() / 3 > n, "num_positions is not larger than the range");
  bool iota = true;
  for (size_t i = 0; i < n; ++i) iota &= s.idx[i] == i;
  CHECK(!iota, "point_index is 0..n-1");
  const float spacing = (float)(s.b.ext(0) / 20.0);  // 20 cells along a node's side at every level
  size_t o_lo = 0, o_hi = 0, d_lo = 0, d_hi = 0;
  uint64_t o_key = 0, d_key = 0;
  busiest_node(s, 0, &o_lo, &o_hi, &o_key);
  busiest_node(s, 2, &d_lo, &d_hi, &d_key);
  CHECK(o_hi - o_lo > 300 && d_hi - d_lo > 50, "inner nodes too small: %zu, %zu", o_hi - o_lo, d_hi - d_lo);
  const size_t few = std::min<size_t>(30, d_hi - d_lo);
  for (int sampler = 0; sampler < 4; ++sampler)
    for (int behaviour = 0; behaviour < 2; ++behaviour) {
      const std::string base = std::string("sample_points ") + cname + " " + SAMPLER_NAMES[sampler] +
                               (behaviour == ORC_ALWAYS_ADHERE ? " adhere" : " take-all");
      int64_t t = run_sample(s, sampler, 1000, 0, n, 0, -1, spacing, behaviour);
      CHECK(t > 0 && (size_t)t < n, "the root takes %lld of %zu: both halves must be non-empty", (long long)t, n);
      ok(base + " root", "%lld of %zu taken", (long long)t, n);
      t = run_sample(s, sampler, 300, o_lo, o_hi, o_key, 0, spacing, behaviour);
      CHECK(t > 0 && (size_t)t < o_hi - o_lo, "the level-0 node takes %lld of %zu", (long long)t, o_hi - o_lo);
      ok(base + " level0", "%lld of %zu taken in r%d", (long long)t, o_hi - o_lo, (int)(o_key >> 60));
      t = run_sample(s, sampler, 50, d_lo, d_hi, d_key, 2, spacing, behaviour);
      CHECK(t > 0 && (size_t)t < d_hi - d_lo, "the level-2 node takes %lld of %zu", (long long)t, d_hi - d_lo);
      ok(base + " level2", "%lld of %zu taken in %s", (long long)t, d_hi - d_lo, seam::node_name(2, d_key).c_str());
      t = run_sample(s, sampler, 50, d_lo, d_lo, d_key, 2, spacing, behaviour);
      CHECK(t == 0, "empty range");
      ok(base + " empty", "nothing taken");
      t = run_sample(s, sampler, 50, d_lo + 3, d_lo + 4, d_key, 2, spacing, behaviour);
      CHECK(t == 1, "a single point is always taken, got %lld", (long long)t);
      ok(base + " single", "1 of 1 taken");
      t = run_sample(s, sampler, 50, d_lo, d_lo + few, d_key, 2, spacing, behaviour);
      if (behaviour == ORC_TAKE_ALL_WHEN_BELOW_MAX) CHECK((size_t)t == few, "n <= max_points_per_node must take all, took %lld", (long long)t);
      ok(base + " few", "%lld of %zu taken", (long long)t, few);
    }
}

static void case_sample_known_answer() {
  // The reference's 32^3 lattice: RANDOM_GRID, 16 points per node, spacing 32, node level 0 -- a 2 x 2 x 2 grid whose
  // first point per cell in Morton order survives.  Through index_points, sort and sample_points like the reference's
  // own unit test runs it.
  const int side = 32;
  const Box b = seam::cube_box(side);
  std::vector<double> xyz;
  for (int x = 0; x < side; ++x)
    for (int y = 0; y < side; ++y)
      for (int z = 0; z < side; ++z) {
        xyz.push_back(x + 0.5);
        xyz.push_back(y + 0.5);
        xyz.push_back(z + 0.5);
      }
  const size_t n = xyz.size() / 3;
  const double expected[8][3] = {{0.5, 0.5, 0.5},  {0.5, 0.5, 16.5},  {0.5, 16.5, 0.5},  {0.5, 16.5, 16.5},
                                 {16.5, 0.5, 0.5}, {16.5, 0.5, 16.5}, {16.5, 16.5, 0.5}, {16.5, 16.5, 16.5}};
  std::vector<IndexedPoint64> pts(n);
  size_t taken = 0;
  if (g_oracle_only) {
    std::vector<uint64_t> k(n), ks(n);
    std::vector<uint32_t> perm(n);
    orc_index_points(xyz.data(), n, b.mn, b.mx, 21, k.data());
    orc_sort_by_key(k.data(), n, perm.data());
    for (size_t i = 0; i < n; ++i) ks[i] = k[perm[i]];
    const int64_t t = orc_sample_points(ORC_RANDOM_GRID, 16, ks.data(), perm.data(), n, xyz.data(), 0, 0, 21, b.mn, b.mx, (float)side,
                                        ORC_TAKE_ALL_WHEN_BELOW_MAX);
    CHECK(t >= 0, "oracle status");
    taken = (size_t)t;
    for (size_t i = 0; i < n; ++i) pts[i] = {perm[i], ks[i]};
  } else {
    index_points(*g_ctx, xyz.data(), n, pts.data(), aabb(b), OutlierPointsBehaviour::ClampToBounds);
    sort_indexed_points(*g_ctx, pts.data(), pts.data() + n);
    IndexedPoint64* p = sample_points(*g_ctx, make_sampling_strategy_from_name("RANDOM_GRID", 16), pts.data(), pts.data() + n, 0, 0,
                                      aabb(b), (float)side, SamplingBehaviour::TakeAllWhenCountBelowMaxPoints, xyz.data(), n);
    taken = (size_t)(p - pts.data());
  }
  CHECK(taken == 8, "%zu survivors", taken);
  for (int i = 0; i < 8; ++i)
    for (int a = 0; a < 3; ++a)
      CHECK(xyz[3 * pts[i].point_index + a] == expected[i][a], "survivor %d", i);
  std::vector<char> seen(n, 0);
  for (size_t i = 0; i < n; ++i) {
    CHECK(pts[i].point_index < n && !seen[pts[i].point_index], "the range is no permutation any more");
    seen[pts[i].point_index] = 1;
    if (i > 8) CHECK(pts[i - 1].morton_index < pts[i].morton_index, "the remaining half lost its order at %zu", i);
  }
  ok("sample_points lattice known answer", "8 survivors in Morton order");
}

static void case_sample_jitter_refusal() {
  // JITTERED with fewer than 16 cells along the node (Sampling.h:632-635 throws): the library refuses, the adapter
  // throws the library's text and leaves the range alone
  const Box b = seam::unit_box();
  Rng r(5);
  const SortedCloud s = sorted_cloud(b, seam::uniform_cloud(r, 5000, b), 10, 6);
  const size_t n = s.keys.size();
  std::vector<uint64_t> k = s.keys;
  std::vector<uint32_t> ix = s.idx;
  const int64_t t = orc_sample_points(ORC_JITTERED, 10, k.data(), ix.data(), n, s.pos.data(), 0, -1, 21, b.mn, b.mx, 0.2f, ORC_ALWAYS_ADHERE);
  CHECK(t == ORC_ERR_JITTER_GRID_TOO_SMALL, "oracle status %lld", (long long)t);
  if (!g_oracle_only) {
    std::vector<IndexedPoint64> range(n), before;
    for (size_t i = 0; i < n; ++i) range[i] = {s.idx[i], s.keys[i]};
    before = range;
    std::string what;
    try {
      sample_points(*g_ctx, make_sampling_strategy_from_name("JITTERED", 10), range.data(), range.data() + n, 0, -1, aabb(b), 0.2f,
                    SamplingBehaviour::AlwaysAdhereToMinSpacing, s.pos.data(), s.pos.size() / 3);
      CHECK(false, "no exception");
    } catch (const std::runtime_error& e) {
      what = e.what();
    }
    CHECK(what.find("Grids smaller than 16x16 are not supported currently!") != std::string::npos, "message: %s", what.c_str());
    for (size_t i = 0; i < n; ++i)
      CHECK(range[i].point_index == before[i].point_index && range[i].morton_index == before[i].morton_index, "the range was touched");
    // the context is usable afterwards
    IndexedPoint64* p = sample_points(*g_ctx, make_sampling_strategy_from_name("RANDOM_GRID", 10), range.data(), range.data() + n, 0, -1,
                                      aabb(b), 0.2f, SamplingBehaviour::AlwaysAdhereToMinSpacing, s.pos.data(), s.pos.size() / 3);
    CHECK(p > range.data() && p < range.data() + n, "the call after the refusal");
  }
  ok("sample_points JITTERED small grid", "refused with the library's text, range untouched");
}

// ------------------------------------------------------------------------------------------ boxes, names, factory (no GPU)
static void case_octant_bounds(const char* bname, const Box& b) {
  Rng r(99);
  const size_t nkeys = 3000;
  size_t compared = 0;
  for (size_t i = 0; i < nkeys; ++i) {
    uint64_t key = r.next() >> 1;
    if (i == 0) key = 0;
    if (i == 1) key = 0x7FFFFFFFFFFFFFFFull;
    for (uint32_t depth = 0; depth <= 21; ++depth) {
      AABB box = aabb(b);
      for (uint32_t l = 0; l < depth; ++l) {
        const uint8_t o = get_octant_at_level(key, l);
        CHECK(o == orc_get_octant_at_level(key, l, 21), "octant digit %u of %llx", l, (unsigned long long)key);
        box = get_octant_bounds(o, box);
      }
      double omn[3], omx[3], lmn[3], lmx[3];
      orc_get_bounds_from_morton_index(key, 21, b.mn, b.mx, depth, omn, omx);
      CHECK(swz_node_bounds((int8_t)((int)depth - 1), key, b.mn, b.mx, lmn, lmx) == SWZ_OK, "swz_node_bounds status");
      const double got[6] = {box.min.x, box.min.y, box.min.z, box.max.x, box.max.y, box.max.z};
      for (int a = 0; a < 3; ++a) {
        CHECK(bits(got[a]) == bits(omn[a]) && bits(got[3 + a]) == bits(omx[a]), "depth %u axis %d: adapter %.17g..%.17g, oracle %.17g..%.17g",
              depth, a, got[a], got[3 + a], omn[a], omx[a]);
        CHECK(bits(lmn[a]) == bits(omn[a]) && bits(lmx[a]) == bits(omx[a]), "depth %u axis %d: swz_node_bounds differs from the oracle", depth, a);
      }
      ++compared;
    }
  }
  ok(std::string("get_octant_bounds ") + bname, "%zu boxes equal the oracle's and swz_node_bounds bit for bit", compared);
}

static void case_node_names() {
  Rng r(7);
  size_t compared = 0;
  for (size_t i = 0; i < 3000; ++i) {
    const uint64_t key = i == 0 ? 0 : (i == 1 ? 0x7FFFFFFFFFFFFFFFull : r.next() >> 1);
    for (int level = -1; level <= 20; ++level) {
      std::string name = "r";
      for (int l = 0; l <= level; ++l) name.push_back((char)('0' + get_octant_at_level(key, (uint32_t)l)));
      char buf[32];
      CHECK(swz_node_name((int8_t)level, key, buf) == SWZ_OK, "swz_node_name status");
      CHECK(name == buf && name == seam::node_name(level, key), "level %d key %llx: %s / %s", level, (unsigned long long)key, name.c_str(), buf);
      ++compared;
    }
  }
  CHECK(seam::node_name(2, 0x7000000000000000ull >> 6 | 5ull << 60) == "r507", "digit order");
  ok("node names", "%zu names equal swz_node_name", compared);
}

static void case_sampler_factory() {
  for (int s = 0; s < 4; ++s) {
    const SamplingStrategy st = make_sampling_strategy_from_name(SAMPLER_NAMES[s], 123);
    CHECK(st.kind == s && st.max_points_per_node == 123, "%s", SAMPLER_NAMES[s]);
  }
  for (const char* bad : {"", "random_grid", "MIN_DISTANCE_FAST", "POISSON"}) {
    bool threw = false;
    try {
      make_sampling_strategy_from_name(bad, 1);
    } catch (const std::runtime_error&) {
      threw = true;
    }
    CHECK(threw, "\"%s\" was accepted", bad);
  }
  ok("make_sampling_strategy_from_name", "4 names, unknown names throw");
}

int main(int argc, char** argv) {
  for (int i = 1; i < argc; ++i) {
    if (std::string(argv[i]) == "--oracle-only") g_oracle_only = true;
    else {
      std::fprintf(stderr, "usage: %s [--oracle-only]\n", argv[0]);
      return 2;
    }
  }
  try {
    std::unique_ptr<Context> ctx;
    if (!g_oracle_only) {
      ctx.reset(new Context(0));
      g_ctx = ctx.get();
    }
    const Box odd = seam::odd_box(), unit = seam::unit_box();
    for (size_t n : {(size_t)0, (size_t)1, (size_t)255, (size_t)256, (size_t)257, (size_t)100003}) {
      case_index_points("odd", odd, n);
      case_index_points("unit", unit, n);
    }
    case_index_lattice();
    case_index_abort();
    for (const char* kind : {"random", "ties", "equal"})
      for (size_t n : {(size_t)0, (size_t)1, (size_t)2, (size_t)4095, (size_t)4096, (size_t)4097, (size_t)300001}) case_sort(kind, n);
    {
      Rng r(17);
      cases_sample("uniform-odd", sorted_cloud(odd, seam::uniform_cloud(r, 80000, odd), 500, 18));
      cases_sample("clustered-unit", sorted_cloud(unit, seam::clustered_surfaces(r, 60000, unit), 500, 19));
    }
    case_sample_known_answer();
    case_sample_jitter_refusal();
    case_octant_bounds("odd", odd);
    case_octant_bounds("unit", unit);
    case_node_names();
    case_sampler_factory();
  } catch (const std::exception& e) {
    std::fflush(stdout);
    std::fprintf(stderr, "FAIL: %s\n", e.what());
    return 1;
  }
  std::printf("%d cases passed (%s)\n", g_ok, mode());
  return 0;
}
