// swz_host::TilingAlgorithmGPU (schwarzwald_amd/host/swz_tiling.hpp) on what real runs feed it: FAST, bounds away
// from the origin, outliers, uneven / tiny / empty / refused batches, terminal nodes, re-rooted subtrees, every
// branch of finalize()'s chunked export, calls after finalize and pools spilled to host memory.  A memory sink
// collects what finalize() hands over; for every case it must equal the multi-batch oracle's export
// (orc_tiler_export): the same node names, per node the same ids in file order, the oracle's clamped positions by
// id (as bits), the oracle's node box (as bits), and the same counts.  No tolerance anywhere.
//
//   test_adapter_tiler                runs every case on the GPU
//   test_adapter_tiler --oracle-only  builds every input, runs the oracle and asserts that each input really holds its
//                                     hard case; creates no swz_host::Context
//
// One "<case> ok: ..." line per case (the same lines in both modes), "FAIL: ..." and exit code 1 at the first failure.
#include <array>
#include <cstdarg>
#include <map>

#include "../../oracle/oracle.h"
#include "../../schwarzwald_amd/host/swz_tiling.hpp"
#include "seam_util.hpp"

using namespace swz_host;
using seam::Box;
using seam::Rng;
using seam::bits;

static bool g_oracle_only = false;
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
static const char* SAMPLER_NAMES[4] = {"RANDOM_GRID", "GRID_CENTER", "MIN_DISTANCE", "JITTERED"};

struct MemorySink : PointsSink {  // cf. core/io/MemoryPersistence.h:14-52
  struct Node {
    std::vector<uint32_t> ids;
    std::vector<double> xyz;
    AABB box;
  };
  std::map<std::string, Node> nodes;
  size_t calls = 0;
  std::string handed_twice;
  void persist_points(const uint32_t* b, const uint32_t* e, const double* xyz, const AABB& nb, const std::string& name) override {
    ++calls;
    if (nodes.count(name)) handed_twice = name;
    Node& n = nodes[name];
    n.ids.assign(b, e);
    n.xyz.assign(xyz, xyz + 3 * (e - b));
    n.box = nb;
  }
};

struct Batch {
  size_t lo, n;
  bool refused;  // FAST: fewer points than num_indexing_threads -- tile_batch must throw and change nothing
};
enum ChunkRule { CHUNK_DEFAULT, CHUNK_ONE, CHUNK_LARGEST, CHUNK_LARGEST_PLUS_1, CHUNK_FIRST_TWO, CHUNK_ALL, CHUNK_ALL_PLUS_1 };

struct Spec {
  std::string name;
  int sampler = ORC_RANDOM_GRID;
  int strategy = ORC_ACCURATE;
  Box b;
  uint64_t max_points = 300;
  float spacing = 0;
  uint32_t max_depth = 100;
  uint32_t concurrency = 2;
  const std::vector<double>* cloud = nullptr;
  std::vector<Batch> batches;
  // what the input must hold (asserted on the oracle's side)
  bool need_outliers = false, need_terminal = false, need_deep = false, need_duplicates_across_batches = false;
  // how the adapter is driven
  ChunkRule chunk = CHUNK_DEFAULT;
  bool spill = false;
  bool calls_after_finalize = false;
};

struct Expected {
  uint64_t nn = 0, ns = 0, np = 0, accepted_batches = 0;
  std::vector<int8_t> nl;
  std::vector<uint64_t> nk, no, nc;
  std::vector<uint32_t> ids;
  std::vector<double> xyz;  // clamped, by id
  int max_level = -1;
};

static Expected run_oracle(const Spec& s) {
  Expected e;
  const orc_tile_params p{s.sampler, s.max_points, s.spacing, s.max_depth, s.strategy, s.concurrency};
  orc_tiler* t = orc_tiler_create(s.b.mn, s.b.mx, &p);
  CHECK(t != nullptr, "orc_tiler_create");
  int beyond[6] = {0, 0, 0, 0, 0, 0};
  for (const Batch& bt : s.batches) {
    std::vector<double> copy(s.cloud->begin() + 3 * bt.lo, s.cloud->begin() + 3 * (bt.lo + bt.n));
    copy.reserve(3);
    const int32_t st = orc_tiler_add_batch(t, copy.data(), bt.n);
    if (bt.refused) {
      CHECK(s.strategy == ORC_FAST && bt.n < s.concurrency, "a refused batch must be a FAST batch below the thread count");
      CHECK(st == ORC_ERR_BAD_ARG, "the oracle's rule accepts the batch of %zu points (status %d)", bt.n, st);
      continue;
    }
    CHECK(st == ORC_OK, "oracle add_batch status %d", st);
    ++e.accepted_batches;
    for (size_t i = bt.lo; i < bt.lo + bt.n; ++i)
      for (int a = 0; a < 3; ++a) {
        beyond[2 * a] += (*s.cloud)[3 * i + a] < s.b.mn[a];
        beyond[2 * a + 1] += (*s.cloud)[3 * i + a] > s.b.mx[a];
      }
  }
  CHECK(orc_tiler_finalize(t) == ORC_OK, "oracle finalize");
  uint64_t unsorted = 0;
  orc_tiler_counts(t, &e.nn, &e.ns, &e.np, &unsorted);
  // (otherwise the library is allowed to differ, include/swz_gpu.h "rekey_inversions": pick another seed)
  CHECK(unsorted == 0, "unsorted_cached_nodes = %llu", (unsigned long long)unsorted);
  e.nl.resize(e.nn);
  e.nk.resize(e.nn);
  e.no.resize(e.nn);
  e.nc.resize(e.nn);
  e.ids.resize(e.ns);
  e.xyz.resize(3 * e.np);
  e.nl.reserve(1), e.nk.reserve(1), e.no.reserve(1), e.nc.reserve(1), e.ids.reserve(1), e.xyz.reserve(1);
  orc_tiler_export(t, e.nl.data(), e.nk.data(), e.no.data(), e.nc.data(), e.ids.data(), e.xyz.data());
  orc_tiler_destroy(t);
  for (uint64_t j = 0; j < e.nn; ++j) e.max_level = std::max<int>(e.max_level, e.nl[j]);

  // ---- the case holds what it claims
  if (s.strategy == ORC_FAST && e.np) CHECK(e.ns > e.np, "FAST stored no copies: %llu stored, %llu points", (unsigned long long)e.ns, (unsigned long long)e.np);
  if (s.strategy == ORC_ACCURATE) CHECK(e.ns == e.np, "ACCURATE stores every point once");
  if (s.need_outliers)
    for (int f = 0; f < 6; ++f) CHECK(beyond[f] > 0, "no point beyond face %d", f);
  if (s.need_terminal) {
    bool found = false;
    for (uint64_t j = 0; j < e.nn; ++j) found |= e.nl[j] == (int)s.max_depth && e.nc[j] > s.max_points;
    CHECK(found && e.max_level == (int)s.max_depth, "no node at max_depth with more than max_points_per_node points");
  }
  if (s.need_deep) {
    const int first_rerooted = 9;  // for this data: the first level whose sampling grid needs more than 21 key levels
    CHECK(orc_required_morton_index_depth(s.sampler, first_rerooted, s.b.mn, s.b.mx, s.spacing) >= 21 &&
            orc_required_morton_index_depth(s.sampler, first_rerooted - 1, s.b.mn, s.b.mx, s.spacing) < 21, "the first re-rooted level is not 9");
    CHECK(e.max_level > first_rerooted, "deepest node level %d", e.max_level);
  }
  if (s.need_duplicates_across_batches) {
    std::map<std::array<uint64_t, 3>, size_t> first_batch;
    bool found = false;
    for (size_t k = 0; k < s.batches.size() && !found; ++k)
      for (size_t i = s.batches[k].lo; i < s.batches[k].lo + s.batches[k].n; ++i) {
        const std::array<uint64_t, 3> key = {bits((*s.cloud)[3 * i]), bits((*s.cloud)[3 * i + 1]), bits((*s.cloud)[3 * i + 2])};
        auto it = first_batch.emplace(key, k).first;
        if (it->second != k) {
          found = true;
          break;
        }
      }
    CHECK(found, "no point is repeated exactly in another batch");
  }
  return e;
}

// the chunk size of finalize()'s export, taken from the oracle's node table
static uint64_t chunk_value(const Expected& e, ChunkRule rule, std::string* why) {
  uint64_t jl = 0;
  for (uint64_t j = 0; j < e.nn; ++j)
    if (e.nc[j] > e.nc[jl]) jl = j;
  char buf[160];
  uint64_t v = 0;
  switch (rule) {
    case CHUNK_DEFAULT: *why = "default chunk"; return 0;
    case CHUNK_ONE: v = 1; std::snprintf(buf, sizeof buf, "chunk 1 (raised to the largest file)"); break;
    case CHUNK_LARGEST:
      v = e.nc[jl];
      std::snprintf(buf, sizeof buf, "chunk %llu = count of node %llu (%s), the largest file", (unsigned long long)v, (unsigned long long)jl,
                    seam::node_name(e.nl[jl], e.nk[jl]).c_str());
      break;
    case CHUNK_LARGEST_PLUS_1:
      v = e.nc[jl] + 1;
      std::snprintf(buf, sizeof buf, "chunk %llu = count of node %llu (%s) + 1", (unsigned long long)v, (unsigned long long)jl,
                    seam::node_name(e.nl[jl], e.nk[jl]).c_str());
      break;
    case CHUNK_FIRST_TWO:
      v = e.nc[0] + e.nc[1];
      std::snprintf(buf, sizeof buf, "chunk %llu = count of node 0 (%s) + count of node 1 (%s)", (unsigned long long)v,
                    seam::node_name(e.nl[0], e.nk[0]).c_str(), seam::node_name(e.nl[1], e.nk[1]).c_str());
      break;
    case CHUNK_ALL: v = e.ns; std::snprintf(buf, sizeof buf, "chunk %llu = num_stored (all %llu nodes)", (unsigned long long)v, (unsigned long long)e.nn); break;
    case CHUNK_ALL_PLUS_1: v = e.ns + 1; std::snprintf(buf, sizeof buf, "chunk %llu = num_stored + 1", (unsigned long long)v); break;
  }
  CHECK(e.nn >= 3 && e.nc[jl] > e.nc[0], "the largest file (%llu) is not larger than file 0 (%llu): raising the cap would not matter",
        (unsigned long long)e.nc[jl], (unsigned long long)e.nc[0]);
  CHECK(e.nc[0] + e.nc[1] >= e.nc[jl] || rule != CHUNK_FIRST_TWO, "count[0] + count[1] is below the largest file and would be raised");
  *why = buf;
  return v;
}

static bool same_info(const swz_tiler_info& a, const swz_tiler_info& b) {
  return a.num_points == b.num_points && a.num_stored == b.num_stored && a.num_nodes == b.num_nodes && a.num_batches == b.num_batches;
}

static void run_gpu(const Spec& s, const Expected& e, uint64_t chunk) {
  const std::vector<double> pristine = *s.cloud;
  MemorySink sink;
  TilerMetaParameters meta;
  meta.spacing_at_root = s.spacing;
  meta.max_depth = s.max_depth;
  meta.max_points_per_node = s.max_points;
  meta.tiling_strategy = s.strategy == ORC_FAST ? TilingStrategy::Fast : TilingStrategy::Accurate;
  meta.num_indexing_threads = s.concurrency;
  TilingAlgorithmGPU tiler(make_sampling_strategy_from_name(SAMPLER_NAMES[s.sampler], s.max_points), sink, meta);
  if (s.spill) tiler.set_option("SWZ_TILER_SPILL", "host");  // the pools live in mapped host memory from the first batch on
  if (s.chunk != CHUNK_DEFAULT) tiler.set_export_chunk_points(chunk);
  const AABB box = aabb(s.b);
  for (const Batch& bt : s.batches) {
    const double* p = s.cloud->data() + 3 * bt.lo;
    if (!bt.refused) {
      tiler.tile_batch(p, bt.n, box);
      continue;
    }
    const swz_tiler_info before = tiler.info();
    bool threw = false;
    try {
      tiler.tile_batch(p, bt.n, box);
    } catch (const std::runtime_error& ex) {
      threw = true;
      CHECK(std::string(ex.what()).find("fast_concurrency") != std::string::npos, "message: %s", ex.what());
    }
    CHECK(threw, "the FAST batch of %zu points was not refused", bt.n);
    CHECK(same_info(before, tiler.info()), "a refused batch changed info()");
  }
  CHECK(tiler.info().num_points == e.np, "num_points before finalize");
  CHECK(sink.calls == 0, "files handed over before finalize");
  const size_t persisted = tiler.finalize(box);
  const swz_tiler_info info = tiler.info();

  CHECK(persisted == e.nn, "finalize returned %zu, the oracle has %llu nodes", persisted, (unsigned long long)e.nn);
  CHECK(sink.handed_twice.empty(), "node %s was handed over twice", sink.handed_twice.c_str());
  CHECK(sink.calls == e.nn && sink.nodes.size() == e.nn, "%zu persist_points calls, %zu names, %llu nodes expected", sink.calls,
        sink.nodes.size(), (unsigned long long)e.nn);
  CHECK(info.num_stored == e.ns && info.num_points == e.np, "info: %llu stored / %llu points, oracle %llu / %llu",
        (unsigned long long)info.num_stored, (unsigned long long)info.num_points, (unsigned long long)e.ns, (unsigned long long)e.np);
  CHECK(info.num_batches == e.accepted_batches, "num_batches %llu, accepted %llu", (unsigned long long)info.num_batches,
        (unsigned long long)e.accepted_batches);
  if (!s.need_terminal) CHECK(info.rekey_inversions == 0, "rekey_inversions %llu", (unsigned long long)info.rekey_inversions);
  for (uint64_t j = 0; j < e.nn; ++j) {
    const std::string name = seam::node_name(e.nl[j], e.nk[j]);
    const auto it = sink.nodes.find(name);
    CHECK(it != sink.nodes.end(), "node %s is missing", name.c_str());
    const MemorySink::Node& nd = it->second;
    CHECK(nd.ids.size() == e.nc[j], "node %s holds %zu points, oracle %llu", name.c_str(), nd.ids.size(), (unsigned long long)e.nc[j]);
    for (uint64_t q = 0; q < e.nc[j]; ++q) {
      const uint32_t id = e.ids[e.no[j] + q];
      CHECK(nd.ids[q] == id, "node %s entry %llu: id %u, oracle %u", name.c_str(), (unsigned long long)q, nd.ids[q], id);
      for (int a = 0; a < 3; ++a)
        CHECK(bits(nd.xyz[3 * q + a]) == bits(e.xyz[3 * (size_t)id + a]), "node %s entry %llu (id %u) axis %d: %.17g, oracle's clamped %.17g",
              name.c_str(), (unsigned long long)q, id, a, nd.xyz[3 * q + a], e.xyz[3 * (size_t)id + a]);
    }
    double omn[3], omx[3];
    orc_get_bounds_from_morton_index(e.nk[j], 21, s.b.mn, s.b.mx, (uint32_t)(e.nl[j] + 1), omn, omx);
    const double got[6] = {nd.box.min.x, nd.box.min.y, nd.box.min.z, nd.box.max.x, nd.box.max.y, nd.box.max.z};
    for (int a = 0; a < 3; ++a)
      CHECK(bits(got[a]) == bits(omn[a]) && bits(got[3 + a]) == bits(omx[a]), "box of node %s axis %d", name.c_str(), a);
  }
  CHECK(std::memcmp(pristine.data(), s.cloud->data(), pristine.size() * 8) == 0, "the caller's positions were changed");

  if (s.calls_after_finalize) {
    bool threw = false;
    try {
      tiler.tile_batch(s.cloud->data(), 100, box);
    } catch (const std::runtime_error&) {
      threw = true;
    }
    CHECK(threw, "tile_batch after finalize did not throw");
    CHECK(tiler.finalize(box) == 0, "the second finalize returned nodes");
    CHECK(sink.calls == e.nn && sink.handed_twice.empty(), "the second finalize handed files over again");
    CHECK(same_info(info, tiler.info()), "calls after finalize changed info()");
  }
}

static void run_case(const Spec& s) {
  const Expected e = run_oracle(s);
  if (!g_oracle_only) run_gpu(s, e, 0);
  ok(s.name, "%llu nodes, %llu stored, %llu points, deepest level %d", (unsigned long long)e.nn, (unsigned long long)e.ns,
     (unsigned long long)e.np, e.max_level);
}

static std::vector<Batch> even_batches(size_t n, int k) {
  std::vector<Batch> out;
  for (int i = 0; i < k; ++i) out.push_back({n * i / k, n * (i + 1) / k - n * i / k, false});
  return out;
}

// every tenth point is pushed beyond one of the six faces in turn
static void add_outliers(Rng& r, std::vector<double>& xyz, const Box& b) {
  const size_t n = xyz.size() / 3;
  for (size_t i = 0; i < n; i += 10) {
    const int face = (int)((i / 10) % 6), a = face / 2;
    const double d = (0.001 + 0.4 * r.uniform()) * b.ext(a);
    xyz[3 * i + a] = (face & 1) ? b.mx[a] + d : b.mn[a] - d;
  }
}

// set_option reaches the tiler's own context: with spilling switched off and the position pool's first allocation
// reported as out of memory (SWZ_FAIL_ALLOC, the library's switch for this), the first batch must be refused
static void case_set_option_is_forwarded(const std::vector<double>& cloud, const Box& b) {
  if (!g_oracle_only) {
    MemorySink sink;
    TilerMetaParameters meta;
    meta.spacing_at_root = seam::spacing_from_diagonal(b, 32);
    meta.max_points_per_node = 300;
    TilingAlgorithmGPU tiler(make_sampling_strategy_from_name("GRID_CENTER", 300), sink, meta);
    tiler.set_option("SWZ_TILER_SPILL", "off");
    tiler.set_option("SWZ_FAIL_ALLOC", "tiler_pool_xyz");
    std::string what;
    try {
      tiler.tile_batch(cloud.data(), 1000, aabb(b));
    } catch (const std::runtime_error& ex) {
      what = ex.what();
    }
    CHECK(what.find("tiler_pool_xyz") != std::string::npos, "the options did not reach the context: \"%s\"", what.c_str());
    tiler.set_option("SWZ_FAIL_ALLOC", nullptr);
    bool threw = false;
    try {
      tiler.set_option(nullptr, "x");
    } catch (const std::runtime_error&) {
      threw = true;
    }
    CHECK(threw, "set_option without a name did not throw");
  }
  ok("set_option reaches the tiler's context", "SWZ_TILER_SPILL=off + SWZ_FAIL_ALLOC=tiler_pool_xyz refuse the first batch");
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
    const Box odd = seam::odd_box(), unit = seam::unit_box(), deep = seam::cube_box(1024.0);
    const size_t n = 60000;
    Rng r(2024);
    std::vector<double> uniform_odd = seam::uniform_cloud(r, n, odd);
    add_outliers(r, uniform_odd, odd);
    const std::vector<double> clustered_odd = seam::clustered_duplicates(r, n, odd);
    const std::vector<double> clustered_unit = seam::clustered_duplicates(r, n, unit);
    std::vector<double> deep_cloud(3 * n);  // a corner 1e-5 of the root's extent wide: the grid samplers re-root from level 9 on
    for (double& v : deep_cloud) v = r.uniform() * 0.01;
    Box low_octant = odd;
    for (int a = 0; a < 3; ++a) low_octant.mx[a] = odd.mn[a] + 0.5 * odd.ext(a);
    const std::vector<double> octant_cloud = seam::uniform_cloud(r, n, low_octant);
    const char* STRATEGY[2] = {"ACCURATE", "FAST"};

    // ---- every sampler x strategy: bounds off the origin, uneven batches, 10 % outliers
    for (int sampler = 0; sampler < 4; ++sampler)
      for (int strategy = 0; strategy < 2; ++strategy) {
        Spec s;
        s.name = std::string("uneven batches + outliers ") + SAMPLER_NAMES[sampler] + " " + STRATEGY[strategy];
        s.sampler = sampler;
        s.strategy = strategy;
        s.b = odd;
        s.spacing = seam::spacing_from_diagonal(odd, 32);
        s.cloud = &uniform_odd;
        // ACCURATE: a batch of one point; FAST: of exactly num_indexing_threads points, the smallest it accepts
        const size_t tiny = strategy == ORC_FAST ? s.concurrency : 1;
        s.batches = {{0, n / 2, false}, {n / 2, tiny, false}, {n / 2 + tiny, n - n / 2 - tiny, false}};
        s.need_outliers = true;
        run_case(s);
      }
    // ---- exact duplicates: equal keys across batches
    for (int sampler : {ORC_GRID_CENTER, ORC_MIN_DISTANCE})
      for (int strategy = 0; strategy < 2; ++strategy) {
        Spec s;
        s.name = std::string("duplicates over 5 batches ") + SAMPLER_NAMES[sampler] + " " + STRATEGY[strategy];
        s.sampler = sampler;
        s.strategy = strategy;
        s.b = odd;
        s.spacing = seam::spacing_from_diagonal(odd, 32);
        s.cloud = &clustered_odd;
        s.batches = even_batches(n, 5);
        s.need_duplicates_across_batches = true;
        run_case(s);
      }
    // ---- terminal nodes: max_depth 2
    for (int sampler : {ORC_RANDOM_GRID, ORC_MIN_DISTANCE}) {
      Spec s;
      s.name = std::string("terminal nodes at max_depth 2 ") + SAMPLER_NAMES[sampler];
      s.sampler = sampler;
      s.b = unit;
      s.max_points = 100;
      s.max_depth = 2;
      s.spacing = seam::spacing_from_diagonal(unit, 32);
      s.cloud = &clustered_unit;
      // two batches: the second one appends to the terminal files (new ++ cached, Node.cpp:24-35).  A third batch would
      // read those files back out of order, which the oracle counts in unsorted_cached_nodes and where the library is
      // allowed to differ.
      s.batches = even_batches(n, 2);
      s.need_terminal = true;
      run_case(s);
    }
    // ---- re-rooted subtrees
    for (int sampler : {ORC_RANDOM_GRID, ORC_GRID_CENTER, ORC_JITTERED})
      for (int k : {1, 3}) {
        Spec s;
        s.name = std::string("re-rooted subtrees ") + SAMPLER_NAMES[sampler] + " " + std::to_string(k) + " batch(es)";
        s.sampler = sampler;
        s.b = deep;
        s.max_points = 200;
        s.spacing = (float)(1024.0 / 4096.0);
        s.cloud = &deep_cloud;
        s.batches = even_batches(n, k);
        s.need_deep = true;
        run_case(s);
      }
    // ---- the chunk loop of finalize(), chunk sizes from the oracle's node table
    for (int strategy = 0; strategy < 2; ++strategy) {
      Spec s;
      s.sampler = ORC_RANDOM_GRID;
      s.strategy = strategy;
      s.b = odd;
      s.spacing = seam::spacing_from_diagonal(odd, 8);
      s.cloud = &octant_cloud;  // the root's grid is mostly empty: its file (node 0) is smaller than the files below it
      s.batches = even_batches(n, 3);
      const Expected e = run_oracle(s);
      for (ChunkRule rule : {CHUNK_ONE, CHUNK_LARGEST, CHUNK_LARGEST_PLUS_1, CHUNK_FIRST_TWO, CHUNK_ALL, CHUNK_ALL_PLUS_1}) {
        s.chunk = rule;
        std::string why;
        const uint64_t chunk = chunk_value(e, rule, &why);
        if (!g_oracle_only) run_gpu(s, e, chunk);
        ok(std::string("export chunks ") + STRATEGY[strategy] + " rule " + std::to_string((int)rule), "%s; %llu nodes, %llu stored", why.c_str(),
           (unsigned long long)e.nn, (unsigned long long)e.ns);
      }
    }
    // ---- empty batch under ACCURATE between two real ones: counted, changes nothing
    {
      Spec s;
      s.name = "empty batch between two batches ACCURATE";
      s.sampler = ORC_GRID_CENTER;
      s.b = odd;
      s.spacing = seam::spacing_from_diagonal(odd, 32);
      s.cloud = &uniform_odd;
      s.batches = {{0, n / 2, false}, {n / 2, 0, false}, {n / 2, n - n / 2, false}};
      run_case(s);
    }
    // ---- FAST refuses a batch below num_indexing_threads and the empty batch; the data set goes on without them
    for (int first : {0, 1}) {
      Spec s;
      s.name = first ? "FAST refusals before the first batch" : "FAST refusals between two batches";
      s.sampler = first ? ORC_JITTERED : ORC_RANDOM_GRID;
      s.strategy = ORC_FAST;
      s.concurrency = 8;
      s.b = odd;
      s.spacing = seam::spacing_from_diagonal(odd, 32);
      s.cloud = &uniform_odd;
      if (first) s.batches = {{0, 7, true}, {7, 0, true}, {7, n / 2, false}, {7 + n / 2, n - n / 2 - 7, false}};
      else s.batches = {{0, n / 2, false}, {n / 2, 7, true}, {n / 2 + 7, 0, true}, {n / 2 + 7, n - n / 2 - 7, false}};
      run_case(s);
    }
    // ---- nothing to hand over
    for (int with_empty_batch : {0, 1}) {
      Spec s;
      s.name = with_empty_batch ? "only an empty batch, then finalize" : "no batch, then finalize";
      s.b = odd;
      s.spacing = seam::spacing_from_diagonal(odd, 32);
      s.cloud = &uniform_odd;
      if (with_empty_batch) s.batches = {{0, 0, false}};
      s.calls_after_finalize = with_empty_batch;
      run_case(s);
    }
    // ---- calls after finalize
    {
      Spec s;
      s.name = "tile_batch and finalize after finalize";
      s.sampler = ORC_JITTERED;
      s.b = odd;
      s.spacing = seam::spacing_from_diagonal(odd, 32);
      s.cloud = &uniform_odd;
      s.batches = even_batches(n, 2);
      s.calls_after_finalize = true;
      run_case(s);
    }
    // ---- pools in mapped host memory: finalize gathers the files out of them
    for (int strategy = 0; strategy < 2; ++strategy) {
      Spec s;
      s.name = std::string("pools spilled to host memory GRID_CENTER ") + STRATEGY[strategy];
      s.sampler = ORC_GRID_CENTER;
      s.strategy = strategy;
      s.b = odd;
      s.spacing = seam::spacing_from_diagonal(odd, 32);
      s.cloud = &clustered_odd;
      s.batches = even_batches(n, 3);
      s.spill = true;
      run_case(s);
    }
    case_set_option_is_forwarded(uniform_odd, odd);
  } catch (const std::exception& e) {
    std::fflush(stdout);
    std::fprintf(stderr, "FAIL: %s\n", e.what());
    return 1;
  }
  std::printf("%d cases passed (%s)\n", g_ok, mode());
  return 0;
}
