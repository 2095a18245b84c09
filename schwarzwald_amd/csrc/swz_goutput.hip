// swz_goutput.hip -- the data set of a group's tilers (swz_gtiler.hip): its node table merged from the shards' tables, and
// its files written in one call.  swz_group_write_output: swz_tiler_write_output's three parts (swz_toutput.h) -- validate
// and plan ONCE on the merged node table, stream the node files per shard, write the metadata ONCE.  The call has a thread
// per shard of its own, output_thread.  Its barriers (every thread, failed or not, passes both):
//   O1  every shard's part of the root's file is gathered (then shard 0 copies the parts, packs and writes the root)
//   O2  every shard's files are written; nobody reads a neighbour's part any more (then the call's workspace goes back)
#include <algorithm>
#include <limits>
#include <map>
#include <thread>

#include "swz_group.h"
#include "swz_toutput.h"

using namespace swz;

namespace {

struct GroupOutput {  // what the threads of one call share
  const swz_output_params* params = nullptr;
  std::vector<swz::OutputPlan> plan;  // per shard: its own node table, the root's part first when it has one
  std::vector<swz_tiler_info> info;
  swz::OutputPlan root;  // the root as a one-node table (no node: the root has no points)
  std::vector<uint64_t> part_cnt, part_off;  // rows of every shard's part of the root's file
  std::vector<const void*> part_xyz;
  std::vector<std::vector<const void*>> part_attr;  // [attribute][shard]
  std::vector<long> writer_threads;
  std::vector<swz_output_stats> stats;
};

void output_thread(swz_group* g, int r, GroupOutput* o) {
  Step s(g, r);
  swz_ctx* c = s.c;
  swz_tiler* t = g->ds.tiler[r];
  const auto t_begin = std::chrono::steady_clock::now();
  swz::OutputWorkspace ow{c};
  swz::OutputPlan& p = o->plan[r];  // (a tight plan gets its boxes from the stream)
  const uint64_t nn = p.count.size(), k0 = (nn && p.level[0] < 0) ? 1 : 0, ns = o->info[r].num_stored;
  const uint64_t root_rows = o->part_off[s.N];
  std::vector<uint64_t> first, root_first;
  uint64_t image_max = 0, root_image = 0;
  swz::output_cuts(c, p, k0, nn, o->params->chunk_points, &first, &image_max);
  if (r == 0 && root_rows) swz::output_cuts(c, o->root, 0, 1, o->params->chunk_points, &root_first, &root_image);

  // ---- the ids of all files, and this shard's part of the root's file as rows
  swz::OutputSource src;
  src.xyz = t->pool_xyz;
  for (int a = 0; a < SWZ_ATTR_COUNT; ++a) src.in.column[a] = (t->attr_mask & (1u << a)) ? t->pool_attr[a] : nullptr;
  uint32_t* d_ids = s.buf<uint32_t>("out_ids", (size_t)std::max<uint64_t>(ns, 1));
  src.ids = d_ids;
  if (s.ok && ns) s.swz(swz_tiler_export_device(t, nullptr, d_ids, nullptr));
  const uint64_t m = o->part_cnt[r];
  if (m) {
    swz_attribute_columns masked{}, part{};
    double* part_xyz = s.buf<double>("out_part_xyz", (size_t)m * 3);
    for (int a = 0; a < SWZ_ATTR_COUNT; ++a) {
      if (!((o->params->attribute_mask >> a) & 1u)) continue;
      masked.column[a] = src.in.column[a];
      part.column[a] = s.buf<void>("out_part_attr" + std::to_string(a), (size_t)m * swz_attribute_row_bytes(a));
      o->part_attr[a][r] = part.column[a];
    }
    if (s.ok) s.swz(swz_gather_payload_device(c, d_ids, nullptr, m, t->pool_xyz, &masked, part_xyz, &part));  // (the root's part is the first file)
    if (s.ok) s.hip(hipStreamSynchronize(c->stream), "hipStreamSynchronize(root part)");
    o->part_xyz[r] = part_xyz;
  }
  const bool go_root = s.vote();  // O1

  swz::OutputStreamStats ss;
  swz::OutputImages images;
  const uint64_t image_bytes = std::max(image_max, root_image);
  if (s.ok && image_bytes) s.swz(images.reserve(c, image_bytes, first.size() > 2));
  if (r == 0 && go_root && s.ok && root_rows) {
    swz::OutputSource all;
    double* all_xyz = s.buf<double>("out_root_xyz", (size_t)root_rows * 3);
    uint32_t* iota = s.buf<uint32_t>("out_root_ids", (size_t)root_rows);
    std::vector<PeerColumn> columns;
    columns.push_back({all_xyz, o->part_xyz, 24});
    for (int a = 0; a < SWZ_ATTR_COUNT; ++a) {
      if (!((o->params->attribute_mask >> a) & 1u)) continue;
      all.in.column[a] = s.buf<void>("out_root_attr" + std::to_string(a), (size_t)root_rows * swz_attribute_row_bytes(a));
      columns.push_back({all.in.column[a], o->part_attr[a], swz_attribute_row_bytes(a)});
    }
    all.xyz = all_xyz;
    all.ids = iota;
    if (s.ok) s.hip(rows_to_shard0(g, o->part_cnt, o->part_off, columns), "copy of the root's parts to shard 0");
    if (s.ok) s.hip(group_iota(c->stream, iota, root_rows), "the ids of the root's rows");
    if (s.ok) s.swz(swz::output_stream(c, o->root, root_first, all, images, o->writer_threads[r], &ss));
  }
  if (s.ok && image_max) s.swz(swz::output_stream(c, p, first, src, images, o->writer_threads[r], &ss));
  (void)hipStreamSynchronize(c->stream);
  g->barrier.wait();  // O2
  swz_output_stats& st = o->stats[r];
  st.nodes = nn;
  st.stored_points = ns;
  st.bytes_written = ss.bytes_written;
  st.chunks = ss.chunks;
  st.pack_ms = ss.pack_ms;
  st.copy_ms = ss.copy_ms;
  st.write_ms = ss.write_ms;
  st.wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
}

// the node tables of the shards' tilers; *st_shard: the shard whose tiler refused
int shard_node_tables(swz_group* g, std::vector<std::vector<int8_t>>& level, std::vector<std::vector<uint64_t>>& key,
                      std::vector<std::vector<uint64_t>>& count) {
  level.assign(g->n, {});
  key.assign(g->n, {});
  count.assign(g->n, {});
  for (int r = 0; r < g->n; ++r) {
    (void)hipSetDevice(g->devices[r]);
    swz_tiler_info info{};
    int st = swz_tiler_get_info(g->ds.tiler[r], &info);
    const uint64_t cap = std::max<uint64_t>(info.num_nodes, 1);
    std::vector<uint64_t> offset(cap);
    level[r].resize(cap);
    key[r].resize(cap);
    count[r].resize(cap);
    uint64_t nn = 0;
    if (st == SWZ_OK) st = swz_tiler_node_table(g->ds.tiler[r], cap, level[r].data(), key[r].data(), offset.data(), count[r].data(), &nn);
    if (st != SWZ_OK) {
      g->err = "shard " + std::to_string(r) + ": " + swz_last_error(g->ctx[r]);
      return st;
    }
    level[r].resize(nn);
    key[r].resize(nn);
    count[r].resize(nn);
  }
  return SWZ_OK;
}

int merge_tables(swz_group* g, const std::vector<std::vector<int8_t>>& level, const std::vector<std::vector<uint64_t>>& key,
                 const std::vector<std::vector<uint64_t>>& count, uint64_t max_nodes, int8_t* level_out, uint64_t* key_out,
                 uint64_t* count_out, int32_t* shard_out, uint64_t* num_nodes_out) {
  std::vector<uint64_t> nn(g->n);
  std::vector<const int8_t*> pl(g->n);
  std::vector<const uint64_t*> pk(g->n), pc(g->n);
  for (int r = 0; r < g->n; ++r) {
    nn[r] = level[r].size();
    pl[r] = level[r].data();
    pk[r] = key[r].data();
    pc[r] = count[r].data();
  }
  const int st = swz_merge_shard_node_tables(g->n, nn.data(), pl.data(), pk.data(), pc.data(), max_nodes, level_out, key_out, count_out, shard_out, num_nodes_out);
  if (st == SWZ_ERR_INTERNAL) g->err = "a node below the root lies on two shards";
  else if (st != SWZ_OK) g->err = "swz_group_node_table: max_nodes too small, or a NULL buffer";
  return st;
}

// The boxes of the merged table out of the shards' (3 doubles per node of a shard's table): a node below the root is found
// by (level, key) in the one table that lists it; the root's box is the min / max of every root part given -- the shards'
// own entries and, when the root's rows were reduced as one file, that box (extra_lo / extra_hi, may be null).
void merge_boxes(const std::vector<std::vector<int8_t>>& level, const std::vector<std::vector<uint64_t>>& key,
                 const std::vector<const double*>& lo, const std::vector<const double*>& hi, const double* extra_lo,
                 const double* extra_hi, uint64_t nn, const int8_t* merged_level, const uint64_t* merged_key, double* lo_out,
                 double* hi_out) {
  const double inf = std::numeric_limits<double>::infinity();
  double root_lo[3] = {inf, inf, inf}, root_hi[3] = {-inf, -inf, -inf};
  auto join_root = [&](const double* a, const double* b) {
    for (int ax = 0; ax < 3; ++ax) {
      root_lo[ax] = std::min(root_lo[ax], a[ax]);
      root_hi[ax] = std::max(root_hi[ax], b[ax]);
    }
  };
  if (extra_lo && extra_hi) join_root(extra_lo, extra_hi);
  std::map<std::pair<int, uint64_t>, std::pair<const double*, const double*>> where;
  for (size_t r = 0; r < level.size(); ++r) {
    for (size_t k = 0; k < level[r].size(); ++k) {
      if (level[r][k] < 0) join_root(lo[r] + 3 * k, hi[r] + 3 * k);
      else where[{level[r][k], key[r][k]}] = {lo[r] + 3 * k, hi[r] + 3 * k};
    }
  }
  for (uint64_t k = 0; k < nn; ++k) {
    const double *a = root_lo, *b = root_hi;
    if (merged_level[k] >= 0) {
      const auto& found = where[{merged_level[k], merged_key[k]}];
      a = found.first;
      b = found.second;
    }
    for (int ax = 0; ax < 3; ++ax) {
      lo_out[3 * k + ax] = a[ax];
      hi_out[3 * k + ax] = b[ax];
    }
  }
}

}  // namespace

extern "C" {

int swz_group_node_boxes(swz_group* g, uint64_t max_nodes, double* box_min_out, double* box_max_out, uint64_t* num_nodes_out) {
  if (!g || !num_nodes_out) return SWZ_ERR_BAD_ARG;
  if (g->ds.tiler.empty()) {
    g->err = "swz_group_node_boxes: no data set is open (swz_group_tiler_open)";
    return SWZ_ERR_BAD_ARG;
  }
  std::vector<std::vector<int8_t>> level;
  std::vector<std::vector<uint64_t>> key, count;
  int st = shard_node_tables(g, level, key, count);
  if (st != SWZ_OK) return st;
  uint64_t nn = 0, cap = 1;
  for (int r = 0; r < g->n; ++r) cap += level[r].size();
  std::vector<int8_t> merged_level(cap);
  std::vector<uint64_t> merged_key(cap), merged_count(cap);
  if ((st = merge_tables(g, level, key, count, cap, merged_level.data(), merged_key.data(), merged_count.data(), nullptr, &nn)) != SWZ_OK) return st;
  *num_nodes_out = nn;
  if (nn > max_nodes || (nn && (!box_min_out || !box_max_out))) {
    g->err = "swz_group_node_boxes: max_nodes too small, or a NULL buffer";
    return SWZ_ERR_BAD_ARG;
  }
  // every shard's own boxes, one shard after the other (each call is bounded by a chunk of that shard)
  std::vector<std::vector<double>> lo(g->n), hi(g->n);
  std::vector<const double*> plo(g->n), phi(g->n);
  for (int r = 0; r < g->n; ++r) {
    (void)hipSetDevice(g->devices[r]);
    const uint64_t m = level[r].size();
    lo[r].resize(3 * std::max<uint64_t>(m, 1));
    hi[r].resize(3 * std::max<uint64_t>(m, 1));
    uint64_t got = 0;
    if ((st = swz_tiler_node_boxes(g->ds.tiler[r], m, lo[r].data(), hi[r].data(), &got)) != SWZ_OK) {
      g->err = "shard " + std::to_string(r) + ": " + swz_last_error(g->ctx[r]);
      return st;
    }
    plo[r] = lo[r].data();
    phi[r] = hi[r].data();
  }
  merge_boxes(level, key, plo, phi, nullptr, nullptr, nn, merged_level.data(), merged_key.data(), box_min_out, box_max_out);
  return SWZ_OK;
}

int swz_group_node_table(swz_group* g, uint64_t max_nodes, int8_t* level_out, uint64_t* key_out, uint64_t* count_out,
                         int32_t* shard_out, uint64_t* num_nodes_out) {
  if (!g || !num_nodes_out) return SWZ_ERR_BAD_ARG;
  if (g->ds.tiler.empty()) {
    g->err = "swz_group_node_table: no data set is open (swz_group_tiler_open)";
    return SWZ_ERR_BAD_ARG;
  }
  std::vector<std::vector<int8_t>> level;
  std::vector<std::vector<uint64_t>> key, count;
  const int st = shard_node_tables(g, level, key, count);
  if (st != SWZ_OK) return st;
  return merge_tables(g, level, key, count, max_nodes, level_out, key_out, count_out, shard_out, num_nodes_out);
}

int swz_group_write_output(swz_group* g, const char* dir, const swz_output_params* params, swz_output_stats* stats_per_shard,
                           swz_output_stats* total) {
  if (!g) return SWZ_ERR_BAD_ARG;
  const char* who = "swz_group_write_output";
  if (!dir || !params) {
    g->err = "swz_group_write_output: NULL argument";
    return SWZ_ERR_BAD_ARG;
  }
  if (g->ds.tiler.empty() || !g->stage.staged.empty()) {
    g->err = g->ds.tiler.empty() ? "swz_group_write_output: no data set is open (swz_group_tiler_open)" : "swz_group_write_output: a batch is staged or open";
    return SWZ_ERR_BAD_ARG;
  }
  const auto t_wall = std::chrono::steady_clock::now();
  const int N = g->n;
  std::fill(g->call.status.begin(), g->call.status.end(), SWZ_OK);
  if (total) *total = swz_output_stats{};
  for (int r = 0; stats_per_shard && r < N; ++r) stats_per_shard[r] = swz_output_stats{};
  auto refuse = [&](int r, int st) {  // r < 0: refused once, for the whole group
    g->err = r < 0 ? std::string(swz_last_error(g->ctx[0])) : "shard " + std::to_string(r) + ": " + swz_last_error(g->ctx[r]);
    return st;
  };

  // ---- every shard's table (a poisoned tiler answers here), the merged one, and everything that is refused before
  // anything is written -- once, on the merged table
  GroupOutput o;
  o.params = params;
  o.plan.resize(N);
  o.info.resize(N);
  uint32_t attr_mask = 0;
  std::vector<std::vector<int8_t>> level(N);
  std::vector<std::vector<uint64_t>> key(N), count(N);
  for (int r = 0; r < N; ++r) {
    (void)hipSetDevice(g->devices[r]);
    const int st = swz::output_tiler_table(g->ds.tiler[r], who, &o.plan[r], &o.info[r]);
    if (st != SWZ_OK) return refuse(r, st);
    attr_mask |= g->ds.tiler[r]->attr_mask;
    level[r] = o.plan[r].level;
    key[r] = o.plan[r].key;
    count[r] = o.plan[r].count;
  }
  // (one merge: the merged table has at most as many nodes as the shards' tables together)
  swz::OutputPlan merged;
  uint64_t nn = 0, cap = 1;
  for (int r = 0; r < N; ++r) cap += level[r].size();
  merged.level.resize(cap);
  merged.key.resize(cap);
  merged.count.resize(cap);
  int st = merge_tables(g, level, key, count, cap, merged.level.data(), merged.key.data(), merged.count.data(), nullptr, &nn);
  if (st != SWZ_OK) return st;
  merged.level.resize(nn);
  merged.key.resize(nn);
  merged.count.resize(nn);
  merged.offset.assign(nn, 0);
  uint64_t stored = 0;
  for (uint64_t k = 0; k < nn; ++k) {
    merged.offset[k] = stored;
    stored += merged.count[k];
  }
  swz_ctx* c0 = g->ctx[0];
  if ((st = swz::output_plan(c0, who, params, attr_mask, g->ds.bmin, g->ds.bmax, g->ds.params.spacing_at_root, dir, &merged)) != SWZ_OK) return refuse(-1, st);
  o.part_cnt.assign(N, 0);
  o.part_off.assign(N + 1, 0);
  o.part_xyz.assign(N, nullptr);
  o.part_attr.assign(SWZ_ATTR_COUNT, std::vector<const void*>(N, nullptr));
  for (int r = 0; r < N; ++r) {
    if (!o.plan[r].count.empty() && o.plan[r].level[0] < 0) o.part_cnt[r] = o.plan[r].count[0];
    o.part_off[r + 1] = o.part_off[r] + o.part_cnt[r];
    if ((st = swz::output_plan(g->ctx[r], who, params, attr_mask, g->ds.bmin, g->ds.bmax, g->ds.params.spacing_at_root, dir, &o.plan[r])) != SWZ_OK) return refuse(r, st);
  }
  if (o.part_off[N]) {
    o.root.level.assign(1, (int8_t)-1);
    o.root.key.assign(1, 0);
    o.root.offset.assign(1, 0);
    o.root.count.assign(1, o.part_off[N]);
    if ((st = swz::output_plan(c0, who, params, attr_mask, g->ds.bmin, g->ds.bmax, g->ds.params.spacing_at_root, dir, &o.root)) != SWZ_OK) return refuse(-1, st);
  }
  if ((st = swz::output_create_dirs(c0, who, &merged, dir)) != SWZ_OK) return refuse(-1, st);
  o.root.data_dir = merged.data_dir;
  for (int r = 0; r < N; ++r) o.plan[r].data_dir = merged.data_dir;

  // ---- SWZ_BIN_WRITER_THREADS is the budget of the whole call: every shard at least one
  const long budget = std::max(1L, c0->opt_int("SWZ_BIN_WRITER_THREADS", (long)std::min(32u, std::max(1u, std::thread::hardware_concurrency()))));
  o.writer_threads.assign(N, 1);
  for (int r = 0; r < N; ++r) o.writer_threads[r] = std::max(1L, budget / N + (r < budget % N ? 1 : 0));
  o.stats.assign(N, swz_output_stats{});

  std::vector<std::thread> threads;
  for (int r = 0; r < N; ++r) threads.emplace_back(output_thread, g, r, &o);
  for (auto& th : threads) th.join();
  for (int r = 0; stats_per_shard && r < N; ++r) stats_per_shard[r] = o.stats[r];
  st = first_failure(g);
  std::fill(g->call.status.begin(), g->call.status.end(), SWZ_OK);  // (a failed write marks no shard: the group stays usable)
  // ---- the metadata, once, from the merged table (and, tight, the merged boxes: the shards' own and the root's)
  if (st == SWZ_OK && merged.tight) {
    std::vector<const double*> plo(N), phi(N);
    for (int r = 0; r < N; ++r) {
      plo[r] = o.plan[r].tight_min.data();
      phi[r] = o.plan[r].tight_max.data();
    }
    const bool root = o.root.tight && !o.root.tight_min.empty();
    merge_boxes(level, key, plo, phi, root ? o.root.tight_min.data() : nullptr, root ? o.root.tight_max.data() : nullptr, nn,
                merged.level.data(), merged.key.data(), merged.tight_min.data(), merged.tight_max.data());
  }
  if (st == SWZ_OK) {
    (void)hipSetDevice(g->devices[0]);
    if ((st = swz::output_metadata(c0, who, merged, dir, params)) != SWZ_OK) g->err = swz_last_error(c0);
  }
  if (total) {
    total->nodes = nn;
    total->stored_points = stored;
    for (int r = 0; r < N; ++r) {
      total->bytes_written += o.stats[r].bytes_written;
      total->chunks += o.stats[r].chunks;
      total->pack_ms = std::max(total->pack_ms, o.stats[r].pack_ms);
      total->copy_ms = std::max(total->copy_ms, o.stats[r].copy_ms);
      total->write_ms = std::max(total->write_ms, o.stats[r].write_ms);
    }
    total->wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_wall).count();
  }
  return st;
}

}  // extern "C"
