// swz_group.hip -- a batch sharded over several GPUs, driven from ONE host process in C++ (SURVEY.md section 8(e);
// BASELINE north star: "host code stays C++ ... points shard across the GPUs of one node by the top-3 Morton bits
// with a single RCCL all-to-all after the encode step").
//
// Schwarzwald is a single process, so its drop-in for several GPUs is one object that owns one context per shard and
// one host thread per shard: encode -> group the rows by destination -> ONE exchange step -> root node -> levels,
// every step through the same C ABI the single-GPU path uses (swz_morton_encode_device, swz_partition_by_octant_device,
// swz_shard_*).  The exchange is either grouped RCCL send/recv (ncclCommInitAll in this process; librccl is loaded
// on demand so that nothing else depends on it) or peer copies (hipMemcpyPeerAsync), which also work with several
// shards on one GPU -- that is how the shard logic is tested on a one-GPU box.  The Python driver (sharded.py) is the
// multi-process counterpart used by bench.py.
//
// How the file reads: shard_thread is the collective skeleton -- the barriers of every path are listed above it -- and
// every step is a function of its own on a Step (swz_group.h: the shard's "do it only while ok, record the first failure"
// context): encode_and_group, exchange (exchange_rccl / exchange_peer_copies), root_step (plain, root_joint,
// root_in_turns; what differs between one batch and a tiler's batch is a RootOps), fast_start_vote, rows_to_shard0 /
// flags_to_shard (the FAST root rebuilt on shard 0, by the threads of one batch and by swz_group_finalize),
// levels_and_result, batch_levels.  swz_group_tile and swz_group_add_batch run their threads through group_run_call.
// The other files of the group (swz_group.h lists them): swz_gtiler.hip, a data set in several batches on the group's
// tilers; swz_goutput.hip, that data set written in one call.
#include <algorithm>
#include <functional>
#include <thread>

#include "swz_group.h"
#include "swz_md.h"

using namespace swz;

namespace {

constexpr size_t kChunkBytes = size_t(1) << 30;  // per message: RCCL 2.26 was measured to lose the tail of one > 2 GB block
constexpr uint64_t kGhostHeadroom = 4u << 20;    // rows kept free in front of the received points (MIN_DISTANCE root ghosts)

int owner_of_octant(int octant, int shards) { return octant * shards / 8; }

void group_barrier(void* p) { static_cast<swz_group*>(p)->barrier.wait(); }

__global__ __launch_bounds__(256) void grp_iota_kernel(uint32_t* __restrict__ out, uint32_t n) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) out[i] = i;
}

struct ShardCall {
  swz_group* g;
  int r;
  double* d_xyz;
  uint64_t n;
  const double* bmin;
  const double* bmax;
  const swz_tile_params* params;
  const swz_attribute_columns* attrs;  // may be NULL
  swz_group_result* result;
  bool batch = false;            // true: one batch of the group's tilers (swz_group_add_batch), result unused
  swz_tile_stats* stats = nullptr;
};

// ---------------------------------------------------------------------------------- step 1: encode, group by destination
struct Grouped {  // this shard's rows in the order of their destination shards, column by column
  double* send = nullptr;
  swz_attribute_columns send_attr{};
  uint32_t row_bytes[SWZ_ATTR_COUNT];  // 0: the batch has no such column
};

// Encodes locally, groups the rows by destination shard and publishes how many go where (send_counts[r]; a failed
// shard sends nothing).
Grouped encode_and_group(Step& s, const ShardCall& a) {
  swz_ctx* c = s.c;
  const uint64_t n = a.n;
  Grouped out;
  uint64_t* d_keys = s.buf<uint64_t>("grp_keys", (size_t)n);
  uint32_t* d_perm = s.buf<uint32_t>("grp_perm", (size_t)n);
  uint64_t oct[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (n && s.ok) s.swz(swz_morton_encode_device(c, a.d_xyz, n, a.bmin, a.bmax, d_keys)) && s.swz(swz_partition_by_octant_device(c, d_keys, n, d_perm, oct));
  std::fill(s.g->call.send_counts[s.r].begin(), s.g->call.send_counts[s.r].end(), 0);
  for (int o = 0; o < 8; ++o) s.g->call.send_counts[s.r][owner_of_octant(o, s.N)] += s.ok ? oct[o] : 0;
  out.send = s.buf<double>("grp_send", (size_t)n * 3);
  for (int t = 0; t < SWZ_ATTR_COUNT; ++t) {
    out.row_bytes[t] = (a.attrs && a.attrs->column[t]) ? swz_attribute_row_bytes(t) : 0;
    if (out.row_bytes[t]) out.send_attr.column[t] = s.buf<void>("grp_send_attr" + std::to_string(t), (size_t)n * out.row_bytes[t]);
  }
  if (n && s.ok) s.swz(swz_gather_payload_device(c, d_perm, nullptr, n, a.d_xyz, a.attrs, out.send, a.attrs ? &out.send_attr : nullptr));
  return out;
}

// ---------------------------------------------------------------------------------------------- step 2: the one exchange
struct Exchanged {  // what a shard owns after the exchange
  double* recv = nullptr;  // m rows, kGhostHeadroom rows free in front of them
  uint64_t m = 0;
  swz_attribute_columns recv_attr{};
  uint64_t global_points = 0;  // of the whole batch
};
// the columns of one row travel as separate blocks: [0] positions, [1 + t] attribute t
struct Column {
  const char* src;
  char* dst_here;
  uint32_t bytes;
  int attr;
};
struct Blocks {
  std::vector<Column> columns;
  std::vector<uint64_t> recv_off, send_off;  // rows: where shard p's block starts in this shard's receive / send buffers
};

// grouped RCCL point-to-point = the all-to-all(v): bounded messages, both sides cut their block the same way
void exchange_rccl(Step& s, const Blocks& b) {
  swz_group* g = s.g;
  const int r = s.r;
  if (g->rccl.GroupStart() != 0) {
    s.fail(SWZ_ERR_HIP, "ncclGroupStart failed");
    return;
  }
  for (const Column& col : b.columns)
    for (int p = 0; p < s.N && s.ok; ++p) {
      if (p == r) continue;
      const size_t sb = (size_t)g->call.send_counts[r][p] * col.bytes, rb = (size_t)g->call.send_counts[p][r] * col.bytes;
      for (size_t at = 0; at < sb && s.ok; at += kChunkBytes)
        if (g->rccl.Send(col.src + b.send_off[p] * col.bytes + at, std::min(kChunkBytes, sb - at), Rccl::kUint8, p, g->comms[r], s.c->stream) != 0)
          s.fail(SWZ_ERR_HIP, "ncclSend failed");
      for (size_t at = 0; at < rb && s.ok; at += kChunkBytes)
        if (g->rccl.Recv(col.dst_here + b.recv_off[p] * col.bytes + at, std::min(kChunkBytes, rb - at), Rccl::kUint8, p, g->comms[r], s.c->stream) != 0)
          s.fail(SWZ_ERR_HIP, "ncclRecv failed");
    }
  if (g->rccl.GroupEnd() != 0 && s.ok) s.fail(SWZ_ERR_HIP, "ncclGroupEnd failed");
  for (const Column& col : b.columns)
    if (s.ok && g->call.send_counts[r][r])
      s.hip(hipMemcpyAsync(col.dst_here + b.recv_off[r] * col.bytes, col.src + b.send_off[r] * col.bytes, (size_t)g->call.send_counts[r][r] * col.bytes,
                           hipMemcpyDeviceToDevice, s.c->stream),
            "hipMemcpyAsync(own block)");
}

// peer copies: every source pushes its blocks
void exchange_peer_copies(Step& s, const Blocks& b) {
  swz_group* g = s.g;
  const int r = s.r;
  for (int d = 0; d < s.N && s.ok; ++d) {
    const uint64_t cnt = g->call.send_counts[r][d];
    if (!cnt || !g->call.recv_rows[d]) continue;
    uint64_t off = 0;  // where this source's block starts on the destination
    for (int p = 0; p < r; ++p) off += g->call.send_counts[p][d];
    for (const Column& col : b.columns) {
      char* dst = col.attr < 0 ? (char*)g->call.recv_rows[d] : g->call.recv_attr[d][col.attr];
      if (!dst || !s.ok) continue;
      s.hip(hipMemcpyPeerAsync(dst + off * col.bytes, g->devices[d], col.src + b.send_off[d] * col.bytes, g->devices[r], (size_t)cnt * col.bytes, s.c->stream),
            "hipMemcpyPeerAsync(exchange)");
    }
  }
}

// Allocates and publishes the receive buffers, meets the others (barrier: every receive buffer exists), sends and
// receives, and meets them again (barrier: all rows have arrived everywhere).
Exchanged exchange(Step& s, const Grouped& rows) {
  swz_group* g = s.g;
  const int r = s.r, N = s.N;
  Exchanged ex;
  Blocks b;
  b.recv_off.assign(N, 0);
  b.send_off.assign(N, 0);
  for (int p = 0; p < N; ++p) {
    b.recv_off[p] = ex.m;
    ex.m += g->call.send_counts[p][r];
  }
  for (int d = 1; d < N; ++d) b.send_off[d] = b.send_off[d - 1] + g->call.send_counts[r][d - 1];
  for (int p = 0; p < N; ++p)
    for (int d = 0; d < N; ++d) ex.global_points += g->call.send_counts[p][d];
  double* front = s.buf<double>("grp_recv", (size_t)(ex.m + kGhostHeadroom) * 3);
  ex.recv = front ? front + kGhostHeadroom * 3 : nullptr;
  g->call.recv_rows[r] = ex.recv;
  g->call.recv_total[r] = ex.m;
  b.columns.push_back({(const char*)rows.send, (char*)ex.recv, 24u, -1});
  for (int t = 0; t < SWZ_ATTR_COUNT; ++t) {
    g->call.recv_attr[r][t] = nullptr;
    if (!rows.row_bytes[t]) continue;
    ex.recv_attr.column[t] = s.buf<void>("grp_recv_attr" + std::to_string(t), (size_t)std::max<uint64_t>(ex.m, 1) * rows.row_bytes[t]);
    g->call.recv_attr[r][t] = s.ok ? (char*)ex.recv_attr.column[t] : nullptr;
    b.columns.push_back({(const char*)rows.send_attr.column[t], (char*)ex.recv_attr.column[t], rows.row_bytes[t], t});
  }
  // A shard that has failed so far posts no sends or receives, and its peers would wait for them for ever (RCCL) or
  // copy into buffers that do not exist: every shard looks at every status right after this barrier -- nobody changes
  // one between it and the one after the exchange -- and they skip the collective step together.
  if (s.vote()) {  // ---- every receive buffer exists
    if (g->transport == 1 && N > 1) exchange_rccl(s, b);
    else exchange_peer_copies(s, b);
    if (s.ok) s.hip(hipStreamSynchronize(s.c->stream), "hipStreamSynchronize(exchange)");
  }
  g->barrier.wait();  // ---- all rows have arrived everywhere
  return ex;
}

// ------------------------------------------------------------------------------------ step 3: the root node, ACCURATE
// What differs between one batch (swz_shard_*) and one batch of the shard's tiler (swz_tiler_shard_*).
struct RootOps {
  // the root samples with MIN_DISTANCE: its greedy order spans the shards (else every shard decides its part by itself,
  // the take-all / sample decision on the counts of the whole root)
  bool sequential = false;
  // one batch: a root taken in turns stamps "root begun" when its turn has come and "root done" before it passes the turn
  // on, so that no shard's root begins before the lower shard's is done (tests/test_shard_seams.py tells the paths apart
  // by it), and "root done" waits for the stream; a tiler's begin returns with the stream idle and stamps after the step
  bool single_batch = false;
  std::function<void(Step&)> before_turn;                                                // work that does not need the lower shards
  std::function<double*(Step&, uint64_t ghosts)> ghost_room;                             // where the ghosts go (NULL: none are copied)
  std::function<int(double* d_ghosts, uint64_t ghosts, uint64_t* taken)> begin;          // the root step; taken: points in the root's file here
  std::function<int(double* d_out)> taken_positions;                                     // the positions the root took here
};

// All shards sweep the root cells of their own octants at the same time; a cell at the face of a lower octant reads that
// shard's records through peer access (swz_mqsweep.hip), exact positions of a tiler through its working index
// (MdPeerView::aidx).  No ghosts, no turns.  One barrier: inside the sweep, or here for a shard that never entered it.
void root_joint(Step& s, const RootOps& ops, uint64_t* taken) {
  swz_group* g = s.g;
  swz::MdShardRoot sr;
  sr.shard = s.r;
  sr.shards = s.N;
  sr.views = g->call.views.data();
  sr.barrier = group_barrier;
  sr.barrier_arg = g;
  g->call.views[s.r] = swz::MdPeerView{};
  s.c->md_shard_root = &sr;
  s.c->md_shard_root_published = true;  // the higher shards read this root's "md_*_sr" arrays until the barrier at the end of the call
  // (a shard whose octants are empty -- flat terrain in a cubic box -- opens its batch all the same: the finish call pairs
  // up with it; it never reaches the sweep, so the group meets the others for it)
  if (s.ok) s.swz(ops.begin(nullptr, 0, taken));
  s.c->md_shard_root = nullptr;
  if (!g->call.views[s.r].entered) {  // nothing to sample here, or the shard failed before its sweep met the others: meet them for it
    g->call.views[s.r].ncells = 0;
    g->call.views[s.r].status = s.ok ? SWZ_OK : SWZ_ERR_INTERNAL;
    g->call.views[s.r].entered = 1;
    g->barrier.wait();
  }
}

// The greedy order visits the shards in turn, each with what the root took on the lower shards as ghosts.  A failed shard
// still waits for its turn and passes it on.
void root_in_turns(Step& s, const RootOps& ops, uint64_t* taken) {
  swz_group* g = s.g;
  const int r = s.r;
  if (ops.before_turn) ops.before_turn(s);
  s.wait_turn();
  if (ops.single_batch) s.stamp(1);
  uint64_t gh = 0;
  for (int p = 0; p < r; ++p) gh += g->call.root_taken_count[p];
  double* gp = ops.ghost_room(s, gh);
  uint64_t at = 0;
  for (int p = 0; p < r && s.ok && gp; ++p) {
    if (!g->call.root_taken_count[p]) continue;
    s.hip(hipMemcpyPeerAsync(gp + at * 3, g->devices[r], g->call.root_taken[p], g->devices[p], (size_t)g->call.root_taken_count[p] * 24, s.c->stream),
          "hipMemcpyPeerAsync(ghosts)");
    at += g->call.root_taken_count[p];
  }
  if (s.ok) s.hip(hipStreamSynchronize(s.c->stream), "hipStreamSynchronize(ghosts)");
  if (s.ok) s.swz(ops.begin(gp, gh, taken));
  double* mine = s.buf<double>("grp_root_taken", (size_t)std::max<uint64_t>(*taken, 1) * 3);
  if (s.ok && *taken) s.swz(ops.taken_positions(mine));
  g->call.root_taken[r] = mine;
  g->call.root_taken_count[r] = s.ok ? *taken : 0;
  if (ops.single_batch) s.stamp(2);  // (both calls above return with the stream idle)
  s.pass_turn();
}

// The root step: plain, swept by all shards at once, or in turns.  Ends with the "root done" stamp.
void root_step(Step& s, const ShardCall& a, const RootOps& ops) {
  uint64_t taken = 0;
  bool in_turns = false;
  if (!ops.sequential) {
    if (s.ok) s.swz(ops.begin(nullptr, 0, &taken));
  } else if (s.N > 1 && s.g->peer_access && swz_shard_joint_root_possible(s.c, a.params, a.bmin, a.bmax)) {
    root_joint(s, ops, &taken);
  } else {
    root_in_turns(s, ops, &taken);
    in_turns = true;
  }
  if (ops.single_batch && s.ok) s.hip(hipStreamSynchronize(s.c->stream), "hipStreamSynchronize(root)");
  if (!(in_turns && ops.single_batch)) s.stamp(2);
}

// one batch: ghosts right in front of the received points (the presort leaves the headroom free)
RootOps tile_root_ops(const ShardCall& a, const Exchanged& ex) {
  swz_ctx* c = a.g->ctx[a.r];
  RootOps ops;
  ops.single_batch = true;
  ops.sequential = a.params->sampler == SWZ_MIN_DISTANCE && ex.global_points > a.params->max_points_per_node;
  ops.before_turn = [=](Step& s) {
    if (ex.m && s.ok) s.swz(swz_shard_presort_device(c, ex.recv, ex.m, a.bmin, a.bmax, a.params, kGhostHeadroom));
  };
  ops.ghost_room = [=](Step& s, uint64_t gh) -> double* {
    if (gh > kGhostHeadroom && s.ok) s.fail(SWZ_ERR_TOO_MANY_POINTS, "more root samples on lower shards than the ghost headroom holds");
    return (ex.recv && ex.m) ? ex.recv - gh * 3 : nullptr;
  };
  ops.begin = [=](double* gp, uint64_t gh, uint64_t* taken) {
    swz_shard_info info{ex.global_points, ex.m ? gp : nullptr, ex.m ? gh : 0};
    return swz_shard_begin_device(c, ex.recv, ex.m, a.bmin, a.bmax, a.params, &info, taken);
  };
  ops.taken_positions = [=](double* out) { return swz_shard_root_taken_device(c, out); };
  return ops;
}

// one batch of the shard's tiler: the root's take-all / sample decision uses the counts of the WHOLE root (cached points
// anywhere force sampling, TilingAlgorithms.cpp:272-275); in turns, the ghosts are the root files of the lower shards as
// they are after this batch, in a buffer of their own
RootOps batch_root_ops(const ShardCall& a, const Exchanged& ex) {
  swz_group* g = a.g;
  swz_tiler* t = g->ds.tiler[a.r];
  uint64_t root_before = 0;
  for (int p = 0; p < g->n; ++p) root_before += g->ds.root_stored[p];
  const bool sample = root_before > 0 || ex.global_points + root_before > a.params->max_points_per_node;
  RootOps ops;
  ops.sequential = a.params->sampler == SWZ_MIN_DISTANCE && sample && ex.global_points > 0;
  ops.ghost_room = [](Step& s, uint64_t gh) { return s.buf<double>("grp_ghosts", (size_t)std::max<uint64_t>(gh, 1) * 3); };
  ops.begin = [=](double* gp, uint64_t gh, uint64_t* have) {
    swz_tiler_shard_info info{ex.global_points, root_before, gh ? gp : nullptr, gh};
    return swz_tiler_shard_begin_device(t, ex.recv, ex.m, &ex.recv_attr, &info, have);
  };
  ops.taken_positions = [=](double* out) { return swz_tiler_level_positions_device(t, -1, out); };
  return ops;
}

// ------------------------------------------------------------------------------------------ FAST (TilingAlgorithmV3)
// The start level from the distribution of the whole batch: every shard has filled hist[r]; shard 0 sums them and writes
// the level to *level between two barriers (every histogram is in place / the level is known).  What a level that cannot
// be had means is the caller's business: on_shard0(status, level) runs on shard 0 before the second barrier.
template <typename F>
void fast_start_vote(Step& s, uint32_t fast_concurrency, int* level, F on_shard0) {
  swz_group* g = s.g;
  g->barrier.wait();
  if (s.r == 0) {
    std::vector<uint64_t> sum(1u << 18, 0);
    for (int p = 0; p < s.N; ++p)
      for (uint32_t b = 0; b < (1u << 18); ++b) sum[b] += g->call.hist[p][b];
    int32_t S = -1;
    const int rc = swz_fast_start_level_from_counts(sum.data(), fast_concurrency, &S);
    *level = S;
    on_shard0(rc, S);
  }
  g->barrier.wait();
}

// One batch, FAST: no root step.  The start level from the distribution of the whole batch, the levels from there down and
// the skipped levels down to 0 on every shard by itself, the root from the level-0 nodes of all shards on shard 0
// (swz_shard_fast_*).  This step: index the batch, count it per 6-octant prefix.
void tile_fast_index(Step& s, const ShardCall& a, const Exchanged& ex) {
  s.g->call.hist[s.r].assign(1u << 18, 0u);
  if (s.ok && ex.global_points < a.params->fast_concurrency) s.fail(SWZ_ERR_BAD_ARG, "FAST: a batch needs at least fast_concurrency points");
  if (s.ok) s.swz(swz_shard_fast_begin_device(s.c, ex.recv, ex.m, a.bmin, a.bmax, a.params, s.g->call.hist[s.r].data()));
}

// the levels from the start level down to 0; publishes what the shard's level-0 nodes hold
uint64_t tile_fast_candidates(Step& s) {
  swz_group* g = s.g;
  uint64_t ncand = 0;
  if (s.ok) s.swz(swz_shard_fast_run(s.c, g->cand.start, &ncand));
  uint64_t* ck = s.buf<uint64_t>("grp_cand_keys", (size_t)std::max<uint64_t>(ncand, 1));
  double* cx = s.buf<double>("grp_cand_xyz", (size_t)std::max<uint64_t>(ncand, 1) * 3);
  if (ncand && s.ok) s.swz(swz_shard_fast_root_candidates_device(s.c, ck, cx));
  if (s.ok) s.hip(hipStreamSynchronize(s.c->stream), "hipStreamSynchronize(candidates)");
  g->cand.keys[s.r] = ck;
  g->cand.xyz[s.r] = cx;
  g->cand.count[s.r] = s.ok ? ncand : 0;
  s.stamp(2);
  return ncand;
}

std::vector<uint64_t> cand_offsets(const swz_group* g) {
  std::vector<uint64_t> off(g->n + 1, 0);
  for (int p = 0; p < g->n; ++p) off[p + 1] = off[p] + g->cand.count[p];
  return off;
}

// shard 0: the root from the candidates of all shards
void tile_fast_root_on_shard0(Step& s, const ShardCall& a) {
  swz_group* g = s.g;
  const std::vector<uint64_t> off = cand_offsets(g);
  const uint64_t total = off[s.N];
  g->cand.flags = nullptr;
  if (total > 0xFFFF0000ull) s.fail(SWZ_ERR_TOO_MANY_POINTS, "more than 2^32-65536 points in the level-0 nodes");
  if (!s.ok || !total) return;
  uint64_t* keys = s.buf<uint64_t>("grp_root_skeys", (size_t)total);
  double* all = s.buf<double>("grp_root_xyz", (size_t)total * 3);
  uint32_t* iota = s.buf<uint32_t>("grp_root_perm", (size_t)total);
  uint8_t* taken = s.buf<uint8_t>("grp_root_taken", (size_t)total);
  if (s.ok)
    s.hip(rows_to_shard0(g, g->cand.count, off,
                         {{keys, {g->cand.keys.begin(), g->cand.keys.end()}, 8}, {all, {g->cand.xyz.begin(), g->cand.xyz.end()}, 24}}),
          "copy of the level-0 nodes to shard 0");
  if (s.ok && s.hip(group_iota(s.c->stream, iota, total), "the ids of the root's rows")) {
    // the candidates of the shards one behind the other are in key order: the shards own ascending octants
    s.swz(swz::sample_points_device(s.c, a.params->sampler, a.params->max_points_per_node, keys, iota, (uint32_t)total, all, 0, -1, a.bmin, a.bmax,
                                    a.params->spacing_at_root, SWZ_ALWAYS_ADHERE_TO_MIN_SPACING, taken, nullptr)) &&
        s.hip(hipStreamSynchronize(s.c->stream), "hipStreamSynchronize(root)");
  }
  g->cand.flags = taken;
}

// every shard: which of its candidates the root took
void tile_fast_take_root(Step& s, uint64_t ncand) {
  swz_group* g = s.g;
  if (!s.ok || !ncand) return;
  uint8_t* mine = g->cand.flags;
  if (s.r != 0) {
    mine = s.buf<uint8_t>("grp_cand_flags", (size_t)ncand);
    if (s.ok) s.hip(flags_to_shard(g, s.r, mine, g->cand.flags + cand_offsets(g)[s.r], ncand), "copy of the root flags");
  }
  if (s.ok) s.swz(swz_shard_fast_set_root_device(s.c, mine));
}

// Step 4 of one batch: everything below the root is local; the result record.  FAST adds the dup mask.
void levels_and_result(Step& s, const ShardCall& a, const Exchanged& ex, bool fast) {
  uint64_t* okeys = s.buf<uint64_t>("grp_out_keys", (size_t)ex.m);
  uint32_t* operm = s.buf<uint32_t>("grp_out_perm", (size_t)ex.m);
  int8_t* olevel = s.buf<int8_t>("grp_out_level", (size_t)ex.m);
  uint32_t* odup = fast ? s.buf<uint32_t>("grp_out_dup", (size_t)ex.m) : nullptr;
  swz_tile_stats stats{};
  if (s.ok) s.swz(fast ? swz_shard_fast_finish_device(s.c, okeys, operm, olevel, odup, &stats) : swz_shard_finish_device(s.c, okeys, operm, olevel, &stats));
  if (s.ok) s.hip(hipStreamSynchronize(s.c->stream), "hipStreamSynchronize(levels)");
  s.stamp(3);
  if (!a.result) return;
  a.result->d_xyz = ex.recv;
  a.result->d_keys = okeys;
  a.result->d_perm = operm;
  a.result->d_level = olevel;
  a.result->attrs = ex.recv_attr;
  a.result->num_points = s.ok ? ex.m : 0;
  a.result->stats = stats;
  a.result->d_dup = odup;
}

// One batch of the shard's tiler, FAST: no root step per batch.  The start level comes from the FIRST batch's distribution
// over all shards (TilingAlgorithms.cpp:1473-1535) and is kept (:1230-1236).  This step: index the batch, and count the
// first one per 6-octant prefix.
void batch_fast_index(Step& s, const ShardCall& a, const Exchanged& ex, bool first) {
  swz_tiler* t = s.g->ds.tiler[s.r];
  uint64_t have = 0;
  if (s.ok && ex.global_points < a.params->fast_concurrency) s.fail(SWZ_ERR_BAD_ARG, "FAST: a batch needs at least fast_concurrency points");
  if (s.ok) s.swz(batch_root_ops(a, ex).begin(nullptr, 0, &have));  // (FAST: begin indexes the batch and leaves the root alone)
  if (!first) return;
  s.g->call.hist[s.r].assign(1u << 18, 0u);
  if (s.ok) s.swz(swz_tiler_shard_fast_histogram(t, s.g->call.hist[s.r].data()));
}

// the levels of a tiler's batch below the root (FAST: from the start level down) and its statistics
void batch_levels(Step& s, const ShardCall& a) {
  swz_tile_stats stats{};
  if (s.ok) s.swz(swz_tiler_shard_finish(s.g->ds.tiler[s.r], &stats));
  if (a.stats) *a.stats = stats;
  (void)hipStreamSynchronize(s.c->stream);
  s.stamp(3);
}

// One shard's part of a call: the collective skeleton.  EVERY shard thread, failed or not, passes the same barriers in the
// same order on a given path -- which path is decided by the call's parameters and by counts every shard knows, never by a
// shard's own state.  Barriers by path (B1..B3 and the last one are common to all):
//
//   every path            B1 every shard knows every count (after encode_and_group)
//                         B2 every receive buffer exists, B3 all rows have arrived (both inside exchange)
//   tile  ACCURATE plain  --
//   tile  ACCURATE joint  J  the views of the root level are published (inside the sweep; root_joint meets the others for
//                            a shard that never entered it)
//   tile  ACCURATE turns  no barrier: wait for turn == r, pass on turn = r + 1 (a failed shard too)
//   tile  FAST            F1 every histogram is in place, F2 the start level is known (fast_start_vote),
//                         F3 every shard's candidates are in place, F4 the root is sampled on shard 0
//   batch ACCURATE plain / joint / turns: as for tile
//   batch FAST, first     F1, F2 (fast_start_vote)
//   batch FAST, later     --
//   every path            L  nobody reads a neighbour's buffers any more; then md_shard_root_published is reset
//   (swz_group_write_output has threads of its own, output_thread below: O1 every part of the root's file is gathered,
//    O2 every shard's files are written)
//
// The stamps of swz_group_shard_timing: 0 after B3, 1 here, 2 and 3 in the steps (root_step / tile_fast_candidates /
// batch FAST below: 2; levels_and_result / batch_levels: 3).
void shard_thread(ShardCall a) {
  Step s(a.g, a.r);
  swz_group* g = a.g;
  const Grouped rows = encode_and_group(s, a);
  g->barrier.wait();  // B1
  const Exchanged ex = exchange(s, rows);  // B2, B3
  s.stamp(0);
  s.agree();  // (the same vote again: a shard whose exchange failed must not keep the others waiting at the root)
  s.stamp(1);  // (a tiler's batch stamps like one batch: root step begun / done, levels done -- for FAST, which has no root step
               // per batch, "root" is the indexing of the batch and the vote on the start level)
  const bool fast = a.params->strategy == SWZ_FAST;
  if (!a.batch && fast) {
    tile_fast_index(s, a, ex);
    fast_start_vote(s, a.params->fast_concurrency, &g->cand.start, [&](int rc, int32_t S) {  // F1, F2
      if (s.ok && (rc != SWZ_OK || S < 0))  // (raised before the barrier: agree() then stops every shard with the real cause)
        s.fail(rc != SWZ_OK ? rc : SWZ_ERR_INTERNAL, "FAST: no start level from the summed prefix histograms of the batch");
    });
    s.agree();
    const uint64_t ncand = tile_fast_candidates(s);
    const bool go_root = s.vote();  // F3
    if (s.r == 0 && go_root) tile_fast_root_on_shard0(s, a);
    s.vote();  // F4 (or shard 0 has failed)
    tile_fast_take_root(s, ncand);
    levels_and_result(s, a, ex, true);
  } else if (!a.batch) {
    g->call.root_taken_count[s.r] = 0;
    root_step(s, a, tile_root_ops(a, ex));  // J, or the turn
    levels_and_result(s, a, ex, false);
  } else if (fast) {
    // (a failed shard goes on: a batch keeps every shard's tiler in step with the collective decisions)
    const bool first = g->ds.fast_start < 0;  // (read before F1; shard 0 writes it after that barrier)
    batch_fast_index(s, a, ex, first);
    // (a level that cannot be had stays as computed: swz_tiler_shard_set_start_level refuses it on every shard)
    if (first) fast_start_vote(s, a.params->fast_concurrency, &g->ds.fast_start, [](int, int32_t) {});  // F1, F2
    if (s.ok) s.swz(swz_tiler_shard_set_start_level(g->ds.tiler[s.r], g->ds.fast_start));
    s.stamp(2);
    batch_levels(s, a);
  } else {
    root_step(s, a, batch_root_ops(a, ex));  // J, or the turn
    batch_levels(s, a);
  }
  g->barrier.wait();  // L
  s.c->md_shard_root_published = false;
}

}  // namespace

hipError_t swz::group_iota(hipStream_t stream, uint32_t* d_out, uint64_t n) {
  hipLaunchKernelGGL(grp_iota_kernel, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, stream, d_out, (uint32_t)n);
  return hipGetLastError();
}

extern "C" {

int swz_group_create(int num_shards, const int* devices, int transport, swz_group** out) {
  if (!out || !devices || num_shards < 1 || (num_shards != 1 && num_shards != 2 && num_shards != 4 && num_shards != 8)) return SWZ_ERR_BAD_ARG;
  *out = nullptr;
  swz_group* g = new swz_group();
  g->n = num_shards;
  g->devices.assign(devices, devices + num_shards);
  g->transport = transport;
  g->barrier.parties = num_shards;
  bool distinct = true;
  for (int i = 0; i < num_shards; ++i)
    for (int j = 0; j < i; ++j) distinct &= devices[i] != devices[j];
  if (transport == 1 && !distinct) {
    delete g;
    return SWZ_ERR_BAD_ARG;  // RCCL refuses two ranks on one GPU; use peer copies (0)
  }
  for (int i = 0; i < num_shards; ++i) {
    swz_ctx* c = nullptr;
    if (swz_create(&c, devices[i]) != SWZ_OK) {
      for (swz_ctx* x : g->ctx) swz_destroy(x);
      delete g;
      return SWZ_ERR_HIP;
    }
    g->ctx.push_back(c);
  }
  if (transport == 1) {
    g->comms.assign(num_shards, nullptr);
    if (!g->rccl.load(g->err) || g->rccl.CommInitAll(g->comms.data(), num_shards, devices) != 0) {
      if (g->err.empty()) g->err = "ncclCommInitAll failed";
      for (swz_ctx* x : g->ctx) swz_destroy(x);
      delete g;
      return SWZ_ERR_HIP;
    }
  }
  // Peer access between all pairs of distinct devices, whatever the transport: peer copies want it, and the MIN_DISTANCE
  // root that all shards sweep at once has cells READ the lower shards' records in place (swz_mdkeys.hip).  Shards that
  // share a device share its memory.  Without it (no xGMI / PCIe peer path) the root is taken in turns instead.
  for (int i = 0; i < num_shards; ++i) {
    (void)hipSetDevice(devices[i]);
    for (int j = 0; j < num_shards; ++j) {
      if (devices[i] == devices[j]) continue;
      int can = 0;
      if (hipDeviceCanAccessPeer(&can, devices[i], devices[j]) != hipSuccess || !can) {
        g->peer_access = false;
        continue;
      }
      const hipError_t e = hipDeviceEnablePeerAccess(devices[j], 0);
      if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) g->peer_access = false;
      (void)hipGetLastError();
    }
  }
  g->call.send_counts.assign(num_shards, std::vector<uint64_t>(num_shards, 0));
  g->call.recv_rows.assign(num_shards, nullptr);
  g->call.recv_attr.assign(num_shards, std::vector<char*>(SWZ_ATTR_COUNT, nullptr));
  g->call.recv_total.assign(num_shards, 0);
  g->call.root_taken.assign(num_shards, nullptr);
  g->call.root_taken_count.assign(num_shards, 0);
  g->call.views.assign(num_shards, swz::MdPeerView{});
  g->call.hist.assign(num_shards, std::vector<uint32_t>());
  g->cand.keys.assign(num_shards, nullptr);
  g->cand.xyz.assign(num_shards, nullptr);
  g->cand.count.assign(num_shards, 0);
  g->timing.assign(num_shards, std::array<double, 4>{{0, 0, 0, 0}});
  g->call.status.assign(num_shards, SWZ_OK);
  g->call.status_msg.assign(num_shards, "");
  *out = g;
  return SWZ_OK;
}


int swz_group_destroy(swz_group* g) {
  if (!g) return SWZ_OK;
  (void)swz_group_tiler_close(g);
  for (void* comm : g->comms)
    if (comm && g->rccl.CommDestroy) (void)g->rccl.CommDestroy(comm);
  for (swz_ctx* c : g->ctx) swz_destroy(c);
  delete g;
  return SWZ_OK;
}

const char* swz_group_last_error(const swz_group* g) { return g ? g->err.c_str() : "swz_group_create failed"; }
int swz_group_num_shards(const swz_group* g) { return g ? g->n : 0; }
int swz_group_shard_timing(const swz_group* g, int shard, double ms_out[4]) {
  if (!g || !ms_out || shard < 0 || shard >= g->n) return SWZ_ERR_BAD_ARG;
  for (int k = 0; k < 4; ++k) ms_out[k] = g->timing[shard][k];
  return SWZ_OK;
}
swz_ctx* swz_group_ctx(swz_group* g, int shard) { return (g && shard >= 0 && shard < g->n) ? g->ctx[shard] : nullptr; }

// One call over all shards: refuses shards that hand over different attribute columns, resets what a call shares (after
// the caller's own `reset`, which may refuse the call), runs a thread per shard and reports the first failure.
static int group_run_call(swz_group* g, double* const* d_xyz, const swz_attribute_columns* d_attrs, const uint64_t* n, ShardCall call,
                          swz_group_result* results, swz_tile_stats* stats, const std::function<int()>& reset) {
  std::fill(g->call.status.begin(), g->call.status.end(), SWZ_OK);  // (first: a call refused below leaves no shard marked as failed)
  uint32_t mask = 0;
  int st = common_columns(g, d_attrs, &mask);
  if (st == SWZ_OK) st = reset();
  if (st != SWZ_OK) return st;
  g->call.turn = 0;
  g->t_call = std::chrono::steady_clock::now();  // (swz_group_shard_timing: milliseconds since this call began)
  for (auto& t4 : g->timing) std::fill(std::begin(t4), std::end(t4), 0.0);  // a stamp a path does not reach reads 0, never an older call's
  std::vector<std::thread> threads;
  for (int r = 0; r < g->n; ++r) {
    call.g = g;
    call.r = r;
    call.d_xyz = d_xyz[r];
    call.n = n[r];
    call.attrs = d_attrs ? &d_attrs[r] : nullptr;
    call.result = results ? &results[r] : nullptr;
    call.stats = stats ? &stats[r] : nullptr;
    threads.emplace_back(shard_thread, call);
  }
  for (auto& t : threads) t.join();
  return first_failure(g);
}

int swz_group_tile(swz_group* g, double* const* d_xyz, const swz_attribute_columns* d_attrs, const uint64_t* n, const double bmin[3],
                   const double bmax[3], const swz_tile_params* params, swz_group_result* results) {
  if (!g || !d_xyz || !n || !bmin || !bmax || !params) return SWZ_ERR_BAD_ARG;
  if (params->strategy != SWZ_ACCURATE && params->strategy != SWZ_FAST) {
    g->err = "unknown strategy";
    return SWZ_ERR_BAD_ARG;
  }
  if (const char* why = swz::sharded_sampler_refusal(params->sampler)) {
    g->err = why;
    return SWZ_ERR_BAD_ARG;
  }
  ShardCall call{};
  call.bmin = bmin;
  call.bmax = bmax;
  call.params = params;
  return group_run_call(g, d_xyz, d_attrs, n, call, results, nullptr, [&] {
    g->cand.start = -1;  // (group state shard 0 writes: nothing of an earlier call, failed or not, may be seen by this one)
    g->cand.flags = nullptr;
    return SWZ_OK;
  });
}


int swz_group_add_batch(swz_group* g, double* const* d_xyz, const swz_attribute_columns* d_attrs, const uint64_t* n,
                        swz_tile_stats* stats) {
  if (!g || !d_xyz || !n) return SWZ_ERR_BAD_ARG;
  if (g->ds.tiler.empty()) {
    g->err = "swz_group_add_batch: no data set is open (swz_group_tiler_open)";
    return SWZ_ERR_BAD_ARG;
  }
  ShardCall call{};
  call.bmin = g->ds.bmin;
  call.bmax = g->ds.bmax;
  call.params = &g->ds.params;
  call.batch = true;
  const int st = group_run_call(g, d_xyz, d_attrs, n, call, nullptr, stats, [&] {
    for (int r = 0; r < g->n; ++r) {
      (void)hipSetDevice(g->devices[r]);
      const int rc = swz_tiler_level_count(g->ds.tiler[r], -1, &g->ds.root_stored[r]);
      if (rc != SWZ_OK) {
        g->err = "shard " + std::to_string(r) + ": " + swz_last_error(g->ctx[r]);
        return rc;
      }
    }
    std::fill(g->call.root_taken_count.begin(), g->call.root_taken_count.end(), 0);
    return (int)SWZ_OK;
  });
  // the shards that did not fail have committed the batch and the failing one has not: nobody goes on (a call refused
  // before its threads started has marked no shard and changed nothing)
  if (st != SWZ_OK && !all_ok(g))
    for (int r = 0; r < g->n; ++r) (void)swz_tiler_poison(g->ds.tiler[r], ("a shard of the group failed to tile a batch: " + g->err).c_str());
  return st;
}



}  // extern "C"
