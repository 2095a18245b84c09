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
// every step is a function of its own on a Step (the shard's "do it only while ok, record the first failure" context):
// encode_and_group, exchange (exchange_rccl / exchange_peer_copies), root_step (plain, root_joint, root_in_turns; what
// differs between one batch and a tiler's batch is a RootOps), fast_start_vote, rows_to_shard0 / flags_to_shard (the
// FAST root rebuilt on shard 0, by the threads of one batch and by swz_group_finalize), levels_and_result, batch_levels.
// swz_group_tile and swz_group_add_batch run their threads through group_run_call.  swz_group_write_output (a data set of
// the group's tilers written in one call) has a thread per shard of its own, output_thread, over the parts of swz_toutput.h.
// swz_group_add_las_files (a data set of LAS files read in one call) has no thread of its own: over the parts of swz_tinput.h
// it fills the stage buffers from the shards' copy streams and hands every batch to swz_group_tile_staged.
#include <dlfcn.h>

#include <algorithm>
#include <array>
#include <chrono>
#include <condition_variable>
#include <cstring>
#include <functional>
#include <map>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "swz_internal.h"
#include "swz_md.h"
#include "swz_srs.h"
#include "swz_tinput.h"
#include "swz_toutput.h"

namespace {

// the few RCCL entry points the exchange needs (rccl.h: ncclCommInitAll :236, ncclCommDestroy :260, ncclSend :700,
// ncclRecv :722, ncclGroupStart :923, ncclGroupEnd :933), resolved with dlsym
struct Rccl {
  void* lib = nullptr;
  int (*CommInitAll)(void** comms, int ndev, const int* devlist) = nullptr;
  int (*CommDestroy)(void* comm) = nullptr;
  int (*Send)(const void* buf, size_t count, int datatype, int peer, void* comm, hipStream_t stream) = nullptr;
  int (*Recv)(void* buf, size_t count, int datatype, int peer, void* comm, hipStream_t stream) = nullptr;
  int (*GroupStart)() = nullptr;
  int (*GroupEnd)() = nullptr;
  const char* (*GetErrorString)(int) = nullptr;
  static constexpr int kUint8 = 1;  // ncclUint8, rccl.h:460
  bool load(std::string& err) {
    for (const char* name : {"librccl.so.1", "librccl.so"}) {
      lib = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
      if (lib) break;
    }
    if (!lib) {
      err = std::string("cannot load librccl: ") + dlerror();
      return false;
    }
    CommInitAll = reinterpret_cast<decltype(CommInitAll)>(dlsym(lib, "ncclCommInitAll"));
    CommDestroy = reinterpret_cast<decltype(CommDestroy)>(dlsym(lib, "ncclCommDestroy"));
    Send = reinterpret_cast<decltype(Send)>(dlsym(lib, "ncclSend"));
    Recv = reinterpret_cast<decltype(Recv)>(dlsym(lib, "ncclRecv"));
    GroupStart = reinterpret_cast<decltype(GroupStart)>(dlsym(lib, "ncclGroupStart"));
    GroupEnd = reinterpret_cast<decltype(GroupEnd)>(dlsym(lib, "ncclGroupEnd"));
    GetErrorString = reinterpret_cast<decltype(GetErrorString)>(dlsym(lib, "ncclGetErrorString"));
    if (!CommInitAll || !CommDestroy || !Send || !Recv || !GroupStart || !GroupEnd) {
      err = "librccl lacks an expected symbol";
      return false;
    }
    return true;
  }
};

struct Barrier {  // all shard threads meet here between the steps
  std::mutex m;
  std::condition_variable cv;
  int count = 0, generation = 0, parties = 1;
  void wait() {
    std::unique_lock<std::mutex> g(m);
    const int gen = generation;
    if (++count == parties) {
      count = 0;
      ++generation;
      cv.notify_all();
    } else {
      cv.wait(g, [&] { return gen != generation; });
    }
  }
};

constexpr size_t kChunkBytes = size_t(1) << 30;  // per message: RCCL 2.26 was measured to lose the tail of one > 2 GB block
constexpr uint64_t kGhostHeadroom = 4u << 20;    // rows kept free in front of the received points (MIN_DISTANCE root ghosts)

}  // namespace

struct swz_group {
  int n = 0;
  int transport = 0;
  std::vector<int> devices;
  std::vector<swz_ctx*> ctx;
  std::vector<void*> comms;
  Rccl rccl;
  std::string err;
  Barrier barrier;
  // per batch, shared between the shard threads
  std::vector<std::vector<uint64_t>> send_counts;  // [source][destination]
  std::vector<double*> recv_rows;                  // device buffers of every shard: positions ...
  std::vector<std::vector<char*>> recv_attr;       // ... and attribute columns [shard][attribute]
  std::vector<uint64_t> recv_total;
  std::vector<double*> root_taken;                 // positions the root took on every shard (ghosts of the higher ones)
  std::vector<uint64_t> root_taken_count;
  std::vector<int> status;
  std::vector<std::string> status_msg;
  int turn = 0;  // MIN_DISTANCE root: the shard whose turn it is
  std::mutex turn_m;
  std::condition_variable turn_cv;
  // a data set in several batches: one swz_tiler per shard (swz_group_tiler_open)
  std::vector<swz_tiler*> tiler;
  std::vector<uint64_t> root_stored;  // points in the root's file on every shard (before / after the batch's root step)
  double tbmin[3] = {0, 0, 0}, tbmax[3] = {0, 0, 0};
  swz_tile_params tparams{};
  bool has_srs = false;  // swz_group_set_source_srs: swz_group_add_las_files projects its input to ECEF
  swz_srs srs{};
  std::vector<std::array<double, 4>> timing;  // per shard, ms since the call began: exchange done, root begun, root done, levels done
  std::chrono::steady_clock::time_point t_call;
  std::vector<swz::MdPeerView> views;        // MIN_DISTANCE root swept by all shards at once: what every shard publishes
  int fast_start = -1;                       // FAST: the start level, known after the first batch
  bool peer_access = true;                   // kernels of one shard may read the memory of every other (the joint MIN_DISTANCE root does)
  std::vector<std::vector<uint32_t>> hist;   // FAST, first batch: every shard's points per 6-octant prefix
  // FAST in swz_group_tile: what every shard's level-0 nodes hold (the root is reconstructed from all of them on shard 0)
  int fast_tile_start = -1;
  std::vector<uint64_t*> cand_keys;
  std::vector<double*> cand_xyz;
  std::vector<uint64_t> cand_count;
  uint8_t* cand_flags = nullptr;
  // batches staged from pinned host memory: two device buffers per shard, filled on a copy stream of their own
  struct Staged {
    std::vector<uint64_t> n;  // per shard
    int slot = 0;
  };
  std::vector<Staged> staged;  // at most two, oldest first
  std::vector<hipStream_t> copy_stream;
  std::vector<hipEvent_t> copy_done[2];
  std::vector<double*> stage_xyz[2];
  std::vector<swz_attribute_columns> stage_attr[2];
  std::vector<uint64_t> stage_cap[2];
  uint32_t stage_mask = 0;  // attribute columns of the staged batches (the same for every batch)
  int next_slot = 0;
};

namespace {

int owner_of_octant(int octant, int shards) { return octant * shards / 8; }

void group_barrier(void* p) { static_cast<swz_group*>(p)->barrier.wait(); }

// Can the shards sweep the MIN_DISTANCE root together (swz_mdkeys.hip, MdShardRoot)?  The same answer on every shard: it
// hangs on the bounds, the spacing and the options only.
bool joint_root_possible(const swz_ctx* c, const swz_tile_params& p, const double bmin[3], const double bmax[3]) {
  if (p.sampler != SWZ_MIN_DISTANCE) return false;  // (with SWZ_FLAG_MIN_DISTANCE_PROPERTY too: the root is always sampled exactly)
  if (!c->opt_on("SWZ_GROUP_JOINT_ROOT", true)) return false;
  const swz::LevelPlan plan = swz::make_plan(-1, p.sampler, p.max_points_per_node, p.spacing_at_root, p.max_depth, bmin, bmax, true, true);
  static const double dummy_xyz = 0.0;
  static const uint32_t dummy_perm = 0;
  swz::SortedPoints sp;
  sp.xyz = &dummy_xyz;
  sp.perm = &dummy_perm;
  return swz::key_metric(c, plan, sp).ok && plan.cell_levels_geo >= 1 && !plan.terminal && !plan.reroot;
}

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

// true when no shard has reported a failure (looked at by every shard thread right after a barrier, so all of them see
// the same answer and leave the collective steps together)
bool all_ok(const swz_group* g) {
  for (int s : g->status)
    if (s != SWZ_OK) return false;
  return true;
}

// What a shard thread carries from step to step.  The rule of every step: do it only while ok, record the first failure.
// A shard that has failed keeps walking through the barriers (with nothing to contribute) so that the others are not
// stranded; the call reports the first failure.  (The methods take a status that has been computed already: a call that
// must not run on a failed shard stands behind `if (s.ok)` or `&&`.)
struct Step {
  swz_group* g;
  int r, N;
  swz_ctx* c;
  bool ok = true;
  Step(swz_group* group, int shard) : g(group), r(shard), N(group->n), c(group->ctx[shard]) { (void)hipSetDevice(g->devices[r]); }
  bool fail(int code, const std::string& msg) {
    g->status[r] = code;
    g->status_msg[r] = msg;
    return ok = false;
  }
  template <typename T>
  T* buf(const std::string& name, size_t count) {  // a named buffer of the shard's workspace (T = void: count bytes)
    T* p = nullptr;
    if (ok && c->get(name.c_str(), count, &p) != SWZ_OK) fail(SWZ_ERR_HIP, c->err);
    return p;
  }
  bool swz(int st) {
    if (ok && st != SWZ_OK) fail(st, swz_last_error(c));
    return ok;
  }
  bool hip(hipError_t e, const char* what) {
    if (ok && e != hipSuccess) fail(SWZ_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
    return ok;
  }
  bool agree() {  // right after a barrier: has any shard failed?
    if (!all_ok(g)) ok = false;  // (this shard's own status stays as it is: the group reports the shard that failed first)
    return ok;
  }
  bool vote() {
    g->barrier.wait();
    return agree();
  }
  void stamp(int k) { g->timing[r][k] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - g->t_call).count(); }
  void wait_turn() {
    std::unique_lock<std::mutex> lk(g->turn_m);
    g->turn_cv.wait(lk, [&] { return g->turn == r; });
  }
  void pass_turn() {
    {
      std::lock_guard<std::mutex> lk(g->turn_m);
      g->turn = r + 1;
    }
    g->turn_cv.notify_all();
  }
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
  std::fill(s.g->send_counts[s.r].begin(), s.g->send_counts[s.r].end(), 0);
  for (int o = 0; o < 8; ++o) s.g->send_counts[s.r][owner_of_octant(o, s.N)] += s.ok ? oct[o] : 0;
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
      const size_t sb = (size_t)g->send_counts[r][p] * col.bytes, rb = (size_t)g->send_counts[p][r] * col.bytes;
      for (size_t at = 0; at < sb && s.ok; at += kChunkBytes)
        if (g->rccl.Send(col.src + b.send_off[p] * col.bytes + at, std::min(kChunkBytes, sb - at), Rccl::kUint8, p, g->comms[r], s.c->stream) != 0)
          s.fail(SWZ_ERR_HIP, "ncclSend failed");
      for (size_t at = 0; at < rb && s.ok; at += kChunkBytes)
        if (g->rccl.Recv(col.dst_here + b.recv_off[p] * col.bytes + at, std::min(kChunkBytes, rb - at), Rccl::kUint8, p, g->comms[r], s.c->stream) != 0)
          s.fail(SWZ_ERR_HIP, "ncclRecv failed");
    }
  if (g->rccl.GroupEnd() != 0 && s.ok) s.fail(SWZ_ERR_HIP, "ncclGroupEnd failed");
  for (const Column& col : b.columns)
    if (s.ok && g->send_counts[r][r])
      s.hip(hipMemcpyAsync(col.dst_here + b.recv_off[r] * col.bytes, col.src + b.send_off[r] * col.bytes, (size_t)g->send_counts[r][r] * col.bytes,
                           hipMemcpyDeviceToDevice, s.c->stream),
            "hipMemcpyAsync(own block)");
}

// peer copies: every source pushes its blocks
void exchange_peer_copies(Step& s, const Blocks& b) {
  swz_group* g = s.g;
  const int r = s.r;
  for (int d = 0; d < s.N && s.ok; ++d) {
    const uint64_t cnt = g->send_counts[r][d];
    if (!cnt || !g->recv_rows[d]) continue;
    uint64_t off = 0;  // where this source's block starts on the destination
    for (int p = 0; p < r; ++p) off += g->send_counts[p][d];
    for (const Column& col : b.columns) {
      char* dst = col.attr < 0 ? (char*)g->recv_rows[d] : g->recv_attr[d][col.attr];
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
    ex.m += g->send_counts[p][r];
  }
  for (int d = 1; d < N; ++d) b.send_off[d] = b.send_off[d - 1] + g->send_counts[r][d - 1];
  for (int p = 0; p < N; ++p)
    for (int d = 0; d < N; ++d) ex.global_points += g->send_counts[p][d];
  double* front = s.buf<double>("grp_recv", (size_t)(ex.m + kGhostHeadroom) * 3);
  ex.recv = front ? front + kGhostHeadroom * 3 : nullptr;
  g->recv_rows[r] = ex.recv;
  g->recv_total[r] = ex.m;
  b.columns.push_back({(const char*)rows.send, (char*)ex.recv, 24u, -1});
  for (int t = 0; t < SWZ_ATTR_COUNT; ++t) {
    g->recv_attr[r][t] = nullptr;
    if (!rows.row_bytes[t]) continue;
    ex.recv_attr.column[t] = s.buf<void>("grp_recv_attr" + std::to_string(t), (size_t)std::max<uint64_t>(ex.m, 1) * rows.row_bytes[t]);
    g->recv_attr[r][t] = s.ok ? (char*)ex.recv_attr.column[t] : nullptr;
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
  sr.views = g->views.data();
  sr.barrier = group_barrier;
  sr.barrier_arg = g;
  g->views[s.r] = swz::MdPeerView{};
  s.c->md_shard_root = &sr;
  s.c->md_shard_root_published = true;  // the higher shards read this root's "md_*_sr" arrays until the barrier at the end of the call
  // (a shard whose octants are empty -- flat terrain in a cubic box -- opens its batch all the same: the finish call pairs
  // up with it; it never reaches the sweep, so the group meets the others for it)
  if (s.ok) s.swz(ops.begin(nullptr, 0, taken));
  s.c->md_shard_root = nullptr;
  if (!g->views[s.r].entered) {  // nothing to sample here, or the shard failed before its sweep met the others: meet them for it
    g->views[s.r].ncells = 0;
    g->views[s.r].status = s.ok ? SWZ_OK : SWZ_ERR_INTERNAL;
    g->views[s.r].entered = 1;
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
  for (int p = 0; p < r; ++p) gh += g->root_taken_count[p];
  double* gp = ops.ghost_room(s, gh);
  uint64_t at = 0;
  for (int p = 0; p < r && s.ok && gp; ++p) {
    if (!g->root_taken_count[p]) continue;
    s.hip(hipMemcpyPeerAsync(gp + at * 3, g->devices[r], g->root_taken[p], g->devices[p], (size_t)g->root_taken_count[p] * 24, s.c->stream),
          "hipMemcpyPeerAsync(ghosts)");
    at += g->root_taken_count[p];
  }
  if (s.ok) s.hip(hipStreamSynchronize(s.c->stream), "hipStreamSynchronize(ghosts)");
  if (s.ok) s.swz(ops.begin(gp, gh, taken));
  double* mine = s.buf<double>("grp_root_taken", (size_t)std::max<uint64_t>(*taken, 1) * 3);
  if (s.ok && *taken) s.swz(ops.taken_positions(mine));
  g->root_taken[r] = mine;
  g->root_taken_count[r] = s.ok ? *taken : 0;
  if (ops.single_batch) s.stamp(2);  // (both calls above return with the stream idle)
  s.pass_turn();
}

// The root step: plain, swept by all shards at once, or in turns.  Ends with the "root done" stamp.
void root_step(Step& s, const ShardCall& a, const RootOps& ops) {
  uint64_t taken = 0;
  bool in_turns = false;
  if (!ops.sequential) {
    if (s.ok) s.swz(ops.begin(nullptr, 0, &taken));
  } else if (s.N > 1 && s.g->peer_access && joint_root_possible(s.c, *a.params, a.bmin, a.bmax)) {
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
  swz_tiler* t = g->tiler[a.r];
  uint64_t root_before = 0;
  for (int p = 0; p < g->n; ++p) root_before += g->root_stored[p];
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
      for (uint32_t b = 0; b < (1u << 18); ++b) sum[b] += g->hist[p][b];
    int32_t S = -1;
    const int rc = swz_fast_start_level_from_counts(sum.data(), fast_concurrency, &S);
    *level = S;
    on_shard0(rc, S);
  }
  g->barrier.wait();
}

// "Rows of all shards onto shard 0": cnt[p] rows of every column from shard p to row off[p] on shard 0, by peer copies on
// the default stream.  Called with shard 0's device current; the sources' streams are idle.  Returns the first error.
struct PeerColumn {
  void* dst;                     // on shard 0
  std::vector<const void*> src;  // per shard
  size_t row_bytes;
};
hipError_t rows_to_shard0(swz_group* g, const std::vector<uint64_t>& cnt, const std::vector<uint64_t>& off, const std::vector<PeerColumn>& columns) {
  // (the peer copies are not ordered with shard 0's stream: nothing queued on it -- the SWZ_POISON fill of a buffer that
  // has just been allocated -- may still be writing the destination)
  hipError_t e = hipStreamSynchronize(g->ctx[0]->stream);
  for (int p = 0; p < g->n; ++p)
    for (const PeerColumn& col : columns)
      if (e == hipSuccess && cnt[p])
        e = hipMemcpyPeer((char*)col.dst + off[p] * col.row_bytes, g->devices[0], col.src[p], g->devices[p], (size_t)cnt[p] * col.row_bytes);
  // (a device-to-device hipMemcpyPeer may return before it is done; shard 0's stream does not wait for it)
  if (e == hipSuccess) e = hipDeviceSynchronize();
  return e;
}

// "Flags back to their shards": count flags from shard 0 to shard r > 0, whose device is current.
hipError_t flags_to_shard(swz_group* g, int r, uint8_t* mine, const uint8_t* d_flags0, uint64_t count) {
  hipError_t e = hipStreamSynchronize(g->ctx[r]->stream);  // (the copy is not ordered with this shard's stream)
  if (e == hipSuccess) e = hipMemcpyPeer(mine, g->devices[r], d_flags0, g->devices[0], (size_t)count);
  if (e == hipSuccess) e = hipDeviceSynchronize();
  return e;
}

// One batch, FAST: no root step.  The start level from the distribution of the whole batch, the levels from there down and
// the skipped levels down to 0 on every shard by itself, the root from the level-0 nodes of all shards on shard 0
// (swz_shard_fast_*).  This step: index the batch, count it per 6-octant prefix.
void tile_fast_index(Step& s, const ShardCall& a, const Exchanged& ex) {
  s.g->hist[s.r].assign(1u << 18, 0u);
  if (s.ok && ex.global_points < a.params->fast_concurrency) s.fail(SWZ_ERR_BAD_ARG, "FAST: a batch needs at least fast_concurrency points");
  if (s.ok) s.swz(swz_shard_fast_begin_device(s.c, ex.recv, ex.m, a.bmin, a.bmax, a.params, s.g->hist[s.r].data()));
}

// the levels from the start level down to 0; publishes what the shard's level-0 nodes hold
uint64_t tile_fast_candidates(Step& s) {
  swz_group* g = s.g;
  uint64_t ncand = 0;
  if (s.ok) s.swz(swz_shard_fast_run(s.c, g->fast_tile_start, &ncand));
  uint64_t* ck = s.buf<uint64_t>("grp_cand_keys", (size_t)std::max<uint64_t>(ncand, 1));
  double* cx = s.buf<double>("grp_cand_xyz", (size_t)std::max<uint64_t>(ncand, 1) * 3);
  if (ncand && s.ok) s.swz(swz_shard_fast_root_candidates_device(s.c, ck, cx));
  if (s.ok) s.hip(hipStreamSynchronize(s.c->stream), "hipStreamSynchronize(candidates)");
  g->cand_keys[s.r] = ck;
  g->cand_xyz[s.r] = cx;
  g->cand_count[s.r] = s.ok ? ncand : 0;
  s.stamp(2);
  return ncand;
}

std::vector<uint64_t> cand_offsets(const swz_group* g) {
  std::vector<uint64_t> off(g->n + 1, 0);
  for (int p = 0; p < g->n; ++p) off[p + 1] = off[p] + g->cand_count[p];
  return off;
}

// shard 0: the root from the candidates of all shards
void tile_fast_root_on_shard0(Step& s, const ShardCall& a) {
  swz_group* g = s.g;
  const std::vector<uint64_t> off = cand_offsets(g);
  const uint64_t total = off[s.N];
  g->cand_flags = nullptr;
  if (total > 0xFFFF0000ull) s.fail(SWZ_ERR_TOO_MANY_POINTS, "more than 2^32-65536 points in the level-0 nodes");
  if (!s.ok || !total) return;
  uint64_t* keys = s.buf<uint64_t>("grp_root_skeys", (size_t)total);
  double* all = s.buf<double>("grp_root_xyz", (size_t)total * 3);
  uint32_t* iota = s.buf<uint32_t>("grp_root_perm", (size_t)total);
  uint8_t* taken = s.buf<uint8_t>("grp_root_taken", (size_t)total);
  if (s.ok)
    s.hip(rows_to_shard0(g, g->cand_count, off,
                         {{keys, {g->cand_keys.begin(), g->cand_keys.end()}, 8}, {all, {g->cand_xyz.begin(), g->cand_xyz.end()}, 24}}),
          "copy of the level-0 nodes to shard 0");
  if (s.ok) {
    hipLaunchKernelGGL(grp_iota_kernel, dim3((uint32_t)((total + 255) / 256)), dim3(256), 0, s.c->stream, iota, (uint32_t)total);
    // the candidates of the shards one behind the other are in key order: the shards own ascending octants
    s.swz(swz::sample_points_device(s.c, a.params->sampler, a.params->max_points_per_node, keys, iota, (uint32_t)total, all, 0, -1, a.bmin, a.bmax,
                                    a.params->spacing_at_root, SWZ_ALWAYS_ADHERE_TO_MIN_SPACING, taken, nullptr)) &&
        s.hip(hipStreamSynchronize(s.c->stream), "hipStreamSynchronize(root)");
  }
  g->cand_flags = taken;
}

// every shard: which of its candidates the root took
void tile_fast_take_root(Step& s, uint64_t ncand) {
  swz_group* g = s.g;
  if (!s.ok || !ncand) return;
  uint8_t* mine = g->cand_flags;
  if (s.r != 0) {
    mine = s.buf<uint8_t>("grp_cand_flags", (size_t)ncand);
    if (s.ok) s.hip(flags_to_shard(g, s.r, mine, g->cand_flags + cand_offsets(g)[s.r], ncand), "copy of the root flags");
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
  swz_tiler* t = s.g->tiler[s.r];
  uint64_t have = 0;
  if (s.ok && ex.global_points < a.params->fast_concurrency) s.fail(SWZ_ERR_BAD_ARG, "FAST: a batch needs at least fast_concurrency points");
  if (s.ok) s.swz(batch_root_ops(a, ex).begin(nullptr, 0, &have));  // (FAST: begin indexes the batch and leaves the root alone)
  if (!first) return;
  s.g->hist[s.r].assign(1u << 18, 0u);
  if (s.ok) s.swz(swz_tiler_shard_fast_histogram(t, s.g->hist[s.r].data()));
}

// the levels of a tiler's batch below the root (FAST: from the start level down) and its statistics
void batch_levels(Step& s, const ShardCall& a) {
  swz_tile_stats stats{};
  if (s.ok) s.swz(swz_tiler_shard_finish(s.g->tiler[s.r], &stats));
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
    fast_start_vote(s, a.params->fast_concurrency, &g->fast_tile_start, [&](int rc, int32_t S) {  // F1, F2
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
    g->root_taken_count[s.r] = 0;
    root_step(s, a, tile_root_ops(a, ex));  // J, or the turn
    levels_and_result(s, a, ex, false);
  } else if (fast) {
    // (a failed shard goes on: a batch keeps every shard's tiler in step with the collective decisions)
    const bool first = g->fast_start < 0;  // (read before F1; shard 0 writes it after that barrier)
    batch_fast_index(s, a, ex, first);
    // (a level that cannot be had stays as computed: swz_tiler_shard_set_start_level refuses it on every shard)
    if (first) fast_start_vote(s, a.params->fast_concurrency, &g->fast_start, [](int, int32_t) {});  // F1, F2
    if (s.ok) s.swz(swz_tiler_shard_set_start_level(g->tiler[s.r], g->fast_start));
    s.stamp(2);
    batch_levels(s, a);
  } else {
    root_step(s, a, batch_root_ops(a, ex));  // J, or the turn
    batch_levels(s, a);
  }
  g->barrier.wait();  // L
  s.c->md_shard_root_published = false;
}

// flag of the i-th sorted element back to the position its element had before the sort
__global__ __launch_bounds__(256) void grp_unsort_flags_kernel(const uint32_t* __restrict__ perm, const uint8_t* __restrict__ taken, uint32_t n,
                                                               uint8_t* __restrict__ flags) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) flags[perm[i]] = taken[i];
}

}  // namespace

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
  g->send_counts.assign(num_shards, std::vector<uint64_t>(num_shards, 0));
  g->recv_rows.assign(num_shards, nullptr);
  g->recv_attr.assign(num_shards, std::vector<char*>(SWZ_ATTR_COUNT, nullptr));
  g->recv_total.assign(num_shards, 0);
  g->root_taken.assign(num_shards, nullptr);
  g->root_taken_count.assign(num_shards, 0);
  g->views.assign(num_shards, swz::MdPeerView{});
  g->hist.assign(num_shards, std::vector<uint32_t>());
  g->cand_keys.assign(num_shards, nullptr);
  g->cand_xyz.assign(num_shards, nullptr);
  g->cand_count.assign(num_shards, 0);
  g->timing.assign(num_shards, std::array<double, 4>{{0, 0, 0, 0}});
  g->status.assign(num_shards, SWZ_OK);
  g->status_msg.assign(num_shards, "");
  *out = g;
  return SWZ_OK;
}

static void group_free_tilers(swz_group* g) {
  for (size_t r = 0; r < g->tiler.size(); ++r)
    if (g->tiler[r]) (void)swz_tiler_destroy(g->tiler[r]);
  g->tiler.clear();
  for (size_t r = 0; r < g->copy_stream.size(); ++r) {
    (void)hipSetDevice(g->devices[r]);
    if (g->copy_stream[r]) {
      (void)hipStreamSynchronize(g->copy_stream[r]);
      (void)hipStreamDestroy(g->copy_stream[r]);
    }
    for (int k = 0; k < 2; ++k) {
      if (r < g->copy_done[k].size() && g->copy_done[k][r]) (void)hipEventDestroy(g->copy_done[k][r]);
      if (r < g->stage_xyz[k].size() && g->stage_xyz[k][r]) (void)hipFree(g->stage_xyz[k][r]);
      if (r < g->stage_attr[k].size())
        for (int t = 0; t < SWZ_ATTR_COUNT; ++t)
          if (g->stage_attr[k][r].column[t]) (void)hipFree(g->stage_attr[k][r].column[t]);
    }
  }
  g->copy_stream.clear();
  for (int k = 0; k < 2; ++k) {
    g->copy_done[k].clear();
    g->stage_xyz[k].clear();
    g->stage_attr[k].clear();
    g->stage_cap[k].clear();
  }
  g->staged.clear();
  g->stage_mask = 0;
  g->next_slot = 0;
}

int swz_group_destroy(swz_group* g) {
  if (!g) return SWZ_OK;
  group_free_tilers(g);
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
  std::fill(g->status.begin(), g->status.end(), SWZ_OK);  // (first: a call refused below leaves no shard marked as failed)
  if (d_attrs)
    for (int r = 1; r < g->n; ++r)
      for (int t = 0; t < SWZ_ATTR_COUNT; ++t)
        if ((d_attrs[r].column[t] != nullptr) != (d_attrs[0].column[t] != nullptr)) {
          g->err = "every shard must hand over the same attribute columns";
          return SWZ_ERR_BAD_ARG;
        }
  const int st = reset();
  if (st != SWZ_OK) return st;
  g->turn = 0;
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
  for (int r = 0; r < g->n; ++r)
    if (g->status[r] != SWZ_OK) {
      g->err = "shard " + std::to_string(r) + ": " + g->status_msg[r];
      return g->status[r];
    }
  return SWZ_OK;
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
    g->fast_tile_start = -1;  // (group state shard 0 writes: nothing of an earlier call, failed or not, may be seen by this one)
    g->cand_flags = nullptr;
    return SWZ_OK;
  });
}

// ---- a data set in several batches (BASELINE config 5 from the C++ host): one swz_tiler per shard -------------------
int swz_group_tiler_open(swz_group* g, const double bmin[3], const double bmax[3], const swz_tile_params* params,
                         uint64_t capacity_hint_per_shard) {
  if (!g || !bmin || !bmax || !params) return SWZ_ERR_BAD_ARG;
  if (!g->tiler.empty()) {
    g->err = "swz_group_tiler_open: a data set is open already (swz_group_tiler_close)";
    return SWZ_ERR_BAD_ARG;
  }
  if (const char* why = swz::sharded_sampler_refusal(params->sampler)) {
    g->err = why;
    return SWZ_ERR_BAD_ARG;
  }
  g->fast_start = -1;
  g->has_srs = false;
  g->hist.assign(g->n, std::vector<uint32_t>());
  for (int a = 0; a < 3; ++a) {
    g->tbmin[a] = bmin[a];
    g->tbmax[a] = bmax[a];
  }
  g->tparams = *params;
  g->tiler.assign(g->n, nullptr);
  for (int r = 0; r < g->n; ++r) {
    (void)hipSetDevice(g->devices[r]);
    const int st = swz_tiler_create(g->ctx[r], bmin, bmax, params, capacity_hint_per_shard, &g->tiler[r]);
    if (st != SWZ_OK) {
      g->err = "shard " + std::to_string(r) + ": " + swz_last_error(g->ctx[r]);
      group_free_tilers(g);
      return st;
    }
  }
  g->root_stored.assign(g->n, 0);
  g->copy_stream.assign(g->n, nullptr);
  for (int k = 0; k < 2; ++k) {
    g->copy_done[k].assign(g->n, nullptr);
    g->stage_xyz[k].assign(g->n, nullptr);
    g->stage_attr[k].assign(g->n, swz_attribute_columns{});
    g->stage_cap[k].assign(g->n, 0);
  }
  return SWZ_OK;
}

int swz_group_tiler_close(swz_group* g) {
  if (!g) return SWZ_ERR_BAD_ARG;
  group_free_tilers(g);
  g->has_srs = false;
  return SWZ_OK;
}

int swz_group_set_source_srs(swz_group* g, const swz_srs* srs) {
  if (!g) return SWZ_ERR_BAD_ARG;
  auto refuse = [&](const std::string& why) {
    g->err = why;
    return (int)SWZ_ERR_BAD_ARG;
  };
  if (g->tiler.empty()) return refuse("swz_group_set_source_srs: no data set is open (swz_group_tiler_open)");
  if (!g->staged.empty()) return refuse("swz_group_set_source_srs: a batch is staged or open");
  for (const swz_tiler* t : g->tiler)
    if (t->failed || t->finalized || t->total || t->staged_total || t->batches || !t->staged_sizes.empty() || t->batch_open)
      return refuse("swz_group_set_source_srs: the data set holds points, or a batch is staged or open");
  if (srs && !swz::srs_valid(srs))
    return refuse("swz_group_set_source_srs: not a definition swz_srs_parse made");
  g->has_srs = srs != nullptr;
  if (srs) g->srs = *srs;
  return SWZ_OK;
}

swz_tiler* swz_group_tiler(swz_group* g, int shard) {
  return (g && shard >= 0 && shard < (int)g->tiler.size()) ? g->tiler[shard] : nullptr;
}

int swz_group_add_batch(swz_group* g, double* const* d_xyz, const swz_attribute_columns* d_attrs, const uint64_t* n,
                        swz_tile_stats* stats) {
  if (!g || !d_xyz || !n) return SWZ_ERR_BAD_ARG;
  if (g->tiler.empty()) {
    g->err = "swz_group_add_batch: no data set is open (swz_group_tiler_open)";
    return SWZ_ERR_BAD_ARG;
  }
  ShardCall call{};
  call.bmin = g->tbmin;
  call.bmax = g->tbmax;
  call.params = &g->tparams;
  call.batch = true;
  const int st = group_run_call(g, d_xyz, d_attrs, n, call, nullptr, stats, [&] {
    for (int r = 0; r < g->n; ++r) {
      (void)hipSetDevice(g->devices[r]);
      const int rc = swz_tiler_level_count(g->tiler[r], -1, &g->root_stored[r]);
      if (rc != SWZ_OK) {
        g->err = "shard " + std::to_string(r) + ": " + swz_last_error(g->ctx[r]);
        return rc;
      }
    }
    std::fill(g->root_taken_count.begin(), g->root_taken_count.end(), 0);
    return (int)SWZ_OK;
  });
  // the shards that did not fail have committed the batch and the failing one has not: nobody goes on (a call refused
  // before its threads started has marked no shard and changed nothing)
  if (st != SWZ_OK && !all_ok(g))
    for (int r = 0; r < g->n; ++r) (void)swz_tiler_poison(g->tiler[r], ("a shard of the group failed to tile a batch: " + g->err).c_str());
  return st;
}

static bool stage_hip(swz_group* g, int r, hipError_t e, const char* what) {
  if (e == hipSuccess) return true;
  g->err = "shard " + std::to_string(r) + ": " + what + ": " + hipGetErrorString(e);
  return false;
}

// shard r's copy stream, the event of the slot and its device buffers for `rows` rows of the columns in `mask` (the device
// of shard r is current); false: g->err.  A buffer that grows is free: the batch it held has been tiled --
// swz_group_tile_staged returns after the shard's stream is idle.
static bool stage_reserve(swz_group* g, int slot, int r, uint64_t rows, uint32_t mask) {
  auto hip = [&](hipError_t e, const char* what) { return stage_hip(g, r, e, what); };
  if (!g->copy_stream[r] && !hip(hipStreamCreateWithFlags(&g->copy_stream[r], hipStreamNonBlocking), "hipStreamCreate")) return false;
  if (!g->copy_done[slot][r] && !hip(hipEventCreateWithFlags(&g->copy_done[slot][r], hipEventDisableTiming), "hipEventCreate")) return false;
  if (g->stage_cap[slot][r] >= std::max<uint64_t>(rows, 1) && !(mask & ~g->stage_mask)) return true;
  const uint64_t cap = std::max<uint64_t>(rows + rows / 8, 1);
  if (g->stage_xyz[slot][r]) (void)hipFree(g->stage_xyz[slot][r]);
  g->stage_xyz[slot][r] = nullptr;
  g->stage_cap[slot][r] = 0;
  if (!hip(hipMalloc(&g->stage_xyz[slot][r], cap * 24), "hipMalloc(stage)")) return false;
  for (int t = 0; t < SWZ_ATTR_COUNT; ++t) {
    if (g->stage_attr[slot][r].column[t]) (void)hipFree(g->stage_attr[slot][r].column[t]);
    g->stage_attr[slot][r].column[t] = nullptr;
    if ((mask >> t) & 1u)
      if (!hip(hipMalloc(&g->stage_attr[slot][r].column[t], cap * swz_attribute_row_bytes(t)), "hipMalloc(stage column)")) return false;
  }
  g->stage_cap[slot][r] = cap;
  return true;
}

// Staging: the batch is copied from pinned host memory into one of two device buffers per shard on the shard's copy
// stream, beside whatever its tiling stream is doing (the batch before).  At most two batches are staged.
int swz_group_stage_batch(swz_group* g, const double* const* xyz_host, const swz_attribute_columns* attrs_host, const uint64_t* n) {
  if (!g || !xyz_host || !n) return SWZ_ERR_BAD_ARG;
  if (g->tiler.empty() || g->staged.size() >= 2) {
    g->err = g->tiler.empty() ? "swz_group_stage_batch: no data set is open" : "swz_group_stage_batch: two batches are staged already";
    return SWZ_ERR_BAD_ARG;
  }
  uint32_t mask = 0;
  for (int t = 0; t < SWZ_ATTR_COUNT; ++t)
    if (attrs_host && attrs_host[0].column[t]) mask |= 1u << t;
  const int slot = g->next_slot;
  swz_group::Staged sb;
  sb.slot = slot;
  sb.n.assign(n, n + g->n);
  for (int r = 0; r < g->n; ++r) {
    (void)hipSetDevice(g->devices[r]);
    auto hip = [&](hipError_t e, const char* what) { return stage_hip(g, r, e, what); };
    uint32_t mine = 0;
    for (int t = 0; t < SWZ_ATTR_COUNT; ++t)
      if (attrs_host && attrs_host[r].column[t]) mine |= 1u << t;
    if (mine != mask) {
      g->err = "every shard must hand over the same attribute columns";
      return SWZ_ERR_BAD_ARG;
    }
    if (!stage_reserve(g, slot, r, n[r], mask)) return SWZ_ERR_HIP;
    if (n[r]) {
      if (!hip(hipMemcpyAsync(g->stage_xyz[slot][r], xyz_host[r], n[r] * 24, hipMemcpyHostToDevice, g->copy_stream[r]), "hipMemcpyAsync")) return SWZ_ERR_HIP;
      for (int t = 0; t < SWZ_ATTR_COUNT; ++t)
        if ((mask >> t) & 1u)
          if (!hip(hipMemcpyAsync(g->stage_attr[slot][r].column[t], attrs_host[r].column[t], n[r] * swz_attribute_row_bytes(t),
                                  hipMemcpyHostToDevice, g->copy_stream[r]), "hipMemcpyAsync")) return SWZ_ERR_HIP;
    }
    if (!hip(hipEventRecord(g->copy_done[slot][r], g->copy_stream[r]), "hipEventRecord")) return SWZ_ERR_HIP;
  }
  g->stage_mask |= mask;
  g->staged.push_back(sb);
  g->next_slot ^= 1;
  return SWZ_OK;
}

int swz_group_tile_staged(swz_group* g, swz_tile_stats* stats) {
  if (!g) return SWZ_ERR_BAD_ARG;
  if (g->staged.empty()) {
    g->err = "swz_group_tile_staged: nothing is staged";
    return SWZ_ERR_BAD_ARG;
  }
  const swz_group::Staged sb = g->staged.front();
  g->staged.erase(g->staged.begin());
  std::vector<double*> xyz(g->n);
  std::vector<swz_attribute_columns> attrs(g->n);
  for (int r = 0; r < g->n; ++r) {
    (void)hipSetDevice(g->devices[r]);
    // the shard's kernels wait for its copy on the device; the host goes on
    const hipError_t e = hipStreamWaitEvent(g->ctx[r]->stream, g->copy_done[sb.slot][r], 0);
    if (e != hipSuccess) {
      g->err = "shard " + std::to_string(r) + ": hipStreamWaitEvent: " + hipGetErrorString(e);
      return SWZ_ERR_HIP;
    }
    xyz[r] = g->stage_xyz[sb.slot][r];
    attrs[r] = g->stage_attr[sb.slot][r];
  }
  return swz_group_add_batch(g, xyz.data(), g->stage_mask ? attrs.data() : nullptr, sb.n.data(), stats);
}

// A data set of LAS files through the group in one call: swz_tiler_add_las_files's scan, refusals and cuts ONCE
// (swz_tinput.h), then per batch every shard reads, copies and decodes its slice of the batch's points -- consecutive
// slices in shard order -- into one of its two stage buffers, and the batch goes the way of swz_group_tile_staged.
int swz_group_add_las_files(swz_group* g, const char* const* paths, uint64_t num_files, const swz_input_params* params,
                            swz_input_stats* stats) {
  if (!g) return SWZ_ERR_BAD_ARG;
  const char* who = "swz_group_add_las_files";
  const auto t_wall = std::chrono::steady_clock::now();
  auto ms_since = [](std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  };
  if (stats) *stats = swz_input_stats{};
  auto refuse = [&](int st, const std::string& why) {
    g->err = why;
    return st;
  };
  if (!params || (num_files && !paths)) return refuse(SWZ_ERR_BAD_ARG, "swz_group_add_las_files: NULL argument");
  if (g->tiler.empty()) return refuse(SWZ_ERR_BAD_ARG, "swz_group_add_las_files: no data set is open (swz_group_tiler_open)");
  if (!g->staged.empty()) return refuse(SWZ_ERR_BAD_ARG, "swz_group_add_las_files: a batch is staged or open");
  const int N = g->n;
  bool mask_fixed = false;
  uint32_t mask_now = 0;
  uint64_t points_now = 0;  // the worst case: one shard receives everything
  for (int r = 0; r < N; ++r) {
    const swz_tiler* t = g->tiler[r];
    const std::string shard = "shard " + std::to_string(r) + ": ";
    if (t->failed) return refuse(SWZ_ERR_TILER_FAILED, shard + "the tiler has failed: " + t->failed_why);
    if (t->finalized) return refuse(SWZ_ERR_BAD_ARG, shard + "swz_tiler: batches cannot be added after finalize");
    if (!t->staged_sizes.empty() || t->batch_open) return refuse(SWZ_ERR_BAD_ARG, shard + "swz_group_add_las_files: a batch is staged or open");
    if (t->staged_total && !mask_fixed) {
      mask_fixed = true;
      mask_now = t->attr_mask;
    }
    points_now = std::max<uint64_t>(points_now, t->staged_total);
  }
  swz_ctx* c0 = g->ctx[0];
  (void)hipSetDevice(g->devices[0]);
  swz::LasInputPlan plan;
  int st = swz::las_input_plan(c0, who, paths, num_files, params, g->tbmin, g->tbmax, g->tparams, mask_fixed, mask_now, points_now,
                               g->has_srs ? &g->srs : nullptr, &plan);
  if (st != SWZ_OK) return refuse(st, swz_last_error(c0));
  const uint64_t num_batches = plan.num_batches();
  const uint32_t mask = plan.mask;

  // ---- every batch's slices, the largest image and the most rows of a shard
  std::vector<std::vector<swz::InputBatch>> slice(num_batches, std::vector<swz::InputBatch>(N));
  std::vector<uint64_t> image_max(N, 0), rows_max(N, 0);
  for (uint64_t j = 0; j < num_batches; ++j) {
    const uint64_t b0 = plan.cuts[j], pts = plan.cuts[j + 1] - b0;
    for (int r = 0; r < N; ++r) {
      swz::las_input_image(plan, b0 + pts * (uint64_t)r / N, b0 + pts * (uint64_t)(r + 1) / N, &slice[j][r]);
      image_max[r] = std::max(image_max[r], slice[j][r].image_bytes);
      rows_max[r] = std::max(rows_max[r], slice[j][r].points);
    }
  }
  // ---- per shard: two raw images, host and device, and the two stage buffers the slices are decoded into
  std::vector<swz::InputBuffers> ib(N);
  for (int r = 0; r < N; ++r) {
    (void)hipSetDevice(g->devices[r]);
    if ((st = ib[r].reserve(g->ctx[r], std::max<uint64_t>(image_max[r], 16), num_batches > 1)) != SWZ_OK)
      return refuse(st, "shard " + std::to_string(r) + ": " + swz_last_error(g->ctx[r]));
    for (int k = 0; k < (num_batches > 1 ? 2 : 1); ++k)
      if (!stage_reserve(g, g->next_slot ^ k, r, rows_max[r], mask)) return SWZ_ERR_HIP;
  }
  g->stage_mask |= mask;

  // ---- SWZ_INPUT_READER_THREADS is the budget of the whole call: every shard at least one
  const long budget = std::max(1L, c0->opt_int("SWZ_INPUT_READER_THREADS", (long)std::min(32u, std::max(1u, std::thread::hardware_concurrency()))));
  std::vector<long> reader_threads(N, 1);
  for (int r = 0; r < N; ++r) reader_threads[r] = std::max(1L, budget / N + (r < budget % N ? 1 : 0));

  // ---- the stream, as in swz_tiler_add_las_files: reads run two batches ahead of the tiling, copy + decode one
  std::vector<double> read_ms(N, 0.0), copy_ms(N, 0.0), decode_ms(N, 0.0);
  double tile_ms = 0, wait_ms = 0;
  uint64_t bytes_read = 0, batches_done = 0, points_done = 0;
  int status = SWZ_OK;
  std::string why;
  bool touched = false;
  std::vector<swz::TicketRun> readers(N);
  auto fail_stream = [&](int code, const std::string& text) {
    if (status == SWZ_OK) {
      status = code;
      why = text;
    }
  };
  auto start_read = [&](uint64_t j) {
    for (int r = 0; r < N; ++r)
      swz::las_start_read(readers[r], g->ctx[r], who, &slice[j][r], static_cast<unsigned char*>(ib[r].host[j & 1]), paths, reader_threads[r]);
  };
  auto wait_read = [&](uint64_t j) -> bool {
    const auto t0 = std::chrono::steady_clock::now();
    bool ok = true;
    for (int r = 0; r < N; ++r) {
      double ms = 0;
      std::string err;
      const int rc = readers[r].wait(&err, &ms);
      read_ms[r] += ms;
      if (rc != SWZ_OK) {
        fail_stream(rc, err);
        ok = false;
      } else {
        bytes_read += slice[j][r].raw_bytes;
      }
    }
    wait_ms += ms_since(t0);
    return ok;
  };
  // batch j: every shard's image to its device and decoded into the stage buffers of the next slot; staged like a pinned batch
  auto enqueue = [&](uint64_t j) -> int {
    const int slot = g->next_slot, s = (int)(j & 1);
    swz_group::Staged sb;
    sb.slot = slot;
    sb.n.assign(N, 0);
    for (int r = 0; r < N; ++r) {
      (void)hipSetDevice(g->devices[r]);
      const swz::InputBatch& b = slice[j][r];
      hipStream_t cs = g->copy_stream[r];
      auto hip = [&](hipError_t e, const char* what) { return stage_hip(g, r, e, what); };
      if (!hip(hipEventRecord(ib[r].begin[s], cs), "hipEventRecord")) return SWZ_ERR_HIP;
      if (b.image_bytes && !hip(hipMemcpyAsync(ib[r].device[s], ib[r].host[s], b.image_bytes, hipMemcpyHostToDevice, cs), "hipMemcpyAsync(image)")) return SWZ_ERR_HIP;
      if (!hip(hipEventRecord(ib[r].copied[s], cs), "hipEventRecord")) return SWZ_ERR_HIP;
      const int rc = swz::las_launch_image(g->ctx[r], cs, ib[r].device[s], b, plan.shift ? plan.ds.center : nullptr, g->stage_xyz[slot][r],
                                           &g->stage_attr[slot][r], mask, g->has_srs ? &g->srs : nullptr);
      if (rc != SWZ_OK) {
        g->err = "shard " + std::to_string(r) + ": " + swz_last_error(g->ctx[r]);
        return rc;
      }
      if (!hip(hipEventRecord(ib[r].decoded[s], cs), "hipEventRecord")) return SWZ_ERR_HIP;
      if (!hip(hipEventRecord(g->copy_done[slot][r], cs), "hipEventRecord")) return SWZ_ERR_HIP;
      sb.n[r] = b.points;
    }
    g->staged.push_back(sb);
    g->next_slot ^= 1;
    return SWZ_OK;
  };

  start_read(0);
  if (wait_read(0)) {
    const int rc = enqueue(0);
    if (rc != SWZ_OK) fail_stream(rc, g->err);
    if (status == SWZ_OK && num_batches > 1) start_read(1);
  }
  for (uint64_t j = 0; j < num_batches && status == SWZ_OK; ++j) {
    if (j + 1 < num_batches) {
      bool next_staged = false;
      if (wait_read(j + 1)) {
        const int rc = enqueue(j + 1);
        if (rc != SWZ_OK) fail_stream(rc, g->err);
        next_staged = rc == SWZ_OK;
      }
      // (a read that failed: batch j, which is staged, is still tiled -- the stream stops after the running batch)
      if (next_staged && j + 2 < num_batches) {
        // the host images of batch j + 2 are batch j's: their copies have left them
        bool left = true;
        for (int r = 0; r < N && left; ++r) {
          (void)hipSetDevice(g->devices[r]);
          left = stage_hip(g, r, hipEventSynchronize(ib[r].copied[j & 1]), "the copy of a slice image");
        }
        if (!left) fail_stream(SWZ_ERR_HIP, g->err);
        else start_read(j + 2);
      }
    }
    if (g->staged.empty()) break;  // (batch j was never staged)
    const auto t_tile = std::chrono::steady_clock::now();
    touched = true;  // (until here the slices lie in the group's stage buffers: no tiler has seen them)
    const int rc = swz_group_tile_staged(g, nullptr);  // (a failure here has poisoned every tiler with its own text)
    tile_ms += ms_since(t_tile);
    if (rc != SWZ_OK) {
      status = rc;
      why = g->err;
      break;
    }
    for (int r = 0; r < N; ++r) {  // batch j has been decoded: its tiling waited for the event behind it
      float ms = 0.f;
      if (hipEventElapsedTime(&ms, ib[r].begin[j & 1], ib[r].copied[j & 1]) == hipSuccess) copy_ms[r] += ms;
      if (hipEventElapsedTime(&ms, ib[r].copied[j & 1], ib[r].decoded[j & 1]) == hipSuccess) decode_ms[r] += ms;
    }
    ++batches_done;
    points_done += plan.cuts[j + 1] - plan.cuts[j];
  }
  for (int r = 0; r < N; ++r) {
    if (readers[r].running()) (void)readers[r].wait(nullptr, nullptr);
    (void)hipSetDevice(g->devices[r]);
    if (g->copy_stream[r]) (void)hipStreamSynchronize(g->copy_stream[r]);
  }
  g->staged.clear();  // (a batch staged behind the one that failed is dropped)
  if (status != SWZ_OK && touched)
    for (int r = 0; r < N; ++r) (void)swz_tiler_poison(g->tiler[r], why.c_str());
  if (stats) {
    stats->files = plan.ds.readable_files;
    stats->points = points_done;
    stats->batches = batches_done;
    stats->bytes_read = bytes_read;
    for (int r = 0; r < N; ++r) {
      stats->read_ms = std::max(stats->read_ms, read_ms[r]);
      stats->copy_ms = std::max(stats->copy_ms, copy_ms[r]);
      stats->decode_ms = std::max(stats->decode_ms, decode_ms[r]);
    }
    stats->tile_ms = tile_ms;
    stats->wait_ms = wait_ms;
    stats->wall_ms = ms_since(t_wall);
  }
  if (status != SWZ_OK) g->err = why;
  return status;
}

// a failure of shard r while the data set is finalized: nobody goes on
static int finalize_fail(swz_group* g, int r, int rc) {
  g->err = "shard " + std::to_string(r) + ": " + swz_last_error(g->ctx[r]);
  for (int s = 0; s < g->n; ++s) (void)swz_tiler_poison(g->tiler[s], ("the group failed to finalize: " + g->err).c_str());
  return rc;
}

// The root of TilingAlgorithmV3::finalize (reconstruct_single_node, :1661-1715) samples what its eight children hold,
// and they lie on different shards: their files come together on shard 0 in shard order (= octant order: the order
// the reference appends them in), are indexed against the root bounds and sampled with AlwaysAdhereToMinSpacing there.
// *d_flags0: one flag per row, in the order the rows came in.
static int finalize_fast_root_on_shard0(swz_group* g, const std::vector<uint64_t>& cnt, const std::vector<uint64_t>& off, uint8_t** d_flags0) {
  const uint64_t total = off[g->n];
  swz_ctx* c0 = g->ctx[0];
  (void)hipSetDevice(g->devices[0]);
  double* all = nullptr;
  uint64_t *keys = nullptr, *skeys = nullptr;
  uint32_t* perm = nullptr;
  uint8_t* taken = nullptr;
  if (c0->get("grp_root_xyz", (size_t)total * 3, &all) != SWZ_OK || c0->get("grp_root_keys", (size_t)total, &keys) != SWZ_OK ||
      c0->get("grp_root_skeys", (size_t)total, &skeys) != SWZ_OK || c0->get("grp_root_perm", (size_t)total, &perm) != SWZ_OK ||
      c0->get("grp_root_taken", (size_t)total, &taken) != SWZ_OK || c0->get("grp_root_flags", (size_t)total, d_flags0) != SWZ_OK)
    return finalize_fail(g, 0, SWZ_ERR_HIP);
  std::vector<const void*> files(g->n, nullptr);
  for (int r = 0; r < g->n; ++r) {
    if (!cnt[r]) continue;
    (void)hipSetDevice(g->devices[r]);
    swz_ctx* c = g->ctx[r];
    double* mine = nullptr;
    if (c->get("grp_l0_xyz", (size_t)cnt[r] * 3, &mine) != SWZ_OK) return finalize_fail(g, r, SWZ_ERR_HIP);
    const int rc = swz_tiler_level_positions_device(g->tiler[r], 0, mine);
    if (rc != SWZ_OK) return finalize_fail(g, r, rc);
    if (hipStreamSynchronize(c->stream) != hipSuccess) {
      c->err = "copy of the level-0 file to shard 0 failed";
      return finalize_fail(g, r, SWZ_ERR_HIP);
    }
    files[r] = mine;
  }
  (void)hipSetDevice(g->devices[0]);
  if (rows_to_shard0(g, cnt, off, {{all, files, 24}}) != hipSuccess) {
    c0->err = "copy of the level-0 files to shard 0 failed";
    return finalize_fail(g, 0, SWZ_ERR_HIP);
  }
  int rc = swz_morton_encode_device(c0, all, total, g->tbmin, g->tbmax, keys);
  if (rc == SWZ_OK) rc = swz_sort_by_key_device(c0, keys, total, perm, skeys);
  if (rc == SWZ_OK)
    rc = swz::sample_points_device(c0, g->tparams.sampler, g->tparams.max_points_per_node, skeys, perm, (uint32_t)total, all, 0, -1, g->tbmin,
                                   g->tbmax, g->tparams.spacing_at_root, SWZ_ALWAYS_ADHERE_TO_MIN_SPACING, taken, nullptr);
  if (rc != SWZ_OK) return finalize_fail(g, 0, rc);
  hipLaunchKernelGGL(grp_unsort_flags_kernel, dim3((uint32_t)((total + 255) / 256)), dim3(256), 0, c0->stream, perm, taken, (uint32_t)total, *d_flags0);
  if (hipStreamSynchronize(c0->stream) != hipSuccess) {
    c0->err = "root reconstruction failed on the device";
    return finalize_fail(g, 0, SWZ_ERR_HIP);
  }
  return SWZ_OK;
}

int swz_group_finalize(swz_group* g, swz_tile_stats* stats) {
  if (!g) return SWZ_ERR_BAD_ARG;
  if (g->tiler.empty() || !g->staged.empty()) {
    g->err = g->tiler.empty() ? "swz_group_finalize: no data set is open" : "swz_group_finalize: staged batches have not been tiled";
    return SWZ_ERR_BAD_ARG;
  }
  const bool fast = g->tparams.strategy == SWZ_FAST && g->fast_start > 0;
  for (int r = 0; r < g->n; ++r) {
    (void)hipSetDevice(g->devices[r]);
    swz_tile_stats st{};
    const int rc = fast ? swz_tiler_shard_fast_finalize_local(g->tiler[r], &st) : swz_tiler_finalize(g->tiler[r], &st);
    if (rc != SWZ_OK) return finalize_fail(g, r, rc);
    if (stats) stats[r] = st;
  }
  if (!fast) return SWZ_OK;
  // FAST: the root is rebuilt from the level-0 files of all shards on shard 0; every shard keeps the part of the root's
  // file that comes from its own points
  std::vector<uint64_t> cnt(g->n, 0), off(g->n + 1, 0);
  for (int r = 0; r < g->n; ++r) {
    (void)hipSetDevice(g->devices[r]);
    const int rc = swz_tiler_level_count(g->tiler[r], 0, &cnt[r]);
    if (rc != SWZ_OK) return finalize_fail(g, r, rc);
    off[r + 1] = off[r] + cnt[r];
  }
  uint8_t* d_flags0 = nullptr;
  if (off[g->n] > 0xFFFF0000ull) {
    g->err = "more than 2^32-65536 points in the level-0 files";
    return SWZ_ERR_TOO_MANY_POINTS;
  }
  if (off[g->n]) {
    const int rc = finalize_fast_root_on_shard0(g, cnt, off, &d_flags0);
    if (rc != SWZ_OK) return rc;
  }
  for (int r = 0; r < g->n; ++r) {
    (void)hipSetDevice(g->devices[r]);
    swz_ctx* c = g->ctx[r];
    uint8_t* mine = (r == 0 && cnt[0]) ? d_flags0 : nullptr;
    if (cnt[r] && r != 0) {
      if (c->get("grp_l0_flags", (size_t)cnt[r], &mine) != SWZ_OK) return finalize_fail(g, r, SWZ_ERR_HIP);
      if (flags_to_shard(g, r, mine, d_flags0 + off[r], cnt[r]) != hipSuccess) {
        c->err = "copy of the root flags failed";
        return finalize_fail(g, r, SWZ_ERR_HIP);
      }
    }
    const int rc = swz_tiler_shard_fast_set_root(g->tiler[r], mine);
    if (rc != SWZ_OK) return finalize_fail(g, r, rc);
  }
  return SWZ_OK;
}

}  // extern "C"

// ------------------------------------------------------------------------------- the data set of a group written in one call
// swz_group_write_output: swz_tiler_write_output's three parts (swz_toutput.h) -- validate and plan ONCE on the merged node
// table, stream the node files per shard, write the metadata ONCE.  Barriers of a shard thread (every thread, failed or not,
// passes both):
//   O1  every shard's part of the root's file is gathered (then shard 0 copies the parts, packs and writes the root)
//   O2  every shard's files are written; nobody reads a neighbour's part any more (then the call's workspace goes back)
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
  swz_tiler* t = g->tiler[r];
  const auto t_begin = std::chrono::steady_clock::now();
  swz::OutputWorkspace ow{c};
  const swz::OutputPlan& p = o->plan[r];
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
    if (s.ok) {
      hipLaunchKernelGGL(grp_iota_kernel, dim3((uint32_t)((root_rows + 255) / 256)), dim3(256), 0, c->stream, iota, (uint32_t)root_rows);
      s.hip(hipGetLastError(), "the ids of the root's rows");
    }
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
    int st = swz_tiler_get_info(g->tiler[r], &info);
    const uint64_t cap = std::max<uint64_t>(info.num_nodes, 1);
    std::vector<uint64_t> offset(cap);
    level[r].resize(cap);
    key[r].resize(cap);
    count[r].resize(cap);
    uint64_t nn = 0;
    if (st == SWZ_OK) st = swz_tiler_node_table(g->tiler[r], cap, level[r].data(), key[r].data(), offset.data(), count[r].data(), &nn);
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

}  // namespace

extern "C" {

int swz_group_node_table(swz_group* g, uint64_t max_nodes, int8_t* level_out, uint64_t* key_out, uint64_t* count_out,
                         int32_t* shard_out, uint64_t* num_nodes_out) {
  if (!g || !num_nodes_out) return SWZ_ERR_BAD_ARG;
  if (g->tiler.empty()) {
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
  if (g->tiler.empty() || !g->staged.empty()) {
    g->err = g->tiler.empty() ? "swz_group_write_output: no data set is open (swz_group_tiler_open)" : "swz_group_write_output: a batch is staged or open";
    return SWZ_ERR_BAD_ARG;
  }
  const auto t_wall = std::chrono::steady_clock::now();
  const int N = g->n;
  std::fill(g->status.begin(), g->status.end(), SWZ_OK);
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
    const int st = swz::output_tiler_table(g->tiler[r], who, &o.plan[r], &o.info[r]);
    if (st != SWZ_OK) return refuse(r, st);
    attr_mask |= g->tiler[r]->attr_mask;
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
  if ((st = swz::output_plan(c0, who, params, attr_mask, g->tbmin, g->tbmax, g->tparams.spacing_at_root, dir, &merged)) != SWZ_OK) return refuse(-1, st);
  o.part_cnt.assign(N, 0);
  o.part_off.assign(N + 1, 0);
  o.part_xyz.assign(N, nullptr);
  o.part_attr.assign(SWZ_ATTR_COUNT, std::vector<const void*>(N, nullptr));
  for (int r = 0; r < N; ++r) {
    if (!o.plan[r].count.empty() && o.plan[r].level[0] < 0) o.part_cnt[r] = o.plan[r].count[0];
    o.part_off[r + 1] = o.part_off[r] + o.part_cnt[r];
    if ((st = swz::output_plan(g->ctx[r], who, params, attr_mask, g->tbmin, g->tbmax, g->tparams.spacing_at_root, dir, &o.plan[r])) != SWZ_OK) return refuse(r, st);
  }
  if (o.part_off[N]) {
    o.root.level.assign(1, (int8_t)-1);
    o.root.key.assign(1, 0);
    o.root.offset.assign(1, 0);
    o.root.count.assign(1, o.part_off[N]);
    if ((st = swz::output_plan(c0, who, params, attr_mask, g->tbmin, g->tbmax, g->tparams.spacing_at_root, dir, &o.root)) != SWZ_OK) return refuse(-1, st);
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
  st = SWZ_OK;
  for (int r = 0; r < N && st == SWZ_OK; ++r)
    if (g->status[r] != SWZ_OK) {
      g->err = "shard " + std::to_string(r) + ": " + g->status_msg[r];
      st = g->status[r];
    }
  std::fill(g->status.begin(), g->status.end(), SWZ_OK);  // (a failed write marks no shard: the group stays usable)
  // ---- the metadata, once, from the merged table
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

// ------------------------------------------------------------------------- the joint root for one PROCESS per GPU
// swz_group sweeps the MIN_DISTANCE root with all shards at once because its shards share an address space.  A driver
// with one process per GPU (torch.distributed) gets the same through IPC: inside the begin call of its batch every rank
// exports the arrays of its root level (hipIpcGetMemHandle on the allocations they live in + offsets), the driver's
// all-gather callback passes the blobs round, and every rank maps the arrays of the LOWER ranks (hipIpcOpenMemHandle).
// From there on the sweep is the one of swz_mdkeys.hip / swz_mqsweep.hip: remote records bracketed by the owner's round word, system-scope
// loads, cells at the faces polling.  swz_shard_joint_root_end -- after the driver's barrier, when every rank has
// finished its root -- unmaps.
}  // extern "C"
namespace {
struct JointBlob {
  hipIpcMemHandle_t handle[9];
  uint64_t offset[9];
  uint8_t has[9];
  uint32_t ncells, rg, cell_shift, npoints;
  int32_t status, entered;
};
struct JointState {
  swz::MdShardRoot sr;
  std::vector<swz::MdPeerView> views;
  swz_exchange_fn exchange = nullptr;
  void* exchange_arg = nullptr;
  std::vector<std::pair<hipIpcMemHandle_t, void*>> opened;  // one mapping per allocation
  std::string err;
  swz_ctx* c = nullptr;
};
std::map<swz_ctx*, JointState*>& joint_states() {
  static std::map<swz_ctx*, JointState*> m;
  return m;
}
std::mutex joint_m;

void* joint_open(JointState* js, const hipIpcMemHandle_t& h) {
  for (auto& kv : js->opened)
    if (std::memcmp(&kv.first, &h, sizeof(h)) == 0) return kv.second;
  void* p = nullptr;
  if (hipIpcOpenMemHandle(&p, h, hipIpcMemLazyEnablePeerAccess) != hipSuccess) {
    (void)hipGetLastError();
    return nullptr;
  }
  js->opened.emplace_back(h, p);
  return p;
}

// the "barrier" of MdShardRoot: every rank has published its view in views[shard] -- exchange them
void joint_exchange(void* arg) {
  JointState* js = static_cast<JointState*>(arg);
  const int N = js->sr.shards, r = js->sr.shard;
  swz::MdPeerView& mine = js->views[r];
  JointBlob blob{};
  const void* ptrs[9] = {mine.rec, mine.qpos, mine.state, mine.ovf, mine.gridmap, mine.round_word, mine.perm, mine.xyz, mine.aidx};
  blob.ncells = mine.ncells;
  blob.npoints = mine.npoints;
  blob.rg = mine.rg;
  blob.cell_shift = mine.cell_shift;
  blob.status = mine.status;
  blob.entered = 1;
  for (int k = 0; k < 9 && mine.ncells; ++k) {
    if (!ptrs[k]) continue;
    void* base = nullptr;
    size_t size = 0;
    if (hipMemGetAddressRange(&base, &size, const_cast<void*>(ptrs[k])) != hipSuccess ||
        hipIpcGetMemHandle(&blob.handle[k], base) != hipSuccess) {
      (void)hipGetLastError();
      blob.status = SWZ_ERR_HIP;  // (e.g. memory that does not come from hipMalloc)
      continue;
    }
    blob.offset[k] = (uint64_t)((const char*)ptrs[k] - (const char*)base);
    blob.has[k] = 1;
  }
  std::vector<JointBlob> all((size_t)N);
  if (js->exchange(js->exchange_arg, &blob, sizeof(JointBlob), all.data()) != 0) {
    // Nobody sweeps.  The other ranks still run the vote below: take part in it (with an error), or this rank would be one
    // collective behind for everything that follows.
    for (int p = 0; p < N; ++p) js->views[p].status = SWZ_ERR_INTERNAL;
    JointBlob vote{};
    vote.status = SWZ_ERR_INTERNAL;
    std::vector<JointBlob> votes((size_t)N);
    (void)js->exchange(js->exchange_arg, &vote, sizeof(JointBlob), votes.data());
    return;
  }
  for (int p = 0; p < N; ++p) {
    if (p == r) {
      js->views[p].status = blob.status;
      continue;
    }
    swz::MdPeerView v{};
    v.ncells = all[p].ncells;
    v.rg = all[p].rg;
    v.npoints = all[p].npoints;
    v.cell_shift = all[p].cell_shift;
    v.status = all[p].status;
    v.entered = all[p].entered;
    if (p < r && v.ncells && v.status == SWZ_OK) {  // only the lower ranks' arrays are read
      const void* got[9] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
      for (int k = 0; k < 9; ++k) {
        if (!all[p].has[k]) continue;
        char* base = static_cast<char*>(joint_open(js, all[p].handle[k]));
        if (!base) {
          v.status = SWZ_ERR_HIP;
          break;
        }
        got[k] = base + all[p].offset[k];
      }
      v.rec = static_cast<const uint4*>(got[0]);
      v.qpos = static_cast<const uint64_t*>(got[1]);
      v.state = static_cast<const uint8_t*>(got[2]);
      v.ovf = static_cast<const float4*>(got[3]);
      v.gridmap = static_cast<const uint32_t*>(got[4]);
      v.round_word = static_cast<const uint32_t*>(got[5]);
      v.perm = static_cast<const uint32_t*>(got[6]);
      v.xyz = static_cast<const double*>(got[7]);
      v.aidx = static_cast<const uint32_t*>(got[8]);
    }
    js->views[p] = v;
  }
  // (a mapping that failed on ONE rank must stop all of them, or the others sweep against a rank that has given up: the
  // statuses are voted on)
  int32_t my_ok = 1;
  for (int p = 0; p < N; ++p) my_ok &= js->views[p].status == SWZ_OK ? 1 : 0;
  JointBlob vote{};
  vote.status = my_ok ? SWZ_OK : SWZ_ERR_INTERNAL;
  std::vector<JointBlob> votes((size_t)N);
  if (js->exchange(js->exchange_arg, &vote, sizeof(JointBlob), votes.data()) != 0) vote.status = SWZ_ERR_INTERNAL;
  for (int p = 0; p < N; ++p)
    if (votes[p].status != SWZ_OK || vote.status != SWZ_OK) js->views[p].status = SWZ_ERR_INTERNAL;
}
}  // namespace
extern "C" {

int swz_shard_joint_root_possible(swz_ctx* c, const swz_tile_params* p, const double bmin[3], const double bmax[3]) {
  if (!c || !p) return 0;
  return joint_root_possible(c, *p, bmin, bmax) ? 1 : 0;
}

// Can the ranks of this run map each other's device memory at all?  Every rank exports a small buffer of its workspace that
// holds a pattern, the lower ranks' buffers are opened and read back, and the outcome is voted on -- two exchanges, like the
// real thing -- so that a driver can settle for the chain of ghosts BEFORE a batch depends on the mappings (containers
// without a shared /dev/shm, devices without a peer path, IPC switched off).  *usable = 1 only when every rank could map
// and read every lower rank's buffer.
int swz_shard_joint_root_probe(swz_ctx* c, int shard, int shards, swz_exchange_fn exchange, void* arg, int* usable) {
  if (!c || !exchange || !usable || shards < 1 || shards > 8 || shard < 0 || shard >= shards) return SWZ_ERR_BAD_ARG;
  *usable = 0;
  (void)hipSetDevice(c->device);
  struct ProbeBlob {
    hipIpcMemHandle_t handle;
    uint64_t offset;
    int32_t status;
    uint32_t pattern;
  };
  ProbeBlob mine{};
  mine.pattern = 0x5C4A0000u + (uint32_t)shard;
  uint32_t* buf = nullptr;
  mine.status = c->get("grp_ipc_probe", (size_t)64, &buf);
  if (mine.status == SWZ_OK) {
    void* base = nullptr;
    size_t size = 0;
    if (hipMemcpy(buf, &mine.pattern, 4, hipMemcpyHostToDevice) != hipSuccess || hipMemGetAddressRange(&base, &size, buf) != hipSuccess ||
        hipIpcGetMemHandle(&mine.handle, base) != hipSuccess) {
      (void)hipGetLastError();
      mine.status = SWZ_ERR_HIP;
    } else {
      mine.offset = (uint64_t)((const char*)buf - (const char*)base);
    }
  }
  std::vector<ProbeBlob> all((size_t)shards);
  int32_t ok = mine.status == SWZ_OK ? 1 : 0;
  std::vector<void*> opened;
  if (exchange(arg, &mine, sizeof(ProbeBlob), all.data()) != 0) {
    ok = 0;
  } else {
    for (int p = 0; p < shards && ok; ++p) ok &= all[p].status == SWZ_OK ? 1 : 0;
    for (int p = 0; p < shard && ok; ++p) {  // only the lower ranks' arrays are ever read
      void* base = nullptr;
      uint32_t got = 0;
      if (hipIpcOpenMemHandle(&base, all[p].handle, hipIpcMemLazyEnablePeerAccess) != hipSuccess) {
        (void)hipGetLastError();
        ok = 0;
        break;
      }
      opened.push_back(base);
      if (hipMemcpy(&got, (const char*)base + all[p].offset, 4, hipMemcpyDeviceToHost) != hipSuccess || got != all[p].pattern) {
        (void)hipGetLastError();
        ok = 0;
      }
    }
  }
  ProbeBlob vote{};
  vote.status = ok ? SWZ_OK : SWZ_ERR_INTERNAL;
  std::vector<ProbeBlob> votes((size_t)shards);
  int all_ok = ok;
  if (exchange(arg, &vote, sizeof(ProbeBlob), votes.data()) != 0) all_ok = 0;
  for (int p = 0; p < shards && all_ok; ++p) all_ok &= votes[p].status == SWZ_OK ? 1 : 0;
  // Unmap, one rank at a time (the exchange is the barrier between them): with several processes closing mappings of one
  // allocation at the same moment the runtime was seen to abort ("Memobj map does not have ptr", one run in four with
  // four processes on one GPU) -- never with the closes taken in turns.
  for (int p = 0; p < shards; ++p) {
    if (p == shard)
      for (void* b : opened) (void)hipIpcCloseMemHandle(b);
    ProbeBlob turn{};
    std::vector<ProbeBlob> turns((size_t)shards);
    if (exchange(arg, &turn, sizeof(ProbeBlob), turns.data()) != 0) all_ok = 0;
  }
  *usable = all_ok;
  return SWZ_OK;
}

int swz_shard_joint_root_begin(swz_ctx* c, int shard, int shards, swz_exchange_fn exchange, void* arg) {
  if (!c || !exchange || shards < 2 || shards > 8 || shard < 0 || shard >= shards) return SWZ_ERR_BAD_ARG;
  std::lock_guard<std::mutex> lk(joint_m);
  JointState*& js = joint_states()[c];
  if (!js) js = new JointState;
  if (!js->opened.empty()) return c->fail(SWZ_ERR_BAD_ARG, "swz_shard_joint_root_begin: the previous joint root was not ended");
  js->c = c;
  js->views.assign((size_t)shards, swz::MdPeerView{});
  js->sr.shard = shard;
  js->sr.shards = shards;
  js->sr.views = js->views.data();
  js->sr.barrier = joint_exchange;
  js->sr.barrier_arg = js;
  js->exchange = exchange;
  js->exchange_arg = arg;
  c->md_shard_root = &js->sr;
  c->md_shard_root_published = true;  // (until swz_shard_joint_root_end, which the driver calls after its barrier)
  return SWZ_OK;
}

// A rank whose begin call did not reach the sweep (no points, or an error before it) meets the others here.
int swz_shard_joint_root_meet(swz_ctx* c, int ok) {
  if (!c) return SWZ_ERR_BAD_ARG;
  JointState* js = nullptr;
  {
    std::lock_guard<std::mutex> lk(joint_m);
    auto it = joint_states().find(c);
    if (it != joint_states().end()) js = it->second;
  }
  if (!js || !c->md_shard_root) return c->fail(SWZ_ERR_BAD_ARG, "swz_shard_joint_root_meet: no joint root is open");
  swz::MdPeerView& mine = js->views[js->sr.shard];
  if (mine.entered) return SWZ_OK;
  mine = swz::MdPeerView{};
  mine.status = ok ? SWZ_OK : SWZ_ERR_INTERNAL;
  mine.entered = 1;
  joint_exchange(js);
  return SWZ_OK;
}

int swz_shard_joint_root_end(swz_ctx* c) {
  if (!c) return SWZ_ERR_BAD_ARG;
  std::lock_guard<std::mutex> lk(joint_m);
  auto it = joint_states().find(c);
  c->md_shard_root = nullptr;
  c->md_shard_root_published = false;
  if (it == joint_states().end()) return SWZ_OK;
  JointState* js = it->second;
  (void)hipSetDevice(c->device);
  for (auto& kv : js->opened) (void)hipIpcCloseMemHandle(kv.second);
  js->opened.clear();
  delete js;
  joint_states().erase(it);
  return SWZ_OK;
}

}  // extern "C"
