// swz_group.h -- what the files of swz_group share: the group itself, the barrier and the RCCL entry points of its shard
// threads, a thread's Step, and the peer copies between shard 0 and the others.
//   swz_group.hip    create / destroy, the steps of a call, shard_thread, swz_group_tile and swz_group_add_batch
//   swz_gtiler.hip   a data set in several batches: the group's tilers, staged batches, LAS files in one call, finalize
//   swz_goutput.hip  that data set's node table, and its files written in one call
// (swz_shardipc.hip, the joint root of a driver with one PROCESS per GPU, completes swz_shard.hip and knows no swz_group.)
#pragma once
#include <dlfcn.h>

#include <array>
#include <chrono>
#include <condition_variable>
#include <mutex>

#include "swz_md.h"
#include "swz_tiler.h"

namespace swz {

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

// one of a shard's two device buffers for staged batches
struct StageSlot {
  double* xyz = nullptr;
  swz_attribute_columns attr{};
  uint64_t cap = 0;           // rows
  hipEvent_t done = nullptr;  // behind the copy (or the decode) that fills it
};

}  // namespace swz

struct swz_group {
  int n = 0;
  int transport = 0;
  std::vector<int> devices;
  std::vector<swz_ctx*> ctx;
  std::vector<void*> comms;
  swz::Rccl rccl;
  std::string err;
  swz::Barrier barrier;
  bool peer_access = true;  // kernels of one shard may read the memory of every other (the joint MIN_DISTANCE root does)
  std::vector<std::array<double, 4>> timing;  // per shard, ms since the call began: exchange done, root begun, root done, levels done
  std::chrono::steady_clock::time_point t_call;
  // per call, shared between the shard threads: what the exchange and the root step pass from shard to shard
  struct Call {
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
    std::vector<swz::MdPeerView> views;       // MIN_DISTANCE root swept by all shards at once: what every shard publishes
    std::vector<std::vector<uint32_t>> hist;  // FAST: every shard's points per 6-octant prefix (a tiler's first batch only)
  } call;
  // FAST in swz_group_tile: what every shard's level-0 nodes hold (the root is reconstructed from all of them on shard 0)
  struct Candidates {
    int start = -1;  // the start level
    std::vector<uint64_t*> keys;
    std::vector<double*> xyz;
    std::vector<uint64_t> count;
    uint8_t* flags = nullptr;
  } cand;
  // a data set in several batches: one swz_tiler per shard (swz_group_tiler_open)
  struct DataSet {
    std::vector<swz_tiler*> tiler;
    std::vector<uint64_t> root_stored;  // points in the root's file on every shard (before / after the batch's root step)
    double bmin[3] = {0, 0, 0}, bmax[3] = {0, 0, 0};
    swz_tile_params params{};
    bool has_srs = false;  // swz_group_set_source_srs: swz_group_add_las_files projects its input to ECEF
    swz_srs srs{};
    int fast_start = -1;  // FAST: the start level, known after the first batch
  } ds;
  // batches staged from pinned host memory: two device buffers per shard, filled on a copy stream of their own
  struct Staged { std::vector<uint64_t> n; int slot = 0; };  // a staged batch: its rows per shard, and the slot it lies in
  struct Stage {
    std::vector<Staged> staged;  // at most two, oldest first
    std::vector<hipStream_t> copy_stream;
    std::vector<std::array<swz::StageSlot, 2>> slot;  // [shard][slot]
    uint32_t mask = 0;  // attribute columns of the staged batches (the same for every batch)
    int next_slot = 0;
  } stage;
};

namespace swz {

// true when no shard has reported a failure (looked at by every shard thread right after a barrier, so all of them see
// the same answer and leave the collective steps together)
inline bool all_ok(const swz_group* g) {
  for (int s : g->call.status)
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
    g->call.status[r] = code;
    g->call.status_msg[r] = msg;
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
    std::unique_lock<std::mutex> lk(g->call.turn_m);
    g->call.turn_cv.wait(lk, [&] { return g->call.turn == r; });
  }
  void pass_turn() {
    {
      std::lock_guard<std::mutex> lk(g->call.turn_m);
      g->call.turn = r + 1;
    }
    g->call.turn_cv.notify_all();
  }
};

// the text of a failure of shard r
inline std::string shard_says(int r, const std::string& what) { return "shard " + std::to_string(r) + ": " + what; }
// after the shard threads of a call have ended: the status of the first shard that failed, its text in g->err
inline int first_failure(swz_group* g) {
  int r = 0;
  while (r < g->n && g->call.status[r] == SWZ_OK) ++r;
  if (r < g->n) g->err = shard_says(r, g->call.status_msg[r]);
  return r < g->n ? g->call.status[r] : SWZ_OK;
}

// The columns every shard hands over (attrs[r], host or device pointers; NULL: none) as a mask, or the refusal: every
// shard must hand over the same ones.
inline int common_columns(swz_group* g, const swz_attribute_columns* attrs, uint32_t* mask) {
  *mask = 0;
  for (int r = 0; attrs && r < g->n; ++r) {
    uint32_t mine = 0;
    for (int t = 0; t < SWZ_ATTR_COUNT; ++t)
      if (attrs[r].column[t]) mine |= 1u << t;
    if (r == 0) *mask = mine;
    if (mine == *mask) continue;
    g->err = "every shard must hand over the same attribute columns";
    return SWZ_ERR_BAD_ARG;
  }
  return SWZ_OK;
}

// "Rows of all shards onto shard 0": cnt[p] rows of every column from shard p to row off[p] on shard 0, by peer copies on
// the default stream.  Called with shard 0's device current; the sources' streams are idle.  Returns the first error.
struct PeerColumn {
  void* dst;                     // on shard 0
  std::vector<const void*> src;  // per shard
  size_t row_bytes;
};
inline hipError_t rows_to_shard0(swz_group* g, const std::vector<uint64_t>& cnt, const std::vector<uint64_t>& off, const std::vector<PeerColumn>& columns) {
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
inline hipError_t flags_to_shard(swz_group* g, int r, uint8_t* mine, const uint8_t* d_flags0, uint64_t count) {
  hipError_t e = hipStreamSynchronize(g->ctx[r]->stream);  // (the copy is not ordered with this shard's stream)
  if (e == hipSuccess) e = hipMemcpyPeer(mine, g->devices[r], d_flags0, g->devices[0], (size_t)count);
  if (e == hipSuccess) e = hipDeviceSynchronize();
  return e;
}

// swz_group.hip, grp_iota_kernel: d_out[i] = i for i < n, on `stream`; the launch's error
hipError_t group_iota(hipStream_t stream, uint32_t* d_out, uint64_t n);

}  // namespace swz
