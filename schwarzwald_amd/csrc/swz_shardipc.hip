// swz_shardipc.hip -- the joint MIN_DISTANCE root for a driver with one PROCESS per GPU; it completes the swz_shard_* calls
// of swz_shard.hip and knows no swz_group.  swz_group sweeps the root with all shards at once because its shards share an
// address space.  A driver with one process per GPU (torch.distributed) gets the same through IPC: inside the begin call of
// its batch every rank exports the arrays of its root level (hipIpcGetMemHandle on the allocations they live in + offsets),
// the driver's all-gather callback passes the blobs round, and every rank maps the arrays of the LOWER ranks
// (hipIpcOpenMemHandle).  From there on the sweep is the one of swz_mdkeys.hip / swz_mqsweep.hip: remote records bracketed
// by the owner's round word, system-scope loads, cells at the faces polling.  swz_shard_joint_root_end -- after the
// driver's barrier, when every rank has finished its root -- unmaps.  swz_shard_joint_root_possible answers for both kinds
// of driver whether the root can be swept jointly at all.
#include <cstring>
#include <mutex>

#include "swz_md.h"

namespace {
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
