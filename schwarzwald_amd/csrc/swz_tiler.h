// swz_tiler.h -- what the files of the multi-batch tiler share: the node store's levels, a batch's working state, the
// tiler itself, and the host functions by which one file reaches another's kernels (the build has no relocatable device
// code: a kernel is launched only from the file that defines it).
//   swz_tstore.hip   the node store and the pools
//   swz_tlevel.hip   one level of a batch: pull, merge, sample, store
//   swz_treroot.hip  re-rooting
//   swz_tiler.hip    the batch life cycle, FAST finalize, the node table and the C ABI
//   swz_toutput.hip  the node files written in one call
//   swz_tinput.hip   a data set of LAS files read in one call
// and, for several GPUs in one process, over swz_group.h:
//   swz_group.hip    the steps of a sharded call   swz_gtiler.hip  the group's tilers   swz_goutput.hip  their output
#pragma once
#include <string>
#include <vector>

#include "swz_md.h"
#include "swz_scan.h"

namespace swz {

static const uint32_t TILER_ATTR_BYTES[SWZ_ATTR_COUNT] = {3, 12, 2, 1, 1, 8, 1, 1, 2, 1, 1, 1};

// The files of one octree level.  Two forms:
//   linear: side `cur` holds exactly the `cnt` live entries, node after node in node order (what every reader but the
//           level loop wants: export, node table, finalize, re-rooting);
//   log:    a batch must not move the files of the nodes it does not reach (batches of a real data set -- LAS tiles --
//           reach a small part of the tree), so the level loop only APPENDS the new versions of the files it rewrites at
//           `end` and keeps a node table {node key, offset, count} that says where each node's current file lies; the
//           old versions stay behind as garbage until the side is full, then the live files are gathered into the other
//           side (store_compact).  Per batch and level the store costs what the batch pulls and writes, not what it holds.
// store_table() / store_linearize() convert between the two.
struct StoreLevel {
  uint64_t* key[2] = {nullptr, nullptr};
  uint32_t* gid[2] = {nullptr, nullptr};
  size_t cap[2] = {0, 0};
  int cur = 0;
  uint32_t cnt = 0;          // live entries
  uint32_t end = 0;          // entries of side `cur` in use (live + garbage)
  bool linear = true;
  bool table_valid = false;
  uint64_t* nkey[2] = {nullptr, nullptr};  // node table, ascending by node key (the key with the bits below the node cleared)
  uint64_t* noff[2] = {nullptr, nullptr};
  uint32_t* ncnt[2] = {nullptr, nullptr};
  int ncur = 0;
  uint32_t nn = 0;
  // every entry carries the key read_pnts_from_disk would give it (relative to its NODE's bounds): files written by the
  // level loop do (TakeStoreG), files written by finalize / re-rooting do not and are re-keyed when they are pulled
  bool rekeyed = true;
};

// One batch on its way through the levels.  `as` (kept beside it) is the active set handed down -- new points and
// displaced old ones --, Morton sorted.
struct BatchWork {
  uint32_t n = 0;          // points of the batch
  uint32_t wused = 0;      // working-pool entries in use
  uint32_t wcap = 0;
  double *wx = nullptr, *wy = nullptr, *wz = nullptr;  // positions by working index -- filled on demand, see work_need_positions
  bool have_pos = false;
  int8_t* wlevel = nullptr;
  uint32_t* wgid = nullptr;
  uint64_t* surv_key[2] = {nullptr, nullptr};
  uint32_t* surv_idx[2] = {nullptr, nullptr};
  int which = 0;
};

// Which way a batch went through the node store: plain host counters, bumped where the host code decides (no kernel knows
// of them), read by swz_tiler_path_counts in this order.  Tests assert that the path they are named after was taken.
enum TilerPath : uint32_t {
  TP_PULL_IN_PLACE = 0,    // level_pull: the batch reaches every node of a linear level, the side is read where it lies
  TP_PULL_GATHERED,        // level_pull: the files were copied out (tl_gather_files_kernel)
  TP_PULL_WHOLE_FILE,      // rr_node: a re-rooted node took its cached file out of a populated level (tl_touch_kernel, SplitG)
  TP_REKEY,                // tl_rekey_kernel launches
  TP_RESORT,               // resort_if_inverted found an inversion and sorted
  TP_COMPACT_FULL,         // level_store: store_compact because the side in use was full
  TP_LINEARIZE_MOVED,      // store_linearize calls that moved data (log form -> linear form)
  TP_APPEND_BEHIND,        // level_store: new files appended behind existing entries (at != 0)
  TP_TABLE_MERGE_NF0,      // tl_table_merge_kernel with no untouched table entry (nf == 0)
  TP_TABLE_MERGE_HEADS0,   // tl_table_merge_kernel with no new file (heads == 0)
  TP_COUNT
};

// what a shard of a multi-GPU batch knows about the other shards (root node only)
struct ShardRoot {
  bool active = false;
  bool sample = false;        // the root samples (global counts), else it takes everything
  const double* ghost_xyz = nullptr;
  uint32_t ghosts = 0;
};

}  // namespace swz

struct swz_tiler {
  swz_ctx* c = nullptr;
  double bmin[3] = {0, 0, 0}, bmax[3] = {0, 0, 0};
  swz_tile_params p{};
  // pools by point id
  double* pool_xyz = nullptr;
  void* pool_attr[SWZ_ATTR_COUNT] = {nullptr};
  uint32_t attr_mask = 0;   // attribute columns the pools hold (fixed by the first staged batch)
  bool has_srs = false;     // swz_tiler_set_source_srs: swz_tiler_add_las_files projects its input to ECEF
  swz_srs srs{};
  size_t pool_cap = 0;      // points
  uint32_t total = 0;       // points tiled so far
  uint32_t staged_total = 0;  // points copied (or being copied) into the pools
  std::vector<uint32_t> staged_sizes;  // batches staged and not yet tiled (at most 2)
  std::vector<hipEvent_t> staged_events;
  hipStream_t copy_stream = nullptr;
  swz::StoreLevel lv[22];  // index = node level + 1
  int fast_start = -1;
  bool finalized = false;
  uint64_t batches = 0;
  uint64_t rekey_inversions = 0;
  uint64_t paths[swz::TP_COUNT] = {0};
  uint64_t staged_bytes = 0;
  double staged_wait_ms = 0.0;  // time swz_tiler_tile_staged had to WAIT for its copy (0 when fully overlapped)
  // a batch between swz_tiler_shard_begin_device and swz_tiler_shard_finish
  bool batch_open = false;
  // A batch that fails part-way leaves levels of the node store merged and its survivors lost: the tiler is poisoned
  // and every later call reports SWZ_ERR_TILER_FAILED (the store must not be read or extended any more).
  bool failed = false;
  std::string failed_why;
  bool shard_fast = false;  // a FAST batch of a sharded data set is open: the start level comes from the driver
  swz::BatchWork bw;
  swz::ActiveSet as;
  int next_level = -1;
  uint64_t acc_visited = 0, acc_nodes = 0;
  uint32_t acc_rounds = 0, acc_levels = 0;
  int acc_max_level = -1;
};

// swz_tiler.hip: what every call of the tiler's API starts with -- SWZ_ERR_TILER_FAILED for a poisoned tiler, else a new
// scratch epoch (swz_tinput.hip's call is one of them)
int tiler_guard(swz_tiler* t);
// the tiler holds no point, has counted no batch, and nothing is staged or open
inline bool tiler_empty(const swz_tiler* t) {
  return !t->total && !t->staged_total && !t->batches && t->staged_sizes.empty() && !t->batch_open;
}
// Why the call `who`, which adds batches, must refuse this tiler: failed (*why = failed_why alone: a tiler and a group word
// that case differently), finalized, or a batch is staged or open.  SWZ_OK: none of them.
inline int tiler_refuses_input(const swz_tiler* t, const char* who, std::string* why) {
  if (t->failed) *why = t->failed_why;
  else if (t->finalized) *why = "swz_tiler: batches cannot be added after finalize";
  else if (!t->staged_sizes.empty() || t->batch_open) *why = std::string(who) + ": a batch is staged or open";
  else return SWZ_OK;
  return t->failed ? SWZ_ERR_TILER_FAILED : SWZ_ERR_BAD_ARG;
}

namespace swz {

struct RrTotals {
  uint64_t nodes = 0, visited = 0;
  int max_level = -1;
};

inline Box root_box(const swz_tiler* t) { return Box{t->bmin[0], t->bmin[1], t->bmin[2], t->bmax[0], t->bmax[1], t->bmax[2]}; }
// key >> store_shift(level_index) is the node prefix of an entry of lv[level_index] (index = node level + 1)
inline uint32_t store_shift(int level_index) { return level_index == 0 ? 63u : level_shift(level_index - 1); }

// static_cast<uint64_t>(double) the way x86-64 gcc compiles it for the reference (cvttsd2si): values in (-1, 0)
// give 0, values <= -1 wrap to huge numbers (which std::min then turns into 2^21 - 1); formally undefined, but it is
// what calculate_morton_index (OctreeAlgorithms.h:76-79) does for a point outside the box it is indexed against.
__device__ __forceinline__ uint64_t cvt_u64_like_x86(double v) {
  return v < 0.0 ? (uint64_t)(int64_t)v : (uint64_t)v;
}
// calculate_morton_index<21>(p, box) without clamping the position -- OctreeAlgorithms.h:64-87
__device__ __forceinline__ uint64_t morton_in_box(double x, double y, double z, const Box& b) {
  const double two21 = 2097152.0;
  const double sx = two21 / (b.maxx - b.minx), sy = two21 / (b.maxy - b.miny), sz = two21 / (b.maxz - b.minz);
  const double nx = (x - b.minx) * sx, ny = (y - b.miny) * sy, nz = (z - b.minz) * sz;
  const uint64_t lim = (1ull << 21) - 1ull;
  uint64_t bx = cvt_u64_like_x86(nx), by = cvt_u64_like_x86(ny), bz = cvt_u64_like_x86(nz);
  bx = bx < lim ? bx : lim;
  by = by < lim ? by : lim;
  bz = bz < lim ? bz : lim;
  return expand_bits_by_3(bz) | (expand_bits_by_3(by) << 1) | (expand_bits_by_3(bx) << 2);
}

struct TakenF {
  const uint8_t* taken;
  __device__ uint32_t operator()(uint32_t i) const { return taken[i] ? 1u : 0u; }
};

// ---- swz_tstore.hip: the node store and the pools
int store_reserve(swz_ctx* c, StoreLevel& s, int level_index, int which, size_t count);
void store_written_linear(StoreLevel& s, int which, uint32_t cnt, bool rekeyed);
int table_reserve(swz_ctx* c, StoreLevel& s, int level_index, int which, size_t count);
int store_table(swz_ctx* c, StoreLevel& s, int level_index);
int store_compact(swz_ctx* c, StoreLevel& s, int level_index, uint64_t* off, const uint32_t* cnt, uint32_t ntab,
                  uint32_t live, size_t room);
int store_linearize(swz_tiler* t, StoreLevel& s, int level_index);  // (counts TP_LINEARIZE_MOVED when it moves data)
int store_write_linear(swz_ctx* c, StoreLevel& dst, int level_index, const uint64_t* tkey, const uint32_t* tgid, uint32_t nt);
int pool_reserve(swz_tiler* t, size_t points);
// The nodes of n keys that ascend by node prefix (key >> shift): where each node starts and its key with the bits below
// the node cleared, in "tl_head_pos" / "tl_head_key".  node_heads_scan leaves their number on the device (*d_heads: slot 3
// of "tl_counters") for a caller that has more to put on the stream before it waits; node_heads reads it back.
int node_heads_scan(swz_ctx* c, const uint64_t* keys, uint32_t n, uint32_t shift, uint32_t** hp, uint64_t** hk, uint32_t** d_heads);
int node_heads(swz_ctx* c, const uint64_t* keys, uint32_t n, uint32_t shift, uint32_t** hp, uint64_t** hk, uint32_t* heads);
// tl_gather_files_kernel: the `segs` segments [psrc[j], + poff[j + 1] - poff[j]) of (skey, sgid), `total` entries in all,
// one behind the other into (okey, ogid)
int gather_files(swz_ctx* c, const uint32_t* poff, const uint64_t* psrc, uint32_t segs, uint32_t total, const uint64_t* skey,
                 const uint32_t* sgid, uint64_t* okey, uint32_t* ogid);

uint32_t gather_lds();  // TL_SEG_LDS: the longest bracket of segment starts tl_gather_files_kernel searches out of LDS

// ---- swz_tlevel.hip: one level of a batch
uint32_t merge_tile();  // TL_MERGE_TILE: elements of a run one workgroup of tl_merge_rank_kernel ranks
uint32_t merge_lds();   // TL_MERGE_LDS: the longest bracket of the other run it searches out of LDS
int tiler_level(swz_tiler* t, BatchWork& w, const LevelPlan& plan_in, ActiveSet& as, LevelResult* res, uint32_t* merged_out,
                const ShardRoot* sr = nullptr);
int work_need_positions(swz_tiler* t, BatchWork& w);
// tl_fill_kernel: wgid[j] = gid[j] (unless wgid is null) and, unless wx is null, (wx, wy, wz)[j] = position gid[j] of the pool
int fill_from_pool(swz_ctx* c, const uint32_t* gid, uint32_t n, const double* pool, double* wx, double* wy, double* wz,
                   uint32_t* wgid);
int merge_pairs(swz_ctx* c, const uint64_t* k1, const uint32_t* v1, uint32_t n1, const uint64_t* k2, const uint32_t* v2,
                uint32_t n2, uint32_t sh, uint32_t base2, uint64_t* ok, uint32_t* ov);
int sort_pairs_by_key(swz_ctx* c, uint64_t* key, uint32_t* gid, uint32_t n);
int resort_if_inverted(swz_tiler* t, uint64_t* key, uint32_t* gid, uint32_t n, uint32_t shift);

// ---- swz_treroot.hip
int tiler_reroot_level(swz_tiler* t, BatchWork& w, const LevelPlan& plan, const ActiveSet& as, RrTotals& tot);

// ---- swz_tiler.hip: the steps of preparing a batch that a level needs as well
// Morton keys of n positions (clamped in place, like index_point) into keys_tmp, then sorted: (keys, perm) receive the
// sorted keys and the index each came from; (keys_tmp, vals_tmp) are scratch
int index_and_sort(swz_ctx* c, double* d_xyz, uint32_t n, const double bmin[3], const double bmax[3], uint64_t* keys_tmp,
                   uint32_t* vals_tmp, uint64_t* keys, uint32_t* perm);
// tl_wgid_kernel: out[i] = base + perm[i]
int add_base(swz_ctx* c, const uint32_t* perm, uint32_t n, uint32_t base, uint32_t* out);

}  // namespace swz
