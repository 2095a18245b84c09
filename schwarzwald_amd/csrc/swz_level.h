// swz_level.h -- the state of one level and the entry points around it: what the drivers of the level loop
// (swz_session.hip, swz_shard.hip, swz_tlevel.hip) hand to level_step (swz_level.hip), and what level_step hands to the
// level's sampler (swz_grid.hip; MIN_DISTANCE: swz_md.h).
#pragma once
#include "swz_device.h"
#include "swz_internal.h"

namespace swz {

enum : uint8_t { MODE_TAKE_ALL = 0, MODE_SAMPLE = 1 };

// the samplers that run the greedy minimum-distance test (MIN_DISTANCE_FAST: on every n-th point of a node, swz_mdfast.hip)
inline bool greedy_sampler(int sampler) { return sampler == SWZ_MIN_DISTANCE || sampler == SWZ_MIN_DISTANCE_FAST; }

// device counters of one level iteration
enum {
  CTR_NUM_NODES = 0,     // nodes at this level
  CTR_SAMPLE_NODES = 1,  // nodes that run the sampler (count > max_points or forced)
  CTR_SAMPLE_POINTS = 2, // points inside those nodes
  CTR_ERROR = 3,         // SWZ_ERR_* raised by a kernel (0 = none)
  CTR_REMAINING = 4,     // points handed to the next level
  CTR_NUM_CELLS = 5,     // MIN_DISTANCE: cells
  CTR_DONE_CELLS = 6,    // MIN_DISTANCE: cells finished
  CTR_LIVE_NODES = 7,    // a level that shares its arrays with the level above (ActiveSet::gone): nodes that hold an open point
  CTR_Q0 = 8,            // MIN_DISTANCE: three rotating queue counters
  // MIN_DISTANCE sweep, builds with -DSWZ_MD_STATS only (printed with SWZ_DEBUG=1): timings of a sample of the
  // activations in 10 ns ticks
  CTR_DBG_TIME = 20,     // total
  CTR_DBG_TMAX = 21,     // longest
  CTR_DBG_HIST = 22,     // +0 activations sampled, +1 prologue, +2 chunk loads and rejection tests, +3 blocker scans,
                         // +4 chunks, +5 cells scanned
  CTR_COUNT = 40
};

// The active set of one level: Morton-sorted survivors.  aidx == nullptr means identity (level -1).
struct ActiveSet {
  const uint64_t* akey = nullptr;  // key of every active point
  const uint32_t* aidx = nullptr;  // its position in the fully sorted arrays (X/Y/Z/level)
  uint32_t m = 0;
  // multi-batch tiling (swz_tlevel.hip): the keys of the points earlier batches persisted in the nodes of this level
  // that the active set touches, ascending by node prefix.  A node that has some is sampled with
  // SamplingBehaviour::AlwaysAdhereToMinSpacing (tile_internal_node, TilingAlgorithms.cpp:272-275).
  const uint64_t* ckey = nullptr;
  uint32_t nc = 0;
  // ... and where they sit among the active points: aidx values in [old_lo, old_hi) are pulled entries.  The entries of a
  // file that holds more than max_points were the OUTPUT of this sampler at this spacing, so they are pairwise at least
  // one spacing apart, and MIN_DISTANCE only has to look at what the new points can change (swz_mdblock.hip).
  uint32_t old_lo = 0, old_hi = 0;
  const uint64_t* new_key = nullptr;  // the batch's own points before the merge, ascending
  uint32_t new_m = 0;
  // the nodes that hold files one level further down (their keys with the bits below the node cleared, ascending): a node with a
  // child there has handed points down, i.e. it has been sampled, and its file -- rewritten by every visit since -- is a sampler's
  // output whatever its size
  const uint64_t* child_nkey = nullptr;
  uint32_t child_nn = 0;
  // the nodes of the level above (LevelResult::node_prefix of the step whose survivors these are), when the caller has
  // them: every node of this level is a child of one of them, so its first point is found by searching the sorted keys
  // instead of by a scan over all points (level_step; null: scan)
  const uint64_t* parent_prefix = nullptr;
  uint32_t parents = 0;
  // A chain of dense exact-MIN_DISTANCE levels shares one active set (level_step, LevelChain): the level above did not
  // compact its survivors, akey / aidx / m are still its arrays.  gone[i] == 0: point i is open; gone[i] == k: it was taken
  // at level k - 2 (the root is level -1: code 1).  live: the open points; gone_tiles[t]: the open points before tile t of
  // FS_TILE points (live_before).  Null and m: every point is open, as everywhere outside a chain.
  const uint8_t* gone = nullptr;
  const uint32_t* gone_tiles = nullptr;
  uint32_t live = 0;
};
// what the host decided about the chain a level belongs to (swz_session.hip decides, once, for every level)
struct LevelChain {
  bool may_defer = false;   // this level may leave its survivors where they are (the static conditions and the next level's plan hold)
  double max_gone = 0.125;  // ... while the share of taken points in the shared arrays stays below this
};

struct SortedPoints {
  const double* X = nullptr;  // positions in Morton order, SoA (null when the sampler decides on the keys: see xyz / perm)
  const double* Y = nullptr;
  const double* Z = nullptr;
  // The clamped input positions (AoS, caller's order) and the sort's permutation: sorted position s is point perm[s].
  // MIN_DISTANCE decides almost every pair on the coordinates its keys already hold (swz_mqsweep.hip) and looks up the
  // few pairs inside the quantisation band here, so the positions are never brought into Morton order.
  const double* xyz = nullptr;
  const uint32_t* perm = nullptr;
  // A sharded batch: the first `ghosts` sorted positions are points of lower shards (they sort first: lower octants); their
  // perm entries index ghost_xyz instead.
  const double* ghost_xyz = nullptr;
  uint32_t ghosts = 0;
};
// exact position of sorted position s
__host__ __device__ inline const double* sorted_point_xyz(const double* xyz, const uint32_t* perm, const double* ghost_xyz, uint32_t ghosts,
                                                          uint32_t s) {
  return (s < ghosts ? ghost_xyz : xyz) + (size_t)perm[s] * 3;
}
// ... of sorted point i of a batch, in Morton order or not, to point o of an AoS array
__device__ __forceinline__ void store_sorted_point(const SortedPoints& sp, uint32_t i, double* __restrict__ out_xyz, uint64_t o) {
  if (sp.X) {
    out_xyz[3 * o] = sp.X[i];
    out_xyz[3 * o + 1] = sp.Y[i];
    out_xyz[3 * o + 2] = sp.Z[i];
  } else {  // the positions were never brought into Morton order (the samplers decided on keys)
    const double* p = sorted_point_xyz(sp.xyz, sp.perm, sp.ghost_xyz, sp.ghosts, i);
    out_xyz[3 * o] = p[0];
    out_xyz[3 * o + 1] = p[1];
    out_xyz[3 * o + 2] = p[2];
  }
}

// What the host decides once per level (all float/libm corner cases of the reference live here,
// evaluated with the host's glibc exactly like the reference evaluates them).
struct LevelPlan {
  int level = -1;           // node level (-1 = root)
  uint32_t node_shift = 63; // key >> node_shift == node prefix
  int sampler = 0;
  uint64_t max_points = 0;
  bool force_sample = false; // SamplingBehaviour::AlwaysAdhereToMinSpacing
  bool terminal = false;     // tile_terminal_node: every node of this level keeps all its points
  bool reroot = false;       // sampling this level would need Morton re-rooting
  bool md_property = false;  // MIN_DISTANCE: SWZ_FLAG_MIN_DISTANCE_PROPERTY (swz_mdprop.hip)
  Box root;
  // RANDOM_GRID / GRID_CENTER / MIN_DISTANCE_FAST: candidate_level_in_octree (Sampling.h:223-229); -1 = first point only
  int cand = -1;
  // JITTERED / MIN_DISTANCE
  double spacing_node = 0.0; // spacing_at_root / pow(2, level + 1)
  uint32_t jitter_start = 0; // (3 * (level + 1)) % 16
  // MIN_DISTANCE
  double sq_spacing = 0.0;   // (double)((float)spacing_node * (float)spacing_node)
  // what a taken point's byte in LevelBuffers::taken receives from the key sweep and from take-all nodes: 1, or -- a level
  // that may start or continue a chain of levels on one active set -- level + 2 (ActiveSet::gone)
  uint8_t take_code = 1;
  int cell_levels_geo = 0;   // finest cell subdivision (levels below the node) whose cells are >= spacing
};

struct LevelBuffers {
  uint32_t* flags = nullptr;   // m
  uint32_t* nid = nullptr;     // m
  uint32_t* nstart = nullptr;  // m + 1
  uint8_t* nmode = nullptr;    // m
  uint8_t* taken = nullptr;    // m
  uint32_t* counters = nullptr; // CTR_COUNT (device)
};

struct LevelResult {
  uint32_t remaining = 0;
  uint32_t num_nodes = 0;
  uint32_t md_rounds = 0;
  uint32_t table_nodes = 0;   // entries of the node table (num_nodes, plus -- inside a chain -- the nodes without an open point)
  bool md_keys_direct = false; // the key sweep with direct numbering sampled the level
  bool deferred = false;      // the survivors stayed where they are: lb.taken is the next level's ActiveSet::gone
  const uint32_t* gone_tiles = nullptr;  // ... and its gone_tiles
  bool needs_flush = false;   // a level inside a chain that the key sweep cannot take: nothing was decided, compact and call again
  // the key prefixes of the level's nodes, ascending (device; only when the step compacted survivors: for the next
  // level's ActiveSet::parent_prefix).  Valid until the step after the next one on this context.
  const uint64_t* node_prefix = nullptr;
};

// What the host decides for the nodes of one level (tiler_rules: the terminal / re-root tests of tile_node,
// TilingAlgorithms.cpp:408-444; off for a bare sample_points call).
LevelPlan make_plan(int level, int sampler, uint64_t max_points, float spacing_at_root, uint32_t max_depth,
                    const double bmin[3], const double bmax[3], bool force_sample, bool tiler_rules);
int alloc_level_buffers(swz_ctx* c, uint32_t m, LevelBuffers* lb);
// required_morton_index_depth -- core/tiling/Sampling.cpp:29-62, for a root node with this x extent and max_spacing
int required_depth_host(int sampler, int node_level, double root_extent_x, float root_max_spacing);
// Samples every node of the level.  When okey/oidx are given the survivors are compacted into them and level_out
// receives plan.level for the taken points; otherwise only lb.taken is produced.
// chain: the level may leave the survivors in place (res->deferred) when the key sweep sampled it; a level that receives
// such arrays (as.gone) either samples them as they are or asks for the compaction (res->needs_flush).
int level_step(swz_ctx* c, const LevelPlan& plan, const ActiveSet& as, const SortedPoints& sp, const LevelBuffers& lb,
               int8_t* level_out, uint64_t* okey, uint32_t* oidx, LevelResult* res, const LevelChain* chain = nullptr);
// the compaction that ends a chain: the open points of as into okey / oidx, level_out = code - 2 for the others
int level_flush_chain(swz_ctx* c, const ActiveSet& as, const LevelBuffers& lb, int8_t* level_out, uint64_t* okey, uint32_t* oidx,
                      uint32_t* remaining);
// what a kernel of the level raised in CTR_ERROR, in words
const char* level_error_message(int code);
// estimate_start_node_level_in_octree (TilingAlgorithms.cpp:1473-1535) of a sorted batch
int fast_start_level(swz_ctx* c, const uint64_t* d_keys_sorted, uint32_t n, uint32_t concurrency, int* start_level);
// the same in two steps for a batch that is spread over several GPUs: counts per 6-octant prefix (2^18, host), summed by
// the driver, then the estimate
int fast_prefix_counts(swz_ctx* c, const uint64_t* d_keys_sorted, uint32_t n, uint32_t* counts_host);
int fast_start_level_from_counts(const uint64_t* counts, uint32_t concurrency);

// ---- the samplers of a level (called by level_step after the node segmentation; each fills lb.taken) ----------------
// RANDOM_GRID (swz_grid.hip): the first point of every candidate cell; candidate level -1 (GRID_CENTER's and
// MIN_DISTANCE_FAST's too): of every node.
int random_grid_level(swz_ctx* c, const LevelPlan& plan, const ActiveSet& as, const LevelBuffers& lb);
// GRID_CENTER / JITTERED (swz_grid.hip): on key coordinates when grid_level_uses_keys, else on sp.X / sp.Y / sp.Z
int grid_level(swz_ctx* c, const LevelPlan& plan, const ActiveSet& as, const SortedPoints& sp, const LevelBuffers& lb);
// true when grid_level will not need sp.X / sp.Y / sp.Z for this level
bool grid_level_uses_keys(const swz_ctx* c, const LevelPlan& plan, const SortedPoints& sp);
// MIN_DISTANCE for one level, exact or (plan.md_property) in property mode; fills lb.taken for the points of
// MODE_SAMPLE nodes (take-all points are flagged by the caller).  rounds_out accumulates the dependency rounds or
// phases executed.  swz_md.hip decides which algorithm samples the level.
// keys_direct (may be null): the key sweep with direct numbering took the level.  Inside a chain (as.gone) no other
// algorithm may: *needs_flush then says that the level was left untouched.
int min_distance_level(swz_ctx* c, const LevelPlan& plan, const ActiveSet& as, const SortedPoints& sp,
                       const LevelBuffers& lb, uint32_t num_nodes, uint32_t sample_nodes,
                       uint32_t sample_points, uint32_t* rounds_out, bool* keys_direct = nullptr, bool* needs_flush = nullptr);
// MIN_DISTANCE_FAST on a level whose stride is above one (swz_mdfast.hip): the candidates -- every stride-th point of every
// MODE_SAMPLE node, counted from the node's first -- as an active set of their own through min_distance_level, the decisions
// scattered back into lb.taken (zero for the points of sampled nodes on entry).
int min_distance_fast_level(swz_ctx* c, const LevelPlan& plan, const ActiveSet& as, const SortedPoints& sp, const LevelBuffers& lb,
                            uint32_t stride, uint32_t num_nodes, uint32_t sample_nodes, uint32_t* rounds_out);

}  // namespace swz
