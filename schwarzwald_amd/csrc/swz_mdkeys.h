// swz_mdkeys.h -- the key sweep's own header (internal to swz_mdkeys.hip, swz_mqbuild.hip, swz_mqsweep.hip): the
// constants and argument structs its kernels share, the state of one level on the host, and the host functions the three
// files call in each other.  The protocol is described at the top of swz_mdkeys.hip.  A kernel is launched only from
// the file that defines it.
#pragma once
#include <string>
#include <vector>

#include "swz_md.h"

namespace swz {

constexpr uint32_t QNONE = 0xFFFFFFFFu;
constexpr unsigned long long QEMPTY = ~0ull;
constexpr uint32_t MQ_WOKEN = 0x80000000u;  // queue entry: activated by a claimed slot (or never slept): no confirm step
constexpr int MQ_LIST_CAP = 128;            // accepted points of the neighbourhood in LDS (window)
constexpr int MQ_FRESH_CAP = 32;            // points a cell may accept per activation
#ifndef MQ_MINW4
#define MQ_MINW4 4
#endif
#ifndef MQ_MINW1
#define MQ_MINW1 6
#endif
constexpr uint32_t MQ_FIRST_ROUND = 2;      // record buffers start with stamps 0 and 1
constexpr uint32_t MQ_ROUND_DONE = 0xFFFFFFF0u;    // a shard's round word after its sweep: every record is complete
constexpr uint32_t MQ_ROUND_FAILED = 0xFFFFFFF1u;  // ... after it has given up: whoever waits for its cells gives up too

enum : uint8_t { QS_OPEN = 0, QS_TAKEN = 1, QS_DEAD = 2 };

// the root of a batch sharded over the GPUs of one process: what the lower shards publish (swz_md.h, MdPeerView)
constexpr uint32_t MQ_PEER_SHIFT = 28;          // neighbour id = (shard + 1) << 28 | cell for a cell of another shard
constexpr uint32_t MQ_ID_MASK = (1u << MQ_PEER_SHIFT) - 1u;
struct MqPeers {
  const uint4* rec[8];
  const uint64_t* qpos[8];
  const uint8_t* state[8];
  const float4* ovf[8];
  const uint32_t* gridmap[8];
  const uint32_t* round_word[8];
  const uint32_t* perm[8];
  const double* xyz[8];
  const uint32_t* aidx[8];
  uint32_t shard, shards;
};

struct MqArgs {
  const uint64_t* akey;
  const uint32_t* aidx;
  uint32_t m;
  const uint32_t* nid;
  const uint8_t* nmode;
  const uint32_t* nstart;
  const double* xyz;      // exact positions: point perm[aidx ? aidx[i] : i] of the caller's array (pairs inside the band are
                          // rare enough on dense levels that the three dependent loads do not matter)
  const uint32_t* perm;
  const double* gxyz;     // a sharded batch: the first ng sorted positions are ghosts, their perm entries index gxyz
  uint32_t ng;
  uint8_t* taken;
  uint32_t* counters;
  uint64_t* qpos;         // [m] key coordinates x | y << 21 | z << 42 of the active points
  uint8_t* state;         // [m] QS_*
  // How the cells are numbered.  Compacted: the occupied cells in Morton order, 0 .. ncells - 1; crel / csnode / gridmap
  // translate between a cell and its place in the grid.  Direct: the cell IS its place in the grid, id = sample node <<
  // cpn_shift | cell code (still ascending in Morton order); every per-cell array has sample nodes * cells_per_node
  // entries, an empty cell has cinfo.x == cinfo.y == 0, is nobody's neighbour and is never queued; the three tables
  // do not exist (see mq_choose_records_and_numbering, swz_mdkeys.hip, for which level takes which).
  uint32_t direct;
  uint32_t cpn_shift;     // log2(cells_per_node)
  uint2* cinfo;           // [cell] {start, end}
  uint32_t* crel;         // [cell] cell code inside its node (build time, compacted)
  uint32_t* csnode;       // [cell] index of its node among the sampled nodes (compacted)
  uint32_t* gridmap;      // [sample node][cell code] -> cell (build time, compacted)
  uint32_t* qnbr;         // [cell][32]: adjacent cell in direction k = (dx+1)*9 + (dy+1)*3 + (dz+1), 13 = the cell itself
  uint4* rec;             // [cell][2][rg]: header {frontier, accepted, stamp, end} + the first rg-1 accepted points
  float4* ovf;            // accepted point j >= rg-1 of the cell ending at `end`: ovf[end - 1 - (j - (rg-1))]
  unsigned long long* slot;  // [cell][32]: {round written << 32 | point waited for} of the sleeper in direction k
  uint4* qst;             // [cell]: {stalled candidate or NONE, blocker direction, point waited for, round of the stall}
  uint32_t* queue[2];     // [nseg][segcap]: the round's cells, in nseg segments so that no single counter takes every push
  uint32_t* qctr;         // [3 rotating rounds][nseg] segment fill counters, one per 128-byte line
  uint32_t* qtotal;       // [3]: entries the round started with (what the host polls: 0 = the level is done)
  uint32_t* qhead;        // [3 rotating rounds][nseg] tickets: the next entry of the segment nobody has taken yet
  uint32_t nseg, nseg_shift, segcap;
  const uint32_t* snode_of;
  uint32_t cell_shift;    // key >> cell_shift = node prefix + cell code
  uint64_t cells_per_node;
  uint32_t cell_bits;     // cell_shift / 3: a cell is 2^cell_bits key cells wide
  uint32_t cell_levels;   // octree levels between node and cell
  uint32_t rg, rg2_shift; // granules per record buffer (4 or 8); log2(2 * rg)
  float f_lo, f_hi;
  double sq_spacing;
  uint32_t patient;
  float lazy_frac;
  uint32_t all_sampled;
  uint32_t group, groups;
  uint32_t no_dead_test;  // debugging / tests: blocker scans do not test for dead points
  uint32_t stats;         // SWZ_DEBUG: count activations by kind in counters[CTR_DBG_HIST ...]
  uint32_t chain;         // cells a wavefront may run one after the other in a launch, each woken by the one before (1: none)
  // dense cells (thousands of points: the blobs and sheets of a clustered cloud), levels of large cells only -- see
  // mq_dense_reject_kernel
  uint32_t dense_min;     // a cell with at least this many points is dense (0: the level has none / the feature is off)
  uint8_t* dirty;         // [cell] set when the cell or an adjacent one has published accepted points since its last reject pass
  uint32_t* bulk_round;   // [cell] round of the cell's last reject pass + 1
  const uint32_t* dlist;  // the dense cells
  uint32_t* round_word;   // sharded root: the round this shard's sweep is in, for the shards that read its records
  MqPeers peers;
  // build time, a level inside a chain of levels on one active set (ActiveSet::gone): a non-zero byte is a point taken
  // further up -- it starts QS_DEAD: never accepted, rejects nobody, keeps nobody waiting --, and qpos already holds the
  // key coordinates of these very keys
  const uint8_t* gone;
  uint32_t keep_qpos;
};

constexpr uint32_t MQ_CHAIN = 8;
// Records staged per activation.  A cell has at most 19 adjacent cells before it in Morton order: the order of a cell and its
// neighbour is decided by the axis whose coordinate changes at the highest bit, a step of -1 changes a higher bit than a step of
// +1 only along axes where the coordinate is even, so the worst case is the cell with three even coordinates, where every offset
// with a -1 in it (27 - 8) leads to an earlier cell.  Plus the cell itself.  Records of other shards are staged whatever their
// place in the order: all 27 there.
__host__ __device__ constexpr uint32_t mq_staged(bool peers) { return peers ? 27u : 20u; }
static inline size_t mq_lds_bytes(uint32_t rg, bool peers) {
  return (size_t)(mq_staged(peers) * 2u * rg + MQ_LIST_CAP + MQ_FRESH_CAP) * 16u + MQ_LIST_CAP + MQ_CHAIN * 4u + 128u;
}

// ---- one level on the host -----------------------------------------------------------------------------------------
// What the steps of min_distance_keys_level (swz_mdkeys.hip) hand to each other.  A parameter list with a name, like
// MdLevel.  Every step returns a status; a step that finds nothing (more) to do sets `over`.
struct MqLevel {
  const MdLevel& L;
  int cl;                          // cell levels below the node
  const MdShardRoot* shard_root;
  bool* used;                      // the caller's: the level is taken by this sweep
  bool sharded = false;            // the joint root of a sharded batch
  std::string sfx;                 // ... whose arrays ("_sr") are read by other shards until the batch ends
  MqArgs a{};                      // the level's arguments; the node groups' copies add their queues
  uint64_t grid_entries = 0;       // sample nodes * cells per node
  uint32_t ncells = 0;             // entries of the per-cell arrays
  uint32_t occ_cells = 0;          // occupied cells, for the scheduling rules: counted, or the caller's estimate
  uint32_t* d_cell_sums = nullptr; // compacted numbering: the count's block sums, for the build
  int set = 0;                     // which set of per-cell buffers the level runs on ("" / "_b"; 1 only after a build ahead)
  bool prebuilt = false;           // the early tables were built under the level before (mq_prebuild_launch): only the late ones are due
  bool coded = false;              // the taken bytes carry a code: see mq_commit_kernel
  bool lazy = false, big_cells = false;
  uint32_t groups = 1, ndense = 0;
  std::vector<MqArgs> ga;          // per node group
  std::vector<hipStream_t> gs;
  uint32_t round = MQ_FIRST_ROUND;
  bool over = false;               // the level ends here, without an error
};

// swz_mqbuild.hip: the level's tables
int mq_count_cells(swz_ctx* c, MqLevel& q);
int mq_alloc_arrays(swz_ctx* c, MqLevel& q);
int mq_build_cell_tables(swz_ctx* c, MqLevel& q);
int mq_list_dense_cells(swz_ctx* c, MqLevel& q);
int mq_start_groups(swz_ctx* c, MqLevel& q);
// ... and the early tables of the level after this one (swz_internal.h, MqPrebuild): launched on the build stream once this
// level's own tables are on their way, joined -- the context's stream waits for them -- behind this level's rounds
int mq_prebuild_launch(swz_ctx* c, MqLevel& q);
int mq_prebuild_join(swz_ctx* c);
// swz_mqsweep.hip: the rounds and what follows them
uint32_t mq_sweep_grid(swz_ctx* c, const MqLevel& q);
void mq_launch_round(const MqLevel& q, uint32_t g, uint32_t sweep_grid);
void mq_set_round_word(hipStream_t stream, uint32_t* word, uint32_t value);
int mq_verify(swz_ctx* c, MqLevel& q);
int mq_commit(swz_ctx* c, MqLevel& q);

}  // namespace swz
