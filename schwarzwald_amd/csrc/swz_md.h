// swz_md.h -- MIN_DISTANCE: what the dispatcher (swz_md.hip) finds out about a level, and the algorithms it hands the
// level to.  Which algorithm samples a level, with which cells, is decided in min_distance_level (swz_md.hip) and nowhere
// else: no algorithm calls another.
#pragma once
#include "swz_level.h"

namespace swz {

// ---- the MIN_DISTANCE root of a batch sharded over several GPUs of ONE process (swz_group)
// Every shard sweeps the root cells of its own octants at the same time.  Cells only depend on EARLIER adjacent cells,
// i.e. on cells of the same or of a lower shard: a cell at the face of a lower octant reads the records, key coordinates
// and state bytes of that shard's adjacent cells through peer access (the halo), as far as that shard's completed rounds
// have published them, and polls when it has to wait.  Nothing else is exchanged and no shard waits for another's whole
// root.  What a shard publishes about its root level:
struct MdPeerView {
  const uint4* rec = nullptr;        // cell records, [cell][2][rg]
  const uint64_t* qpos = nullptr;    // key coordinates of its active points
  const uint8_t* state = nullptr;
  const float4* ovf = nullptr;
  const uint32_t* gridmap = nullptr; // [cell code of the root node] -> cell
  const uint32_t* round_word = nullptr;  // the round its sweep is in: records stamped with an earlier round are complete
  const uint32_t* perm = nullptr;    // exact positions of its points: xyz[3 * perm[aidx ? aidx[i] : i]]
  const double* xyz = nullptr;
  const uint32_t* aidx = nullptr;    // null: the active points are the sorted points (the root of a single batch); a tiler's root
                                     // level -- batch + cached root file, merged -- has an index into its working arrays
  uint32_t ncells = 0, rg = 0, cell_shift = 0;
  uint32_t npoints = 0;              // points of its root level (the readers size their round limit by the lower shards' work too)
  int status = 0;                    // SWZ_OK, or why this shard cannot take part
  int entered = 0;                   // the shard's sweep has met the others at the barrier (else its driver does so for it)
};
struct MdShardRoot {
  int shard = 0, shards = 1;
  MdPeerView* views = nullptr;       // [shards], shared by the group's shards
  void (*barrier)(void*) = nullptr;  // all shards of the group meet
  void* barrier_arg = nullptr;
};

// ---- MIN_DISTANCE on key coordinates (swz_mdkeys.hip; tables: swz_mqbuild.hip, rounds: swz_mqsweep.hip) --------
// The key of a point is its position quantised to 2^-21 of the (cubic) bounds: the integer coordinates of two points
// bound their distance to +-sqrt(3) key cells, so a compare against the spacing is decided on the keys alone unless the
// integer distance lies within that band around it; those pairs -- a few in ten thousand at the root, a few per cent of
// the near pairs at level 3 -- are evaluated on the exact positions with the reference's arithmetic.  The result is
// therefore the exact one.  KeyMetric holds the thresholds in key cells.
struct KeyMetric {
  bool ok = false;     // the level can be decided on keys (cubic bounds, spacing of at least key_min_cells key cells)
  double T = 0.0;      // spacing in key cells
  float f_lo = 0.f;    // float squared integer distance <  f_lo: closer than the spacing for sure
  float f_hi = 0.f;    //                                >= f_hi: at least the spacing apart for sure
};
KeyMetric key_metric(const swz_ctx* c, const LevelPlan& plan, const SortedPoints& sp);
// The caller's index of every active point: perm[aidx[i]] in one array (a streaming pass: aidx ascends), so that the exact
// compare of a pair costs two dependent loads per point instead of three.  At the root this is perm itself.
int key_point_ids(swz_ctx* c, const ActiveSet& as, const SortedPoints& sp, const uint32_t** ids);
// true when min_distance_level will not need sp.X / sp.Y / sp.Z for this level
bool min_distance_level_uses_keys(const swz_ctx* c, const LevelPlan& plan, const SortedPoints& sp);
// no sampler of this level reads sp.X / Y / Z: RANDOM_GRID never does, the others decide on key coordinates and look up
// sp.xyz through sp.perm (swz_mqsweep.hip, grid_argmin_keys_kernel)
bool level_decides_on_keys(const swz_ctx* c, const LevelPlan& plan, const SortedPoints& sp);
// ---- one level as every algorithm sees it ------------------------------------------------------------------------
// Filled by the dispatcher's survey of the level.  A parameter list with a name, not an interface.
struct MdLevel {
  const LevelPlan& plan;
  const ActiveSet& as;
  const SortedPoints& sp;
  const LevelBuffers& lb;
  uint32_t num_nodes, sample_nodes, sample_points;
  bool all_sampled;           // every node of the level is sampled (the usual case)
  const uint32_t* snode_of = nullptr;   // node -> index among the sampled nodes (device, "md_snode")
  KeyMetric km;
  // occupied cells at every candidate cell level, from every skip-th tile of 256 points (skip = max(1, m >> 23): the
  // counts only steer the choice of cell size and algorithm; on large levels a sample of some million points says the
  // same as all of them and saves a pass over the keys).  sampled_hist: skip > 1, the counts are scaled estimates.
  uint32_t occupied[12] = {0};
  bool sampled_hist = false;
  // points-weighted mean cell population at cell level cl_geo, cl_geo - 1, - 2, - 3 (md_populations; exact mode has
  // them from the survey, property mode when a cell-size rule first asks)
  double pop[4] = {0, 0, 0, 0};
  bool have_pop = false;
};
// the dense [node][cell] tables of all algorithms: at most 2^31 entries (8.6 GB; memset once per level, a few ms)
int md_clamp_cell_levels(uint32_t sample_nodes, int cl);
// occupied[] once more from ALL points (for who sizes arrays by the counts)
int md_count_cells_exact(swz_ctx* c, const MdLevel& L, uint32_t occupied[12]);
// Positions of the active points in active order.  Below the root the survivors are a subsequence: gathered into
// "md_pos", x[], y[], z[] of m doubles each in a buffer of per_point doubles per point; at the root sp.X / Y / Z.
int md_active_positions(swz_ctx* c, const MdLevel& L, size_t per_point, const double** X, const double** Y, const double** Z);

// ---- the algorithms, in the order the dispatcher offers a level to them ------------------------------------------
// Frontier sweep on key coordinates for a dense level (swz_mdkeys.hip); *used = false when the level does not qualify.
// cl: cell levels below the node.  The points-weighted mean cell population at cl and the estimate of the occupied cells
// at cl (it decides how the cells are numbered) come from the survey.
// *direct (may be null): the cells were numbered by their place in the grid.  A level inside a chain (L.as.gone) is taken
// with direct numbering or not at all.
int min_distance_keys_level(swz_ctx* c, const MdLevel& L, int cl, uint32_t* rounds_out, bool* used,
                            const MdShardRoot* shard_root = nullptr, bool* direct = nullptr);
// granules per record buffer (4 or 8) for cells of 2^cell_bits key cells at a spacing of T key cells
uint32_t key_sweep_record_granules(const swz_ctx* c, uint32_t cell_bits, double T);
// The grid the key sweep would most likely be given for the level of `plan` if about `points` points, spread evenly,
// reached it inside a chain: the ladder's rules of min_distance_level (swz_md.hip) on an estimate instead of a survey.
// false: the level would probably go elsewhere (take-all nodes, a sparse level, no key metric, compacted cells).  Only
// a guess -- it decides what mq_prebuild_launch builds ahead, never what the level does.
bool md_guess_chained_level(const swz_ctx* c, const LevelPlan& plan, const SortedPoints& sp, uint32_t points, MqPrebuild* want);
// Sparse levels by blocks of 8^3 cells staged in LDS, blocks in Morton order, decisions in the same launch
// (swz_mdblock.hip); *done = false: the level does not qualify or a block did not fit, nothing is lost.
int min_distance_block_level(swz_ctx* c, const MdLevel& L, bool* done);
// Sparse levels, one thread per point (swz_mdsparse.hip), cells at level cl; *used = false: it gave up half way
// (locally dense data) -- every decision taken so far is exact.
int min_distance_sparse_level(swz_ctx* c, const MdLevel& L, int cl, uint32_t* rounds_out, bool* used);
// Property mode on key coordinates in data-parallel rounds (swz_mdrounds.hip): candidates per cell, winners by a hashed
// priority, a kill pass; *used = false when the level does not qualify (then nothing has been decided).
int min_distance_rounds_level(swz_ctx* c, const MdLevel& L, uint32_t* rounds_out, bool* used);
// Frontier sweep on positions in Morton order (swz_mindist.hip), cells at level cl.
int min_distance_sweep_level(swz_ctx* c, const MdLevel& L, int cl, uint32_t* rounds_out);
// Property mode on positions: eight coloured cell phases (swz_mdprop.hip), cells at level cl.
int min_distance_phases_level(swz_ctx* c, const MdLevel& L, int cl, uint32_t* phases_out);

}  // namespace swz
