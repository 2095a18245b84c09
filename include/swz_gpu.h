/*
 * swz_gpu.h -- C ABI of the MI355X-native Schwarzwald tiler hot path (libswz_gpu.so).
 *
 * The reference (igd-geo/schwarzwald, paths below relative to schwarzwald/) has no plugin
 * loader or C ABI for this path; its "plugin surface" is three compile-time C++ seams
 * (SURVEY.md section 8(b)).  This header is the C-ABI boundary a maintainer binds behind
 * those seams (INTEGRATION.md shows the adapter).  Conventions follow the only C ABI the
 * reference itself consumes (LASzip, core/io/LASFile.cpp:14-75): every call returns an int
 * status, 0 = OK, and the message of the last failure is read with swz_last_error().
 *
 * Ownership: the library owns all device workspace inside swz_ctx.  "host" entry points take
 * caller-owned host buffers (what PointBuffer::positions().data() hands over,
 * core/datastructures/PointBuffer.h:291-304); "_device" entry points take device pointers
 * (hipMalloc'd or a torch tensor's data_ptr()) and run on the context's stream.
 * Threading: one call in flight per context; independent contexts (one per GPU) may run
 * concurrently.  Nothing here throws; the adapter turns a non-zero status into
 * std::runtime_error like the rest of the tiler does (executable/main.cpp:599-602).
 * There is NO CPU fallback: without a usable HIP device swz_create() fails.
 */
#ifndef SWZ_GPU_H
#define SWZ_GPU_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SWZ_ABI_VERSION 3

/* status codes */
enum {
  SWZ_OK = 0,
  SWZ_ERR_HIP = 1,                   /* a HIP runtime call failed (message has the HIP error) */
  SWZ_ERR_BAD_ARG = 2,
  SWZ_ERR_JITTER_GRID_TOO_SMALL = 3, /* JitteredSampling throws: Sampling.h:632-635 */
  SWZ_ERR_JITTER_NODE_TOO_DEEP = 4,  /* JitteredSampling throws: Sampling.h:642-653 */
  SWZ_ERR_REROOT_UNSUPPORTED = 5,    /* node needs Morton re-rooting, TilingAlgorithms.cpp:444-483 */
  SWZ_ERR_TOO_MANY_POINTS = 6,       /* more than 2^32-65536 points in one batch */
  SWZ_ERR_INTERNAL = 7,
  SWZ_ERR_TILER_FAILED = 8           /* swz_tiler: an earlier batch failed part-way; the node store is incomplete */
};

/* --sampling values, TilerProcess::make_sampling_strategy (core/process/TilerProcess.cpp:491-516)
 * -> Sampling.h:187-308 / :314-416 / :421-471 / :598-759 / :477-542.
 * MIN_DISTANCE_FAST is AdaptivePoissonDiskSampling with the densities of the command line (TilerProcess.cpp:500-508): a
 * sampled node offers only every n-th point of its Morton-ordered range, counted from its own first point, to MIN_DISTANCE's
 * greedy test (n = swz_min_distance_fast_stride); the others are passed down unexamined.  A node whose candidate level is -1
 * keeps its first point only.  Not with SWZ_FLAG_MIN_DISTANCE_PROPERTY and not on the sharded entry points (swz_shard_*,
 * swz_tiler_shard_*, swz_group_*): both return SWZ_ERR_BAD_ARG. */
enum { SWZ_RANDOM_GRID = 0, SWZ_GRID_CENTER = 1, SWZ_MIN_DISTANCE = 2, SWZ_JITTERED = 3, SWZ_MIN_DISTANCE_FAST = 4 };
/* The n of MIN_DISTANCE_FAST at a node level (relative to the root, -1 = the root): (uint32_t)std::round(1 / density) with
 * density 0.25f below level 0, 0.5f below level 1, else 1.f -- 4, 2, 1.  Host arithmetic only; the one place that decides n. */
int32_t swz_min_distance_fast_stride(int32_t node_level);
/* SamplingBehaviour, Sampling.h:170-181 */
enum { SWZ_TAKE_ALL_WHEN_COUNT_BELOW_MAX_POINTS = 0, SWZ_ALWAYS_ADHERE_TO_MIN_SPACING = 1 };
/* --tiling-strategy values, executable/main.cpp:484-497 -> TilingAlgorithmV1 / V3 */
enum { SWZ_ACCURATE = 0, SWZ_FAST = 1 };

typedef struct swz_ctx swz_ctx;

/* Creates a context on HIP device `device` (ordinal).  Fails with SWZ_ERR_HIP when no device. */
int swz_create(swz_ctx** ctx_out, int device);
int swz_destroy(swz_ctx* ctx);
const char* swz_last_error(const swz_ctx* ctx); /* ctx may be NULL: returns the create() error */
int swz_abi_version(void);
/* A context launches on its OWN non-blocking stream: device buffers handed to the *_device entry points must be
 * complete before the call (synchronise, or wait on an event), and the entry points return after their own work
 * finished (they synchronise that stream).  swz_set_stream makes the context run on an existing hipStream_t
 * instead (e.g. torch's current stream), which orders it with the caller's kernels on that stream.  NULL is the
 * device's default stream (a real stream: PyTorch's default); SWZ_OWN_STREAM restores the own stream. */
#define SWZ_OWN_STREAM ((void*)(intptr_t)-1)
int swz_set_stream(swz_ctx* ctx, void* hip_stream);
/* Debug / tuning switches.  A context reads the SWZ_* variables of the environment once, when it is
 * created; afterwards they change only through this call (value NULL removes the switch).  Every name is accepted; one the
 * library does not read has no effect.  Production code needs none of them.  The library reads these:
 * - Diagnostics: SWZ_DEBUG (per-level lines on stderr), SWZ_TRACE (synchronise and report after every stage),
 *   SWZ_SYNC_ENTRY (synchronise the device when swz_tile_device starts), SWZ_MD_STATS (count the key sweep's activations by
 *   kind), SWZ_POISON=<byte> and SWZ_POISON_ONLY=<part of a buffer name> (fill new workspace memory),
 *   SWZ_BIN_WRITER_THREADS (host threads that write node files), SWZ_INPUT_READER_THREADS (host threads that read the
 *   LAS files of swz_tiler_add_las_files and the node files of swz_convert_dataset).
 * - Switches that only force a path, a schedule or a capacity -- the samplers' results stay what they are:
 *   sort: SWZ_SORT_ONESWEEP=0, SWZ_SORT_HYBRID_MIN_N, SWZ_SORT_HYBRID_TOP, SWZ_SORT_FIX_SHORT, SWZ_SORT_FIX_LONG,
 *   SWZ_SORT_WIDE_MIN_N (keys from which a scatter pass takes its 8192-key tile);
 *   GRID_CENTER / JITTERED: SWZ_GRID_KEYS=0, SWZ_GRID_KEYS_SLACK >= 0 (a large one sends every run of more than one point
 *   through the exact pass), SWZ_GRID_TABLE_DEPTH, SWZ_JITTER_TABLE=0, SWZ_LEVEL_NODES_SCAN;
 *   MIN_DISTANCE, the path of a level: SWZ_MD_SPARSE_LIMIT, SWZ_MD_KEYS=0, SWZ_MD_KEYS_MIN_CELLS, SWZ_MD_KEYS_BAND >= 0 (a
 *   wider band sends more pairs to the compare on the exact positions), SWZ_SP_FILTER_EPS (1e30: every compare within reach
 *   exact), SWZ_GROUP_JOINT_ROOT=0; how the key sweep numbers its cells: SWZ_MD_DIRECT (1: by their place in the grid
 *   whatever the occupancy, 0: always the occupied cells compacted), SWZ_MD_DIRECT_MIN_OCCUPANCY (0.5: the estimated share of
 *   occupied grid cells from which a level is numbered directly), SWZ_MD_DIRECT_MAX_CELLS (the largest grid that is numbered
 *   directly; default: what fits the free device memory); chains of dense levels that share one active set:
 *   SWZ_MD_DEFER=0 (every level compacts its survivors, as the other paths do), SWZ_MD_DEFER_MAX_GONE (1/8: the share of
 *   taken points in the shared arrays from which a chain ends), SWZ_MD_PREBUILD=0 (no level of a chain builds the next
 *   level's cell tables ahead, under its own rounds: every level builds all of its tables itself);
 *   the frontier sweeps: SWZ_MD_PATIENT, SWZ_MD_LAZY, SWZ_MD_LAZY_FRAC, SWZ_MD_BIG, SWZ_MD_GROUPS, SWZ_MD_GRID,
 *   SWZ_MD_NBR_GRID, SWZ_MD_BATCH, SWZ_MD_COARSEN, SWZ_MD_COARSEN_MIN, SWZ_MD_FF_MIN, SWZ_MD_NO_DEAD_TEST=1 (blocker scans
 *   without the dead-point test), SWZ_MD_CHAIN, SWZ_MD_KEYS_RG, SWZ_MD_DENSE_MIN;
 *   the blocks of cells (swz_mdblock.hip): SWZ_SP_BLOCK=0 (the thread-per-point path instead), SWZ_SP_BLOCK_WIDE=1,
 *   SWZ_SP_BLOCK_CL, SWZ_SP_BLOCK_OWN, SWZ_SP_BLOCK_HALO, SWZ_SP_BLOCK_PER_CU, SWZ_SP_BLOCK_MIN (point format, cell level,
 *   LDS capacities, workgroups per CU, points a block should hold), SWZ_SP_BLOCK_CAP_SCALE (scales the estimated capacities:
 *   a block that does not fit stops the launch, which is repeated with larger capacities or finer cells; with forced
 *   capacities the level falls back), SWZ_SP_INCREMENTAL (multi-batch tilers: a batch merged with node files samples only
 *   what its points can change; = 0 never, = a share in (0, 1]: whenever the files are that much of a level; default: half
 *   of it, and files of max_points/2 per node on average), SWZ_SP_INCREMENTAL_MAX (0.35: the largest share of a level that
 *   is still sampled as a subset);
 *   property mode (SWZ_FLAG_MIN_DISTANCE_PROPERTY): SWZ_MD_ROUNDS=0, SWZ_MD_ROUNDS_LIST=0, SWZ_MD_ROUNDS_CELL_LISTS=0,
 *   SWZ_MD_ROUNDS_BLOCK=0, SWZ_MD_ROUNDS_BLOCK_MIN_POP, SWZ_MD_ROUNDS_WLIST_MIN_POP -- the set keeps the mode's properties
 *   on every path; which set it is may depend on the path a level takes;
 *   the tiler's memory: SWZ_TILER_SPILL=off|host, SWZ_TILER_DEVICE_BUDGET_MB; SWZ_OUTPUT_CHUNK_POINTS (stored points per
 *   chunk of swz_tiler_write_output when its parameters say 0; default 16 Mi).
 * - Switches that can make a call FAIL: SWZ_MD_TIME_LIMIT and SWZ_MD_ROUND_LIMIT (a MIN_DISTANCE level that exceeds them is
 *   abandoned with an error), SWZ_SP_BLOCK_TIMEOUT_MS (default 10 000: how long a wavefront waits for an earlier block;
 *   when it expires the call returns SWZ_ERR_INTERNAL, nothing is restarted), SWZ_FAIL_ALLOC=<buffer name, or prefix*>
 *   (every first attempt to allocate that buffer reports out of memory: tests of the paths that recover).
 * - Values that change a RESULT on purpose, so that a test can show that a bound is needed: a negative SWZ_MD_KEYS_BAND
 *   (narrows the band in which MIN_DISTANCE repeats a compare on the exact positions below its proven width,
 *   tests/test_min_distance_keys.py) and a negative SWZ_GRID_KEYS_SLACK (the same for the grid samplers on keys,
 *   tests/test_grid_keys.py). */
int swz_set_option(swz_ctx* ctx, const char* name, const char* value);
/* Frees all device workspace held by the context (it regrows on demand). */
int swz_release_workspace(swz_ctx* ctx);
/* Bytes of device workspace currently held. */
uint64_t swz_workspace_bytes(const swz_ctx* ctx);

/* ---- index_points<21>(..., ClampToBounds): core/tiling/OctreeAlgorithms.h:145-197 with
 * calculate_morton_index<21> :64-87.  xyz is N x 3 doubles (AoS).  Outliers are clamped to the
 * bounds IN PLACE (index_point mutates the PointBuffer, :167-169), so xyz is read-write.
 * keys_out[i] is the 63-bit MortonIndex64 of point i.
 * Bounds (here and in every call that takes a root box): finite, max > min on every axis, and 2^21 / (max - min)
 * finite and positive -- else SWZ_ERR_BAD_ARG before anything is launched.  (An extent below about 1.2e-302, one
 * that overflows, or an infinite face makes the scale inf or 0 and the products NaN or inf, whose conversion to a
 * cell index differs between x86-64 and the GPU.) */
int swz_morton_encode(swz_ctx* ctx, double* xyz, uint64_t n, const double bounds_min[3],
                      const double bounds_max[3], uint64_t* keys_out);
int swz_morton_encode_device(swz_ctx* ctx, double* d_xyz, uint64_t n, const double bounds_min[3],
                             const double bounds_max[3], uint64_t* d_keys_out);

/* ---- Range::sort of IndexedPoint64 by key: util/containers/Range.h:62-66, operator<
 * core/tiling/Sampling.h:159-164.  std::sort leaves the order of equal keys unspecified; this
 * sort is stable: perm_out lists original indices ordered by (key, original index).
 * keys_sorted_out may be NULL. */
int swz_sort_by_key(swz_ctx* ctx, const uint64_t* keys, uint64_t n, uint32_t* perm_out,
                    uint64_t* keys_sorted_out);
int swz_sort_by_key_device(swz_ctx* ctx, const uint64_t* d_keys, uint64_t n, uint32_t* d_perm_out,
                           uint64_t* d_keys_sorted_out);

/* ---- sample_points(strategy, begin, end, node_key, node_level, root_bounds, spacing_at_root,
 * behaviour): core/tiling/Sampling.h:799-821.  keys/idx describe a Morton-sorted range of n
 * IndexedPoint64 (idx[i] = row of xyz).  taken_out[i] = 1 when element i belongs to the
 * [begin, partition_point) half of the reference's stable partition, else 0 (both halves keep
 * their order, so the partition itself is a stable compaction by this flag).
 * RANDOM_GRID and GRID_CENTER ignore node_key like the reference does (the range is the node).  For MIN_DISTANCE
 * and JITTERED, which take the node's box from node_key (Sampling.h:441, 622), every key of the range must have
 * node_key's first node_level + 1 octants (checked on the device, SWZ_ERR_BAD_ARG otherwise). */
int swz_sample_points(swz_ctx* ctx, int sampler, uint64_t max_points_per_node, const uint64_t* keys,
                      const uint32_t* idx, uint64_t n, const double* xyz, uint64_t num_points,
                      uint64_t node_key, int32_t node_level, const double root_min[3],
                      const double root_max[3], float spacing_at_root, int behaviour,
                      uint8_t* taken_out, uint64_t* num_taken_out);
/* The same on device buffers (d_xyz: num_points x 3); the flags stay on the device. */
int swz_sample_points_device(swz_ctx* ctx, int sampler, uint64_t max_points_per_node, const uint64_t* d_keys,
                             const uint32_t* d_idx, uint64_t n, const double* d_xyz, uint64_t num_points,
                             uint64_t node_key, int32_t node_level, const double root_min[3],
                             const double root_max[3], float spacing_at_root, int behaviour,
                             uint8_t* d_taken_out, uint64_t* num_taken_out);

/* required_morton_index_depth (core/tiling/Sampling.cpp:29-62 with get_node_level_to_sample_from /
 * first_node_level_obeying_spacing, core/tiling/Node.cpp:37-57): the depth of key bits a sampler needs at a node of
 * level node_level -- what tile_node's terminal / re-root tests use (TilingAlgorithms.cpp:408-444).  Host function,
 * evaluated with the host's libm exactly like the reference (std::log2f of the ratio narrowed to float). */
int32_t swz_required_morton_index_depth(int sampler, int32_t node_level, const double root_min[3],
                                        const double root_max[3], float spacing_at_root);

/* ---- one batch through the tiling algorithm: TilingAlgorithmBase::build_execution_graph
 * (core/tiling/TilingAlgorithms.h:81-85), V1 = ACCURATE (TilingAlgorithms.cpp:577-626),
 * V3 = FAST first iteration + finalize (:1250-1360, :1661-1784). */
typedef struct {
  int32_t sampler;              /* SWZ_RANDOM_GRID ... */
  uint64_t max_points_per_node; /* TilerMetaParameters::max_points_per_node (Tiler.h:64-75) */
  float spacing_at_root;        /* TilerMetaParameters::spacing_at_root */
  uint32_t max_depth;           /* TilerMetaParameters::max_depth (<=0 means 100 upstream) */
  int32_t strategy;             /* SWZ_ACCURATE | SWZ_FAST */
  uint32_t fast_concurrency;    /* FAST: num_indexing_threads, decides the start level
                                   (TilingAlgorithms.cpp:1473-1535) */
  uint32_t flags;               /* SWZ_FLAG_*; 0 = the reference's semantics everywhere */
} swz_tile_params;
/* MIN_DISTANCE "property" mode (not the reference's result): the taken set of every sampled
 * node is still a maximal set of points pairwise >= the node's spacing apart under the reference's compare
 * (squared double distance against the float-squared spacing, GridCell.cpp:52) and deterministic, but the greedy
 * priority is (cell colour, Morton order) instead of Morton order alone: the node is cut into octree cells >= one
 * spacing wide, cells of equal colour (parity of the cell coordinates) are never adjacent and are decided together,
 * eight phases per level instead of thousands of dependent rounds.  Take-all, terminal and all other rules are
 * unchanged.  What the reference's author tests for this sampler (test/TestTiler.cpp:361-421: min distance on
 * sampled nodes) holds; point-for-point equality with the reference does not. */
#define SWZ_FLAG_MIN_DISTANCE_PROPERTY 1u

typedef struct {
  uint64_t num_nodes;         /* nodes that persisted points (incl. FAST reconstructed ones) */
  uint64_t points_visited;    /* sum over levels of the points handed to sample_points/terminal */
  int32_t max_level;          /* deepest node level that took points (-1 = root) */
  int32_t fast_start_levels;  /* FAST: _level_of_start_nodes, else -1 */
  uint32_t num_levels;        /* level iterations executed */
  uint32_t min_distance_rounds; /* MIN_DISTANCE: dependency rounds executed, all levels */
} swz_tile_stats;

/* Outputs are in Morton-sorted order: keys_out[i] ascending (ties by original index),
 * perm_out[i] = original point index, level_out[i] = level of the octree node that persists the
 * point (-1 = root "r"); the node is the first level_out[i]+1 octants of keys_out[i]
 * (node name "r" + digits, TilingAlgorithms.cpp:139).  dup_mask_out (may be NULL; FAST only)
 * has bit (l+1) set when the point is additionally stored in the reconstructed node at level l.
 * xyz is clamped in place like index_point does. */
int swz_tile(swz_ctx* ctx, double* xyz, uint64_t n, const double bounds_min[3],
             const double bounds_max[3], const swz_tile_params* params, uint64_t* keys_out,
             uint32_t* perm_out, int8_t* level_out, uint32_t* dup_mask_out, swz_tile_stats* stats);
int swz_tile_device(swz_ctx* ctx, double* d_xyz, uint64_t n, const double bounds_min[3],
                    const double bounds_max[3], const swz_tile_params* params, uint64_t* d_keys_out,
                    uint32_t* d_perm_out, int8_t* d_level_out, uint32_t* d_dup_mask_out,
                    swz_tile_stats* stats);

/* ---- what PointsPersistence::persist_points needs (core/io/PointsPersistence.h:23-31): the
 * points of every node, contiguous and in Morton order.  From swz_tile's outputs builds
 * order_out[n] (sorted positions grouped by node; nodes ordered by (level, key prefix)) and the
 * node table.  node_* arrays must hold max_nodes entries; *num_nodes_out is the count found
 * (SWZ_ERR_BAD_ARG when it exceeds max_nodes).  Host buffers. */
int swz_build_node_lists(swz_ctx* ctx, const uint64_t* keys_sorted, const int8_t* level, uint64_t n,
                         uint32_t* order_out, uint64_t max_nodes, int8_t* node_level_out,
                         uint64_t* node_key_out, uint64_t* node_offset_out, uint64_t* node_count_out,
                         uint64_t* num_nodes_out);

/* Same on the device: d_keys_sorted / d_level are swz_tile_device's outputs, d_order_out[n] is device
 * memory; the node table (at most max_nodes entries) is written to the host arrays. */
int swz_build_node_lists_device(swz_ctx* ctx, const uint64_t* d_keys_sorted, const int8_t* d_level, uint64_t n,
                                uint32_t* d_order_out, uint64_t max_nodes, int8_t* node_level_out,
                                uint64_t* node_key_out, uint64_t* node_offset_out, uint64_t* node_count_out,
                                uint64_t* num_nodes_out);

/* ---- node payload: what a lossless PointsPersistence stores for a node.
 * The attribute columns of a point batch, SoA like PointBuffer (core/datastructures/PointBuffer.h:109-121,
 * 292-304); a NULL column is absent.  Indices double as bit numbers of BinaryPersistence's properties
 * bitmask (core/io/BinaryPersistence.h:24-35) and give the order of the arrays in a node file. */
enum {
  SWZ_ATTR_RGB = 0,                 /* 3 x uint8  */
  SWZ_ATTR_NORMAL = 1,              /* 3 x float  */
  SWZ_ATTR_INTENSITY = 2,           /* uint16     */
  SWZ_ATTR_CLASSIFICATION = 3,      /* uint8      */
  SWZ_ATTR_EDGE_OF_FLIGHT_LINE = 4, /* uint8      */
  SWZ_ATTR_GPS_TIME = 5,            /* double     */
  SWZ_ATTR_NUMBER_OF_RETURNS = 6,   /* uint8      */
  SWZ_ATTR_RETURN_NUMBER = 7,       /* uint8      */
  SWZ_ATTR_POINT_SOURCE_ID = 8,     /* uint16     */
  SWZ_ATTR_SCAN_DIRECTION_FLAG = 9, /* uint8      */
  SWZ_ATTR_SCAN_ANGLE_RANK = 10,    /* int8       */
  SWZ_ATTR_USER_DATA = 11,          /* uint8      */
  SWZ_ATTR_COUNT = 12
};
typedef struct {
  void* column[SWZ_ATTR_COUNT];
} swz_attribute_columns;
/* bytes per point of attribute a (0 for an invalid index) */
uint32_t swz_attribute_row_bytes(int attribute);

/* Permuted gather into node order: row i of every output column = row d_perm[d_order[i]] of the input
 * column (positions N x 3 doubles plus every attribute present in BOTH column sets).  d_perm and d_order
 * are swz_tile_device's perm and swz_build_node_lists_device's order.  After this the points of node k
 * are rows [node_offset[k], node_offset[k] + node_count[k]) of every column, in Morton order -- exactly
 * the iterator range tile_node hands to persist_points (TilingAlgorithms.cpp:232-236, 316-322). */
int swz_gather_payload_device(swz_ctx* ctx, const uint32_t* d_perm, const uint32_t* d_order, uint64_t n,
                              const double* d_xyz, const swz_attribute_columns* d_in, double* d_xyz_out,
                              const swz_attribute_columns* d_out);

/* BinaryPersistence node files (core/io/BinaryPersistence.h:45-193, BinaryPersistence.cpp:200-375):
 * uint32 properties bitmask, uint64 point count, positions (24 B each), then every present attribute
 * array in the order RGB, normal, intensity, classification, edge of flight line, GPS time, number of
 * returns, return number, point source id, scan angle rank, scan direction flag, user data (bit order
 * except that the reference writes bit 10 before bit 9); little-endian, no padding.  compressed != 0 wraps the same bytes in one zlib stream (level 1,
 * "<name>.binz"), else "<name>.bin".  Host functions, no GPU involved; ctx only carries the error text
 * and may be NULL.
 *   swz_bin_write_node: columns point at the node's first row.  count == 0 writes nothing (like
 *     persist_points).
 *   swz_bin_read_header / swz_bin_read_node: retrieve_points; read_node fills xyz_out (count x 3) and
 *     every non-NULL column whose bit is set in the file.
 *   swz_bin_persist_nodes: one file per node of a node table, named "r" + octant digits
 *     (TilingAlgorithms.cpp:139) in directory dir; xyz / columns are the gathered payload of the batch.  The files are
 *     written by several host threads (option SWZ_BIN_WRITER_THREADS; default: the host's, at most 32). */
int swz_bin_write_node(swz_ctx* ctx, const char* path, uint64_t count, const double* xyz,
                       const swz_attribute_columns* columns, int compressed);
int swz_bin_read_header(swz_ctx* ctx, const char* path, int compressed, uint32_t* bitmask_out, uint64_t* count_out);
int swz_bin_read_node(swz_ctx* ctx, const char* path, int compressed, double* xyz_out,
                      const swz_attribute_columns* columns_out);
int swz_bin_persist_nodes(swz_ctx* ctx, const char* dir, uint64_t num_nodes, const int8_t* node_level,
                          const uint64_t* node_key, const uint64_t* node_offset, const uint64_t* node_count,
                          const double* xyz, const swz_attribute_columns* columns, int compressed);
/* BIN node files packed on the device, like swz_pnts_pack_device and swz_las_pack_device below.  A node's BODY is its whole
 * uncompressed file: the 12 bytes of mask and count, count x 24 bytes of positions, the arrays of `mask` in file order, no
 * padding inside.  The IMAGE holds the bodies in table order; every body starts on a multiple of 8, the bytes up to the next
 * multiple of 8 are zeros and no part of the file.  A node of count 0 has no file and size 0.
 *   swz_bin_layout (host): offset and size (a multiple of 8) of every body in the image, the size of every file, the image's
 *     total size.  Any output may be NULL.  SWZ_ERR_BAD_ARG for a mask bit that does not exist or a count above 2^32 - 65536.
 *   swz_bin_pack_device: writes the image of a node table into d_image_out (device, 8-byte aligned, image_bytes >= the
 *     layout's total) with one kernel: the permuted gather (row i = row d_perm[d_order[i]] of d_xyz and of the columns of
 *     d_in; d_order NULL = identity, what a tiler's export ids need) and the layout, headers and padding included -- no byte
 *     of the image depends on what the buffer held.  node_offset / node_count (host) are rows of the gathered order.
 *     SWZ_ERR_BAD_ARG before anything is launched for: offsets that do not ascend, ranges that overlap or pass n, a mask that
 *     names an absent column or a bit that does not exist, n above 2^32 - 65536, an image that is too small or not 8-byte
 *     aligned.  n == 0 or no nodes is valid and launches nothing.  swz_bin_pack_tile: the stored rows one workgroup takes.
 *   swz_bin_persist_nodes_image: one file "r" + octant digits + ".bin" per node of a table out of a HOST copy of the image,
 *     a verbatim slice of it; compressed != 0: that slice as one zlib stream, level 1, ".binz", the way swz_bin_write_node
 *     compresses.  Written by the pool of host threads of swz_bin_persist_nodes. */
int swz_bin_layout(uint64_t num_nodes, const uint64_t* node_count, uint32_t mask, uint64_t* body_offset_out,
                   uint64_t* body_size_out, uint64_t* file_size_out, uint64_t* total_out);
uint32_t swz_bin_pack_tile(void);
int swz_bin_pack_device(swz_ctx* ctx, const uint32_t* d_perm, const uint32_t* d_order, uint64_t n, const double* d_xyz,
                        const swz_attribute_columns* d_in, uint64_t num_nodes, const uint64_t* node_offset,
                        const uint64_t* node_count, uint32_t mask, void* d_image_out, uint64_t image_bytes);
int swz_bin_persist_nodes_image(swz_ctx* ctx, const char* dir, uint64_t num_nodes, const int8_t* node_level,
                                const uint64_t* node_key, const uint64_t* node_count, const void* image, uint64_t image_bytes,
                                uint32_t mask, int compressed);
/* "r" + octant digits of a node; name_out must hold 23 bytes */
int swz_node_name(int8_t node_level, uint64_t node_key, char* name_out);

/* ---- hierarchy metadata of the node table; host functions.
 *   swz_node_name_entwine / swz_node_from_entwine_name: "D-X-Y-Z" (depth = number of octants, then the node's
 *     grid coordinates at that depth; OctreeNodeIndex::to_string_entwine / from_string, core/datastructures/
 *     OctreeNodeIndex.h:556-573, 480-540).  name_out must hold 72 bytes.
 *   swz_node_bounds: the node's box by descending from the root box octant by octant (get_octant_bounds,
 *     core/tiling/OctreeAlgorithms.cpp:3-18, the way Cesium3DTilesPersistence::on_write_node walks down,
 *     core/io/Cesium3DTilesPersistence.cpp:100-112).
 *   swz_node_geometric_error: spacing_at_root / 2^depth (Cesium3DTilesPersistence.cpp:91-92). */
int swz_node_name_entwine(int8_t node_level, uint64_t node_key, char* name_out);
int swz_node_from_entwine_name(const char* name, int8_t* node_level_out, uint64_t* node_key_out);
int swz_node_bounds(int8_t node_level, uint64_t node_key, const double root_min[3], const double root_max[3],
                    double min_out[3], double max_out[3]);
double swz_node_geometric_error(int8_t node_level, float spacing_at_root);

/* Tileset tree of a node table (Cesium3DTilesPersistence::on_write_node / write_tilesets, core/io/
 * Cesium3DTilesPersistence.cpp:80-156, 175-199): one entry per node of the table AND per ancestor the table does not
 * list, ordered by (level, Morton index) so that the children of an entry are contiguous, by octant.
 *   has_content: the node is in the table (it has a point file); is_tileset_root: a new tileset.json starts here
 *   (every third level); bounds are the node box translated by global_offset (NULL = none).
 * out == NULL only counts (*num_out). */
typedef struct {
  int8_t level;              /* -1 = root "r" */
  uint8_t has_content;
  uint8_t is_tileset_root;
  uint8_t tight;             /* swz_tileset_build_boxes: bounds are the points' box; written with HALF-axes */
  uint32_t num_children;
  uint64_t key;
  int64_t parent;            /* index into the output, -1 for the root */
  int64_t first_child;       /* -1 when there are none */
  double geometric_error;
  double bounds_min[3], bounds_max[3];
} swz_tileset_node;
int swz_tileset_build(uint64_t num_nodes, const int8_t* node_level, const uint64_t* node_key, const double root_min[3],
                      const double root_max[3], float spacing_at_root, const double global_offset[3], uint64_t max_out,
                      swz_tileset_node* out, uint64_t* num_out);
/* The same tree with the boxes of the POINTS instead of the octree cubes: node_box_min / node_box_max hold 3 doubles per
 * node of the table (what swz_node_boxes_device / swz_tiler_node_boxes return; a node without points has min = +inf, max =
 * -inf).  bounds of an entry = the union of its own box (if has_content) and the bounds of all its descendants -- 3D Tiles
 * requires a tile's volume to enclose its children's --, so an ancestor without a file gets the union of its children; one
 * bottom-up pass over the output, whose (level, Morton index) order puts children behind their parent.  The boxes are
 * translated by global_offset first, like the cubes.  Such entries are marked `tight`, and swz_tileset_write writes them as
 * the 3D Tiles specification defines boundingVolume.box (HALF-axes).  An entry with no point below it keeps its cube and
 * stays unmarked.  geometric_error, is_tileset_root and the links are swz_tileset_build's.  OURS: the reference only knows
 * the cubes. */
int swz_tileset_build_boxes(uint64_t num_nodes, const int8_t* node_level, const uint64_t* node_key, const double* node_box_min,
                            const double* node_box_max, const double root_min[3], const double root_max[3], float spacing_at_root,
                            const double global_offset[3], uint64_t max_out, swz_tileset_node* out, uint64_t* num_out);

/* ---- the tight box of every node of a table: a segmented min/max over the stored rows, on the device.  OURS -- the
 * reference writes the octree cube of a node wherever a box is asked for (Cesium3DTilesPersistence.cpp:100-112,
 * LASPersistence.cpp:113-136), which wraps a thin, tilted sheet of airborne LiDAR in mostly empty volume.
 *   swz_node_boxes_device: row i of node k is d_xyz[d_perm[d_order[node_offset[k] + i]]], composed as in
 *     swz_pnts_pack_device (d_order NULL = identity, what a tiler's export ids need); node_offset / node_count are host
 *     arrays, box_min_out / box_max_out host arrays of num_nodes x 3 doubles.  The result is EXACT: the componentwise min and
 *     max of the node's doubles, nothing is computed on them (they are compared as order-preserving integer codes; -0.0 and
 *     +0.0 compare equal in IEEE, either may come back).  A node of count 0 gets min = +inf, max = -inf.  The pools hold
 *     finite, clamped positions; what a NaN does is not specified.  One workgroup takes swz_node_boxes_tile() consecutive
 *     stored rows (tests place their edges by it): a shuffle reduction per wave and window entry, one LDS combine per entry,
 *     then six 64-bit atomic min/max per (tile, node) on a table a small kernel presets -- the result does not depend on what
 *     the workspace held nor on the order of the atomics.  Pools spilled to page-locked host memory are read in place.
 *     SWZ_ERR_BAD_ARG before anything is launched for: offsets that do not ascend, ranges that overlap or pass n, a NULL
 *     buffer when a node holds points, n above 2^32 - 65536.  n == 0, no nodes or only empty nodes launches nothing. */
uint32_t swz_node_boxes_tile(void);
int swz_node_boxes_device(swz_ctx* ctx, const uint32_t* d_perm, const uint32_t* d_order, uint64_t n, const double* d_xyz,
                          uint64_t num_nodes, const uint64_t* node_offset, const uint64_t* node_count, double* box_min_out,
                          double* box_max_out);

/* ---- 3D Tiles node files and tileset JSON: Cesium3DTilesPersistence, the reference's default persistence
 * (executable/main.cpp:241-242; core/io/Cesium3DTilesPersistence.cpp:53-210, core/io/PNTSWriter.cpp:109-264).
 * A "<name>.pnts" file is a 28-byte header ("pnts", u32 version 1, u32 byteLength, u32 JSON length, u32 binary length,
 * u32 0, u32 0), the feature-table JSON {POINTS_LENGTH, RTC_CENTER, then {"byteOffset"} per array} padded with spaces to a
 * multiple of 8 counted from the start of the JSON (PNTSWriter.cpp:241-258), and the feature-table binary, the BODY: every
 * array at the running offset rounded up to its alignment, the whole zero-padded to a multiple of 8 (:198-213).
 * supported_output_attributes() is Position, RGB, Intensity: POSITION 3 x f32 (alignment 4; the PointBuffer's positions
 * narrowed with static_cast<float>, NOT shifted by RTC_CENTER, which only carries the persistence's global_offset), RGB
 * 3 x u8 (1), INTENSITY u16 (2).  The reference iterates an unordered_set, so it defines no order of the arrays; here it is
 * POSITION, RGB, INTENSITY, and the JSON carries every offset.  `mask` says which arrays besides POSITION a file holds.
 * Numbers in JSON are written in the shortest text that parses back to the same double.  rapidjson's Grisu2 does not always
 * find the shortest form, so a file agrees with the reference's in every parsed value and in every byte of the binary, but
 * not necessarily in the length of the JSON text (the spelling of a number is no part of either format).
 * --calculate-rgb-from (RGBFromIntensityAttribute, PNTSWriter.cpp:507-527): with a mapping RGB is the grey value of the
 * point's intensity (LINEAR: intensity >> 8; LOG: (uint8_t)(255 * logf(intensity + 1.f) / log(65535.)), a float numerator
 * divided in double), written whether or not the batch has a colour column, and only if it has intensities.  The 65 536 grey
 * values are evaluated once, on the host, with the host's libm (like swz_required_morton_index_depth).
 *   swz_pnts_layout (host): size and offset of every node's body in one contiguous IMAGE (bodies in table order, each a
 *     multiple of 8; a node of count 0 has size 0), the offsets of the RGB and intensity arrays inside a body (0 when absent),
 *     and the image's total size.  Any output may be NULL.
 *   swz_pnts_pack_device: writes the image of a node table into d_image_out (device, 8-byte aligned, image_bytes >= the
 *     layout's total) in one pass: the permuted gather (row i = row d_perm[d_order[i]] of d_xyz and of the columns of d_in,
 *     composed as in swz_gather_payload_device; d_order NULL = identity, what a tiler's export ids need), the narrowing, the
 *     colour mapping and the layout, padding included -- no byte of the image depends on what the buffer held, the caller
 *     need not clear it.  node_offset / node_count (host) are rows of the gathered order.  SWZ_ERR_BAD_ARG before anything
 *     is launched for: offsets that do not ascend, ranges that overlap or pass n, a mask that names an absent column, a
 *     mapping without the intensity column, n above 2^32 - 65536.  n == 0 or no nodes is valid and launches nothing.
 *   swz_pnts_write_node: one file from a packed body (count == 0 writes nothing, like swz_bin_write_node); rtc_center NULL
 *     = zeros.  swz_pnts_write_node_rows: the same file from unpacked rows (double positions + columns, what a PointsSink
 *     receives), converted on the host.  swz_pnts_persist_nodes: one file "r" + octant digits + ".pnts" per node of a table
 *     out of a HOST copy of the image, written by the pool of host threads of swz_bin_persist_nodes.
 *   swz_pnts_read_header / swz_pnts_read_node: retrieve_points.  Positions come back as the stored floats widened to double
 *     (the format is lossy), RGB and intensity into the non-NULL columns if the file has them.  The arrays are found through
 *     the offsets in the file's JSON, whatever their order.  SWZ_ERR_BAD_ARG, without reading outside the file, for a short
 *     file, a wrong magic, lengths that do not add up, an array that passes the binary, a JSON that cannot be read, a
 *     feature table without POSITION (POSITION_QUANTIZED is not read).  swz_pnts_read_header reads the header and the JSON
 *     only.  swz_pnts_parse_image: the same checks on a file image in memory, never reading outside [file, file +
 *     file_bytes); the three offsets count from the first byte of the image (0 for an array the file lacks), members other
 *     than POINTS_LENGTH, RTC_CENTER, POSITION, RGB and INTENSITY and a batch table are ignored; any output may be NULL.
 *   swz_tileset_write: the JSON files of swz_tileset_build's output (write_tilesets, Cesium3DTilesPersistence.cpp:173-210;
 *     writeTilesetJSON, core/io/TileSetWriter.cpp:42-210): "<name>.json" per is_tileset_root entry with asset.version "0.0",
 *     the entry's geometricError and its tile as root.  A tile holds boundingVolume.box = [centre, then the FULL extent on the
 *     diagonal] (boundingBoxFromAABB, core/pointcloud/Tileset.cpp:94-118: not halved) -- an entry marked `tight`
 *     (swz_tileset_build_boxes) instead [centre, then the HALF extent on the diagonal], as the 3D Tiles specification has
 *     it, the half-axes widened by the few ulps it takes for centre -/+ half, evaluated in double, to enclose bounds_min and
 *     bounds_max --, geometricError, refine "ADD",
 *     content.uri and children (by octant); three levels below the file's root the uri is "<name>.json" and there are no
 *     children, everywhere else "<name>.pnts" -- for ancestors without a file of their own too, as setup_tileset does.
 *     Compact, no whitespace.
 * The host functions need no GPU; their ctx only carries the error text and may be NULL. */
enum { SWZ_PNTS_RGB = 1u << SWZ_ATTR_RGB, SWZ_PNTS_INTENSITY = 1u << SWZ_ATTR_INTENSITY };
enum { SWZ_PNTS_RGB_FROM_COLOR = 0, SWZ_PNTS_RGB_FROM_INTENSITY_LINEAR = 1, SWZ_PNTS_RGB_FROM_INTENSITY_LOG = 2 };
int swz_pnts_layout(uint64_t num_nodes, const uint64_t* node_count, uint32_t mask, int rgb_mapping, uint64_t* body_offset_out,
                    uint64_t* body_size_out, uint64_t* rgb_offset_out, uint64_t* intensity_offset_out, uint64_t* total_out);
int swz_pnts_pack_device(swz_ctx* ctx, const uint32_t* d_perm, const uint32_t* d_order, uint64_t n, const double* d_xyz,
                         const swz_attribute_columns* d_in, uint64_t num_nodes, const uint64_t* node_offset,
                         const uint64_t* node_count, uint32_t mask, int rgb_mapping, void* d_image_out, uint64_t image_bytes);
int swz_pnts_write_node(swz_ctx* ctx, const char* path, uint64_t count, const void* body, uint64_t body_bytes, uint32_t mask,
                        const double rtc_center[3]);
int swz_pnts_write_node_rows(swz_ctx* ctx, const char* path, uint64_t count, const double* xyz,
                             const swz_attribute_columns* columns, uint32_t mask, int rgb_mapping, const double rtc_center[3]);
int swz_pnts_persist_nodes(swz_ctx* ctx, const char* dir, uint64_t num_nodes, const int8_t* node_level, const uint64_t* node_key,
                           const uint64_t* node_count, const void* image, uint64_t image_bytes, uint32_t mask,
                           const double rtc_center[3]);
int swz_pnts_read_header(swz_ctx* ctx, const char* path, uint64_t* count_out, uint32_t* mask_out, double rtc_center_out[3]);
int swz_pnts_read_node(swz_ctx* ctx, const char* path, double* xyz_out, const swz_attribute_columns* columns_out);
int swz_pnts_parse_image(swz_ctx* ctx, const void* file, uint64_t file_bytes, uint64_t* count_out, uint32_t* mask_out,
                         double rtc_center_out[3], uint64_t* position_offset_out, uint64_t* rgb_offset_out,
                         uint64_t* intensity_offset_out);
/* one value of the grey table (0 for SWZ_PNTS_RGB_FROM_COLOR) */
uint8_t swz_pnts_rgb_from_intensity(int rgb_mapping, uint16_t intensity);
int swz_tileset_write(swz_ctx* ctx, const swz_tileset_node* nodes, uint64_t num, const char* dir);
/* ---- 3D Tiles in a world frame: node files relative to their own origin, tile volumes as oriented boxes (what
 * swz_convert_dataset_world writes; struct swz_srs: see "a source projection" below).
 *   swz_pnts_pack_origin_device: swz_pnts_pack_device with an origin per node (node_origin: host, 3 doubles per node of the
 *     table): a position is stored as (float)(pos[c] - origin[c]), the subtraction in double, then the plain cast -- what
 *     setOriginToSmallestPoint + PNTSWriter do (Transformation.cpp:213-227).  A second instantiation of the pack kernel that
 *     keeps the origins of its window's nodes beside their bases; layout, RGB mapping and padding are swz_pnts_pack_device's,
 *     whose own instantiation and output are untouched.  Refuses what swz_pnts_pack_device refuses, and an origin that is
 *     not finite for a node that holds points (for an empty node it is not looked at).
 *   swz_pnts_persist_nodes_rtc: swz_pnts_persist_nodes with an RTC_CENTER per node (3 doubles per node; must be finite for
 *     a node that holds points).
 *   swz_tileset_oriented_boxes (host): boundingBoxFromAABB(aabb, transform) (core/pointcloud/Tileset.cpp:52-92) for every
 *     entry: with c = bounds_min + (bounds_max - bounds_min) / 2 the four points c, (max.x, c.y, c.z), (c.x, max.y, c.z),
 *     (c.x, c.y, max.z) go through swz_srs_transform to SWZ_SRS_ECEF; obb_out gets 12 doubles per entry: the mapped centre,
 *     then the three differences to it.  srs == NULL maps nothing: the centre and the axis-aligned HALF extents on the
 *     diagonal -- what the reference's converter writes with its IdentityTransform, and not the full extents its tiler
 *     writes (swz_tileset_write keeps those).  The four-point box follows the reference; it does not enclose the bulge of
 *     a flat tile's image.
 *   swz_tileset_write_oriented: swz_tileset_write with boundingVolume.box taken from obb (12 per entry, finite); an entry
 *     marked `tight` keeps its own axis-aligned centre and half-axes.  Everything else in the files is swz_tileset_write's. */
struct swz_srs_s;
int swz_pnts_pack_origin_device(swz_ctx* ctx, const uint32_t* d_perm, const uint32_t* d_order, uint64_t n, const double* d_xyz,
                                const swz_attribute_columns* d_in, uint64_t num_nodes, const uint64_t* node_offset,
                                const uint64_t* node_count, uint32_t mask, int rgb_mapping, void* d_image_out, uint64_t image_bytes,
                                const double* node_origin /* host, 3 per node */);
int swz_pnts_persist_nodes_rtc(swz_ctx* ctx, const char* dir, uint64_t num_nodes, const int8_t* node_level, const uint64_t* node_key,
                               const uint64_t* node_count, const void* image, uint64_t image_bytes, uint32_t mask,
                               const double* node_rtc_center /* 3 per node */);
int swz_tileset_oriented_boxes(const struct swz_srs_s* srs /* NULL: identity */, const swz_tileset_node* nodes, uint64_t num,
                               double* obb_out /* 12 per entry */);
int swz_tileset_write_oriented(swz_ctx* ctx, const swz_tileset_node* nodes, uint64_t num, const double* obb, const char* dir);

/* ---- LAS point records -> positions + attribute columns: the step right in
 * front of the path.  The reference reads points through LASzip into a laszip_point and converts them in
 * position_from_las_point (core/io/LASFile.cpp:79-94: offset + X * scale per axis, then clamped into the
 * header's bounding box) and las_read_points_into (:578-632: RGB >> 8, the other attributes copied).  LASzip
 * itself (github.com/LASzip/LASzip, built from LAStools per the reference's README.md:24-37, version not
 * pinned there) is not part of the reference tree; for UNCOMPRESSED files its reader only unpacks the fixed
 * point data record of the LAS specification, which is restated here for formats 0-10 (LASFile.cpp:421-426 lists the
 * formats that carry RGB: 2, 3, 5, 7, 8, 10):
 *   formats 0-5 (LAS 1.2 / 1.3): X,Y,Z i32 | intensity u16 | return number:3, number of returns:3, scan direction:1, edge
 *   of flight line:1 | classification:5 (+3 flag bits) | scan angle rank i8 | user data u8 | point source id u16 (20
 *   bytes) | format 1,3,4,5: gps time f64 | format 2,3,5: R,G,B u16 | format 4,5: 29 bytes of wave packet (skipped);
 *   formats 6-10 (LAS 1.4): X,Y,Z i32 | intensity u16 | return number:4, number of returns:4 | classification flags:4,
 *   scanner channel:2, scan direction:1, edge of flight line:1 | classification u8 | user data u8 | scan angle i16 (0.006
 *   degree) | point source id u16 | gps time f64 (30 bytes) | format 7,8,10: R,G,B u16 | 8,10: NIR u16 | 9,10: wave
 *   packet -- mapped onto the legacy fields the reference reads the way LASzip's raw reader does (returns above 7
 *   saturate, classes above 31 read 0, the scan angle is rounded to degrees and clamped to a signed byte).
 * d_records: n records of record_bytes each (>= the format's size; trailing extra bytes are skipped), device
 * memory, 4-byte aligned.  Columns absent from d_out are skipped; attributes the format lacks (gps time in
 * format 0/2, RGB in 0/1) are written as 0 like an untouched laszip_point. */
typedef struct {
  double scale[3];       /* laszip_header::x_scale_factor, y_, z_ */
  double offset[3];      /* x_offset, ... */
  double min[3];         /* min_x, ... : positions are clamped into [min, max] */
  double max[3];
  uint32_t point_format; /* 0..10 */
  uint32_t record_bytes; /* point data record length */
} swz_las_layout;
int swz_las_decode_device(swz_ctx* ctx, const uint8_t* d_records, uint64_t n, const swz_las_layout* layout,
                          double* d_xyz_out, const swz_attribute_columns* d_out);

/* ---- LAS node files and Entwine (EPT) output: LASPersistence and EntwinePersistence, --output-format LAS / ENTWINE_LAS
 * (executable/main.cpp:421-428; core/io/LASPersistence.cpp:16-271, core/io/EntwinePersistence.cpp:31-130, 197-333).  LAZ is
 * LASzip's compression and is not written.
 * A node file is a LAS 1.2 file: the 227-byte public header, no VLRs, then `count` point records of format (gps times ? 1
 * : 0) + (colours ? 2 : 0), 20 + 8 * gps + 6 * rgb bytes each (the record of formats 0-3 as swz_las_decode_device states it).
 * The header as the reference sets it (LASPersistence.cpp:113-136): number of point records = count, by return {count, 0,
 * 0, 0, 0}, version 1.2, generating software "pointcloud_tiler", header size = offset to point data = 227, the offsets = the
 * NODE BOX minimum, max/min x, y, z = the node box (the box handed to persist_points, not the extent of the points), one
 * scale for the three axes.  Everything else is what a fresh laszip_header happens to hold, and those bytes are NOT pinned
 * against LASzip: file source id, global encoding, GUID, system identifier, creation day and year are written as zeros, the
 * software string is padded with zeros.
 * Records: X = I32_QUANTIZE((x - offset) / scale) with I32_QUANTIZE(n) = n >= 0 ? (int32)(n + 0.5) : (int32)(n - 0.5)
 * (laszip_set_coordinates: a double subtraction, a division, an addition, not contracted, then truncation); intensity u16;
 * return number & 7 | (number of returns & 7) << 3 | (scan direction flag & 1) << 6 | (edge of flight line & 1) << 7;
 * classification & 31 (the flag bits zero); scan angle rank i8; user data u8; point source id u16; gps time f64 (formats 1,
 * 3); R, G, B as u8 << 8 in u16 (formats 2, 3; LASPersistence.cpp:215-217).  `mask` is a bit set over SWZ_ATTR_*: the
 * columns that are written; an attribute outside it is 0 like an untouched laszip_point.  Bit SWZ_ATTR_NORMAL is accepted and
 * ignored: normals are in supported_output_attributes(), but no LAS field takes them.  OURS, not the reference's: its
 * (int32) cast of a quotient outside int32 is undefined behaviour; here it saturates to INT32_MIN / INT32_MAX, and NaN
 * becomes 0.
 *   swz_las_scale_from_bounds: compute_las_scale_from_bounds (:16-28) on the box diagonal d: d > 1e6 -> 0.01, d > 1 -> 0.001,
 *     else 0.0001.  The writers take any finite positive scale.
 *   swz_las_record_layout: point format (0-3) and record bytes of a mask; SWZ_ERR_BAD_ARG for a bit above SWZ_ATTR_COUNT.
 *   swz_las_image_layout (host): the IMAGE holds the point records of every node in table order; each body is count x
 *     record bytes rounded up to a multiple of 8 (the padding is part of the image, not of the file), a node of count 0 has
 *     size 0.  Any output may be NULL.  SWZ_ERR_BAD_ARG for a count above 2^32 - 1 (the header's u32).
 *   swz_las_pack_device: writes the image of a node table into d_image_out (device, 8-byte aligned, image_bytes >= the
 *     layout's total) in one kernel: the permuted gather (row i = row d_perm[d_order[i]] of d_xyz and of the columns of
 *     d_in; d_order NULL = identity), the quantisation against node k's node_las_offset[3 k ..] and node_las_scale[k] (the
 *     box minimum of swz_node_bounds and the scale rule), the bit packing, the colour shift, the interleaved records and the
 *     zero padding -- no byte of the image depends on what the buffer held.  SWZ_ERR_BAD_ARG before anything is launched
 *     for: offsets that do not ascend, ranges that overlap or pass n, a mask that names an absent column or a bit that does
 *     not exist, n above 2^32 - 65536, an image that is too small or not 8-byte aligned, a scale that is not finite and
 *     positive, an offset that is not finite.  n == 0 or no nodes is valid and launches nothing.  swz_las_pack_tile: the
 *     stored rows one workgroup takes (tests place their edge cases by it).
 *   swz_las_write_node: header + count x record bytes of a packed body; count == 0 writes nothing (LASPersistence would
 *     write an empty file, EntwinePersistence returns before it does).  swz_las_write_node_rows: the same file from unpacked
 *     rows (what a PointsSink receives), converted on the host with the identical arithmetic.  Both refuse a box or scale
 *     that is not finite (scale: and positive) and a count above 2^32 - 1.
 *   swz_las_persist_nodes: one file per node of a table out of a HOST copy of the image, written by the pool of host threads
 *     of swz_bin_persist_nodes; node_box_min / node_box_max hold 3 doubles per node, node_scale one.  naming: "r" + octant
 *     digits + ".las" (SWZ_LAS_NAMING_POTREE) or "D-X-Y-Z.las" (SWZ_LAS_NAMING_ENTWINE).
 *   swz_las_read_header / swz_las_read_node: retrieve_points for formats 0-3.  Positions are offset + X * scale clamped into
 *     the header's box (position_from_las_point, core/io/LASFile.cpp:79-94), RGB is >> 8, the non-NULL columns are filled
 *     (0 where the format lacks the attribute).  Any output of read_header may be NULL.  SWZ_ERR_BAD_ARG, without reading
 *     outside the file, for a short file, a wrong signature, a header size or data offset that passes the file, a record
 *     length below the format's, a format above 3 (swz_las_decode_device decodes those), a count whose records pass the end.
 *   swz_ept_create_dirs: dir, dir/ept-data, dir/ept-hierarchy, dir/ept-sources (existing ones are kept).
 *   swz_ept_hierarchy_write: the files dir/ept-hierarchy/<D-X-Y-Z>.json of create_hierarchy_files (:51-130), split every 5
 *     levels: a node belongs to the file of its nearest ancestor-or-self whose depth is a multiple of 5, an object
 *     {"D-X-Y-Z": count, ...}; a subtree root carries its count in its own file and -1 in the file of the subtree root above
 *     it, up to 0-0-0-0, whether or not those ancestors are in the table.  Nodes of count 0 are skipped.  Compact; members
 *     ordered by (depth, Morton index) -- the reference iterates unordered maps, the order is no part of the format.
 *   swz_ept_json_write: ept.json of write_ept_json (:197-269) with the members bounds, boundsConforming, dataType "las",
 *     hierarchyType "json", points, schema, span, srs {authority, horizontal, wkt}, version, in this order.  The schema
 *     (point_attributes_to_ept_schema, :132-194) is X, Y, Z (the only entries with "offset" 0 and "scale" 1), then the
 *     attributes of attribute_mask by SWZ_ATTR_* -- the reference iterates an unordered set; entries are {name, size, type}.
 *     Numbers are written like swz_tileset_write writes them; a NULL string is "".
 * The host functions need no GPU; their ctx only carries the error text and may be NULL. */
enum { SWZ_LAS_NAMING_POTREE = 0, SWZ_LAS_NAMING_ENTWINE = 1 };
typedef struct {
  double bounds_min[3], bounds_max[3];         /* the cubic root box */
  double conforming_min[3], conforming_max[3]; /* the box of the points */
  uint64_t points;
  uint32_t attribute_mask;                     /* bits SWZ_ATTR_*; the position is always part of the schema */
  uint32_t reserved;
  double span;
  const char* srs_authority;
  const char* srs_horizontal;
  const char* srs_wkt;
  const char* version;
} swz_ept_json;
double swz_las_scale_from_bounds(const double box_min[3], const double box_max[3]);
/* The box of the STORED records of a node whose points have the box [box_min, box_max]: both corners sent through the
 * quantisation of the row writers against las_offset and scale and back the way swz_las_read_node dequantises (offset + X *
 * scale).  The map is monotonic, so this is the min / max of the positions swz_las_read_node returns -- what a LAS header's
 * max / min x, y, z should hold (swz_tiler_write_output with SWZ_OUT_TIGHT_BOUNDS). */
int swz_las_stored_box(const double box_min[3], const double box_max[3], const double las_offset[3], double scale,
                       double min_out[3], double max_out[3]);
/* swz_las_write_node with a header whose max / min x, y, z are [extent_min, extent_max]; the offsets stay box_min. */
int swz_las_write_node_extent(swz_ctx* ctx, const char* path, uint64_t count, const void* body, uint32_t mask,
                              const double box_min[3], const double box_max[3], double scale, const double extent_min[3],
                              const double extent_max[3]);
int swz_las_record_layout(uint32_t mask, uint32_t* point_format_out, uint32_t* record_bytes_out);
int swz_las_image_layout(uint64_t num_nodes, const uint64_t* node_count, uint32_t mask, uint64_t* body_offset_out,
                         uint64_t* body_size_out, uint64_t* total_out);
uint32_t swz_las_pack_tile(void);
int swz_las_pack_device(swz_ctx* ctx, const uint32_t* d_perm, const uint32_t* d_order, uint64_t n, const double* d_xyz,
                        const swz_attribute_columns* d_in, uint64_t num_nodes, const uint64_t* node_offset,
                        const uint64_t* node_count, const double* node_las_offset, const double* node_las_scale, uint32_t mask,
                        void* d_image_out, uint64_t image_bytes);
int swz_las_write_node(swz_ctx* ctx, const char* path, uint64_t count, const void* body, uint32_t mask, const double box_min[3],
                       const double box_max[3], double scale);
int swz_las_write_node_rows(swz_ctx* ctx, const char* path, uint64_t count, const double* xyz,
                            const swz_attribute_columns* columns, uint32_t mask, const double box_min[3], const double box_max[3],
                            double scale);
int swz_las_persist_nodes(swz_ctx* ctx, const char* dir, uint64_t num_nodes, const int8_t* node_level, const uint64_t* node_key,
                          const uint64_t* node_count, const double* node_box_min, const double* node_box_max,
                          const double* node_scale, const void* image, uint64_t image_bytes, uint32_t mask, int naming);
int swz_las_read_header(swz_ctx* ctx, const char* path, uint64_t* count_out, uint32_t* point_format_out,
                        uint32_t* record_bytes_out, uint32_t* offset_to_point_data_out, swz_las_layout* layout_out);
int swz_las_read_node(swz_ctx* ctx, const char* path, double* xyz_out, const swz_attribute_columns* columns_out);
int swz_ept_create_dirs(swz_ctx* ctx, const char* dir);
int swz_ept_hierarchy_write(swz_ctx* ctx, const char* dir, uint64_t num_nodes, const int8_t* node_level,
                            const uint64_t* node_key, const uint64_t* node_count);
int swz_ept_json_write(swz_ctx* ctx, const char* path, const swz_ept_json* ept);

/* ---- multi-GPU sharding: one context per GPU, points owned by their top
 * Morton bits (level-0 octant, MortonIndex::get_octant_at_level(0), MortonIndex.h:133-138), so every
 * node at level >= 0 lives on exactly one GPU.  The reference has no counterpart (it is a single
 * process); the exchange itself (RCCL all-to-all) is done by the host driver, the library provides
 * the device-side pieces:
 *   swz_partition_by_octant_device: perm groups point indices by octant 0..7 (stable inside an
 *     octant); counts_out[o] = points of octant o.  Drivers may rely on the order (octant, original
 *     index): the key bits below the octant play no part, and points of equal key keep their index order.
 *   swz_shard_begin_device: indexes + sorts the shard's points (d_xyz_local stays referenced until
 *     swz_shard_finish_device returns and may be clamped in place) and samples the ROOT node, whose
 *     take-all/sample decision uses shard->global_points.  For MIN_DISTANCE the root couples the
 *     shards: the points the root took on all lower octants are passed as ghosts (they sort first and
 *     are accepted again, rejecting exactly what the single-GPU sweep would reject).
 *   swz_shard_root_taken_device: positions (N x 3) of the LOCAL points the root took, Morton order:
 *     the ghosts to hand to the shards owning higher octants.
 *   swz_shard_finish_device: tiles levels >= 0 and writes the outputs of swz_tile_device for the n
 *     local points (keys ascending, perm = index into the local xyz, level).
 *   A shard without points (n == 0: its octants are empty) is valid everywhere: presort is a no-op, begin takes
 *   nothing of the root, finish reports zero points. */
typedef struct {
  uint64_t global_points;      /* points of the whole batch over all shards */
  const double* d_ghost_xyz;   /* device, num_ghosts x 3; all ghosts must lie in lower octants.  When the
                                  ghosts end exactly where d_xyz_local starts, no staging copy is made */
  uint64_t num_ghosts;
} swz_shard_info;
int swz_partition_by_octant_device(swz_ctx* ctx, const uint64_t* d_keys, uint64_t n, uint32_t* d_perm_out,
                                   uint64_t counts_out[8]);
/* Optional, before swz_shard_begin_device with the same d_xyz_local / n: does the part of it that does not
 * depend on the ghosts (index + sort + gather of the local points), leaving room for up to ghost_capacity
 * ghosts.  When the root couples the shards (MIN_DISTANCE) every shard calls this right after the exchange,
 * all at the same time, and only the root node itself remains in the chain that hands the ghosts from shard
 * to shard (ghosts sort in front of all local points: they lie in lower octants). */
int swz_shard_presort_device(swz_ctx* ctx, const double* d_xyz_local, uint64_t n, const double bounds_min[3],
                             const double bounds_max[3], const swz_tile_params* params, uint64_t ghost_capacity);
int swz_shard_begin_device(swz_ctx* ctx, const double* d_xyz_local, uint64_t n, const double bounds_min[3],
                           const double bounds_max[3], const swz_tile_params* params,
                           const swz_shard_info* shard, uint64_t* num_root_taken_out);
int swz_shard_root_taken_device(swz_ctx* ctx, double* d_xyz_out);
int swz_shard_finish_device(swz_ctx* ctx, uint64_t* d_keys_out, uint32_t* d_perm_out, int8_t* d_level_out,
                            swz_tile_stats* stats);
/* FAST (TilingAlgorithmV3, the reference's default: executable/main.cpp:299-301) on a sharded batch.  The start level comes
 * from the distribution of the WHOLE batch (estimate_start_node_level_in_octree, TilingAlgorithms.cpp:1473-1535); start nodes
 * lie at level >= 2, inside one shard's octants, so the levels from there down and the reconstruction of the skipped levels
 * down to level 0 (reconstruct_left_out_nodes, :1717-1784) are local, and only the root is reconstructed across the shards:
 *   swz_shard_fast_begin_device: indexes + sorts the shard's points; prefix_counts_out[8^6] (host) = its points per
 *     6-octant prefix.  The driver sums the counts of all shards and calls swz_fast_start_level_from_counts.
 *   swz_shard_fast_run: the levels from start_level - 1 down, then the skipped levels down to 0;
 *     num_root_candidates_out = the points this shard's level-0 nodes hold.
 *   swz_shard_fast_root_candidates_device: their keys and positions, in key order.  The root samples the candidates of ALL
 *     shards, one behind the other in shard order (= octant order, the order the reference appends its children in), with
 *     AlwaysAdhereToMinSpacing: swz_sample_points_device(..., node_level -1, SWZ_ALWAYS_ADHERE_TO_MIN_SPACING, ...).
 *   swz_shard_fast_set_root_device: d_taken = the flags of this shard's candidates (bit 0 of dup is set for them).
 *   swz_shard_fast_finish_device: the outputs of swz_tile_device with the FAST strategy for the local points (d_dup_out:
 *     bit l + 1 set = the point is also stored in its ancestor at node level l).
 *   A shard without points takes part in every step with zero counts. */
int swz_shard_fast_begin_device(swz_ctx* ctx, const double* d_xyz_local, uint64_t n, const double bounds_min[3],
                                const double bounds_max[3], const swz_tile_params* params, uint32_t* prefix_counts_out);
int swz_shard_fast_run(swz_ctx* ctx, int32_t start_level, uint64_t* num_root_candidates_out);
int swz_shard_fast_root_candidates_device(swz_ctx* ctx, uint64_t* d_keys_out, double* d_xyz_out);
int swz_shard_fast_set_root_device(swz_ctx* ctx, const uint8_t* d_taken);
int swz_shard_fast_finish_device(swz_ctx* ctx, uint64_t* d_keys_out, uint32_t* d_perm_out, int8_t* d_level_out,
                                 uint32_t* d_dup_out, swz_tile_stats* stats);

/* ---- multi-batch tiling (BASELINE config 5's single-GPU shape).
 * The reference calls TilingAlgorithmBase::build_execution_graph once per batch of at most internal_cache_size
 * points (core/process/Tiler.cpp:509-510; executable/main.cpp:233-236, default 10 M) on one algorithm object;
 * every node a batch reaches re-reads its file, re-keys those points relative to the node
 * (read_pnts_from_disk, core/tiling/TilingAlgorithms.cpp:50-109), merges them with the new ones
 * (merge_node_data_sorted, core/tiling/Node.cpp:4-22), samples with AlwaysAdhereToMinSpacing (:272-275) and
 * REPLACES the file (BinaryPersistence.h:46-57).  FAST: later iterations (:1362-1453, 1620-1659) + finalize
 * (:1661-1784).  swz_tiler keeps the node files in device memory: one context, one tiler per data set.
 *   Point ids count the points of all batches in input order (batch 0's points are 0..n0-1, ...).
 *   swz_tiler_add_batch_device: d_xyz (n x 3, device) is clamped in place like index_point does and copied
 *     into the tiler's position pool.
 *   swz_tiler_stage_batch / swz_tiler_tile_staged: the same from HOST memory (pinned: swz_host_alloc_pinned, or
 *     hipHostRegister'ed by the caller), copied with hipMemcpyAsync on a copy stream straight into the pools; up
 *     to two batches may be staged, so the copy of batch k+1 runs while batch k is tiled:
 *         stage(0); for k: { if (k+1 < K) stage(k+1); tile_staged(); }
 *     attrs_host (may be NULL) are the batch's attribute columns (host pointers); every batch must carry the same
 *     set.  The host copy of the positions is NOT clamped; the pools (swz_tiler_pools_device) hold the clamped ones.
 *   Refused batches: swz_tiler_add_batch_device, swz_tiler_stage_batch and swz_tiler_add_batch answer SWZ_ERR_BAD_ARG
 *     for a batch after swz_tiler_finalize and, under SWZ_FAST, for a batch of fewer than fast_concurrency points,
 *     the EMPTY batch included (parallel::scatter throws, util/threading/Parallel.h:181-186).  The check comes before
 *     anything is reserved, copied, staged or counted: a refused batch leaves the tiler as it was (not poisoned,
 *     num_batches and num_points unchanged, no point id used up) and the data set goes on with the next batch.
 *     Under SWZ_ACCURATE an empty batch (n = 0, d_xyz / xyz_host may be NULL) is counted in num_batches and changes
 *     no file.  (swz_tiler_shard_begin_device is exempt from the FAST rule: the driver checks the whole batch.)
 *   swz_tiler_finalize: TilingAlgorithmBase::finalize (FAST: reconstruct_left_out_nodes); no more batches after.
 *   swz_tiler_export_device / swz_tiler_node_table: the node files: nodes ordered by (level, Morton index);
 *     entries [node_offset[k], +node_count[k]) of keys/ids/level are node k's points in file order (FAST stores
 *     copies of a point in reconstructed ancestors, so num_stored >= num_points).  ids index the pools: rows of
 *     the files are swz_gather_payload_device(ctx, d_ids, NULL, num_stored, pool_xyz, pool_attrs, ...).
 *   rekey_inversions: re-keyed file contents whose order was not ascending any more (a point within an ulp of a
 *     cell boundary); the reference merges them unsorted for a lossless persistence (:103-106), this library sorts
 *     them like the reference does for a lossy one -- results may differ from the reference only when > 0.
 *   A node that needs Morton re-rooting (:444-483) is re-rooted like the reference does (its subtree's files are
 *     ordered by the re-rooted keys); only the single-batch swz_tile*, whose outputs cannot express that order,
 *     returns SWZ_ERR_REROOT_UNSUPPORTED there. */
typedef struct swz_tiler swz_tiler;
typedef struct {
  uint64_t num_points;       /* points added so far */
  uint64_t num_stored;       /* entries in node files */
  uint64_t num_nodes;        /* node files */
  uint64_t num_batches;
  uint64_t rekey_inversions;
  int32_t fast_start_levels; /* FAST: _level_of_start_nodes once known, else -1 */
  uint64_t staged_bytes;     /* bytes copied by swz_tiler_stage_batch */
  double staged_wait_ms;     /* time swz_tiler_tile_staged waited for its copy (0 = fully hidden behind tiling) */
} swz_tiler_info;
int swz_tiler_create(swz_ctx* ctx, const double bounds_min[3], const double bounds_max[3],
                     const swz_tile_params* params, uint64_t capacity_hint_points, swz_tiler** tiler_out);
int swz_tiler_destroy(swz_tiler* tiler); /* before swz_destroy of its context */
int swz_tiler_add_batch_device(swz_tiler* tiler, double* d_xyz, uint64_t n, swz_tile_stats* stats);
int swz_tiler_stage_batch(swz_tiler* tiler, const double* xyz_host, uint64_t n, const swz_attribute_columns* attrs_host);
int swz_tiler_tile_staged(swz_tiler* tiler, swz_tile_stats* stats);
/* stage + tile of one host batch, no overlap */
int swz_tiler_add_batch(swz_tiler* tiler, const double* xyz_host, uint64_t n, const swz_attribute_columns* attrs_host,
                        swz_tile_stats* stats);
int swz_tiler_finalize(swz_tiler* tiler, swz_tile_stats* stats);
int swz_tiler_get_info(swz_tiler* tiler, swz_tiler_info* info);
/* SPILL.  The pools (24 bytes + the attribute rows of every point of the data set, by point id) are the bulk of a
 * tiler's memory.  When they cannot grow in device memory -- hipMalloc is out of memory, or the context's workspace
 * would pass SWZ_TILER_DEVICE_BUDGET_MB -- they move to page-locked host memory that is mapped into the device's address
 * space, and the kernels keep reading and writing them in place over the host link (a batch's own points once, the
 * cached points a batch pulls in, by id; the attribute columns only when files are exported).  Results do not change;
 * swz_tiler_pools_device then hands out device-accessible HOST pointers.  The node store (12 bytes per stored point and
 * side) stays in device memory.  Option SWZ_TILER_SPILL: "auto" (default), "host" (from the start), "off" (fail with
 * SWZ_ERR_HIP as before).  Replaces nothing in the reference, whose node files live on disk between batches
 * (core/tiling/TilingAlgorithms.cpp:50-109); this is what bounds the size of a data set per GPU here. */
int swz_tiler_pool_residency(swz_tiler* tiler, uint64_t* device_bytes_out, uint64_t* host_bytes_out);
/* Makes room in the pools for `total_points` points of the data set NOW (what the next batch would do on its own).  A
 * driver that must know where the pools will live while a batch is tiled -- the joint MIN_DISTANCE root of one process per
 * GPU exports them as IPC handles, which page-locked host memory does not have -- reserves first and asks
 * swz_tiler_pool_residency afterwards. */
int swz_tiler_reserve(swz_tiler* tiler, uint64_t total_points);
/* The same for the node store (the files' {key, point id} entries, two sides per octree level): a side that finds no device
 * memory, or would push the workspace over SWZ_TILER_DEVICE_BUDGET_MB, is placed in mapped pinned host memory like a pool
 * and the merges stream through it over the host link. */
int swz_tiler_store_residency(swz_tiler* tiler, uint64_t* device_bytes_out, uint64_t* host_bytes_out);
/* OBSERVABILITY FOR TESTS (read-only; no kernel knows of either).
 *   swz_tiler_merge_tile / swz_tiler_merge_lds: the merge of a level's active set with the files it pulled ranks
 *     swz_tiler_merge_tile() consecutive elements of one run per workgroup against the bracket of the other run that its
 *     first and last element span, out of LDS when the bracket holds at most swz_tiler_merge_lds() keys, else out of global
 *     memory.  swz_tiler_gather_lds: the copy of pulled (or compacted) files takes 256 consecutive output entries per
 *     workgroup and searches the segments they span out of LDS when they are at most swz_tiler_gather_lds().  Tests place
 *     their run lengths, brackets and empty segments by these, like swz_las_input_tile / swz_bin_pack_tile.
 *   swz_tiler_path_counts: how often this tiler's batches went which way through the node store, counted on the host where
 *     the decision is made; the first min(n, SWZ_TILER_PATH_COUNT) slots of out, in the order of the SWZ_TILER_PATH_*
 *     indices, further slots 0.  A test asserts that the path it is named after was taken. */
#define SWZ_TILER_PATH_PULL_IN_PLACE 0       /* a level's side read where it lies: the batch reaches all of a linear level */
#define SWZ_TILER_PATH_PULL_GATHERED 1       /* the files of the reached nodes copied out */
#define SWZ_TILER_PATH_PULL_WHOLE_FILE 2     /* a re-rooted node took its cached file out of a populated level */
#define SWZ_TILER_PATH_REKEY 3               /* pulled files re-keyed against their node (files finalize / re-rooting wrote) */
#define SWZ_TILER_PATH_RESORT 4              /* pulled files sorted again after an inversion (see rekey_inversions) */
#define SWZ_TILER_PATH_COMPACT_FULL 5        /* a level's live files gathered into the other side because the side was full */
#define SWZ_TILER_PATH_LINEARIZE_MOVED 6     /* log form -> linear form that moved data (node table, export, FAST finalize) */
#define SWZ_TILER_PATH_APPEND_BEHIND 7       /* new files appended behind the entries a side already held */
#define SWZ_TILER_PATH_TABLE_MERGE_NF0 8     /* node tables merged with no untouched entry */
#define SWZ_TILER_PATH_TABLE_MERGE_HEADS0 9  /* node tables merged with no new file */
#define SWZ_TILER_PATH_COUNT 10
uint32_t swz_tiler_merge_tile(void);
uint32_t swz_tiler_merge_lds(void);
uint32_t swz_tiler_gather_lds(void);
int swz_tiler_path_counts(swz_tiler* tiler, uint64_t* out, uint32_t n);
int swz_tiler_export_device(swz_tiler* tiler, uint64_t* d_keys_out, uint32_t* d_ids_out, int8_t* d_level_out);
int swz_tiler_node_table(swz_tiler* tiler, uint64_t max_nodes, int8_t* node_level_out, uint64_t* node_key_out,
                         uint64_t* node_offset_out, uint64_t* node_count_out, uint64_t* num_nodes_out);
/* ONE batch as node files -- the single-batch call for batches whose nodes may need Morton re-rooting
 * (core/tiling/TilingAlgorithms.cpp:444-483).  swz_tile's outputs (a level per point of the sorted batch, the node being
 * a prefix of the point's root key) cannot express a re-rooted subtree -- its children are contiguous chunks of the
 * re-indexed points, :479-482 -- and swz_tile returns SWZ_ERR_REROOT_UNSUPPORTED there; this pair of calls returns the
 * node table and the files' contents instead, in the form swz_tiler_node_table / swz_tiler_export_device hand out (it
 * runs the batch through a tiler of its own: one batch, finalize).  In two steps so that the caller can size its buffers:
 *   swz_tile_nodes_begin_device: tiles d_xyz (device, clamped in place like index_point does); *num_stored_out entries
 *     in *num_nodes_out node files;
 *   swz_tile_nodes_end_device: the files -- d_keys_out / d_ids_out / d_level_out (device, num_stored entries, any may be
 *     NULL; ids are rows of d_xyz) -- and the node table (host arrays of max_nodes >= num_nodes entries: level, Morton
 *     index, offset and count of every node, nodes ordered by (level, Morton index)); closes the call.
 * swz_tile_nodes_end_device with every pointer NULL and max_nodes 0 just closes it.  One open call per context; a context
 * that has a swz_tiler open cannot take it (SWZ_ERR_BAD_ARG). */
int swz_tile_nodes_begin_device(swz_ctx* ctx, double* d_xyz, uint64_t n, const double bounds_min[3], const double bounds_max[3],
                                const swz_tile_params* params, uint64_t* num_stored_out, uint64_t* num_nodes_out,
                                swz_tile_stats* stats);
int swz_tile_nodes_end_device(swz_ctx* ctx, uint64_t* d_keys_out, uint32_t* d_ids_out, int8_t* d_level_out, uint64_t max_nodes,
                              int8_t* node_level_out, uint64_t* node_key_out, uint64_t* node_offset_out,
                              uint64_t* node_count_out);
/* the pools by point id: positions (num_points x 3, clamped) and the attribute columns staged so far */
int swz_tiler_pools_device(swz_tiler* tiler, const double** d_xyz_out, swz_attribute_columns* d_attrs_out);
/* ---- the node files of a tiler, written in ONE call, in any of the reference's uncompressed output formats (--output-format
 * BIN, BINZ, 3DTILES, LAS, ENTWINE_LAS; executable/main.cpp:421-428) with the attribute columns the batches carried.
 * Precondition: that of swz_tiler_export_device -- the tiler is not poisoned and no batch is staged or open; the files are
 * the node store's as it stands, so a data set is written after swz_tiler_finalize.  The tiler stays usable, a failed write
 * does not poison it.
 *   Files: node k of swz_tiler_node_table becomes dir/<swz_node_name>.bin | .binz | .pnts | .las, or
 *     dir/ept-data/<swz_node_name_entwine>.las; boxes are swz_node_bounds of the tiler's root box, a LAS file's offset is its
 *     box minimum and its scale swz_las_scale_from_bounds of its box -- what TilingAlgorithmGPU::finalize and the sinks of
 *     schwarzwald_amd/host/swz_tiling.hpp compute.  dir is created when it does not exist (one level).
 *   attribute_mask: the columns to write, a subset of what the batches carried.  3DTILES writes RGB and INTENSITY of it and
 *     ignores the rest, like Cesium3DTilesSink: with an rgb_mapping RGB is the grey value of the intensity.
 *   Metadata, at the end: 3DTILES swz_tileset_build + swz_tileset_write (global_offset: RTC_CENTER and the boxes' shift);
 *     ENTWINE_LAS swz_ept_create_dirs first, swz_ept_hierarchy_write last, and ept.json from `ept` unless it is NULL.
 *   Streaming: the ids of all files are exported once (4 bytes per stored point); the node table is cut into chunks of
 *     whole consecutive nodes of at most chunk_points stored points (0: option SWZ_OUTPUT_CHUNK_POINTS, else 16 Mi; never
 *     less than the largest node); per chunk the format's pack kernel writes the chunk's image from the pools (spilled ones
 *     are read in place) into one of two device buffers, a copy stream moves it into one of two page-locked host buffers,
 *     and the writer threads (SWZ_BIN_WRITER_THREADS) write chunk k's files while chunk k + 1 is packed and copied.  Device
 *     and host hold two chunk images at most, whatever the size of the data set.
 *   SWZ_ERR_BAD_ARG before anything is written for: an unknown format, a mask that names a column the pools do not have, an
 *     rgb_mapping without intensities in the mask, a global_offset that is not finite, a dir that cannot be created.  A file
 *     that cannot be written stops the stream after the running chunk and is reported by name.
 *   stats (may be NULL): pack_ms is the time in the pack calls, copy_ms the copy stream's, write_ms the writer threads',
 *     each summed over the chunks; wall_ms the whole call; bytes_written the chunk images that went into files.
 *   flags: 0 is everything above, byte for byte; an unknown bit is SWZ_ERR_BAD_ARG.  SWZ_OUT_TIGHT_BOUNDS (OURS): the boxes
 *     in the metadata are the boxes of the POINTS, not the octree cubes.  swz_node_boxes_device runs on every chunk's ids
 *     beside the pack call (its time counts into pack_ms); no point record and no .pnts file changes.
 *       3DTILES: the tileset goes through swz_tileset_build_boxes (unions bottom-up, half-axes); the box of a node is the box
 *         of what its file HOLDS, the double box narrowed to float and widened again (narrowing is monotonic).
 *       LAS, ENTWINE_LAS: offset, scale and records are unchanged; the header's max / min x, y, z become swz_las_stored_box
 *         of the node's box -- exactly the min / max of what swz_las_read_node returns.
 *       ENTWINE_LAS with ept: boundsConforming is the union of those boxes, overriding ept->conforming_*; bounds stays.
 *       BIN, BINZ hold no box: the flag is refused by name.
 *   swz_tiler_node_boxes: the double boxes of the nodes, in the order of swz_tiler_node_table (max_nodes x 3 doubles each;
 *     a node without points: +inf / -inf).  Precondition: that of swz_tiler_export_device.  The ids are exported once and
 *     swz_node_boxes_device runs over the pools chunk by chunk (SWZ_OUTPUT_CHUNK_POINTS), so memory stays bounded by a
 *     chunk.  The tiler stays usable, a failure does not poison it. */
enum { SWZ_OUT_BIN = 0, SWZ_OUT_BINZ = 1, SWZ_OUT_3DTILES = 2, SWZ_OUT_LAS = 3, SWZ_OUT_ENTWINE_LAS = 4 };
enum { SWZ_OUT_TIGHT_BOUNDS = 1u };
typedef struct {
  int format;
  uint32_t attribute_mask;   /* bits SWZ_ATTR_*, a subset of what the batches carried */
  int rgb_mapping;           /* 3DTILES only: SWZ_PNTS_RGB_FROM_* */
  uint32_t flags;            /* SWZ_OUT_TIGHT_BOUNDS; 0 = none (these four bytes were padding: size and offsets are unchanged) */
  double global_offset[3];   /* 3DTILES: RTC_CENTER / the tileset boxes */
  uint64_t chunk_points;     /* 0 = default */
  const swz_ept_json* ept;   /* ENTWINE_LAS: NULL = do not write ept.json */
} swz_output_params;
typedef struct {
  uint64_t nodes, stored_points, bytes_written, chunks;
  double pack_ms, copy_ms, write_ms, wall_ms;
} swz_output_stats;
int swz_tiler_write_output(swz_tiler* tiler, const char* dir, const swz_output_params* params, swz_output_stats* stats);
/* what swz_tiler_write_output / swz_group_write_output refuse of `flags` for a format (host, no GPU): SWZ_ERR_BAD_ARG and
 * the text of the refusal in *what_out (static; NULL when the flags are fine). */
int swz_output_flags_check(int format, uint32_t flags, const char** what_out);
int swz_tiler_node_boxes(swz_tiler* tiler, uint64_t max_nodes, double* box_min_out, double* box_max_out, uint64_t* num_nodes_out);
/* The chunks swz_tiler_write_output cuts a node table into (host): chunk j holds the nodes [first_node_out[j],
 * first_node_out[j + 1]); first_node_out takes up to max_chunks + 1 entries and may be NULL (then only *num_chunks_out). */
int swz_output_chunks(uint64_t num_nodes, const uint64_t* node_count, uint64_t chunk_points, uint64_t max_chunks,
                      uint64_t* first_node_out, uint64_t* num_chunks_out);
/* ---- a data set of uncompressed LAS files read in ONE call: the input side of swz_tiler_write_output.  What the reference
 * does in TilerProcess::prepare / calculate_dataset_metadata (core/process/TilerProcess.cpp:250-390, 570-600) and
 * MultiReaderPointSource, for files that need neither a PROJ transformation nor LASzip ("LAZ is not read").
 *   swz_las_scan_files (host, no GPU; ctx only carries the error text and may be NULL): parses the LAS 1.0 - 1.4 public
 *     header of every file, little-endian, without reading past the file.  Per file (files_out, may be NULL): the point count
 *     -- the legacy u32, or the LAS 1.4 extended u64 count when the legacy one is 0 or the point format is >= 6
 *     (LASFile::size, core/io/LASFile.cpp:268-276) --, the swz_las_layout, the offset to the point data, the SWZ_ATTR_* the
 *     file has by the rules of las_file_has_attribute (LASFile.cpp:415-445, as written: GPS time is credited to formats 1
 *     and 3 only, colours to 2, 3, 5, 7, 8, 10, normals to none) and a status.  The data set: the total point count, the
 *     union of the headers' boxes (get_bounds_from_las_header, :402-406; every readable file, an empty one included, as
 *     DatasetMetadata::add_file_metadata does), that box made cubic exactly as AABB::makeCubic computes it
 *     (core/math/AABB.h:50-70: centre = min + extent / 2, then -+ the largest extent / 2 -- bit for bit), the cubic box at
 *     the origin (cubic min / max minus the cubic box's own centre, core/pointcloud/FileStats.cpp:30-37), that centre, and
 *     the attributes common to all readable files.
 *     SWZ_ERR_BAD_ARG, naming the file, for: a file that cannot be opened, a short file or a wrong signature, a point format
 *     above 10, a record length below the format's, an offset to the point data or count x record length that passes the
 *     end of the file, a compressed file (bit 7 of the point format or a LASzip VLR).  With SWZ_LAS_SCAN_SKIP_UNREADABLE
 *     such a file gets count 0 and its status instead (IgnoreErrors::InaccessibleFiles) and takes no part in the data set.
 *     No points at all: SWZ_ERR_BAD_ARG ("Found no points to process", TilerProcess.cpp:587-589).
 *   swz_input_batches (host): the cuts of the data set into batches, as swz_output_chunks does for output.  Batches are
 *     runs of batch_points consecutive points of the files concatenated in the given order (a batch of the reference is
 *     internal_cache_size points of the concatenated sources); batch j holds the points [first_point_out[j],
 *     first_point_out[j + 1]); first_point_out takes up to max_batches + 1 entries and may be NULL (then only
 *     *num_batches_out).  A tail of fewer than min_last points is folded into the batch before it -- min_last is
 *     fast_concurrency under SWZ_FAST, which refuses a shorter batch, and 0 otherwise.  The folding is OURS: the
 *     reference's reader threads define no batch order.  SWZ_ERR_BAD_ARG for batch_points 0, a data set of fewer than
 *     min_last points, and max_batches too small.
 *   swz_las_decode_segments_device: one kernel for a batch that spans files.  d_raw holds raw point records; segment s is
 *     count records of layout.record_bytes each, the first at byte byte_offset of d_raw, decoded into the output rows
 *     [first_row, first_row + count).  d_raw, the byte offsets and the record lengths have ANY alignment and parity.  A
 *     workgroup takes swz_las_input_tile() consecutive rows, whatever segments they belong to (it finds them in a table in
 *     LDS), loads the aligned words that cover its records into LDS -- whole words only where they lie inside
 *     [d_raw, d_raw + raw_bytes), single bytes at the two ends -- and unpacks from there; a tile whose records span more
 *     than swz_las_input_tile() x 96 bytes (records longer than 96 bytes, or gaps between segments) is read directly.  The
 *     field mapping is swz_las_decode_device's.  shift_center (NULL = none): after the clamp into the header box every
 *     axis becomes (double)(float)(p - centre), the 3D Tiles transformation of TilerProcess::make_tiler
 *     (TilerProcess.cpp:552-559).  Columns absent from d_out are skipped, d_xyz_out may be NULL.
 *     SWZ_ERR_BAD_ARG before anything is launched for: rows that do not ascend contiguously from 0, a segment whose
 *     records pass raw_bytes, a format above 10 or a record length below the format's, more than 2^32 - 65536 points, a
 *     centre that is not finite.  Zero segments or zero points launches nothing.
 *   swz_tiler_add_las_files: scans the headers, refuses what can be refused, then streams the files through the tiler.
 *     params: batch_points (0 = 10 M, the reference's --internal-cache-size), attribute_mask (a subset of the data set's
 *     common mask; ~0u = all of it; bit SWZ_ATTR_NORMAL is refused), shift_to_center (positions become (double)(float)(p -
 *     the cubic box's centre): the tiler's root box must then be the box at the origin), flags (SWZ_LAS_SCAN_*).  Point ids
 *     are the input order: file by file, record by record.  SWZ_ERR_BAD_ARG when the tiler's root box does not contain the
 *     data set's (shifted) tight box -- up to 4 ulp of the coordinates: makeCubic's own box can miss its tight box by one,
 *     and what lies outside by a rounding is clamped by the indexing as in the reference --, when the mask is not the one the tiler's first batch fixed, when batches are staged
 *     or open; SWZ_ERR_TOO_MANY_POINTS before anything is read.  The pools are reserved once for the total
 *     (swz_tiler_reserve), so nothing grows while a batch is in flight.  Per batch: reader threads (option
 *     SWZ_INPUT_READER_THREADS; default: the host's, at most 32) pread the raw record ranges of the batch's segments back to
 *     back into one of TWO page-locked buffers, the tiler's copy stream moves the buffer into one of two device buffers
 *     and decodes it there with the segment kernel STRAIGHT into the pool rows of the batch (positions and the masked
 *     columns, spilled pools included), and the batch is tiled as swz_tiler_tile_staged does -- read, copy and decode of
 *     batch k + 1 run beside the tiling of batch k.  Host and device hold two raw batch images at most, whatever the size
 *     of the data set.  A read that fails stops the stream after the running batch and is reported by the file's name.  A
 *     failure before the first batch leaves the tiler untouched, a later one poisons it as a failed staged batch does.
 *     The call does not finalize.  stats (may be NULL): read_ms the reader threads', copy_ms and decode_ms the copy
 *     stream's, tile_ms the tiling calls', wait_ms the time tiling waited for its input, each summed over the batches. */
enum { SWZ_LAS_FILE_OK = 0, SWZ_LAS_FILE_UNREADABLE = 1, SWZ_LAS_FILE_BAD_HEADER = 2, SWZ_LAS_FILE_COMPRESSED = 3 };
#define SWZ_LAS_SCAN_SKIP_UNREADABLE 1u
typedef struct {
  uint64_t point_count;
  uint64_t offset_to_point_data;
  swz_las_layout layout;
  uint32_t attribute_mask; /* bits SWZ_ATTR_* */
  int32_t status;          /* SWZ_LAS_FILE_* */
} swz_las_file_info;
typedef struct {
  uint64_t total_points;
  uint64_t readable_files;
  double tight_min[3], tight_max[3];
  double cubic_min[3], cubic_max[3];
  double origin_min[3], origin_max[3]; /* the cubic box at the origin */
  double center[3];                    /* the cubic box's centre: what shift_to_center subtracts */
  uint32_t attribute_mask;             /* common to all readable files */
  uint32_t reserved;
} swz_las_dataset;
int swz_las_scan_files(swz_ctx* ctx, const char* const* paths, uint64_t num_files, uint32_t flags,
                       swz_las_file_info* files_out, swz_las_dataset* dataset_out);
int swz_input_batches(uint64_t num_files, const uint64_t* file_count, uint64_t batch_points, uint64_t min_last,
                      uint64_t max_batches, uint64_t* first_point_out, uint64_t* num_batches_out);
typedef struct {
  uint64_t first_row;   /* output row of the segment's first record */
  uint64_t count;       /* records */
  uint64_t byte_offset; /* of the first record in d_raw */
  swz_las_layout layout;
} swz_las_segment;
uint32_t swz_las_input_tile(void); /* points one workgroup takes; tests place their edges by it */
int swz_las_decode_segments_device(swz_ctx* ctx, const uint8_t* d_raw, uint64_t raw_bytes, uint64_t num_segments,
                                   const swz_las_segment* segments /* host */, const double shift_center[3] /* or NULL */,
                                   double* d_xyz_out, const swz_attribute_columns* d_out);
typedef struct {
  uint64_t batch_points;   /* 0 = 10 M */
  uint32_t attribute_mask; /* bits SWZ_ATTR_*; ~0u = every attribute the files have in common */
  uint32_t shift_to_center;
  uint32_t flags;          /* SWZ_LAS_SCAN_* */
  uint32_t reserved;
} swz_input_params;
typedef struct {
  uint64_t files, points, batches, bytes_read;
  double read_ms, copy_ms, decode_ms, tile_ms, wait_ms, wall_ms;
} swz_input_stats;
int swz_tiler_add_las_files(swz_tiler* tiler, const char* const* paths, uint64_t num_files, const swz_input_params* params,
                            swz_input_stats* stats);
/* ---- a written data set converted to another format in ONE call: the reference's --converter mode
 * (core/process/ConverterProcess.cpp).  Tile once into the lossless format (BIN keeps the doubles and all twelve columns),
 * derive the delivery formats from those files, optionally down to a maximum depth, never tile again.
 *   properties.json (host; ctx only carries the error text and may be NULL): what write_properties_json writes
 *     (TilerProcess.cpp:76-151) and parse_properties_json reads (ConverterProcess.cpp:55-99), same names and nesting:
 *     {"source_properties":{"bounds":{"min":[x,y,z],"max":[x,y,z]},"root_spacing":s,"processed_points":n},
 *      "performance_stats":{"prepare_duration":0,"indexing_duration":0}}.  Numbers are the shortest text that parses back to
 *     the same double; root_spacing is the float widened to double, as rapidjson writes it.  swz_properties_json_read is the
 *     inverse (any output may be NULL).  swz_tiler_write_properties fills the file from the tiler's root box, spacing and
 *     point count.  swz_tiler_write_output writes no such file: the file comes from a call of its own.
 *   swz_dataset_scan (host, no GPU): what find_all_octree_node_files (:296-323) and the two metadata parsers find in dir.
 *     The format is that of the node files: dir/r*.bin | r*.binz | r*.las | r*.pnts, or dir/ept-data/D-X-Y-Z.las; two kinds
 *     together or none is SWZ_ERR_BAD_ARG.  A name becomes (level, Morton index), level -1 for "r"; a file with a node
 *     extension whose stem is no node name is refused by name (OURS: the reference prints a message and skips it).
 *     max_depth < 0: every node; else the nodes of depth (level + 1) <= max_depth, 0 is the root alone.  The table is
 *     ordered by (level, Morton index) like swz_tiler_node_table; the counts are the file headers' (swz_bin_read_header,
 *     swz_las_read_header; of a BINZ file the first 12 inflated bytes; of a .pnts file swz_pnts_read_header).  The attribute
 *     mask -- the BIN bit mask, or what the LAS point format carries (everything but normals; RGB with formats 2 and 3, GPS
 *     time with 1 and 3) -- must be the same in every file, else the first file that differs is named.  root_source says
 *     where root_min / root_max / spacing_at_root come from: properties.json, else ept.json (bounds, x extent / span), else
 *     SWZ_DATASET_ROOT_ABSENT.  The table outputs may be NULL (then only *num_nodes_out and the info); max_nodes too small
 *     is SWZ_ERR_BAD_ARG.  A .laz file and a cloud.js without node files are refused by name: neither is read.
 *   swz_bin_unpack_segments_device: the inverse of swz_bin_pack_device, shaped like swz_las_decode_segments_device.  Segment
 *     s is one uncompressed BIN file image -- 12 bytes of mask and count, count x 24 bytes of positions, the arrays of the
 *     segment's mask in file order (scan angle rank before scan direction flag) -- that starts at byte_offset of d_raw AT
 *     ANY ALIGNMENT and goes to the output rows [first_row, first_row + count).  Row first_row + i of d_xyz_out and of every
 *     column of d_out whose bit is in the segment's mask gets the file's value, a column of d_out outside the segment's mask
 *     zeros for the segment's rows; columns absent from d_out are skipped, d_xyz_out may be NULL.  One kernel: a workgroup
 *     takes swz_bin_unpack_tile() consecutive rows whatever segments they belong to, reads the segment table once into LDS
 *     and searches it there; array by array the aligned words that cover the tile's part of it are loaded into LDS -- whole
 *     words only where they lie inside [d_raw, d_raw + raw_bytes), single bytes at the two ends -- and every lane takes its
 *     row's value from there as integer words: nothing is computed, NaN payloads and -0.0 survive.  No byte of an output row
 *     depends on what the buffers held.  Output columns are aligned to their element (8 bytes positions and GPS times, 4
 *     normals, 2 intensities and point source ids).  SWZ_ERR_BAD_ARG before anything is launched for: rows that do not
 *     ascend contiguously from 0, a segment whose image passes raw_bytes, a mask bit that does not exist, more than 2^32 -
 *     65536 rows.  Zero segments or zero rows launches nothing.  The kernel trusts the table: whoever reads the files checks
 *     their 12-byte headers against it (swz_convert_dataset does).
 *   swz_pnts_unpack_segments_device: the inverse of swz_pnts_pack_device, shaped like swz_bin_unpack_segments_device.  A
 *     segment names where its arrays lie in d_raw (swz_pnts_parse_image's offsets plus the file's place in the image), each
 *     AT ANY BYTE ALIGNMENT and in any order.  Row first_row + i of d_xyz_out gets (double)f of the three stored floats --
 *     exact, nothing is added, the sign of zero, denormals and infinities survive, a NaN stays a NaN --, its RGB column the
 *     three stored bytes, its intensity column the stored u16; a column of d_out outside the segment's mask gets zeros for
 *     the segment's rows, any other column in d_out is refused (the format cannot carry it), d_xyz_out may be NULL.  One
 *     kernel with the staging of the BIN unpack (swz_pnts_unpack_tile() rows per workgroup; whole dwords only inside [d_raw,
 *     d_raw + raw_bytes), single bytes at the two ends); the widened positions of a tile are put together in LDS and leave
 *     as consecutive 16-byte pieces.  SWZ_ERR_BAD_ARG before anything is launched for: rows that do not ascend contiguously
 *     from 0, an array that passes raw_bytes, a mask bit outside RGB | INTENSITY, reserved != 0, an output column the format
 *     lacks, more than 2^32 - 65536 rows.  Zero segments or zero rows launches nothing.
 *   swz_convert_dataset: scans src_dir, refuses what can be refused before anything is written -- what
 *     swz_tiler_write_output refuses of `out`, a 3DTILES source without SWZ_CONVERT_LOSSY_SOURCE in source_flags (its
 *     positions are floats and it carries no attribute beyond RGB and intensity: converting it is opt-in; the flag does
 *     nothing for another source, any other bit is refused), a 3DTILES source whose files do not all carry the same
 *     RTC_CENTER (a data set of swz_convert_dataset_world; the first file that differs is named), dst_dir equal to src_dir, a mask outside the source's, no root box and spacing from the metadata
 *     files or the parameters, reserved words that are not 0 --, plans the target layout for the (depth-limited) table from
 *     the source's root box and spacing, and streams chunks of whole consecutive nodes of at most out.chunk_points points
 *     (the cuts of swz_output_chunks): reader threads (SWZ_INPUT_READER_THREADS) read the chunk's files back to back, each
 *     at a multiple of 8, into one of two page-locked buffers (BINZ files are inflated into it, LAS files contribute their
 *     record ranges, BIN headers are checked against the scanned table, .pnts files are read whole, run through
 *     swz_pnts_parse_image and checked against the scanned table), a copy stream moves the buffer to the device, the
 *     unpack kernel (LAS sources: the segment kernel of swz_las_decode_segments_device, one layout per file, so the result
 *     is swz_las_read_node's; .pnts sources: swz_pnts_unpack_segments_device's kernel, so the result is swz_pnts_read_node's
 *     and nothing is inferred from the source's RTC_CENTER) fills chunk-local positions and columns, and the target format's pack kernel, the copy back
 *     and the writer threads (SWZ_BIN_WRITER_THREADS) produce the files exactly as swz_tiler_write_output does, tight
 *     bounds included.  Chunk k + 1 is read while chunk k is packed and written.  Device and host hold a bounded number of
 *     chunk images whatever the size of the data set; row numbers are chunk-local, so a data set may hold more than 2^32
 *     points: only a chunk, and therefore a node, is bound by 2^32 - 65536.  At the end: the format's metadata for the
 *     table as swz_tiler_write_output writes it, and properties.json into dst_dir for every target (processed_points: the
 *     converted table's total).  out.attribute_mask: a subset of the source's, ~0u = all it has.  root_given != 0:
 *     root_min / root_max / spacing_at_root override the metadata files.  A file that changed since the scan or cannot be
 *     read stops the stream after the running chunk and is reported by name.  The call never writes to or deletes from
 *     src_dir.  --source-projection inside the converter is swz_convert_dataset_world (below, behind the projection).  Not
 *     offered (the reference's --delete-source, LAZ or cloud.js sources, a multi-GPU driver): delete what you no
 *     longer need yourself. */
enum { SWZ_DATASET_ROOT_ABSENT = 0, SWZ_DATASET_ROOT_PROPERTIES = 1, SWZ_DATASET_ROOT_EPT = 2 };
typedef struct {
  int32_t format;          /* SWZ_OUT_* */
  uint32_t attribute_mask; /* bits SWZ_ATTR_*, the same in every file */
  uint32_t root_source;    /* SWZ_DATASET_ROOT_* */
  float spacing_at_root;
  double root_min[3], root_max[3];
  uint64_t num_nodes, points; /* of the (depth-limited) table */
  int32_t max_level;          /* deepest level of the table; -1: the root alone, or no node */
  uint32_t reserved;
} swz_dataset_info;
typedef struct {
  uint64_t first_row;   /* output row of the segment's first point */
  uint64_t count;       /* points */
  uint64_t byte_offset; /* of the file image in d_raw */
  uint32_t mask;        /* bits SWZ_ATTR_*: the arrays the image holds */
  uint32_t reserved;
} swz_bin_segment;
typedef struct {
  uint64_t first_row, count;                              /* output rows [first_row, first_row + count) */
  uint64_t position_offset, rgb_offset, intensity_offset; /* absolute in d_raw, any byte alignment */
  uint32_t mask;                                          /* SWZ_PNTS_RGB | SWZ_PNTS_INTENSITY: the arrays the segment holds */
  uint32_t reserved;                                      /* 0 */
} swz_pnts_segment;
enum { SWZ_CONVERT_LOSSY_SOURCE = 1u }; /* admits a 3DTILES source: float positions, RGB and intensity only */
typedef struct {
  swz_output_params out;
  int32_t max_depth;   /* < 0: every node */
  uint32_t root_given; /* != 0: root_min, root_max and spacing_at_root below override the metadata files */
  double root_min[3], root_max[3];
  float spacing_at_root;
  uint32_t source_flags; /* SWZ_CONVERT_* */
  uint32_t reserved[2];  /* 0 */
} swz_convert_params;
typedef struct {
  uint64_t nodes, points, bytes_read, bytes_written, chunks;
  double read_ms, unpack_ms, pack_ms, copy_ms, write_ms, wall_ms;
} swz_convert_stats;
int swz_properties_json_write(swz_ctx* ctx, const char* dir, const double root_min[3], const double root_max[3],
                              float spacing_at_root, uint64_t processed_points);
int swz_properties_json_read(swz_ctx* ctx, const char* dir, double root_min_out[3], double root_max_out[3], float* spacing_out,
                             uint64_t* points_out);
int swz_tiler_write_properties(swz_tiler* tiler, const char* dir);
int swz_dataset_scan(swz_ctx* ctx, const char* dir, int32_t max_depth, swz_dataset_info* info_out, uint64_t max_nodes,
                     int8_t* node_level_out, uint64_t* node_key_out, uint64_t* node_count_out, uint64_t* num_nodes_out);
/* swz_dataset_scan without a context: the text of a refusal goes into why_out (why_bytes bytes, may be NULL) */
int swz_dataset_scan_why(const char* dir, int32_t max_depth, swz_dataset_info* info_out, uint64_t max_nodes, int8_t* node_level_out,
                         uint64_t* node_key_out, uint64_t* node_count_out, uint64_t* num_nodes_out, char* why_out, uint64_t why_bytes);
uint32_t swz_bin_unpack_tile(void); /* rows one workgroup takes; tests place their edges by it */
int swz_bin_unpack_segments_device(swz_ctx* ctx, const uint8_t* d_raw, uint64_t raw_bytes, const swz_bin_segment* segments /* host */,
                                   uint64_t num_segments, double* d_xyz_out, const swz_attribute_columns* d_out);
uint32_t swz_pnts_unpack_tile(void); /* rows one workgroup takes */
int swz_pnts_unpack_segments_device(swz_ctx* ctx, const uint8_t* d_raw, uint64_t raw_bytes, const swz_pnts_segment* segments /* host */,
                                    uint64_t num_segments, double* d_xyz_out, const swz_attribute_columns* d_out);
int swz_convert_dataset(swz_ctx* ctx, const char* src_dir, const char* dst_dir, const swz_convert_params* params,
                        swz_convert_stats* stats);
/* ---- a written data set queried: the points of a closed box down to a chosen depth, selected on the device.
 *   swz_box_select_device: the stable compaction of the rows with box_min[a] <= p[a] <= box_max[a] on all three axes -- plain
 *     double compares on the stored positions, no tolerance, a NaN coordinate is outside.  Output row i is the i-th selected
 *     input row: its position, every column of attribute_mask (rows of 1, 2, 3, 8 and 12 bytes; columns aligned to their
 *     element as for swz_bin_unpack_segments_device) and, where d_row_out is given, its input row number.  Two launches
 *     around the library's scan: a count per tile of swz_box_select_tile() rows (wave ballot and popcount), the exclusive
 *     scan of the tile counts, whose total the host reads, and a scatter that evaluates the predicate again, ranks inside
 *     the tile and stores the tile's compacted positions out of LDS as consecutive words.  No atomic decides a place: the
 *     same bytes on every run.  Exactly the rows [0, *count_out) of every output are written, nothing is read from them.
 *     d_xyz_out == NULL with capacity == 0 counts only.  *count_out > capacity is SWZ_ERR_BAD_ARG ("capacity ..."):
 *     *count_out holds the needed number and no byte of the outputs is touched.  SWZ_ERR_BAD_ARG before anything is
 *     launched for: n above 2^32 - 65536, a mask bit that does not exist or lacks its input or (unless counting) output
 *     column, box_min > box_max or a bound that is not finite, an output (capacity rows) that overlaps an input (n rows),
 *     a misaligned array.  n == 0 launches nothing and counts 0.
 *   swz_dataset_query_nodes (host; ctx only carries the error text): the nodes of dir a query reads, in the scanned table's
 *     order (level, Morton index).  Depth is as swz_dataset_scan counts it.  A node is dropped only if its box cannot hold a
 *     point of the query box: the box is swz_node_bounds on the root box of properties.json / ept.json, widened on every
 *     face by two key cells (2^-20 of the root's side: positions are tiled by their key, whose cell edges are rounded) and
 *     by the rounding of its own bounds; for LAS sources also by the file's scale on that axis (stored points are rounded
 *     to the scale's grid), for a 3DTILES source moved by the files' RTC_CENTER -- the stored positions are relative to it
 *     -- and widened by the float rounding of the bounds.  points_bound_out: the sum of the kept nodes' counts, the
 *     capacity that always suffices.  level_out / key_out / count_out may all be NULL (only the numbers), else max_nodes
 *     must hold the kept nodes.  Refused: everything swz_dataset_scan and swz_convert_dataset refuse of a source (LAZ,
 *     cloud.js, a 3DTILES source without SWZ_CONVERT_LOSSY_SOURCE, .pnts files whose RTC_CENTER differ, ...), a source
 *     without a root box, box_min > box_max or a bound that is not finite, an unknown bit in source_flags, reserved != 0.
 *   swz_dataset_query: streams the kept nodes as swz_convert_dataset streams its source -- chunks of whole nodes of at most
 *     chunk_points points (0: the default of swz_output_params), reader threads into two page-locked images, the copy
 *     stream, the source format's unpack into chunk-local arrays, chunk j + 1 read while chunk j is selected -- and runs
 *     swz_box_select_device on every chunk into the caller's arrays at the running offset.  The output order is the node
 *     table's, then the file's: defined byte for byte.  attribute_mask: a subset of the source's, ~0u = all it holds.
 *     d_node_out (may be NULL): per output point the index of its node in swz_dataset_query_nodes' table.  If the running
 *     total would pass capacity the stream stops after that chunk's count with the "capacity" refusal (*count_out: the
 *     total up to and including that chunk); nothing is written at or beyond capacity rows.  d_xyz_out == NULL with
 *     capacity == 0 counts only.  A file that changed since the scan or cannot be read stops the stream and is named.
 *     Device and host hold two raw images and one set of chunk-local arrays whatever the data set's size.
 *   A region (swz_region; swz_region_select_device, swz_dataset_query_region_nodes[_why], swz_dataset_query_region) is the
 *     closed box of the call cut by one more test on the stored positions.  A row is in the region iff it passes the box test
 *     above AND the test of the region's kind -- the box test keeps NaN coordinates out of the kind tests.  Every *, + and -
 *     below is ONE rounded double operation, in the order written (no fused multiply-add, no tolerance, no division):
 *       SWZ_REGION_BOX (count 0, values ignored; so is region == NULL): nothing more -- the bytes of the box calls.
 *       SWZ_REGION_PLANES, 1..SWZ_REGION_MAX_PLANES rows (a, b, c, d): for every plane  ((a*x + b*y) + c*z) + d >= 0.
 *         A frustum is six.  A row whose expression is exactly 0 is in.
 *       SWZ_REGION_POLYGON, 3..SWZ_REGION_MAX_VERTICES vertices (x, y) of one outline in the x-y plane, extruded over the
 *         box's z range; even-odd rule, so concave and self-intersecting outlines are defined.  With vertex i = (x0, y0) and
 *         vertex (i+1) mod m = (x1, y1), edge i counts for the row (px, py, .) iff  (y0 > py) != (y1 > py)  and, with
 *         t = (x1 - x0)*(py - y0) - (px - x0)*(y1 - y0),  (t > 0) == (y1 > y0).  The row is inside iff an odd number of
 *         edges count.  Rows on an edge, on a vertex or level with a vertex are decided by exactly that: a horizontal edge
 *         never counts (its two compares agree); a row level with a vertex sees the vertex on one side only (y > py is
 *         false for it on both edges that share it), so a crossing there is counted once, not twice; reversing an edge
 *         negates t and swaps y0, y1, so both vertex orders give the same set for every row with t != 0 on the edges whose
 *         y range holds it -- a row exactly ON a non-horizontal edge (t == 0) counts that edge iff it runs downwards
 *         (y1 < y0), which makes such rows outside for a counter-clockwise simple outline and inside for a clockwise one.
 *     values is HOST memory, read before the call returns.  Coordinates are the stored ones: for a 3DTILES source relative to
 *     the files' RTC_CENTER, as the box.  SWZ_ERR_BAD_ARG with a message, before anything is launched or any file is read:
 *     an unknown kind, reserved != 0, a count outside 1..16 (planes) or 3..1024 (polygon) or not 0 (box), values == NULL, a
 *     coefficient or vertex that is not finite, a plane with a = b = c = 0.
 *   swz_region_select_device is swz_box_select_device with a region: the same output order, count-only mode, capacity refusal
 *     that touches no output, aliasing and alignment refusals, n == 0 and determinism.  Planes travel in the kernel
 *     arguments; a polygon's vertices are uploaded once per call and staged in LDS by every workgroup of the count pass (a
 *     lane runs the edge loop only if its row passed the box test).  For these two kinds the count pass stores every wave's
 *     ballot (8 bytes per 64 rows) and the scatter reads it back: the predicate is evaluated once per row.
 *   swz_dataset_query_region_nodes / swz_dataset_query_region are swz_dataset_query_nodes / swz_dataset_query with a region,
 *     word for word; the vertices are uploaded once per query.  The node rule starts from the same widened node box and drops
 *     a node iff it misses the query box or cannot hold a row the kind's test accepts: for planes, if for some plane the
 *     largest value of its expression over the widened box (the corner the coefficients' signs choose) plus a bound on the
 *     expression's rounding is < 0; for a polygon, if no edge touches the widened x-y rectangle (segment against rectangle,
 *     widened again by the rounding of t) and the rectangle's centre is outside by the formula above.  The rule errs
 *     towards reading a file.
 *   A filter (swz_filter; swz_filter_check, swz_filter_select_device, swz_dataset_query_filtered) is a predicate over the
 *     attribute columns, evaluated behind the region: a row is selected iff it is in the region AND passes EVERY one of the
 *     filter's 1..SWZ_FILTER_MAX_CLAUSES clauses.  Two clauses may name the same attribute.  count == 0 and filter == NULL both
 *     mean no filter: the bytes of the region calls.  A clause tests the value v its `attribute` column holds for the row:
 *       SWZ_FILTER_RANGE, on every scalar column -- INTENSITY and POINT_SOURCE_ID (uint16), GPS_TIME (double),
 *         SCAN_ANGLE_RANK (int8, compared as its signed value) and the uint8 columns: v is converted to double, which is
 *         exact for every one of these types, and the row passes iff  lo <= (double)v && (double)v <= hi,  two plain double
 *         compares, closed at both ends.  lo and hi may be -infinity and +infinity, which gives an open end.  A NaN GPS time
 *         fails both compares, so it fails a RANGE and passes a RANGE with SWZ_FILTER_NOT.
 *       SWZ_FILTER_SET, on the one-byte columns only: the row passes iff bit b of the 256-bit map is set, b the stored byte
 *         read as unsigned (bit b is bit b % 64 of set[b / 64]); scan-angle rank -1 is bit 255.
 *       SWZ_FILTER_NOT in `kind` inverts the clause's test.
 *     The fields a kind does not use are 0, so that they can mean something later.  SWZ_ERR_BAD_ARG with a message that names
 *     the clause ("clause 3: ..."), before anything is launched or any file is read: count > 8, reserved != 0, an attribute
 *     outside the table, SWZ_ATTR_RGB or SWZ_ATTR_NORMAL (not scalars), an unknown kind or flag bit, SET on a column wider
 *     than a byte, a RANGE with lo > hi or a NaN bound, a SET with a nonzero lo or hi, a RANGE with a nonzero set.
 *     swz_filter_check is the one place these rules live (host only, no context; the text goes into why_out, which may be
 *     NULL); every call that takes a filter goes through it.
 *   swz_filter_select_device is swz_region_select_device with a filter: the same output order, count-only mode, capacity
 *     refusal that touches no output, aliasing and alignment refusals, n == 0 and determinism.  d_in must hold every column
 *     that attribute_mask OR the filter names, d_out every column attribute_mask names; a filtered column outside
 *     attribute_mask is read and never written.  With a filter the count pass of all three kinds is one kernel: a lane does the
 *     box test, then the kind's test, then the clauses in order, and loads a clause's column element only while its row is
 *     still in -- rows outside the region cost no column traffic.  The filter travels in the kernel arguments; the ballots go
 *     to the scatter of the region call, so every test, the box's included, is evaluated once per row.
 *   swz_dataset_query_filtered is swz_dataset_query_region with a filter.  The stream unpacks attribute_mask | the filter's
 *     attributes into its chunk-local arrays and hands the caller attribute_mask (~0u: all the source holds).  The filter sees
 *     exactly the values an unfiltered query of that source returns (a LAS source: what its decode yields).  Refused before any
 *     file of points is read: a filtered attribute the source does not hold (named, with the source's mask) and, for a
 *     3DTILES source, any filtered attribute .pnts files do not carry.  The node table is swz_dataset_query_region_nodes',
 *     d_node_out indexes it, points_bound stays the safe capacity, and points_read less points_out shows what region and filter
 *     refused.  Without node-summaries.swz in dir (below) no node is dropped for a filter.
 *   Per-node attribute summaries let a filtered query skip the node files that cannot contribute a row.
 *     swz_node_summaries_device: n rows in STORED order (chunk-local columns as the unpack kernels leave them, no perm or order),
 *       a host node table checked as swz_node_boxes_device checks its own, and per node and summarised column one
 *       swz_attr_summary in summaries_out (HOST, num_nodes x popcount(attribute_mask) entries; entry (k, j) is node k and the
 *       j-th set bit of the mask in ascending SWZ_ATTR_* order).  Summarised are the scalar columns a filter knows
 *       (SWZ_SUMMARY_SCALARS).  One-byte columns: set holds bit (uint8_t)v of every value of the node, lo / hi are derived from
 *       it on the host (SCAN_ANGLE_RANK as signed: bit 255 is -1, bit 128 is -128).  uint16 columns and GPS_TIME: lo / hi are
 *       the exact min and max as doubles, set is 0; a NaN GPS time is left out of lo / hi and sets SWZ_SUMMARY_HAS_NAN; of
 *       +0.0 and -0.0 either may come back.  A node of count 0, or one whose GPS times are all NaN, has lo = +inf, hi = -inf.
 *       One workgroup takes swz_node_summaries_tile() consecutive rows and handles the columns one after the other: an
 *       element per lane, runs of lanes of one node combined with shuffles, the runs of a node combined in LDS, then per
 *       (tile, node, column) one round of relaxed agent-scope atomics on a table a small kernel preset (64-bit OR, words that
 *       are 0 skipped; 32-bit min / max; 64-bit min / max on order-preserving codes).  OR, min and max are idempotent and
 *       commute: the result is exact and depends neither on what the workspace held nor on any order.  SWZ_ERR_BAD_ARG with
 *       a message before anything is launched: what swz_node_boxes_device refuses of the table, n above 2^32 - 65536, a mask
 *       bit without its column, SWZ_ATTR_RGB, SWZ_ATTR_NORMAL or an unknown bit, a column not aligned to its element.
 *       n == 0, no nodes, only empty nodes or an empty mask launch nothing; the output is preset on the host.
 *     The sidecar is dir/node-summaries.swz (swz_dataset_scan skips extensions it does not know, so readers that ignore it are
 *       not disturbed).  Little-endian: 8 bytes magic "SWZNSUM\0", u32 version 1, u32 format (SWZ_OUT_*), u32 mask, u32 entry
 *       bytes (56), u64 nodes, u64 points, u64 0; then per node in (level, Morton index) order u64 key, u64 count, i8 level and
 *       7 zero bytes; then the entries.  swz_dataset_summaries_write writes it under a temporary name in dir and renames it.
 *       swz_dataset_summaries_read (all arrays NULL: the sizes only; else max_nodes must hold the nodes) checks the exact size
 *       and refuses by name a wrong magic, version, entry size or file size, nodes out of order or twice, a nonzero reserved
 *       field.  A directory without the file is no error: *present_out = 0.  Both are host only and take no context.
 *     swz_dataset_summarize opens dir as the query does (every depth), streams all nodes through the query's stream with the
 *       source's scalar columns unpacked (a 3DTILES source with SWZ_CONVERT_LOSSY_SOURCE: intensity, if the files carry it),
 *       runs swz_node_summaries_device's kernel on every chunk and writes the sidecar at the end: it describes exactly the
 *       values a query of that source sees.  A source without a scalar column gets a sidecar with mask 0.  Refused: what the
 *       query refuses of a source.  Memory as the query.  The writers (swz_tiler_write_output, swz_convert_dataset) do not
 *       write the sidecar: what a LAS target stores is not what the pools hold.
 *     swz_dataset_query_filtered_nodes[_why] (host): swz_dataset_query_region_nodes' table, unchanged and in the same order,
 *       and read_out[k] = 0 for every node the filter cannot reach; points_bound_out: the sum of the counts of the nodes that
 *       are read.  Without a sidecar, with filter == NULL or count == 0, every node is read.  A node is dropped iff SOME
 *       clause has no row of the node that could pass it, judged from that attribute's entry alone.  One-byte column: with P
 *       the 256-bit set of byte values the clause's test accepts (SET: the clause's set; RANGE: the two double compares on
 *       each of the 256 values, signed for the scan-angle rank; with SWZ_FILTER_NOT the complement), drop iff entry.set & P
 *       == 0 -- exact: a single such clause drops a node iff no row passes.  uint16 column or GPS time, RANGE: drop iff
 *       entry.hi < lo || entry.lo > hi (which covers a node without non-NaN values); NOT RANGE: drop iff the node has no NaN
 *       and lo <= entry.lo && entry.hi <= hi.  A clause whose attribute the sidecar's mask lacks drops nothing.  The rule
 *       errs towards reading a file.  Every node of the region table must be found in the sidecar by (level, key) with the
 *       scan's count, and the sidecar must name the scan's format; else the call is refused ("node-summaries.swz is stale:
 *       node r04 holds 120 points, the summary 118 -- run swz_dataset_summarize again"), as is a sidecar that fails its read
 *       checks.  A data set rewritten with equal counts per node cannot be told from the one that was summarised.
 *     swz_dataset_query_filtered applies the rule when the sidecar is there: the dropped nodes are neither read nor chunked.
 *       d_node_out keeps indexing the region table; positions, columns, d_node_out and *count_out are byte for byte what they
 *       are without the sidecar, only nodes_read, points_read, bytes_read, chunks and the times change.
 *   Not offered: a multi-GPU driver, polygons with holes or several rings, a shortcut that copies nodes wholly inside a
 *     region without testing their rows, depth chosen by screen-space error. */
typedef struct {
  double box_min[3], box_max[3]; /* closed */
  int32_t max_depth;             /* < 0: every node; else nodes of depth <= max_depth, as swz_dataset_scan counts depth */
  uint32_t attribute_mask;       /* ~0u: all the source holds */
  uint32_t source_flags;         /* SWZ_CONVERT_LOSSY_SOURCE admits a 3DTILES source, as in the converter */
  uint32_t reserved;             /* 0 */
  uint64_t chunk_points;         /* 0: the library's default, as in swz_output_params */
} swz_query_params;
typedef struct {
  uint64_t nodes_scanned, nodes_read, points_read, points_out, bytes_read, chunks;
  double read_ms, unpack_ms, select_ms, copy_ms, wall_ms;
} swz_query_stats;
uint32_t swz_box_select_tile(void); /* rows one workgroup takes; tests place their edges by it */
int swz_box_select_device(swz_ctx* ctx, const double* d_xyz, uint64_t n, const swz_attribute_columns* d_in, uint32_t attribute_mask,
                          const double box_min[3], const double box_max[3], uint64_t capacity, double* d_xyz_out,
                          const swz_attribute_columns* d_out, uint32_t* d_row_out /* may be NULL: the input row of every output row */,
                          uint64_t* count_out);
int swz_dataset_query_nodes(swz_ctx* ctx, const char* dir, const swz_query_params* params, uint64_t max_nodes, int8_t* level_out,
                            uint64_t* key_out, uint64_t* count_out, uint64_t* num_out, uint64_t* points_bound_out);
/* swz_dataset_query_nodes without a context: the text of a refusal goes into why_out (why_bytes bytes, may be NULL) */
int swz_dataset_query_nodes_why(const char* dir, const swz_query_params* params, uint64_t max_nodes, int8_t* level_out, uint64_t* key_out,
                                uint64_t* count_out, uint64_t* num_out, uint64_t* points_bound_out, char* why_out, uint64_t why_bytes);
int swz_dataset_query(swz_ctx* ctx, const char* dir, const swz_query_params* params, uint64_t capacity, double* d_xyz_out,
                      const swz_attribute_columns* d_out, uint32_t* d_node_out /* may be NULL */, uint64_t* count_out,
                      swz_query_stats* stats);
enum { SWZ_REGION_BOX = 0, SWZ_REGION_PLANES = 1, SWZ_REGION_POLYGON = 2 };
#define SWZ_REGION_MAX_PLANES 16
#define SWZ_REGION_MAX_VERTICES 1024
typedef struct {
  int32_t kind;         /* SWZ_REGION_* */
  uint32_t count;       /* planes or vertices; 0 for SWZ_REGION_BOX */
  const double* values; /* HOST memory: count x (a, b, c, d) or count x (x, y) */
  uint64_t reserved;    /* 0 */
} swz_region;
int swz_region_select_device(swz_ctx* ctx, const double* d_xyz, uint64_t n, const swz_attribute_columns* d_in, uint32_t attribute_mask,
                             const double box_min[3], const double box_max[3], const swz_region* region /* NULL: the box alone */,
                             uint64_t capacity, double* d_xyz_out, const swz_attribute_columns* d_out, uint32_t* d_row_out,
                             uint64_t* count_out);
int swz_dataset_query_region_nodes(swz_ctx* ctx, const char* dir, const swz_query_params* params, const swz_region* region,
                                   uint64_t max_nodes, int8_t* level_out, uint64_t* key_out, uint64_t* count_out, uint64_t* num_out,
                                   uint64_t* points_bound_out);
int swz_dataset_query_region_nodes_why(const char* dir, const swz_query_params* params, const swz_region* region, uint64_t max_nodes,
                                       int8_t* level_out, uint64_t* key_out, uint64_t* count_out, uint64_t* num_out,
                                       uint64_t* points_bound_out, char* why_out, uint64_t why_bytes);
int swz_dataset_query_region(swz_ctx* ctx, const char* dir, const swz_query_params* params, const swz_region* region, uint64_t capacity,
                             double* d_xyz_out, const swz_attribute_columns* d_out, uint32_t* d_node_out /* may be NULL */,
                             uint64_t* count_out, swz_query_stats* stats);
enum { SWZ_FILTER_RANGE = 0, SWZ_FILTER_SET = 1 };
#define SWZ_FILTER_NOT 0x100u /* in `kind`: the clause's test is inverted */
#define SWZ_FILTER_MAX_CLAUSES 8
typedef struct {
  int32_t attribute; /* SWZ_ATTR_* */
  uint32_t kind;     /* SWZ_FILTER_RANGE | SWZ_FILTER_SET, optionally | SWZ_FILTER_NOT */
  double lo, hi;     /* RANGE: lo <= (double)v && (double)v <= hi, closed; SET: 0 */
  uint64_t set[4];   /* SET: bit (uint8_t)v of the 256-bit map; RANGE: 0 */
} swz_filter_clause;
typedef struct {
  uint32_t count;    /* 0: no filter */
  uint32_t reserved; /* 0 */
  swz_filter_clause clause[SWZ_FILTER_MAX_CLAUSES];
} swz_filter;
/* SWZ_OK, or SWZ_ERR_BAD_ARG with the refusal in why_out (why_bytes bytes, may be NULL).  NULL and count == 0 are in order. */
int swz_filter_check(const swz_filter* filter, char* why_out, uint64_t why_bytes);
int swz_filter_select_device(swz_ctx* ctx, const double* d_xyz, uint64_t n, const swz_attribute_columns* d_in, uint32_t attribute_mask,
                             const double box_min[3], const double box_max[3], const swz_region* region /* NULL: the box alone */,
                             const swz_filter* filter /* NULL: no filter */, uint64_t capacity, double* d_xyz_out,
                             const swz_attribute_columns* d_out, uint32_t* d_row_out, uint64_t* count_out);
int swz_dataset_query_filtered(swz_ctx* ctx, const char* dir, const swz_query_params* params, const swz_region* region,
                               const swz_filter* filter, uint64_t capacity, double* d_xyz_out, const swz_attribute_columns* d_out,
                               uint32_t* d_node_out /* may be NULL */, uint64_t* count_out, swz_query_stats* stats);
enum { SWZ_SUMMARY_HAS_NAN = 1u };
/* the columns that are summarised: every scalar column, bits SWZ_ATTR_INTENSITY .. SWZ_ATTR_USER_DATA */
#define SWZ_SUMMARY_SCALARS 0xFFCu
typedef struct {
  double lo, hi;     /* min and max of the node's values as doubles (exact for every scalar type); NaN rows excluded */
  uint64_t set[4];   /* one-byte columns: bit (uint8_t)v for every value the node holds; wider columns: 0 */
  uint32_t flags;    /* SWZ_SUMMARY_HAS_NAN: a GPS time of the node is NaN */
  uint32_t reserved; /* 0 */
} swz_attr_summary;  /* 56 bytes */
typedef struct {
  uint64_t nodes, points, bytes_read, chunks;
  double read_ms, unpack_ms, summary_ms, copy_ms, wall_ms;
} swz_summarize_stats;
uint32_t swz_node_summaries_tile(void); /* rows one workgroup takes; tests place their edges by it */
int swz_node_summaries_device(swz_ctx* ctx, uint64_t n, const swz_attribute_columns* d_in, uint32_t attribute_mask, uint64_t num_nodes,
                              const uint64_t* node_offset, const uint64_t* node_count, swz_attr_summary* summaries_out);
int swz_dataset_summaries_write(const char* dir, int32_t format, uint32_t mask, uint64_t num_nodes, const int8_t* level,
                                const uint64_t* key, const uint64_t* count, const swz_attr_summary* entries, char* why_out,
                                uint64_t why_bytes);
int swz_dataset_summaries_read(const char* dir, int32_t* present_out, int32_t* format_out, uint32_t* mask_out, uint64_t* num_nodes_out,
                               uint64_t* points_out, uint64_t max_nodes, int8_t* level_out, uint64_t* key_out, uint64_t* count_out,
                               swz_attr_summary* entries_out, char* why_out, uint64_t why_bytes);
int swz_dataset_summarize(swz_ctx* ctx, const char* dir, uint32_t source_flags, uint64_t chunk_points, swz_summarize_stats* stats);
int swz_dataset_query_filtered_nodes(swz_ctx* ctx, const char* dir, const swz_query_params* params, const swz_region* region,
                                     const swz_filter* filter, uint64_t max_nodes, int8_t* level_out, uint64_t* key_out,
                                     uint64_t* count_out, uint8_t* read_out, uint64_t* num_out, uint64_t* points_bound_out);
int swz_dataset_query_filtered_nodes_why(const char* dir, const swz_query_params* params, const swz_region* region,
                                         const swz_filter* filter, uint64_t max_nodes, int8_t* level_out, uint64_t* key_out,
                                         uint64_t* count_out, uint8_t* read_out, uint64_t* num_out, uint64_t* points_bound_out,
                                         char* why_out, uint64_t why_bytes);
/* ---- a written data set rasterized: per cell of a grid in x-y the count, min, max and mean of a value of the selected rows,
 * accumulated on the device in integers.  The result is a few MB whatever the number of rows, and bit-exact: it depends on
 * no order, on no chunking and -- where the formats store the same values -- on no format.
 *   The grid (swz_raster_grid) has nx x ny cells over the x-y rectangle of the query's closed box [box_min, box_max].  All six
 *     bounds must be finite with box_min[i] <= box_max[i].  cw = (box_max[0] - box_min[0]) / nx and ch = (box_max[1] -
 *     box_min[1]) / ny are computed once, on the host.  A row (x, y, z) that the selection keeps falls into
 *       ix = min((uint32)floor((x - box_min[0]) / cw), nx - 1),  iy = min((uint32)floor((y - box_min[1]) / ch), ny - 1),
 *     cell iy * nx + ix: iy ascends with y.  The subtraction, the division and the floor are three separately rounded double
 *     operations (the library is built without contraction; numpy reproduces them bit for bit).  A row on box_max lands in the
 *     last cell, because the box is closed.  An axis with box_max == box_min has a cell size of 0: that is taken only with ONE
 *     cell along that axis, whose index is then 0 without a division; with more cells it is refused.
 *   The value v (swz_raster_grid::value): SWZ_RASTER_VALUE_Z (-1), the row's z, or a scalar attribute of one or two bytes --
 *     SWZ_ATTR_INTENSITY, SWZ_ATTR_POINT_SOURCE_ID or a one-byte column; SWZ_ATTR_SCAN_ANGLE_RANK is read as signed -- whose
 *     element becomes a double as a filter's RANGE clause makes it one (exact).  SWZ_ATTR_GPS_TIME, SWZ_ATTR_RGB and
 *     SWZ_ATTR_NORMAL are refused by name.
 *   Per cell one swz_raster_cell (32 bytes):
 *       count     the rows of the cell.
 *       sum       the sum of q = llrint((v - v0) * scale) over them (round to nearest, ties to even).  z: v0 = box_min[2] and
 *                 scale = 2^k, k = 0 for range = box_max[2] - box_min[2] == 0, else k = 30 - ilogb(range) clamped to
 *                 [-900, 900], so that 2^30 <= range * scale < 2^31 without the clamp.  An attribute: v0 = 0, scale = 1, q is the
 *                 element.  |q| < 2^31 and a call holds at most 2^32 - 1 rows, hence |sum| < 2^63: a data set whose read nodes
 *                 hold more rows is refused before a node file is read.
 *       min_code, max_code   the smallest and the largest v as ORDER-PRESERVING codes: of the double's 64 bits b, ~b for a
 *                 negative and b | 2^63 otherwise, so the codes ascend with the values and -0.0 lies just below +0.0.  They are
 *                 preset to the codes of +inf (0xFFF0000000000000) and -inf (0x000FFFFFFFFFFFFF).
 *     swz_raster_frame holds what a kernel and a reader of the table need: x0, y0, cw, ch, v0, scale, nx, ny, value.
 *   swz_raster_frame_of (host only, no context: it runs on a machine without a GPU) checks the inputs and derives the frame.
 *     SWZ_ERR_BAD_ARG with the text in why_out (why_bytes bytes, may be NULL), by name: nx or ny equal to 0, nx * ny above
 *     SWZ_RASTER_MAX_CELLS, a bound that is not finite, box_min > box_max, a flat axis with more than one cell, a value the
 *     raster does not take, reserved != 0.
 *   swz_raster_finish (host only) decodes a table of frame->nx * frame->ny cells into arrays of as many elements (each may be
 *     NULL): count; min and max, exact -- of +0.0 and -0.0 either may come back --; and
 *       mean = v0 + ((double)sum / (double)count) / scale,  three separately rounded operations.
 *     An empty cell has count 0, min +inf, max -inf and mean NaN.  q is off (v - v0) * scale by half a unit at the most, so
 *     mean is off the exact mean of the doubles by at most half a step, 1 / (2 scale) <= range * 2^-31 (z; an attribute's sum
 *     is exact), and by the rounding of its own three operations.
 *   swz_raster_clear_device presets the nx * ny cells of d_cells (a small kernel on the context's stream).
 *   swz_raster_accumulate_device ADDS n rows to d_cells and does not clear it: that is how chunks accumulate.  d_value is the
 *     value's column (NULL for z).  One workgroup takes swz_raster_tile() consecutive rows, one per lane, and applies the closed
 *     box test of swz_box_select_device to x, y and z itself: a NaN is outside, rows outside the box are skipped, and the clamp
 *     keeps every index inside the table whatever the input holds.  Stored rows are close to Morton order, so neighbouring
 *     lanes often share a cell: a lane whose cell differs from the lane below it (a shuffle) heads a run, an outside lane
 *     breaks one; the runs of a wave are reduced with segmented shuffles over count, sum, min code and max code, and the head
 *     of a run issues four relaxed agent-scope 64-bit atomics: add, add, min, max.  Integer add, min and max commute: the table
 *     depends on no order.  SWZ_ERR_BAD_ARG with a message before anything is launched: n above 2^32 - 65536, a NULL d_xyz
 *     with n > 0, an attribute value without its column or with a misaligned one, misaligned positions or cells, a frame that
 *     swz_raster_frame_of does not produce from box_min, box_max and the frame's nx, ny and value.  n == 0 launches nothing.
 *     Both synchronise the context's stream.
 *   swz_dataset_rasterize: the rows swz_dataset_query_filtered selects for params, region and filter (each of the two may be
 *     NULL), rastered into cells_out (HOST, nx * ny cells); frame_out receives the frame.  Planning is the query's: the same
 *     refusals, the same node rule, the same use of node-summaries.swz when it is there.  The stream unpacks only what is
 *     needed -- the filter's columns and the value's -- never the caller's columns: params->attribute_mask must be 0 or ~0u
 *     and is ignored.  Refused before a file of points is read: a value attribute the source does not hold (named, with the
 *     source's mask) and, for a 3DTILES source, any value .pnts files do not carry.  Per chunk: the box alone (no region, no
 *     filter) runs the accumulate kernel straight on the chunk-local arrays, one pass and nothing compacted; otherwise
 *     swz_filter_select_device's selection compacts positions and the value column into the workspace and the kernel runs on
 *     the compacted rows.  The table lives in the workspace, is cleared once before the first chunk and copied out after the
 *     last.  stats: points_out is the sum of the counts, select_ms the time of the chunks' bodies.  A file that cannot be read
 *     stops the stream and is named, as for the query; cells_out is then unspecified.
 *   Not offered: GPS time or colours as values, percentiles, a multi-GPU driver, grid files (GeoTIFF, ASCII). */
#define SWZ_RASTER_VALUE_Z (-1)
#define SWZ_RASTER_MAX_CELLS (1u << 26)
typedef struct {
  uint32_t nx, ny;   /* cells along x and y */
  int32_t value;     /* SWZ_RASTER_VALUE_Z or SWZ_ATTR_* */
  uint32_t reserved; /* 0 */
} swz_raster_grid;   /* 16 bytes */
typedef struct {
  double x0, y0;     /* box_min[0], box_min[1] */
  double cw, ch;     /* the cell's sides; 0 along a flat axis */
  double v0, scale;  /* q = llrint((v - v0) * scale) */
  uint32_t nx, ny;
  int32_t value;
  uint32_t reserved; /* 0 */
} swz_raster_frame;  /* 64 bytes */
typedef struct {
  uint64_t count;
  int64_t sum;
  uint64_t min_code, max_code;
} swz_raster_cell; /* 32 bytes */
uint32_t swz_raster_tile(void); /* rows one workgroup takes; tests place their edges by it */
int swz_raster_frame_of(const double box_min[3], const double box_max[3], const swz_raster_grid* grid, swz_raster_frame* frame_out,
                        char* why_out, uint64_t why_bytes);
int swz_raster_finish(const swz_raster_frame* frame, const swz_raster_cell* cells, uint64_t* count_out, double* min_out, double* max_out,
                      double* mean_out);
int swz_raster_clear_device(swz_ctx* ctx, const swz_raster_frame* frame, swz_raster_cell* d_cells);
int swz_raster_accumulate_device(swz_ctx* ctx, const double* d_xyz, uint64_t n, const void* d_value /* NULL for z */, const double box_min[3],
                                 const double box_max[3], const swz_raster_frame* frame, swz_raster_cell* d_cells);
int swz_dataset_rasterize(swz_ctx* ctx, const char* dir, const swz_query_params* params, const swz_region* region /* may be NULL */,
                          const swz_filter* filter /* may be NULL */, const swz_raster_grid* grid, swz_raster_cell* cells_out /* HOST */,
                          swz_raster_frame* frame_out, swz_query_stats* stats);
/* ---- a source projection (the reference's --source-projection: Proj4Transform, core/util/Transformation.cpp:74-211, source
 * -> "+proj=geocent +datum=WGS84").  PROJ is not linked: the library maps the projection families LAS data comes in itself,
 * in double, and refuses every other definition by name.
 *   swz_srs_parse (host; ctx only carries the error text and may be NULL).  Accepted, as whitespace-separated +key[=value]:
 *     +proj=utm +zone=1..60 [+south] | +proj=tmerc [+lat_0 +lon_0 +k | +k_0 +x_0 +y_0] (degrees, metres; defaults 0, 0, 1, 0, 0)
 *     | +proj=longlat / latlong (x = longitude, y = latitude in degrees, z = ellipsoidal height); the ellipsoid, which must be
 *     given, by +ellps=WGS84|GRS80, +datum=WGS84 or +a with +rf or +b (+ellps beside +datum only when they agree); +units=m,
 *     +no_defs, +type=crs; the shorthands EPSG:32601-32660, EPSG:32701-32760 (WGS 84 / UTM) and EPSG:25828-25838 (ETRS89 /
 *     UTM on GRS80).  On an ellipsoid other than WGS84 the inverse projection runs on THAT ellipsoid; latitude, longitude and
 *     height are then carried unchanged onto WGS84 (no datum shift), and the geocentric step is always WGS84's.
 *     SWZ_ERR_BAD_ARG, naming the token, for everything else: another +proj, +towgs84, +nadgrids, +geoidgrids, +vunits,
 *     +units other than m, +axis, +pm, +approx, any other key, a key a projection does not take (+zone with tmerc, ...),
 *     a key given twice, other EPSG codes (EPSG:4326 too: its axis order differs between PROJ versions, write +proj=longlat
 *     +datum=WGS84), WKT, a zone out of range, ellipsoid parameters that are not finite and positive, no ellipsoid, an
 *     empty string.
 *   The map, per point (swz_srs_transform on the host, swz_srs_transform_device in place on AoS rows of 24 bytes, staged
 *     through LDS by tiles of swz_srs_tile() rows; n = 0 launches nothing, more than 2^32 - 65536 rows are refused): the
 *     inverse transverse Mercator is the Krueger series in the third flattening n to order n^6 (Karney 2011, "Transverse
 *     Mercator with an accuracy of a few nanometers"): false origin and scale removed, the six beta coefficients summed by a
 *     complex Clenshaw recurrence on sin / cos / sinh / cosh of the doubled arguments, longitude = lon_0 + atan2(sinh eta',
 *     cos xi'), conformal -> geodetic latitude by the six-term series in n as well (no iteration: a point far outside the
 *     domain costs what every point costs and yields a meaningless or non-finite value).  The coefficients are computed once,
 *     by swz_srs_parse (tools/srs_series.py derives them).  Geodetic -> ECEF is the closed form.  Targets: SWZ_SRS_ECEF (X,
 *     Y, Z in metres) and SWZ_SRS_WGS84 (longitude and latitude in RADIANS, longitude in [-pi, pi], and the height: the
 *     reference's TargetSRS::WGS84).  Non-finite input gives non-finite output; nothing traps.  Floating-point contraction
 *     is off inside the map, so the device result for given input bits is the same in every kernel it is inlined into.
 *   swz_srs_transform_box (host): the eight corners of the box, corner i = (i & 1 ? max : min).x, (i & 2 ? max : min).y,
 *     (i & 4 ? max : min).z, mapped and then min / max per axis: transformAABBWithProj4 (Transformation.cpp:10-44).  The
 *     image of a flat tile bulges, so a point INSIDE the source box can land a few centimetres OUTSIDE this box.  The
 *     reference has the same property and clamps such a point in place when it indexes it (index_point); so does this
 *     library.  The box is neither widened nor are such points refused.
 *   swz_las_scan_files_srs: swz_las_scan_files with the header box of every readable file sent through
 *     swz_srs_transform_box to ECEF BEFORE it joins the union (TilerProcess::calculate_dataset_metadata,
 *     TilerProcess.cpp:352-387; not the transformed union); cubic, origin box and centre come from that union by the same
 *     arithmetic.  files_out[i].layout keeps the file's own header values: the decode clamps against them in the source CRS,
 *     as the reference's reader does.  srs == NULL is swz_las_scan_files.
 *   swz_las_decode_segments_srs_device: swz_las_decode_segments_device with the map to ECEF after the clamp into the header
 *     box and before the shift (make_tiler, TilerProcess.cpp:539-561), in a kernel instantiation of its own -- the one
 *     without a projection is untouched.  srs == NULL is swz_las_decode_segments_device.
 *   swz_tiler_set_source_srs (NULL clears): swz_tiler_add_las_files then scans with swz_las_scan_files_srs -- the
 *     containment check against the root box and the centre of the shift use the ECEF boxes -- and decodes with the map.
 *     SWZ_ERR_BAD_ARG unless the tiler holds no points and no batch is staged or open: set and clear alike, so a tiler
 *     that has read points with a projection keeps it for its life and every later swz_tiler_add_las_files projects too.  swz_group_set_source_srs: the same
 *     for swz_group_add_las_files, between swz_group_tiler_open and the first batch (the close forgets it). */
enum { SWZ_SRS_LONGLAT = 0, SWZ_SRS_TMERC = 1 };
enum { SWZ_SRS_ECEF = 0, SWZ_SRS_WGS84 = 1 };
typedef struct swz_srs_s {
  int32_t kind; /* SWZ_SRS_LONGLAT / SWZ_SRS_TMERC (utm is a tmerc) */
  int32_t reserved;
  double a, f, e2, n;      /* the source ellipsoid: semi-major axis, flattening, e^2 = f (2 - f), n = f / (2 - f) */
  double lat_0, lon_0;     /* radians */
  double k_0, x_0, y_0;
  double radius;           /* k_0 A, A = a / (1 + n) (1 + n^2/4 + n^4/64 + n^6/256) the rectifying radius */
  double xi_0;             /* the rectifying latitude of lat_0 */
  double beta[6];          /* rectifying -> conformal: chi = mu - sum beta_j sin 2 j mu */
  double delta[6];         /* conformal -> geodetic: phi = chi + sum delta_j sin 2 j chi */
} swz_srs;
int swz_srs_parse(swz_ctx* ctx, const char* definition, swz_srs* out);
/* swz_srs_parse for callers without a context: the refusal's text goes into why_out (why_bytes bytes, cut and terminated) */
int swz_srs_parse_why(const char* definition, swz_srs* out, char* why_out, uint64_t why_bytes);
int swz_srs_transform(const swz_srs* srs, int target, double* xyz, uint64_t n);
uint32_t swz_srs_tile(void); /* rows one workgroup takes at a time; tests place their edges by it */
int swz_srs_transform_device(swz_ctx* ctx, const swz_srs* srs, int target, double* d_xyz, uint64_t n);
int swz_srs_transform_box(const swz_srs* srs, int target, const double min[3], const double max[3], double out_min[3],
                          double out_max[3]);
int swz_las_scan_files_srs(swz_ctx* ctx, const char* const* paths, uint64_t num_files, uint32_t flags, const swz_srs* srs,
                           swz_las_file_info* files_out, swz_las_dataset* dataset_out);
int swz_las_decode_segments_srs_device(swz_ctx* ctx, const uint8_t* d_raw, uint64_t raw_bytes, uint64_t num_segments,
                                       const swz_las_segment* segments /* host */, const double shift_center[3] /* or NULL */,
                                       double* d_xyz_out, const swz_attribute_columns* d_out, const swz_srs* srs /* or NULL */);
int swz_tiler_set_source_srs(swz_tiler* tiler, const swz_srs* srs /* NULL clears */);
/* ---- a written data set converted to georeferenced 3D Tiles: the conversion the reference's --converter mode exists for
 * (convert_to_pnts_file, core/process/ConverterProcess.cpp:505-530).  Tile once in the source CRS into BIN, derive the
 * Cesium tileset from those files.
 *   swz_srs_project_node_boxes_device: n rows of 24 bytes at d_xyz, IN STORED ORDER (no perm or order indirection: the
 *     converter's chunk-local arrays), mapped in place to SWZ_SRS_ECEF, and the exact box of every node's mapped rows, in ONE
 *     launch (plus the preset of the table).  A workgroup stages a tile of swz_srs_tile() rows through LDS as
 *     swz_srs_transform_device does and every lane maps its row with the same inlined map, contraction off: the stored bits
 *     are swz_srs_transform_device's.  The block finds the nodes of its rows like the pack kernels do, a wave reduces the
 *     runs of lanes of one node with shuffles on the order-preserving codes of swz_node_boxes_device, and one 64-bit atomic
 *     min and max per run, axis and wave go into the table, which starts at +inf / -inf.  ALL n rows are mapped, rows
 *     outside every node range included.  node_offset / node_count / box_min_out / box_max_out: host, as in
 *     swz_node_boxes_device; a node of count 0 gets min = +inf, max = -inf.  srs == NULL maps nothing and only reduces.
 *     Refused before anything is launched: what swz_node_boxes_device refuses of the table (SWZ_ERR_BAD_ARG), a struct
 *     swz_srs_parse did not make, more than 2^32 - 65536 rows (SWZ_ERR_TOO_MANY_POINTS).  n == 0, or no node that holds
 *     points and no projection, launches nothing.
 *   swz_convert_dataset_world: swz_convert_dataset for the target SWZ_OUT_3DTILES only, sources BIN, BINZ, LAS,
 *     ENTWINE_LAS and (SWZ_CONVERT_LOSSY_SOURCE) 3DTILES as there.  Between the unpack and the pack of every chunk swz_srs_project_node_boxes_device maps the
 *     chunk's positions to ECEF (srs == NULL: they stay, and only the origins apply); the box minima are the origins of the
 *     chunk's nodes (setOriginToSmallestPoint, Transformation.cpp:213-227), the pack goes through
 *     swz_pnts_pack_origin_device, and every file carries its node's origin as RTC_CENTER: a float offset within a node
 *     instead of a float at 6.4e6 m.  Metadata: the tileset tree is built on the SOURCE root box (swz_tileset_build) and
 *     written with swz_tileset_oriented_boxes / swz_tileset_write_oriented.  With SWZ_OUT_TIGHT_BOUNDS the ECEF boxes of the
 *     kernel, collected over the chunks and widened to what the files hold (origin + the narrowed float of the largest
 *     offset), go through swz_tileset_build_boxes (unions bottom-up, half-axes): those boxes are axis-aligned in ECEF and DO
 *     enclose the points, which the reference's four-point oriented box does not where a flat tile bulges.  properties.json
 *     keeps the source's box and spacing.  Refused by name before anything is written: everything swz_convert_dataset
 *     refuses, a format other than 3DTILES, a non-zero out.global_offset (the origin is the node's), a struct swz_srs_parse
 *     did not make.  swz_convert_stats does not grow: the projection's time is part of pack_ms.  Not offered: LAS or BIN
 *     targets with a projection (the reference's convert_to_las_file takes the transformation and never uses it),
 *     boundingRegion, --delete-source, .pnts and LAZ sources, a multi-GPU driver. */
int swz_srs_project_node_boxes_device(swz_ctx* ctx, const swz_srs* srs /* NULL: identity */, double* d_xyz, uint64_t n,
                                      uint64_t num_nodes, const uint64_t* node_offset, const uint64_t* node_count /* host */,
                                      double* box_min_out, double* box_max_out /* host, 3 per node */);
int swz_convert_dataset_world(swz_ctx* ctx, const char* src_dir, const char* dst_dir, const swz_convert_params* params,
                              const swz_srs* srs /* NULL: no projection, per-node origins only */, swz_convert_stats* stats);
/* ---- one tiler per GPU of a multi-GPU run (BASELINE config 5: sharded + multi-batch).  Points are owned by their
 * level-0 octant as in swz_shard_* above; every shard keeps the subtrees of its octants and ITS part of the root's
 * file.  Per batch, after the exchange of the batch's points (and attribute columns) by octant:
 *   swz_tiler_shard_begin_device: d_xyz / d_attrs (device; attrs may be NULL) are the points this shard received
 *     (n may be 0).  Indexes + sorts them and decides the ROOT node: take-all / sample from the counts of the whole
 *     root (tile_internal_node, TilingAlgorithms.cpp:272-275: global_root_stored > 0 forces sampling); the whole
 *     local part of the root's file takes part whenever the batch has points anywhere; for MIN_DISTANCE
 *     d_ghost_xyz are the positions of what the root holds on all LOWER shards after their begin of THIS batch
 *     (swz_tiler_level_positions_device(tiler, -1, ...) there): they sort first and are taken again.
 *     *root_file_count_out = points of the root's file on this shard afterwards.
 *   swz_tiler_shard_finish: the levels >= 0 (local).
 * ACCURATE and exact MIN_DISTANCE only.  The node table of a shard lists the root with the shard's part of its file;
 * the root's file is the concatenation over the shards in rank order. */
typedef struct {
  uint64_t global_new_points;  /* points of this batch over all shards */
  uint64_t global_root_stored; /* points in the root's file over all shards before this batch */
  const double* d_ghost_xyz;   /* device, num_ghosts x 3 */
  uint64_t num_ghosts;
} swz_tiler_shard_info;
int swz_tiler_shard_begin_device(swz_tiler* tiler, double* d_xyz, uint64_t n, const swz_attribute_columns* d_attrs,
                                 const swz_tiler_shard_info* info, uint64_t* root_file_count_out);
int swz_tiler_shard_finish(swz_tiler* tiler, swz_tile_stats* stats);
/* FAST (TilingAlgorithmV3) on a sharded data set: swz_tiler_shard_begin_device indexes and sorts only (FAST has no root
 * step per batch); after the FIRST batch's begin every shard reports its points per 6-octant prefix (2^18 counts, host),
 * the driver sums them over the shards, derives the start level (TilingAlgorithms.cpp:1473-1535) and tells every shard
 * before swz_tiler_shard_finish.  At the end of the data set: swz_tiler_shard_fast_finalize_local rebuilds the skipped
 * levels of the shard's octants down to level 0; the driver samples the root from the level-0 files of ALL shards (in
 * shard order, swz_tiler_level_positions_device(0)) and hands every shard the flags of its entries. */
int swz_tiler_shard_fast_histogram(swz_tiler* tiler, uint32_t* counts_out /* 262144, host */);
int swz_fast_start_level_from_counts(const uint64_t* counts /* 262144, host */, uint32_t fast_concurrency, int32_t* start_level_out);
int swz_tiler_shard_set_start_level(swz_tiler* tiler, int32_t start_level);
int swz_tiler_shard_fast_finalize_local(swz_tiler* tiler, swz_tile_stats* stats);
int swz_tiler_shard_fast_set_root(swz_tiler* tiler, const uint8_t* d_taken);
/* A batch that fails part-way (workspace out of memory, a MIN_DISTANCE level that does not terminate, a HIP error)
 * leaves the node store half updated: the tiler is then POISONED -- every later swz_tiler_* call except
 * swz_tiler_destroy / swz_tiler_get_info returns SWZ_ERR_TILER_FAILED and names the original failure.  A driver that
 * keeps several tilers in step (one per GPU) poisons the others itself when one of them fails. */
int swz_tiler_poison(swz_tiler* tiler, const char* why);
/* points stored in the files of one octree level (-1 = root) and their positions in file order */
int swz_tiler_level_count(swz_tiler* tiler, int level, uint64_t* count_out);
int swz_tiler_level_positions_device(swz_tiler* tiler, int level, double* d_xyz_out);
/* ---- one batch sharded over several GPUs from ONE host process (the reference's host is a
 * single C++ process, so this is its multi-GPU drop-in: TilingAlgorithmBase::build_execution_graph,
 * core/tiling/TilingAlgorithms.cpp:1362-1784, for a batch whose points lie on several devices).
 *   swz_group_create: one context per shard on devices[shard] (1, 2, 4 or 8 shards; shard s owns the level-0 octants
 *     o with o * num_shards / 8 == s).  transport 0 = peer copies (hipMemcpyPeerAsync; several shards may share a
 *     device), 1 = RCCL grouped ncclSend / ncclRecv on communicators made by ncclCommInitAll (distinct devices only;
 *     librccl is loaded on demand, the library does not link it).
 *   swz_group_tile: d_xyz[s] / n[s] are the points that currently lie on shard s's device (any octants; clamped in
 *     place), d_attrs (may be NULL) is an array of num_shards column sets: d_attrs[s] holds shard s's attribute
 *     columns (device, n[s] rows; the same attributes on every shard), which travel with the points.  One host thread per shard: encode, group by destination, ONE exchange step, root node (for
 *     MIN_DISTANCE swept by all shards at once, cells at a lower octant's face reading that shard's records through peer
 *     access -- cubic bounds, one address space; otherwise the chain of ghosts from lower to higher shards), levels.  results[s] describes what shard s
 *     ended up with, exactly as swz_shard_finish_device does: device pointers owned by the shard's context, valid
 *     until the group's next call.  ACCURATE, or FAST (TilingAlgorithmV3: the start level from the whole batch's distribution, the
 *     skipped levels rebuilt per shard and the root from all shards' level-0 nodes on shard 0 -- swz_shard_fast_*; d_dup then
 *     says in which ancestors a point is stored as well); MIN_DISTANCE exact or in property mode (below the root).
 *   swz_group_ctx: the shard's context, e.g. for swz_copy_to_host, swz_build_node_lists_device or
 *     swz_gather_payload_device on that shard's results. */
typedef struct swz_group swz_group;
typedef struct {
  const double* d_xyz;     /* the shard's points after the exchange (num_points x 3) */
  const uint64_t* d_keys;  /* ascending */
  const uint32_t* d_perm;  /* index into d_xyz */
  const int8_t* d_level;
  swz_attribute_columns attrs; /* the attribute columns that travelled with the points (rows like d_xyz) */
  uint64_t num_points;
  swz_tile_stats stats;
  const uint32_t* d_dup;   /* FAST: bit l + 1 set = the point is also stored in its ancestor at node level l (else NULL) */
} swz_group_result;
int swz_group_create(int num_shards, const int* devices, int transport, swz_group** group_out);
int swz_group_destroy(swz_group* group);
const char* swz_group_last_error(const swz_group* group);
int swz_group_num_shards(const swz_group* group);
swz_ctx* swz_group_ctx(swz_group* group, int shard);
/* host wall clock of shard `shard` in the last swz_group_tile, ms since the call began: exchange done, root begun, root
 * done, levels done (the MIN_DISTANCE root: all shards at once when the level can be decided on keys, else in turns --
 * then "root begun" is taken when the shard's turn has come and "root done" before the turn passes on, so that no
 * shard's root begins before the lower shard's is done) */
int swz_group_shard_timing(const swz_group* group, int shard, double ms_out[4]);
int swz_group_tile(swz_group* group, double* const* d_xyz, const swz_attribute_columns* d_attrs, const uint64_t* n,
                   const double bounds_min[3], const double bounds_max[3], const swz_tile_params* params,
                   swz_group_result* results);

/* A data set that arrives in several batches, sharded over the group's GPUs from ONE C++ process (BASELINE config 5;
 * the reference is one process too: core/process/Tiler.cpp:189-198, 499-527).  One swz_tiler per shard owns the subtrees
 * of the shard's level-0 octants and ITS part of the root's file.  Per batch: encode, group by destination, ONE
 * exchange step of the point rows and of every attribute column, then the root node -- its take-all / sample decision
 * uses the counts of the whole root, and for MIN_DISTANCE the shards take turns with the lower shards' root files as
 * ghosts -- and, without communication, the levels below.
 *   swz_group_tiler_open / _close: creates / destroys the shards' tilers (ACCURATE or FAST strategy, exact samplers).
 *     FAST: per batch every shard adds the prefix histogram of its keys, the sum over the shards gives the start level the
 *     single tiler would choose (TilingAlgorithms.cpp:1473-1535), the levels below it run per shard.
 *   swz_group_add_batch: d_xyz[s] / n[s] / d_attrs[s] as in swz_group_tile; stats (may be NULL) receives one entry per shard.
 *   swz_group_stage_batch / swz_group_tile_staged: the same from PINNED host memory -- the copies of batch k + 1 run on a
 *     copy stream per shard (hipMemcpyAsync) beside the kernels of batch k; at most two batches are staged.
 *   swz_group_finalize: ends the data set.  FAST rebuilds the skipped levels: each shard those of its octants down to
 *     level 0, shard 0 the root from the level-0 files of all shards (TilingAlgorithms.cpp:1661-1784); ACCURATE has
 *     nothing left to do.
 *   swz_group_tiler: shard s's tiler, for swz_tiler_node_table / _export_device / _pools_device / _get_info.  The
 *     root's file is the concatenation of the shards' parts in shard order.
 * Every exchange is preceded by a status vote: a shard that failed makes all shards skip the step and return its error
 * (nobody waits for a peer that is gone).  A batch that fails on one shard poisons every shard's tiler (swz_tiler_poison). */
int swz_group_tiler_open(swz_group* group, const double bounds_min[3], const double bounds_max[3], const swz_tile_params* params,
                         uint64_t capacity_hint_per_shard);
int swz_group_tiler_close(swz_group* group);
swz_tiler* swz_group_tiler(swz_group* group, int shard);
int swz_group_add_batch(swz_group* group, double* const* d_xyz, const swz_attribute_columns* d_attrs, const uint64_t* n,
                        swz_tile_stats* stats_per_shard);
int swz_group_stage_batch(swz_group* group, const double* const* xyz_host, const swz_attribute_columns* attrs_host, const uint64_t* n);
int swz_group_tile_staged(swz_group* group, swz_tile_stats* stats_per_shard);
int swz_group_finalize(swz_group* group, swz_tile_stats* stats_per_shard);
/* ---- the node table and the output of a data set tiled on a group.
 *   swz_merge_shard_node_tables (host, no GPU): the tables swz_tiler_node_table gives for the shards' tilers, merged into the
 *     table a single tiler fed the same batches gives.  Order: swz_tiler_node_table lists level after level, and inside a
 *     level the runs of equal node prefix of a store that ascends by it -- ascending node key, the key being the Morton key
 *     with the bits below the node's level cleared.  A re-rooted subtree keeps that rule: its nodes carry the key of the node
 *     that was re-rooted with the child octants appended at their ABSOLUTE levels (swz_treroot.hip), and every entry of such a
 *     node carries the node's key, so the store of a level still ascends by node key.  The merged table is therefore ordered
 *     by (level, node key), whatever the shards' tables contain.  The root (level -1) appears once, its count the sum of
 *     the shards' parts, with shard_out -1; for every other node shard_out is the shard whose table lists it.  A node below
 *     the root on two shards, or listed twice by one, is SWZ_ERR_INTERNAL.  *num_nodes_out is always set; max_nodes too small
 *     is SWZ_ERR_BAD_ARG; with every output array NULL only the count is given (max_nodes is ignored).  shard_out alone may
 *     be NULL.
 *   swz_group_node_table: the same from the tilers of an open data set (swz_group_tiler_open).
 *   swz_group_node_boxes: swz_tiler_node_boxes of every shard's tiler, in the order of swz_group_node_table (max_nodes x 3
 *     doubles each); the root's box is the min / max of the shards' parts.  swz_group_write_output honours
 *     SWZ_OUT_TIGHT_BOUNDS the same way: every shard reduces its own nodes while it streams them, shard 0 the root's
 *     gathered rows, and the metadata is written once from the merged table and the merged boxes.  Both have only ever run
 *     with all shards on ONE device.
 *   swz_group_write_output: the directory swz_tiler_write_output writes for a single tiler fed the same batches -- the same
 *     file names and the same bytes, metadata included.  Preconditions: a data set is open, no batch is staged on the group,
 *     and on every shard's tiler what swz_tiler_write_output asks (not poisoned, nothing staged or open).  What that call
 *     refuses with SWZ_ERR_BAD_ARG (an unknown format, a mask naming a column the batches did not carry, an rgb_mapping
 *     without intensities, a global_offset that is not finite, a dir that cannot be created) is refused ONCE, before any
 *     directory or file is created.  A failed write names the file through swz_group_last_error, poisons nothing and leaves
 *     the group usable.
 *     Below the root every node lives on one shard: each shard streams its own nodes on its own host thread, device and copy
 *     stream with its own two chunk images, all into the same dir (dir/ept-data for ENTWINE_LAS); boxes, LAS scales and
 *     offsets are swz_node_bounds of the group's root box.  The root's file is the concatenation of the shards' parts in
 *     shard order (after a FAST swz_group_finalize too): every shard gathers the rows of its part (positions and the masked
 *     columns, swz_gather_payload_device), after a status vote the parts are copied to shard 0, which packs them as a
 *     one-node table with the format's pack call and writes the file through its own chunk images (the root's size enters
 *     their maximum).  A root without points writes no file.  The metadata is written once, from the merged table, after
 *     every shard's files are done and a second vote is clean.
 *     Threads: SWZ_BIN_WRITER_THREADS (read from shard 0's context) is the budget of the whole call, divided among the
 *     shards with at least one each.  chunk_points 0 reads SWZ_OUTPUT_CHUNK_POINTS from every shard's own context.
 *     stats_per_shard (num_shards entries or NULL): as swz_tiler_write_output fills them for the shard's own nodes (shard
 *     0: the root's file included; nodes and stored_points of the shard's own table).  total (or NULL): nodes and stored
 *     points of the merged table, bytes and chunks summed, wall_ms of the call, the other *_ms the maximum over the shards.
 *   swz_group_add_las_files: swz_tiler_add_las_files for the group.  The scan (swz_las_scan_files), the refusals before
 *     anything is read (the mask rules, SWZ_ATTR_NORMAL, the box check with its 4 ulp against the group's root box,
 *     SWZ_ERR_TOO_MANY_POINTS against the per-shard limit in the worst case that one shard receives everything), the cuts
 *     (swz_input_batches, under FAST min_last = fast_concurrency, checked for the whole batch) and shift_to_center are that
 *     call's.  Refused too: no data set open, a batch staged on the group or on a shard's tiler, a tiler that is poisoned or
 *     finalized.  Per batch the point range is cut into num_shards consecutive slices in shard order (slice s: the points
 *     [P * s / N, P * (s + 1) / N) of the batch's P); a slice is a list of swz_las_segment.  Shard s's share of the reader
 *     threads preads its slice into one of its two page-locked images, its copy stream moves the image to its device and the
 *     segment kernel decodes it there into one of the shard's two stage buffers (positions and the masked columns: the
 *     buffers of swz_group_stage_batch), and the batch goes the way of swz_group_tile_staged -- encode, group, one exchange,
 *     root, levels.  Read, copy and decode of batch k + 1 run beside the tiling of batch k.  Host and device hold two raw
 *     slice images and two decoded batch buffers per shard at most, whatever the size of the data set.
 *     Threads: SWZ_INPUT_READER_THREADS (read from shard 0's context) is the budget of the whole call, divided among the
 *     shards with at least one each.
 *     A read that fails ends the stream after the batch in flight and names the file (swz_group_last_error).  A failure
 *     before the first batch is tiled leaves every tiler as it was, a later one poisons all of them as a failed group batch
 *     does.  The call does not finalize.  stats (may be NULL): the fields of the single call -- files, points, batches and
 *     bytes_read of the whole call, read_ms / copy_ms / decode_ms the maximum over the shards of their sums over the
 *     batches, tile_ms the tiling calls', wait_ms the time the call waited for its readers. */
int swz_group_add_las_files(swz_group* group, const char* const* paths, uint64_t num_files, const swz_input_params* params,
                            swz_input_stats* stats);
/* swz_tiler_set_source_srs for the group's data set: allowed between swz_group_tiler_open and the first batch (NULL clears;
 * swz_group_tiler_close forgets it).  The data set's ECEF boxes are computed once on the host, not per shard. */
int swz_group_set_source_srs(swz_group* group, const swz_srs* srs);
int swz_merge_shard_node_tables(int num_shards, const uint64_t* num_nodes, const int8_t* const* node_level,
                                const uint64_t* const* node_key, const uint64_t* const* node_count, uint64_t max_nodes,
                                int8_t* level_out, uint64_t* key_out, uint64_t* count_out, int32_t* shard_out,
                                uint64_t* num_nodes_out);
int swz_group_node_table(swz_group* group, uint64_t max_nodes, int8_t* level_out, uint64_t* key_out, uint64_t* count_out,
                         int32_t* shard_out, uint64_t* num_nodes_out);
int swz_group_node_boxes(swz_group* group, uint64_t max_nodes, double* box_min_out, double* box_max_out, uint64_t* num_nodes_out);
int swz_group_write_output(swz_group* group, const char* dir, const swz_output_params* params,
                           swz_output_stats* stats_per_shard, swz_output_stats* total);

/* ---- the MIN_DISTANCE root of a sharded batch swept by all ranks at once, ONE PROCESS PER GPU (the torch driver;
 * swz_group_tile does this by itself for the shards of one process).  Instead of the chain of ghosts from rank to rank
 * (swz_shard_begin_device with ghosts), every rank sweeps the root cells of its own octants concurrently and cells at the
 * face of a lower octant read that rank's records in place, through IPC mappings (hipIpcGetMemHandle /
 * hipIpcOpenMemHandle) that the library exchanges through the driver's all-gather:
 *   swz_shard_joint_root_possible: exact MIN_DISTANCE, cubic bounds, a root that can be decided on key coordinates.
 *   swz_shard_joint_root_begin: before swz_shard_begin_device (without ghosts).  exchange(arg, mine, bytes, all) must
 *     all-gather `bytes` bytes of every rank into all[rank * bytes] and return 0; the library calls it twice per batch
 *     on every rank, from inside swz_shard_begin_device (or from swz_shard_joint_root_meet).
 *   swz_shard_joint_root_meet: a rank whose swz_shard_begin_device was not called (it owns no points) or failed before
 *     its sweep began calls this instead, so that the others are not left waiting in the exchange.
 *   swz_shard_joint_root_end: after a barrier of the driver behind swz_shard_begin_device (the other ranks may read this
 *     rank's root arrays until they have finished theirs); unmaps.
 * Results are those of the chain, point for point (tests/test_sharded_gloo.py, two processes on one GPU). */
typedef int (*swz_exchange_fn)(void* arg, const void* mine, uint64_t bytes, void* all);
int swz_shard_joint_root_possible(swz_ctx* ctx, const swz_tile_params* params, const double bounds_min[3], const double bounds_max[3]);
int swz_shard_joint_root_begin(swz_ctx* ctx, int shard, int num_shards, swz_exchange_fn exchange, void* arg);
/* Collective, before the first batch: can every rank map and read the lower ranks' device memory (IPC handles through the
 * same all-gather callback: two exchanges, then one per rank while the mappings are closed in turns)?  *usable = 1 only when all ranks could; a driver that gets 0 keeps the chain of
 * ghosts -- nothing has been started that would have to be undone. */
int swz_shard_joint_root_probe(swz_ctx* ctx, int shard, int num_shards, swz_exchange_fn exchange, void* arg, int* usable);
int swz_shard_joint_root_meet(swz_ctx* ctx, int ok);
int swz_shard_joint_root_end(swz_ctx* ctx);

/* page-locked host memory for the staging entry points (hipHostMalloc / hipHostFree) */
int swz_host_alloc_pinned(uint64_t bytes, void** out);
int swz_host_free_pinned(void* p);
/* device memory and copies for host code that does not include HIP headers itself (hipMalloc / hipFree on the
 * current device; the copies run on the context's stream and return when done) */
int swz_device_alloc(uint64_t bytes, void** d_out);
int swz_device_alloc_on(swz_ctx* ctx, uint64_t bytes, void** d_out); /* on the context's device (several GPUs) */
int swz_device_free(void* d_ptr);
int swz_copy_to_host(swz_ctx* ctx, void* dst_host, const void* d_src, uint64_t bytes);
int swz_copy_to_device(swz_ctx* ctx, void* d_dst, const void* src_host, uint64_t bytes);

/* ---- synthetic workload of BASELINE.json / SURVEY.md section 8(d): uniform points in the unit
 * cube from a counter-based splitmix64 stream (point i draws x,y,z = draws 3i..3i+2). */
int swz_generate_uniform_device(swz_ctx* ctx, uint64_t seed, uint64_t first_point, uint64_t n,
                                double* d_xyz_out);

/* ---- per-kernel timing (HIP events on the context's stream) for bench.py's roofline.
 * When enabled every kernel class is bracketed by events; totals accumulate until reset. */
typedef struct {
  char name[48];
  uint64_t launches;
  double total_ms;
  uint64_t algorithmic_bytes; /* bytes the launches had to move at minimum */
} swz_kernel_stat;
int swz_profile_enable(swz_ctx* ctx, int enabled);
int swz_profile_reset(swz_ctx* ctx);
/* Copies up to max_stats entries; returns the number of kernel classes via *num_out.
 * Five entries are COUNTS, not timed classes (total_ms and algorithmic_bytes stay 0): what the key sweep did with the cell
 * tables of a chain of dense MIN_DISTANCE levels -- mq_tables_ahead (kernels that built a next level's early tables on the
 * build stream, two per level), mq_prebuild_taken / mq_prebuild_dropped (levels that took such tables / tables nobody could
 * use), mq_tables_late (the two late kernels of a level that took them), mq_tables_at_setup (the two table kernels of a
 * directly numbered level that built everything itself). */
int swz_profile_get(swz_ctx* ctx, swz_kernel_stat* stats_out, uint32_t max_stats, uint32_t* num_out);

#ifdef __cplusplus
}
#endif
#endif
