// swz_internal.h -- context, workspace and launch bookkeeping shared by the HIP translation units.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <map>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../include/swz_gpu.h"

namespace swz {

constexpr uint32_t MAX_LEVELS = 21;  // MortonIndex64Levels, core/datastructures/MortonIndex.h:222-226

struct DevBuf {
  void* ptr = nullptr;
  size_t cap = 0;
  uint64_t epoch = 0;  // swz_ctx::scratch_epoch at the last get()
  bool host = false;   // page-locked host memory mapped into the device's address space (a spilled pool of swz_tiler)
};

struct KernelStat {
  uint64_t launches = 0;
  double total_ms = 0.0;
  uint64_t bytes = 0;
};

struct PendingEvent {
  std::string name;
  hipEvent_t e0, e1;
  uint64_t launches;
  uint64_t bytes;
};

// The key sweep's early per-cell tables of the NEXT level of a chain, built on a side stream under the running level's rounds
// (swz_mqbuild.hip, mq_prebuild_launch).  A guess that costs only time: the next level compares `key` fields
// with what it really is (mq_prebuilt_matches) and builds everything itself when one differs.
struct MqPrebuild {
  // the request: session_run_levels in front of a level that may leave its survivors in place, for the level after it
  bool wanted = false;
  uint32_t want_node_shift = 0, want_cl = 0, want_rg = 0;
  // the product: which keys, which grid, which set of per-cell buffers ("" / "_b") and where they were when it was built
  bool valid = false;
  uint32_t serial = 0;  // counts the products: tells the one a level found from the one it built
  int set = 0;
  const void* akey = nullptr;
  uint32_t m = 0, node_shift = 0, cl = 0, rg = 0, ncells = 0, nodes = 0;
  const void *cinfo = nullptr, *qnbr = nullptr, *rec = nullptr, *slot = nullptr, *qst = nullptr;
  hipEvent_t done = nullptr;  // behind the last early kernel on the build stream; null: the context's stream has waited for it
  hipEvent_t t0 = nullptr, t1 = nullptr;  // SWZ_DEBUG: around the early kernels
};

}  // namespace swz

struct swz_ctx {
  int device = 0;
  hipStream_t own_stream = nullptr;
  hipStream_t stream = nullptr;
  std::string err;
  std::map<std::string, swz::DevBuf> bufs;
  // profiling
  bool profile = false;
  std::map<std::string, swz::KernelStat> kstats;
  std::vector<swz::PendingEvent> pending;
  std::vector<hipEvent_t> event_pool;
  std::vector<hipStream_t> aux_streams;  // side streams for work that may overlap (MIN_DISTANCE node groups), made on demand

  // ---- error helpers
  int fail(int code, const std::string& msg) {
    err = msg;
    return code;
  }
  int hip_fail(hipError_t e, const char* what, const char* file, int line) {
    err = std::string(what) + ": " + hipGetErrorString(e) + " (" + file + ":" + std::to_string(line) + ")";
    return SWZ_ERR_HIP;
  }

  // ---- grow-only named workspace.  The MIN_DISTANCE samplers (buffers "md_*", "sp_*", "pm_*") use theirs for one level
  // at a time and say so (next_scratch_epoch() at the start of a level): when the device is out of memory, get() frees
  // such buffers of earlier levels or calls and tries again -- a cloud whose levels need very different per-cell and
  // per-point arrays then needs the largest level's memory, not the sum over the levels.
  uint64_t scratch_epoch = 1;
  void next_scratch_epoch() { ++scratch_epoch; }
  int get(const char* name, size_t bytes, void** out);
  template <typename T>
  int get(const char* name, size_t count, T** out) {
    return get(name, count * sizeof(T), reinterpret_cast<void**>(out));
  }
  void release_all();
  void free_buf(swz::DevBuf& b);   // device or mapped host memory, whichever it is
  uint64_t held_bytes() const;      // device memory only
  uint64_t held_host_bytes() const; // spilled to page-locked host memory

  // ---- timing: bracket [begin, end) launches of one kernel class with events when profiling
  hipEvent_t take_event();
  void prof_begin(const char* name);
  void prof_end(const char* name, uint64_t launches, uint64_t bytes);
  void prof_collect();  // after a stream sync: fold pending events into kstats
  hipEvent_t cur_e0_ = nullptr;
  void* shard = nullptr;  // swz::ShardState of an open sharded batch (swz_shard.hip)
  const void* md_shard_root = nullptr;  // swz::MdShardRoot while swz_group runs the MIN_DISTANCE root of a sharded batch on all shards at once
  bool md_shard_root_published = false;  // the "md_*_sr" arrays of this context are mapped by other shards: they stay (see get())
  // swz_mdblock.hip, sb_incremental: [sbi_clean_ptr, + sbi_clean_bytes) of the "sbi_bits" buffer is known to be zero
  const void* sbi_clean_ptr = nullptr;
  size_t sbi_clean_bytes = 0;
  // the key sweep (swz_mqbuild.hip, mq_alloc_arrays): "md_qpos" at mq_qpos_buf holds the packed key coordinates of the mq_qpos_m keys at mq_qpos_keys (the
  // next level of a chain on the same arrays does not write them again); free_buf forgets it with the buffer
  const void* mq_qpos_buf = nullptr;
  const void* mq_qpos_keys = nullptr;
  uint32_t mq_qpos_m = 0;
  // ... and its tables built ahead: the build stream (made on demand, lowest priority) and the one product in flight;
  // free_buf forgets a product whose buffer it frees
  hipStream_t mq_build_stream = nullptr;
  swz::MqPrebuild mq_pre;
  void prof_count(const char* name, uint64_t launches) {  // launches that no event pair brackets (another stream's, or skipped ones)
    if (profile) kstats[name].launches += launches;
  }
  bool tiler_active = false;  // a swz_tiler lives on this context: its node store is part of the workspace
  swz_tiler* nodes_tiler = nullptr;  // the tiler of an open swz_tile_nodes_begin_device / _end_device pair
  // no batch of the tiler is open: its per-batch scratch ("tl_*") holds nothing anybody will read again, and get() may free
  // what was not asked for since the last next_scratch_epoch() when the device runs out of memory (a data set of 3 B points
  // could be tiled but not exported: 100 GB of merge and survivor buffers of the last batch stood in the way)
  bool tiler_scratch_dead = false;
  // Debug / tuning switches ("SWZ_DEBUG", "SWZ_MD_*", ...): read from the environment ONCE, when the context is
  // created, and changed afterwards only through swz_set_option -- no entry point looks at the environment.
  std::map<std::string, std::string> options;
  const char* opt(const char* name) const {
    const auto it = options.find(name);
    return it == options.end() ? nullptr : it->second.c_str();
  }
  // typed reads: `def` when the switch is absent, else its value as atoll / atof / atoi(v) != 0 read it
  long opt_int(const char* name, long def) const {
    const char* v = opt(name);
    return v ? (long)atoll(v) : def;
  }
  double opt_num(const char* name, double def) const {
    const char* v = opt(name);
    return v ? atof(v) : def;
  }
  bool opt_on(const char* name, bool def) const {
    const char* v = opt(name);
    return v ? atoi(v) != 0 : def;
  }
};

#define SWZ_HIP(ctx, expr)                                                \
  do {                                                                    \
    hipError_t _e = (expr);                                               \
    if (_e != hipSuccess) return (ctx)->hip_fail(_e, #expr, __FILE__, __LINE__); \
  } while (0)

#define SWZ_TRY(expr)            \
  do {                           \
    int _s = (expr);             \
    if (_s != SWZ_OK) return _s; \
  } while (0)

// checks the launch itself (configuration errors); execution errors surface at the next sync
#define SWZ_LAUNCH_CHECK(ctx) SWZ_HIP(ctx, hipGetLastError())

namespace swz {

inline uint32_t div_up(uint64_t a, uint64_t b) { return (uint32_t)((a + b - 1) / b); }

// RAII-less helper: time one kernel class
struct ProfScope {
  swz_ctx* c;
  const char* name;
  uint64_t launches, bytes;
  ProfScope(swz_ctx* ctx, const char* n, uint64_t b, uint64_t l = 1) : c(ctx), name(n), launches(l), bytes(b) {
    c->prof_begin(name);
  }
  ~ProfScope() { c->prof_end(name, launches, bytes); }
};

// SWZ_TRACE=1: synchronise and report after a stage (debugging hangs; never on in production)
#define SWZ_STAGE(ctx, what)                                                              \
  do {                                                                                    \
    if ((ctx)->opt("SWZ_TRACE")) {                                                            \
      const hipError_t _e = hipStreamSynchronize((ctx)->stream);                          \
      fprintf(stderr, "[swz trace] %s:%d %s -> %s\n", __FILE__, __LINE__, what, hipGetErrorString(_e)); \
      fflush(stderr);                                                                     \
    }                                                                                     \
  } while (0)

// hipMemsetAsync in pieces of 1 GiB: a single call of exactly 4 GiB (512 nodes x 2^21 cells x 4 bytes) was
// observed not to fill the buffer on ROCm 7.0 / gfx950 (tools/debug_fullsize.py: neighbour cells went missing)
inline hipError_t memset_large(void* p, int value, size_t bytes, hipStream_t stream) {
  const size_t piece = size_t(1) << 30;
  for (size_t at = 0; at < bytes; at += piece) {
    const hipError_t e = hipMemsetAsync(static_cast<char*>(p) + at, value, bytes - at < piece ? bytes - at : piece, stream);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

// one device counter to the host: a 4-byte copy and a synchronisation of the context's stream (swz_api.hip)
int read_u32(swz_ctx* c, const uint32_t* d, uint32_t* h);

// ---- stage entry points (each in its own .hip file) -------------------------------------------
int encode_device(swz_ctx* c, double* d_xyz, uint32_t n, const double bmin[3], const double bmax[3],
                  uint64_t* d_keys);
int generate_uniform_device(swz_ctx* c, uint64_t seed, uint64_t first, uint64_t n, double* d_xyz);
// what every entry point that takes swz_tile_params refuses (swz_api.hip)
int check_params(swz_ctx* c, const swz_tile_params* p);
// ... and what the sharded entry points refuse on top of that; nullptr: the sampler may be sharded
const char* sharded_sampler_refusal(int sampler);

// Stable LSD radix sort of (key, value) pairs.  The input goes in the FIRST pair: the keys in d_keys_in and, unless
// vals_identity, the values in d_vals_tmp (with vals_identity the first pass synthesises value = element index instead of
// reading them).  The sorted result comes out in the SECOND pair (d_keys_out, d_vals_out), on every path: the hybrid
// moves the data an odd number of times (4 or 6 passes and the run pass); the plain eight passes -- small inputs, 2^30
// points and more, keys with long runs of equal top bits -- end in the first pair and are copied over.  Both pairs are
// clobbered.
int radix_sort_pairs(swz_ctx* c, uint64_t* d_keys_in, uint32_t* d_vals_tmp, uint64_t* d_keys_out,
                     uint32_t* d_vals_out, uint32_t n, bool vals_identity);

// Device-wide exclusive scan of a u32 array (in place allowed).  *d_total receives the sum.
int scan_exclusive_u32(swz_ctx* c, const uint32_t* d_in, uint32_t* d_out, uint64_t n, uint32_t* d_total,
                       const char* tag);

// Gather positions into Morton order, SoA: X[i] = xyz[3*perm[i]] ...
int gather_positions(swz_ctx* c, const double* d_xyz, const uint32_t* d_perm, uint32_t n, double* d_x,
                     double* d_y, double* d_z);

struct TileDeviceOut {
  uint64_t* keys;   // sorted keys (n)
  uint32_t* perm;   // original index (n)
  int8_t* level;    // taken level per sorted position (n)
  uint32_t* dup;    // may be null
};

int tile_device(swz_ctx* c, double* d_xyz, uint32_t n, const double bmin[3], const double bmax[3],
                const swz_tile_params& p, const TileDeviceOut& out, swz_tile_stats* stats);

int shard_begin_device(swz_ctx* c, const double* d_xyz_local, uint32_t n, const double bmin[3],
                       const double bmax[3], const swz_tile_params& p, uint64_t global_points,
                       const double* d_ghost_xyz, uint32_t ghosts, uint64_t* num_root_taken);
int shard_presort_device(swz_ctx* c, const double* d_xyz_local, uint32_t n, const double bmin[3], const double bmax[3],
                         const swz_tile_params& p, uint32_t ghost_capacity);
int shard_root_taken_device(swz_ctx* c, double* d_xyz_out);
int shard_finish_device(swz_ctx* c, uint64_t* d_keys_out, uint32_t* d_perm_out, int8_t* d_level_out,
                        swz_tile_stats* stats);
int shard_begin_empty(swz_ctx* c);
void shard_free(swz_ctx* c);
// FAST on a sharded batch (swz_shard_fast_*)
int shard_fast_begin_device(swz_ctx* c, const double* d_xyz_local, uint32_t n, const double bmin[3], const double bmax[3],
                            const swz_tile_params& p, uint32_t* counts_host);
int shard_fast_run_device(swz_ctx* c, int start_level, uint64_t* num_root_candidates);
int shard_fast_root_candidates_device(swz_ctx* c, uint64_t* d_keys_out, double* d_xyz_out);
int shard_fast_set_root_device(swz_ctx* c, const uint8_t* d_taken);
int shard_fast_finish_device(swz_ctx* c, uint64_t* d_keys_out, uint32_t* d_perm_out, int8_t* d_level_out, uint32_t* d_dup_out,
                             swz_tile_stats* stats);
// One radix pass on the octant (key bits 60..62): perm groups the points by octant (stable); octants (host)
// receives the eight counts.  Callers may rely on the order (octant, original index): points of equal key keep
// their index order.
int partition_top_digit(swz_ctx* c, const uint64_t* d_keys, uint32_t n, uint32_t* d_perm_out, uint64_t octants[8]);
// Stable partition by the top byte of the keys: d_perm_out[i] = index of the i-th element, starts[d] = first
// position of byte value d.
int partition_by_top_byte(swz_ctx* c, const uint64_t* d_keys, uint32_t n, uint32_t* d_perm_out, uint32_t starts[256]);

int sample_points_device(swz_ctx* c, int sampler, uint64_t max_points, const uint64_t* d_keys,
                         const uint32_t* d_idx, uint32_t n, const double* d_xyz, uint64_t node_key,
                         int32_t node_level, const double rmin[3], const double rmax[3], float spacing,
                         int behaviour, uint8_t* d_taken, uint64_t* num_taken);

}  // namespace swz
