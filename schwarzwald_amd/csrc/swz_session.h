// swz_session.h -- one batch between "indexed + sorted" and "all levels done" (swz_session.hip), as far as the drivers of
// sharded batches (swz_shard.hip) run it themselves.
#pragma once
#include "swz_level.h"

namespace swz {

// State of one batch between "indexed + sorted" and "all levels done".  Held in the context while a
// sharded batch waits for its neighbours' root samples (swz_shard_begin / swz_shard_finish).
struct TileSession {
  uint32_t n = 0;
  double bmin[3] = {0, 0, 0}, bmax[3] = {0, 0, 0};
  swz_tile_params params{};
  uint64_t* keys = nullptr;  // sorted keys
  uint32_t* perm = nullptr;  // original index per sorted position
  int8_t* level = nullptr;
  uint32_t* dup = nullptr;
  const double* xyz_in = nullptr;  // the caller's positions (clamped by the encode)
  SortedPoints sp;
  LevelBuffers lb;
  uint64_t* key_buf[2] = {nullptr, nullptr};
  uint32_t* idx_buf[2] = {nullptr, nullptr};
  int which = 0;
  ActiveSet as;
  int next_level = -1;
  uint64_t visited = 0, nodes = 0;
  uint32_t rounds = 0, nlevels = 0;
  int max_level = -1;
  int fast_start = -1;
  uint32_t ghosts = 0;  // leading points that belong to other shards (sharded batches only)
  uint32_t front = 0;   // entries kept free in front of the per-position arrays (sharded batches)
};

// K1 + K2 + gather: index, sort, positions into Morton order where the root level needs them
// `front`: entries kept free in FRONT of every per-sorted-position array (sharded batches prepend ghosts).
int session_prepare(swz_ctx* c, TileSession& t, double* d_xyz, uint32_t n, const double bmin[3], const double bmax[3],
                    const swz_tile_params& p, const TileDeviceOut& out, uint32_t front = 0);
// Runs the level loop from t.next_level while points remain and level <= last_level.
// first_mode: -1 = decide per node from its count; 0/1 force take-all/sample for the FIRST level run
// (sharded batches decide the root from the global point count).
// chains: dense exact-MIN_DISTANCE levels may share one active set instead of compacting after each (the single batch of
// swz_tile* only: see session_run_levels for who defers).
int session_run_levels(swz_ctx* c, TileSession& t, int last_level, int first_mode, bool chains = false);
void session_stats(const TileSession& t, swz_tile_stats* stats);

// FAST: is sorted point i a candidate of a reconstruct level?  Persisted at level S - 1 by a start node (child_bit == 0),
// or flagged in dup as stored in the reconstructed node one level below.
__device__ __forceinline__ bool recon_candidate(const int8_t* level, const uint32_t* dup, uint32_t i, int start_node_level,
                                                uint32_t child_bit) {
  return child_bit ? (dup[i] & child_bit) != 0 : level[i] == (int8_t)start_node_level;
}
// pos[i] = rank of sorted point i among those candidates (exclusive scan of their flags); their number is left in
// t.lb.counters[CTR_REMAINING]
int session_recon_ranks(swz_ctx* c, TileSession& t, int S, uint32_t child_bit, uint32_t* pos);
// FAST: reconstruct the skipped levels S-1 .. lowest_lv, deepest first
int session_fast_reconstruct(swz_ctx* c, TileSession& t, const swz_tile_params& p, int S, int lowest_lv);

}  // namespace swz
