// swz_mqsweep.hip -- the key sweep's rounds (protocol: swz_mdkeys.hip): one activation of a cell, the launch of a round,
// the reject pass of dense cells between two rounds, a shard's round word, and what follows the last round -- the check
// that every cell has reached its end and the level's code for the taken points.  The host functions at the end launch
// them; the round loop itself is in swz_mdkeys.hip.
#include <algorithm>
#include <cstdio>
#include <cstdlib>

#include "swz_mdkeys.h"

namespace swz {

// ----------------------------------------------------------------------------- device helpers
__device__ __forceinline__ uint32_t uni(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
__device__ __forceinline__ uint32_t qb_u32(uint32_t v, int src) { return (uint32_t)__builtin_amdgcn_readlane((int)v, src); }
__device__ __forceinline__ float qb_f32(float v, int src) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), src));
}
__device__ __forceinline__ unsigned long long qb_u64(unsigned long long v, int src) {
  const uint32_t lo = qb_u32((uint32_t)v, src), hi = qb_u32((uint32_t)(v >> 32), src);
  return ((unsigned long long)hi << 32) | lo;
}
template <typename Op>
__device__ __forceinline__ uint32_t mq_wave_scan(uint32_t v, Op op, uint32_t identity) {
  v = op(v, (uint32_t)__builtin_amdgcn_update_dpp((int)identity, (int)v, 0x111, 0xF, 0xF, false));  // row_shr:1
  v = op(v, (uint32_t)__builtin_amdgcn_update_dpp((int)identity, (int)v, 0x112, 0xF, 0xF, false));  // row_shr:2
  v = op(v, (uint32_t)__builtin_amdgcn_update_dpp((int)identity, (int)v, 0x114, 0xF, 0xF, false));  // row_shr:4
  v = op(v, (uint32_t)__builtin_amdgcn_update_dpp((int)identity, (int)v, 0x118, 0xF, 0xF, false));  // row_shr:8
  v = op(v, (uint32_t)__builtin_amdgcn_update_dpp((int)identity, (int)v, 0x142, 0xA, 0xF, false));  // row_bcast:15
  v = op(v, (uint32_t)__builtin_amdgcn_update_dpp((int)identity, (int)v, 0x143, 0xC, 0xF, false));  // row_bcast:31
  return v;
}
struct MqAdd {
  __device__ uint32_t operator()(uint32_t a, uint32_t b) const { return a + b; }
};
struct MqMax {
  __device__ uint32_t operator()(uint32_t a, uint32_t b) const { return a > b ? a : b; }
};
struct MqMin {
  __device__ uint32_t operator()(uint32_t a, uint32_t b) const { return a < b ? a : b; }
};
__device__ __forceinline__ void mq_unpack(uint64_t v, float& x, float& y, float& z) {
  const uint32_t lo = (uint32_t)v, hi = (uint32_t)(v >> 32);
  x = (float)(lo & 0x1FFFFFu);
  y = (float)(((lo >> 21) | (hi << 11)) & 0x1FFFFFu);
  z = (float)(hi >> 10);
}
// squared distance of two points in key cells: the differences of integers below 2^21 are exact in float, the three
// roundings of the sum are part of the band (key_metric)
__device__ __forceinline__ float mq_d2(float ax, float ay, float az, float bx, float by, float bz) {
  const float dx = ax - bx, dy = ay - by, dz = az - bz;
  return __builtin_fmaf(dz, dz, __builtin_fmaf(dy, dy, dx * dx));
}
// the reference's compare on the exact positions (GridCell.cpp:52) for active points i and j
__device__ __forceinline__ bool mq_exact_near(const MqArgs& a, uint32_t i, uint32_t j) {
  const double* p = sorted_point_xyz(a.xyz, a.perm, a.gxyz, a.ng, a.aidx ? a.aidx[i] : i);
  const double* q = sorted_point_xyz(a.xyz, a.perm, a.gxyz, a.ng, a.aidx ? a.aidx[j] : j);
  return sq_dist(p[0], p[1], p[2], q[0], q[1], q[2]) < a.sq_spacing;
}

#ifdef SWZ_MQ_STATS
#define MQ_T(var) const uint64_t var = wall_clock64()
#define MQ_TACC(idx, t0, t1) do { if (l == 0 && (c & 31u) == 0u) atomicAdd(&a.counters[CTR_DBG_HIST + 8 + (idx)], (uint32_t)((t1) - (t0))); } while (0)
#else
#define MQ_T(var) do { } while (0)
#define MQ_TACC(idx, t0, t1) do { } while (0)
#endif
#define MQ_STAT(idx) do { if (a.stats && l == 0) atomicAdd(&a.counters[CTR_DBG_HIST + (idx)], 1u); } while (0)

// Loads that see what another GPU's kernel has written back by now (nothing cached on this side): records and overflow
// entries of a lower shard's cells.  Two 8-byte halves; tearing is caught by bracketing the reads with that shard's
// round word (see mq_activate).
__device__ __forceinline__ uint4 mq_ld_sys(const uint4* p) {
  const unsigned long long* q = reinterpret_cast<const unsigned long long*>(p);
  const unsigned long long lo = __hip_atomic_load(q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  const unsigned long long hi = __hip_atomic_load(q + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  return make_uint4((uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)hi, (uint32_t)(hi >> 32));
}
// ... and what another wavefront of THIS GPU -- or this one, earlier in the launch -- has written: past the CU's L1
__device__ __forceinline__ uint4 mq_ld_agent(const uint4* p) {
  const unsigned long long* q = reinterpret_cast<const unsigned long long*>(p);
  const unsigned long long lo = __hip_atomic_load(q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const unsigned long long hi = __hip_atomic_load(q + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return make_uint4((uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)hi, (uint32_t)(hi >> 32));
}
__device__ __forceinline__ uint32_t mq_ld_sys(const uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM); }

// ... for a local point i and an accepted point j of shard `tag - 1` (0: this shard)
__device__ __forceinline__ bool mq_exact_near_peer(const MqArgs& a, uint32_t i, uint32_t j, uint32_t tag) {
  const double* p = sorted_point_xyz(a.xyz, a.perm, a.gxyz, a.ng, a.aidx ? a.aidx[i] : i);
  const double* q = tag ? a.peers.xyz[tag - 1u] + (size_t)a.peers.perm[tag - 1u][a.peers.aidx[tag - 1u] ? a.peers.aidx[tag - 1u][j] : j] * 3
                        : sorted_point_xyz(a.xyz, a.perm, a.gxyz, a.ng, a.aidx ? a.aidx[j] : j);
  return sq_dist(p[0], p[1], p[2], q[0], q[1], q[2]) < a.sq_spacing;
}

struct MqLds {
  uint4* stage;   // [27][2][rg]: both record buffers of the 27 cells of the neighbourhood
  float4* list;   // [MQ_LIST_CAP]: accepted points of the earlier adjacent cells and of this cell (window)
  float4* fresh;  // [MQ_FRESH_CAP]: accepted in this activation
  uint8_t* tag;   // [MQ_LIST_CAP]: sharded root: which shard a list entry comes from (0 = this one)
  uint32_t* trust;  // [MQ_CHAIN]: the cells this wavefront has run earlier in the launch, one after the other (see mq_sweep_kernel)
  uint32_t* sid;    // [32]: the adjacent cells whose records are staged (the earlier ones and the cell itself: at most mq_staged()), by rank
};

// ----------------------------------------------------------------------------- the sweep
// First point of [qs, qe) that may keep a candidate at (cx, cy, cz) waiting: not known dead and possibly closer than the
// spacing (inside the band counts: waiting is always allowed), or NONE.  A point that is closer than the spacing for sure
// to one of the live_wn accepted points in LDS is dead as well (its cell has not looked at it since).
template <int SU>
__device__ __forceinline__ uint32_t mq_scan(const MqArgs& a, const uint64_t* __restrict__ qpos, const uint8_t* __restrict__ state,
                                            const MqLds& lds, uint32_t live_wn, uint32_t qs, uint32_t qe, float cx, float cy, float cz) {
  const uint32_t l = lane_id();
  for (uint32_t q0 = qs; q0 < qe; q0 += (uint32_t)SU * WAVE) {
    uint64_t v[SU];
    uint8_t s[SU];
#pragma unroll
    for (int u = 0; u < SU; ++u) {
      const uint32_t q = q0 + (uint32_t)u * WAVE + l;
      const bool inb = q < qe;
      v[u] = inb ? qpos[q] : 0ull;
      s[u] = inb ? state[q] : (uint8_t)QS_DEAD;
    }
#pragma unroll
    for (int u = 0; u < SU; ++u) {
      float x, y, z;
      mq_unpack(v[u], x, y, z);
      bool hit = s[u] != QS_DEAD && mq_d2(x, y, z, cx, cy, cz) < a.f_hi;
      uint64_t hb = __ballot(hit);
      if (hb && live_wn) {
        if (hit) {
          for (uint32_t i = 0; i < live_wn; ++i) {
            const float4 e = lds.list[i];
            if (mq_d2(x, y, z, e.x, e.y, e.z) < a.f_lo) {
              hit = false;
              break;
            }
          }
        }
        hb = __ballot(hit);
      }
      if (hb) return q0 + (uint32_t)u * WAVE + (uint32_t)__ffsll((unsigned long long)hb) - 1u;
    }
  }
  return QNONE;
}

// First point of [q0, qe) that is not known dead, by the state bytes alone: 1024 per look (16 bytes per lane).  qe when
// there is none.
__device__ __forceinline__ uint32_t mq_first_open(const uint8_t* __restrict__ state, uint32_t q0, uint32_t qe) {
  const uint32_t l = lane_id();
  while (q0 < qe) {
    const uint32_t base = q0 & ~15u;
    const uint32_t at = base + l * 16u;
    uint4 sb = make_uint4(0x02020202u, 0x02020202u, 0x02020202u, 0x02020202u);  // QS_DEAD
    if (at < qe) sb = *reinterpret_cast<const uint4*>(state + at);
    const uint32_t w[4] = {sb.x, sb.y, sb.z, sb.w};
    uint32_t first = 16u;  // first byte of this lane's 16 that is not dead and lies in [q0, qe)
#pragma unroll
    for (int q = 3; q >= 0; --q)
#pragma unroll
      for (int bt = 3; bt >= 0; --bt) {
        const uint32_t idx = at + (uint32_t)q * 4u + (uint32_t)bt;
        if (((w[q] >> (8 * bt)) & 0xFFu) != (uint32_t)QS_DEAD && idx >= q0 && idx < qe) first = (uint32_t)q * 4u + (uint32_t)bt;
      }
    const uint64_t hit = __ballot(first < 16u);
    if (hit) {
      const int hl = __ffsll((unsigned long long)hit) - 1;
      return base + (uint32_t)hl * 16u + qb_u32(first, hl);
    }
    q0 = base + 1024u;
  }
  return qe;
}

// mq_scan over the undecided points of a DENSE adjacent cell: most of them have been killed by the cell's reject passes
// (mq_dense_reject_kernel), so the walk jumps from one point that is not dead to the next on the state bytes.
template <int SU>
__device__ __forceinline__ uint32_t mq_scan_dense(const MqArgs& a, const uint64_t* __restrict__ qpos, const uint8_t* __restrict__ state,
                                                  const MqLds& lds, uint32_t live_wn, uint32_t qs, uint32_t qe, float cx, float cy, float cz) {
  for (uint32_t q0 = mq_first_open(state, qs, qe); q0 < qe;) {
    const uint32_t wend = (qe - q0) > (uint32_t)SU * WAVE ? q0 + (uint32_t)SU * WAVE : qe;
    const uint32_t hq = mq_scan<SU>(a, qpos, state, lds, live_wn, q0, wend, cx, cy, cz);
    if (hq != QNONE) return hq;
    q0 = mq_first_open(state, wend, qe);
  }
  return QNONE;
}

enum : uint32_t { QO_FINISHED = 0, QO_STALLED = 1, QO_YIELD = 2 };

// One wavefront advances one cell as far as it can.  U: chunks of 64 points held in registers at a time.
template <int U, bool PEERS>
__device__ void mq_activate(const MqArgs& a, uint32_t round, uint32_t qentry, const MqLds& lds, uint32_t* qout, uint32_t* cout, uint32_t seg0,
                            uint32_t ntrust, bool may_chain, uint32_t& chain_next) {
  chain_next = QNONE;
  const uint32_t l = lane_id();
  const bool woken = (qentry & MQ_WOKEN) != 0u;
  const uint32_t c = qentry & ~MQ_WOKEN;
  const uint32_t rg = a.rg, rg2s = a.rg2_shift, cap = rg - 1u;
  const float f_lo = a.f_lo, f_hi = a.f_hi;

  MQ_T(t_begin);
  // ---- first round trip: everything that hangs on the cell index alone
  const uint32_t nbv = a.qnbr[(size_t)c * 32 + (l & 31u)];
  const unsigned long long myslot = a.slot[(size_t)c * 32 + (l & 31u)];
  const uint2 ci = a.cinfo[c];
  const uint4 st = a.qst[c];
  uint4* myrec = a.rec + ((size_t)c << rg2s);
  const uint4 h0 = myrec[0], h1 = myrec[rg];
  const uint32_t sbuf = h1.z > h0.z ? 1u : 0u;  // the newer of this cell's own records (both are from earlier rounds)
  const uint32_t e = ci.y, P = sbuf ? h1.x : h0.x, CNT = sbuf ? h1.y : h0.y;
  if (P >= e) return;  // (a finished cell is never queued)
  // adjacent cell of lane k: on this shard, or -- the root of a sharded batch -- on a lower one
  const bool nb_have = nbv != QNONE;
  const uint32_t nb_peer = (PEERS && nb_have) ? (nbv >> MQ_PEER_SHIFT) : 0u;  // 0: this shard, p + 1: shard p
  const uint32_t nb_id = PEERS ? (nbv & MQ_ID_MASK) : nbv;
  // this cell once more into the next round's queue, unchanged (a look at another shard that came too early or too late)
  auto push_again = [&](uint32_t entry) {
    uint32_t base = 0, seg = (seg0 + c * 0x9E3779B1u + (c >> 7)) & (a.nseg - 1u);
    if (l == 0) {
      uint32_t tries = 0;
      for (; tries < a.nseg; ++tries) {
        base = atomicAdd(cout + (size_t)seg * 32u, 1u);
        if (base + 1u <= a.segcap) break;
        seg = (seg + 1u) & (a.nseg - 1u);
      }
      if (tries == a.nseg) atomicMax(&a.counters[CTR_ERROR], (uint32_t)SWZ_ERR_INTERNAL);
      else qout[(size_t)seg * a.segcap + base] = entry;
    }
  };
  bool claimed = woken;  // the next activation must not go through the confirm step again

  // ---- confirm: this cell stalled last time it ran and nobody has claimed its slot since
  if (!woken) {
    // (An entry without the WOKEN flag was queued by a cell that stalled and is good for THAT stall only.  When the cell
    // has been woken and run since by the wavefront that passed its blocking point -- in this very launch, see
    // mq_sweep_kernel --, there is no stall on record any more, or one of this round: the entry is void.)
    if (st.x == QNONE || st.w == round) return;
    const uint32_t bk = uni(st.y);
    const uint32_t Bv = qb_u32(nbv, (int)bk);
    const uint32_t Bp = PEERS ? (Bv >> MQ_PEER_SHIFT) : 0u, B = PEERS ? (Bv & MQ_ID_MASK) : Bv;
    if (PEERS && Bp) {
      // a cell of a lower shard: nobody wakes this one, it looks again every round
      const uint32_t rb = mq_ld_sys(a.peers.round_word[Bp - 1u]);
      if (rb == MQ_ROUND_FAILED) {  // that shard's sweep has failed: nobody will ever pass the point this cell waits for
        if (l == 0) atomicMax(&a.counters[CTR_ERROR], (uint32_t)SWZ_ERR_INTERNAL);
        return;
      }
      const uint4* brec = a.peers.rec[Bp - 1u] + ((size_t)B << rg2s);
      const uint4 b0 = mq_ld_sys(brec), b1 = mq_ld_sys(brec + rg);
      const uint32_t ra = mq_ld_sys(a.peers.round_word[Bp - 1u]);
      const bool use1 = b1.z < rb && (b0.z >= rb || b1.z > b0.z);
      const uint4 hb = use1 ? b1 : b0;
      const bool seen = ra == rb && (use1 || b0.z < rb);
      if (!seen || !(hb.x > st.z || hb.x >= hb.w)) {
        push_again(c);
        return;
      }
      claimed = true;
    } else {
    const uint4* brec = a.rec + ((size_t)B << rg2s);
    const uint4 b0 = brec[0], b1 = brec[rg];
    const bool use1 = b1.z < round && (b0.z >= round || b1.z > b0.z);
    const uint4 hb = use1 ? b1 : b0;
    const bool passed = hb.x > st.z || hb.x >= hb.w;
    if (!passed) {
      MQ_STAT(1);
      return;  // still asleep: the blocker wakes this cell when it gets there
    }
    const unsigned long long expect = ((unsigned long long)st.w << 32) | st.z;
    unsigned long long old = expect;
    if (l == 0) old = atomicCAS(&a.slot[(size_t)B * 32 + (26u - bk)], expect, QEMPTY);
    old = qb_u64(old, 0);
    if (old != expect) {
      MQ_STAT(2);
      return;  // the blocker got there first and has queued this cell for the next round
    }
    claimed = true;
    }
  }

  MQ_STAT(0);
  MQ_T(t_rt1);
  MQ_TACC(0, t_begin, t_rt1);
  // ---- second round trip: the records of the neighbourhood (staged in LDS), the window of own points at the frontier
  uint64_t pv[U];
  uint8_t ps[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const uint32_t p = P + (uint32_t)u * WAVE + l;
    const bool inb = p < e;
    pv[u] = inb ? a.qpos[p] : 0ull;
    ps[u] = inb ? a.state[p] : (uint8_t)QS_DEAD;
  }
  // Only the earlier adjacent cells and the cell itself are looked at: their records are staged side by side, by rank.
  const bool valid = l < 27u && nb_have && (nb_peer != 0u || nb_id <= c);
  const uint32_t vmask = (uint32_t)__ballot(valid);
  const uint32_t srank = (uint32_t)__popc(vmask & ((1u << (l & 31u)) - 1u));
  const uint32_t rank13 = (uint32_t)__popc(vmask & ((1u << 13) - 1u));
  if (valid) lds.sid[srank] = nbv;
  __builtin_amdgcn_wave_barrier();
  // (records of another shard: bracketed by that shard's round word -- a record stamped before the round it is in NOW is
  // complete, and it stays untouched while that round lasts; when the round has moved on meanwhile the look is repeated)
  uint32_t r_before = round;
  if (PEERS && nb_peer && l < 27u) r_before = mq_ld_sys(a.peers.round_word[nb_peer - 1u]);
  {
    const uint32_t ngran = (uint32_t)__popc(vmask) << rg2s;
    constexpr int NT = (int)(mq_staged(PEERS) * 16u + WAVE - 1u) / (int)WAVE;  // (records of 8 granules per buffer at most)
    uint4 tmp[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      const uint32_t g = (uint32_t)j * WAVE + l;
      tmp[j] = make_uint4(0u, 0u, 0u, 0u);
      if (g < ngran) {
        const uint32_t nb = lds.sid[g >> rg2s], part = g & ((1u << rg2s) - 1u);
        if (PEERS) {
          const uint32_t np = nb >> MQ_PEER_SHIFT, ni = nb & MQ_ID_MASK;
          if (np) tmp[j] = mq_ld_sys(a.peers.rec[np - 1u] + ((size_t)ni << rg2s) + part);
          else tmp[j] = ntrust ? mq_ld_agent(a.rec + ((size_t)ni << rg2s) + part) : a.rec[((size_t)ni << rg2s) + part];
        } else {
          // (a chained activation: the record its predecessor in the chain has just written must not come from this CU's L1)
          tmp[j] = ntrust ? mq_ld_agent(a.rec + ((size_t)nb << rg2s) + part) : a.rec[((size_t)nb << rg2s) + part];
        }
      }
    }
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      const uint32_t g = (uint32_t)j * WAVE + l;
      if (g < ngran) lds.stage[g] = tmp[j];
    }
  }
  __builtin_amdgcn_wave_barrier();
  if (PEERS) {
    bool late = false;
    if (nb_peer && l < 27u) late = mq_ld_sys(a.peers.round_word[nb_peer - 1u]) != r_before;
    if (__ballot(PEERS && nb_peer && l < 27u && r_before == MQ_ROUND_FAILED)) {  // a lower shard has given up
      if (l == 0) atomicMax(&a.counters[CTR_ERROR], (uint32_t)SWZ_ERR_INTERNAL);
      return;
    }
    if (__ballot(late)) {
      push_again(claimed ? (c | MQ_WOKEN) : c);
      return;
    }
  }

  MQ_T(t_rt2);
  MQ_TACC(1, t_rt1, t_rt2);
  // lane k < 27: adjacent cell k (13: this cell).  Of its two records the newer one written before this round.
  const bool earlier = valid && l != 13u;
  uint32_t n_pos = 0, n_cnt = 0, n_end = 0, pick = 0;
  if (valid) {
    const uint4 a0 = lds.stage[srank << rg2s], a1 = lds.stage[(srank << rg2s) + rg];
    uint32_t rr = (PEERS && nb_peer) ? r_before : round;  // stamps count in the owner's rounds
    if (ntrust && !(PEERS && nb_peer)) {
      // a record this very wavefront wrote earlier in the launch is complete, whatever its stamp says to the others
      bool mine = false;
      for (uint32_t j = 0; j < ntrust; ++j) mine |= lds.trust[j] == nb_id;
      if (mine) rr = round + 1u;
    }
    pick = (a1.z < rr && (a0.z >= rr || a1.z > a0.z)) ? 1u : 0u;
    const uint4 hd = pick ? a1 : a0;
    n_pos = hd.x;
    n_cnt = hd.y;
    n_end = hd.w;
  }
  // The flattened list of accepted points holds first what is NEW to this cell: the entries of adjacent cells whose record
  // was written in or after the round this cell last ran in (its own newest record carries that round) -- it could not
  // see that record then.  The points this cell tested last time (those below `tested`) only meet the new entries.
  const uint32_t my_last = sbuf ? h1.z : h0.z;
  const bool k_new = valid && l != 13u && (nb_peer != 0u || (pick ? lds.stage[(srank << rg2s) + rg].z : lds.stage[srank << rg2s].z) >= my_last);
  const uint32_t incl_new = mq_wave_scan(k_new ? n_cnt : 0u, MqAdd{}, 0u);
  const uint32_t incl_old = mq_wave_scan(k_new ? 0u : n_cnt, MqAdd{}, 0u);
  const uint32_t Tnew = qb_u32(incl_new, WAVE - 1);
  const uint32_t T = Tnew + qb_u32(incl_old, WAVE - 1);  // accepted points of the neighbourhood, own committed ones included
  const uint32_t off = k_new ? incl_new - n_cnt : Tnew + incl_old - n_cnt;
  const uint32_t maxcnt = qb_u32(mq_wave_scan(n_cnt, MqMax{}, 0u), WAVE - 1);
  const uint32_t tested = (st.x != QNONE && my_last >= MQ_FIRST_ROUND) ? st.x : P;
  // entries [base, base + MQ_LIST_CAP) of the flattened list -> LDS (lane k copies what adjacent cell k contributes;
  // the ones beyond the record's inline capacity are fetched four at a time)
  auto fill = [&](uint32_t base) -> uint32_t {
    __builtin_amdgcn_wave_barrier();
    for (uint32_t j = 0; j < maxcnt && j < cap; ++j) {
      const uint32_t ti = off + j;
      if (j < n_cnt && ti >= base && ti < base + (uint32_t)MQ_LIST_CAP) {
        *reinterpret_cast<uint4*>(&lds.list[ti - base]) = lds.stage[(srank << rg2s) + pick * rg + 1u + j];
        if (PEERS) lds.tag[ti - base] = (uint8_t)nb_peer;
      }
    }
    const float4* ovf = a.ovf;
    if (PEERS) {
      if (nb_peer) ovf = a.peers.ovf[(nb_peer - 1u) & 7u];
    }
    for (uint32_t j0 = cap; j0 < maxcnt; j0 += 2u) {  // (two loads in flight; no arrays: they would live in scratch)
      const uint32_t ja = j0, jb = j0 + 1u, ta = off + ja, tb = off + jb;
      const bool ma = ja < n_cnt && ta >= base && ta < base + (uint32_t)MQ_LIST_CAP;
      const bool mb = jb < n_cnt && tb >= base && tb < base + (uint32_t)MQ_LIST_CAP;
      uint4 sa = make_uint4(0u, 0u, 0u, 0u), sb = sa;
      if (PEERS && nb_peer) {
        if (ma) sa = mq_ld_sys(reinterpret_cast<const uint4*>(ovf + (n_end - 1u - (ja - cap))));
        if (mb) sb = mq_ld_sys(reinterpret_cast<const uint4*>(ovf + (n_end - 1u - (jb - cap))));
      } else if (ntrust) {
        if (ma) sa = mq_ld_agent(reinterpret_cast<const uint4*>(ovf + (n_end - 1u - (ja - cap))));
        if (mb) sb = mq_ld_agent(reinterpret_cast<const uint4*>(ovf + (n_end - 1u - (jb - cap))));
      } else {
        if (ma) sa = *reinterpret_cast<const uint4*>(ovf + (n_end - 1u - (ja - cap)));
        if (mb) sb = *reinterpret_cast<const uint4*>(ovf + (n_end - 1u - (jb - cap)));
      }
      if (ma) *reinterpret_cast<uint4*>(&lds.list[ta - base]) = sa;
      if (mb) *reinterpret_cast<uint4*>(&lds.list[tb - base]) = sb;
      if (PEERS) {
        if (ma) lds.tag[ta - base] = (uint8_t)nb_peer;
        if (mb) lds.tag[tb - base] = (uint8_t)nb_peer;
      }
    }
    __builtin_amdgcn_wave_barrier();
    return (T - base) < (uint32_t)MQ_LIST_CAP ? (T - base) : (uint32_t)MQ_LIST_CAP;
  };
  const uint32_t wn0 = T ? fill(0u) : 0u;
  uint32_t resident = 0;  // first entry of the list window LDS holds
  const uint32_t live_wn = (T <= (uint32_t)MQ_LIST_CAP && !a.no_dead_test) ? wn0 : 0u;  // the whole list is resident: scans can tell dead points

  MQ_T(t_fill);
  MQ_TACC(2, t_rt2, t_fill);
  uint32_t fresh = 0;
  uint32_t out_pos = e, out_status = QO_FINISHED, b_k = 0, b_q = 0;
  uint32_t tested_now = P;  // the end of the last window whose points have met the whole list
  const uint32_t S = 1u << a.cell_bits;

  for (uint32_t W0 = P; W0 < e; W0 += (uint32_t)U * WAVE) {
    float fx[U], fy[U], fz[U];
    uint32_t alive = 0;  // bit u: this lane's point of chunk u is open (neither decided nor known dead)
    if (W0 != P) {
      // Dead stretches are skipped on the state bytes alone, 1024 points per look (a cell of thousands of points -- a
      // dense blob of a clustered cloud -- is mostly dead after its first pass; window by window that was a memory round
      // trip per 64 * U points).
      while (W0 < e) {
        const uint32_t base = W0 & ~15u;
        const uint32_t at = base + l * 16u;
        uint4 sb = make_uint4(0x02020202u, 0x02020202u, 0x02020202u, 0x02020202u);  // QS_DEAD
        if (at < e) sb = *reinterpret_cast<const uint4*>(a.state + at);
        const uint32_t w[4] = {sb.x, sb.y, sb.z, sb.w};
        uint32_t first = 16u;  // first open byte of this lane's 16 that lies in [W0, e)
#pragma unroll
        for (int q = 3; q >= 0; --q)
#pragma unroll
          for (int bt = 3; bt >= 0; --bt) {
            const uint32_t idx = at + (uint32_t)q * 4u + (uint32_t)bt;
            if (((w[q] >> (8 * bt)) & 0xFFu) == (uint32_t)QS_OPEN && idx >= W0 && idx < e) first = (uint32_t)q * 4u + (uint32_t)bt;
          }
        const uint64_t hit = __ballot(first < 16u);
        if (hit) {
          const int hl = __ffsll((unsigned long long)hit) - 1;
          W0 = base + (uint32_t)hl * 16u + qb_u32(first, hl);
          break;
        }
        W0 = base + 1024u;
      }
      if (W0 >= e) break;
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const uint32_t p = W0 + (uint32_t)u * WAVE + l;
        const bool inb = p < e;
        pv[u] = inb ? a.qpos[p] : 0ull;
        ps[u] = inb ? a.state[p] : (uint8_t)QS_DEAD;
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      mq_unpack(pv[u], fx[u], fy[u], fz[u]);
      alive |= (ps[u] == QS_OPEN ? 1u : 0u) << u;
    }
    tested_now = W0 + (uint32_t)U * WAVE;
    if (!__ballot(alive != 0u)) continue;  // a window of dead points

    // (R) against the committed accepted points of the neighbourhood, window by window, then against the points
    // accepted earlier in this activation (they matter for the windows after the first).  The kernel is bound by its
    // vector ALU work here (a root cell's first activation: 478 points x 40 accepted points), so every chunk first
    // finds the list entries that can matter to it at all -- one lane per ENTRY: is it within reach of the bounding
    // box of the chunk's open points? -- and tests only those.  64 consecutive points in Morton order fill a small
    // block, and on later activations the few open points of a cell a tiny one: most entries drop out.
    // Per chunk the smallest squared key distance to a tested entry decides: below f_lo some accepted point is closer
    // than the spacing for sure; below f_hi at least one pair lies inside the band and goes to the exact compare.
    {
      // Levels of small cells (one chunk per window) first find the entries that can matter at all -- one lane per
      // ENTRY: is it within reach of the bounding box of the open points? -- and test only those: a coarsened cell of
      // level 1 sees ~120 accepted points around it, and a point can be close to a handful.  Cells of hundreds of
      // points (several chunks per window) gain nothing from that on their first activation; they save on the later
      // ones by testing the points they have tested before against the new entries only.
      float bx0 = 0.f, bx1 = 0.f, by0 = 0.f, by1 = 0.f, bz0 = 0.f, bz1 = 0.f;
      if (U == 1) {
        const bool al = alive & 1u;
        const uint32_t hi_id = 0xFFFFFFFFu;  // coordinates are non-negative floats: their bit patterns order like they do
        bx0 = __uint_as_float(qb_u32(mq_wave_scan(al ? __float_as_uint(fx[0]) : hi_id, MqMin{}, hi_id), WAVE - 1));
        by0 = __uint_as_float(qb_u32(mq_wave_scan(al ? __float_as_uint(fy[0]) : hi_id, MqMin{}, hi_id), WAVE - 1));
        bz0 = __uint_as_float(qb_u32(mq_wave_scan(al ? __float_as_uint(fz[0]) : hi_id, MqMin{}, hi_id), WAVE - 1));
        bx1 = __uint_as_float(qb_u32(mq_wave_scan(al ? __float_as_uint(fx[0]) : 0u, MqMax{}, 0u), WAVE - 1));
        by1 = __uint_as_float(qb_u32(mq_wave_scan(al ? __float_as_uint(fy[0]) : 0u, MqMax{}, 0u), WAVE - 1));
        bz1 = __uint_as_float(qb_u32(mq_wave_scan(al ? __float_as_uint(fz[0]) : 0u, MqMax{}, 0u), WAVE - 1));
      }
      // chunks whose points were all tested by the last activation (uniform)
      uint32_t oldc = 0;
#pragma unroll
      for (int u = 0; u < U; ++u)
        if (W0 + (uint32_t)(u + 1) * WAVE <= tested) oldc |= 1u << u;
      uint32_t nearb = 0;
      for (uint32_t base = 0;; base += (uint32_t)MQ_LIST_CAP) {
        const bool last = base >= T;  // the extra pass: the points accepted earlier in this activation
        uint32_t wn = fresh;
        if (!last) {
          if (oldc == (1u << U) - 1u && base >= Tnew) {  // nothing in this window of the list is new to any chunk
            base = T;  // (on to the pass over the points accepted in this activation)
            continue;
          }
          if (resident != base) {
            (void)fill(base);
            resident = base;
          }
          wn = (T - base) < (uint32_t)MQ_LIST_CAP ? (T - base) : (uint32_t)MQ_LIST_CAP;
        }
        const float4* lst = last ? lds.fresh : lds.list;
        float dmin[U];
#pragma unroll
        for (int u = 0; u < U; ++u) dmin[u] = __builtin_inff();
        if (U == 1) {
          const uint32_t lim = (last || !(oldc & 1u)) ? wn : (Tnew > base ? ((Tnew - base) < wn ? (Tnew - base) : wn) : 0u);
          for (uint32_t b0 = 0; b0 < lim; b0 += WAVE) {
            bool rel = false;  // lane i: is entry b0 + i within reach of the box?
            if (b0 + l < lim) {
              const float4 en = lst[b0 + l];
              const float gx = fmaxf(fmaxf(bx0 - en.x, en.x - bx1), 0.f);
              const float gy = fmaxf(fmaxf(by0 - en.y, en.y - by1), 0.f);
              const float gz = fmaxf(fmaxf(bz0 - en.z, en.z - bz1), 0.f);
              rel = __builtin_fmaf(gz, gz, __builtin_fmaf(gy, gy, gx * gx)) < f_hi;
            }
            uint64_t rm = __ballot(rel);
            while (rm) {
              const int bit = __ffsll((unsigned long long)rm) - 1;
              rm &= rm - 1ull;
              const float4 en = lst[b0 + (uint32_t)bit];
              dmin[0] = fminf(dmin[0], mq_d2(fx[0], fy[0], fz[0], en.x, en.y, en.z));
            }
          }
        } else {
          // every entry against every chunk -- only the new ones when all chunks met the others last time
          const uint32_t nnew = last ? wn : (Tnew > base ? ((Tnew - base) < wn ? (Tnew - base) : wn) : 0u);
          const uint32_t lim = oldc == (1u << U) - 1u ? nnew : wn;
          for (uint32_t i = 0; i < lim; ++i) {
            const float4 en = lst[i];
#pragma unroll
            for (int u = 0; u < U; ++u) dmin[u] = fminf(dmin[u], mq_d2(fx[u], fy[u], fz[u], en.x, en.y, en.z));
          }
        }
        uint32_t pend = 0;
#pragma unroll
        for (int u = 0; u < U; ++u) {
          nearb |= (dmin[u] < f_lo ? 1u : 0u) << u;
          pend |= (dmin[u] >= f_lo && dmin[u] < f_hi ? 1u : 0u) << u;
        }
        pend &= alive & ~nearb;
        if (__ballot(pend != 0u)) {  // pairs inside the band: the exact compare on the original positions
          for (uint32_t i = 0; i < wn; ++i) {
            const float4 en = lst[i];
#pragma unroll
            for (int u = 0; u < U; ++u) {
              if ((pend >> u) & 1u) {
                const float d2 = mq_d2(fx[u], fy[u], fz[u], en.x, en.y, en.z);
                if (d2 >= f_lo && d2 < f_hi &&
                    ((PEERS && !last) ? mq_exact_near_peer(a, W0 + (uint32_t)u * WAVE + l, __float_as_uint(en.w), lds.tag[i])
                                      : mq_exact_near(a, W0 + (uint32_t)u * WAVE + l, __float_as_uint(en.w)))) {
                  nearb |= 1u << u;
                  pend &= ~(1u << u);
                }
              }
            }
          }
        }
        if (last) break;
      }
      const uint32_t died = alive & nearb;
#pragma unroll
      for (int u = 0; u < U; ++u)
        if ((died >> u) & 1u) a.state[W0 + (uint32_t)u * WAVE + l] = QS_DEAD;
      alive &= ~nearb;
    }

    MQ_T(t_r);
    MQ_TACC(3, t_fill, t_r);
    // (A) surviving points in order: accept, or stall on a possibly undecided earlier point
    bool stop = false;
    for (;;) {
      int cu = -1;
      uint64_t bm = 0;
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const uint64_t b = __ballot((alive >> u) & 1u);
        if (cu < 0 && b) {
          cu = u;
          bm = b;
        }
      }
      if (cu < 0) break;
      const int j = __ffsll((unsigned long long)bm) - 1;
      const uint32_t cand = W0 + (uint32_t)cu * WAVE + (uint32_t)j;
      float cx = 0.f, cy = 0.f, cz = 0.f;
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (u == cu) {
          cx = qb_f32(fx[u], j);
          cy = qb_f32(fy[u], j);
          cz = qb_f32(fz[u], j);
        }
      }
      // earlier adjacent cells that still hold undecided points and lie within reach of the candidate (gap between its
      // key cell and the adjacent cell, per axis: a point over there differs by more than that many cells)
      uint32_t need;
      {
        const uint32_t lx = (uint32_t)cx & (S - 1u), ly = (uint32_t)cy & (S - 1u), lz = (uint32_t)cz & (S - 1u);
        const uint32_t dxk = l / 9u, dyk = (l / 3u) % 3u, dzk = l % 3u;
        const float gx = dxk == 0u ? (float)lx : (dxk == 2u ? (float)(S - 1u - lx) : 0.f);
        const float gy = dyk == 0u ? (float)ly : (dyk == 2u ? (float)(S - 1u - ly) : 0.f);
        const float gz = dzk == 0u ? (float)lz : (dzk == 2u ? (float)(S - 1u - lz) : 0.f);
        const float gap2 = __builtin_fmaf(gz, gz, __builtin_fmaf(gy, gy, gx * gx));
        need = (uint32_t)__ballot(earlier && n_pos < n_end && gap2 < f_hi);
      }
      bool blocked = false;
      // (Measured and dropped, both on the 100 M clustered cloud: not scanning an adjacent cell that still has thousands of
      // undecided points within reach but waiting for all of it -- root 105 -> 140 .. 180 ms: dense cells overlap, a cell
      // moves on as soon as the one point that blocks it has been passed --, and the reverse, cutting long scans short.)
      while (need && !blocked) {
        const int k = __ffs((int)need) - 1;
        need &= need - 1u;
        const uint32_t qs = qb_u32(n_pos, k), qe = qb_u32(n_end, k);
        MQ_STAT(4);
        const uint32_t kp = PEERS ? qb_u32(nb_peer, k) : 0u;
        // (Measured and dropped: a scan that reads the state bytes first and fetches the coordinates of the open points
        // only.  Where it would pay -- the dense blob of a clustered cloud -- the root went 107 -> 101 ms; on uniform data,
        // whose neighbours' points are mostly still open when they are scanned, 73 -> 113 ms.)
        uint32_t hq;
        if (U > 1 && a.dense_min && !kp && qe - qs >= a.dense_min)
          hq = mq_scan_dense<4>(a, a.qpos, a.state, lds, live_wn, qs, qe, cx, cy, cz);
        else
          hq = mq_scan<(U > 1 ? 4 : 1)>(a, kp ? a.peers.qpos[kp - 1u] : a.qpos, kp ? a.peers.state[kp - 1u] : a.state, lds, live_wn, qs, qe,
                                        cx, cy, cz);
        if (hq != QNONE) {
          blocked = true;
          b_k = (uint32_t)k;
          b_q = a.patient ? qe - 1u : hq;
        }
      }
      if (blocked) {
        MQ_STAT(3);
        out_pos = cand;
        out_status = QO_STALLED;
        stop = true;
        break;
      }
      // accepted
      if ((int)l == j) {
        a.taken[cand] = 1;
        a.state[cand] = QS_TAKEN;
        alive &= ~(1u << cu);
      }
      if (l == 0) lds.fresh[fresh] = make_float4(cx, cy, cz, __uint_as_float(cand));
      ++fresh;
      // the points it rejects (all open points of the window are later ones)
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if ((alive >> u) & 1u) {
          const float d2 = mq_d2(fx[u], fy[u], fz[u], cx, cy, cz);
          bool nr = d2 < f_lo;
          if (!nr && d2 < f_hi) nr = mq_exact_near(a, W0 + (uint32_t)u * WAVE + l, cand);
          if (nr) {
            a.state[W0 + (uint32_t)u * WAVE + l] = QS_DEAD;
            alive &= ~(1u << u);
          }
        }
      }
      __builtin_amdgcn_wave_barrier();
      if (fresh == (uint32_t)MQ_FRESH_CAP) {  // LDS list full: publish and go on in the next round
        uint32_t next = W0 + (uint32_t)U * WAVE;
#pragma unroll
        for (int u = U - 1; u >= 0; --u) {
          const uint64_t b = __ballot((alive >> u) & 1u);
          if (b) next = W0 + (uint32_t)u * WAVE + (uint32_t)__ffsll((unsigned long long)b) - 1u;
        }
        if (next < e) {
          out_pos = next;
          out_status = QO_YIELD;
          stop = true;
        }
        break;
      }
    }
    if (stop) break;
    // (Measured and dropped: cells of thousands of points taking their turn in slices of 1024 .. 4096 points, so that a
    // launch does not last as long as its longest activation -- the clustered root went 105 -> 120 .. 153 ms.)
    // (... or a dense cell that has accepted a point: what that point rejects in the thousands of points behind it is
    // killed by a whole workgroup between the launches, mq_dense_reject_kernel, and the walk goes on next round)
    if ((fresh == (uint32_t)MQ_FRESH_CAP || (U > 1 && fresh && a.dense_min && e - ci.x >= a.dense_min)) &&
        W0 + (uint32_t)U * WAVE < e) {  // (full exactly at the end of a window)
      out_pos = W0 + (uint32_t)U * WAVE;
      out_status = QO_YIELD;
      break;
    }
  }

  MQ_T(t_cand);
  MQ_TACC(4, t_fill, t_cand);
  // ---- publish: the new record goes into the buffer that does NOT hold the newest one
  const uint32_t wb = sbuf ^ 1u;
  const uint32_t ncnt = CNT + fresh;
  __builtin_amdgcn_wave_barrier();
  for (uint32_t j = l; j < ncnt && j < cap; j += WAVE) {
    uint4 src;
    if (j < CNT) src = lds.stage[(rank13 << rg2s) + sbuf * rg + 1u + j];
    else src = *reinterpret_cast<const uint4*>(&lds.fresh[j - CNT]);
    myrec[wb * rg + 1u + j] = src;
  }
  for (uint32_t jj = l; jj < fresh; jj += WAVE) {
    const uint32_t j = CNT + jj;
    if (j >= cap) a.ovf[e - 1u - (j - cap)] = lds.fresh[jj];
  }
  const bool fin = out_pos >= e;
  if (l == 0) {
    myrec[wb * rg] = make_uint4(fin ? e : out_pos, ncnt, round, e);
    a.qst[c] = out_status == QO_STALLED ? make_uint4(tested_now, b_k, b_q, round) : make_uint4(QNONE, 0u, 0u, 0u);
  }
  if (U > 1 && a.dirty && fresh && l < 27u && nb_have && nb_peer == 0u) a.dirty[nb_id] = 1;  // (k = 13: the cell itself)
  // ---- wake the later adjacent cells that sleep on a point the frontier has passed (slots written in THIS round belong
  // to cells that confirm themselves next round); go to sleep / come back next round
  bool won = false;
  if (l < 27u && nb_have && nb_peer == 0u && nb_id > c && myslot != QEMPTY && (uint32_t)(myslot >> 32) != round &&
      (fin || (uint32_t)myslot < out_pos)) {
    won = atomicCAS(&a.slot[(size_t)c * 32 + l], myslot, QEMPTY) == myslot;
  }
  if (out_status == QO_STALLED && l == 0) {
    const uint32_t Bv = qb_u32(nbv, (int)uni(b_k));
    // (a blocker on a lower shard has no slot for this cell: it confirms itself every round until the point is passed)
    if (!(PEERS && (Bv >> MQ_PEER_SHIFT))) a.slot[(size_t)(PEERS ? (Bv & MQ_ID_MASK) : Bv) * 32 + (26u - b_k)] = ((unsigned long long)round << 32) | b_q;
  }
  uint64_t wm = __ballot(won);
  if (may_chain && wm) {
    // the first sleeper this activation has woken is run by this wavefront right away, in this launch: it will read the
    // record just written (complete: same wavefront, program order) instead of waiting a round for it
    const int first = __ffsll((unsigned long long)wm) - 1;
    chain_next = qb_u32(nb_id, first);
    wm &= wm - 1ull;
    if ((int)l == first) won = false;
  }
  const uint32_t self = fin ? 0u : 1u;
  const uint32_t total = (uint32_t)__popcll(wm) + self;
  if (total) {
    // into one segment of the next round's queue -- chosen by the cell so that the work spreads over all workgroups
    // whatever this one read -- or, that one full, into the next that has room (the segments hold twice the cells
    // between them and a round never has more entries than cells)
    uint32_t base = 0, seg = (seg0 + c * 0x9E3779B1u + (c >> 7)) & (a.nseg - 1u);
    if (l == 0) {
      uint32_t tries = 0;
      for (; tries < a.nseg; ++tries) {
        base = atomicAdd(cout + (size_t)seg * 32u, total);
        if (base + total <= a.segcap) break;
        seg = (seg + 1u) & (a.nseg - 1u);
      }
      if (tries == a.nseg) {
        atomicMax(&a.counters[CTR_ERROR], (uint32_t)SWZ_ERR_INTERNAL);
        base = QNONE;
      }
    }
    base = qb_u32(base, 0);
    seg = qb_u32(seg, 0);
    if (base != QNONE) {
      uint32_t* q = qout + (size_t)seg * a.segcap + base;
      if (won) q[(uint32_t)__popcll(wm & lanemask_lt())] = nb_id | MQ_WOKEN;
      if (self && l == 0) q[(uint32_t)__popcll(wm)] = out_status == QO_YIELD ? (c | MQ_WOKEN) : c;
    }
  }
  MQ_T(t_end);
  MQ_TACC(5, t_cand, t_end);
  MQ_TACC(6, t_begin, t_end);
#ifdef SWZ_MQ_STATS
  if (l == 0 && (c & 31u) == 0u) atomicAdd(&a.counters[CTR_DBG_HIST + 8 + 7], 1u);
#endif
}

template <int U, bool PEERS>
__global__ __launch_bounds__(WAVE, (U == 1 && !PEERS) ? MQ_MINW1 : ((U == 4 && !PEERS) ? MQ_MINW4 : 4)) void mq_sweep_kernel(MqArgs a, uint32_t round) {
  extern __shared__ uint4 mq_smem[];
  MqLds lds;
  lds.stage = mq_smem;
  lds.list = reinterpret_cast<float4*>(mq_smem + mq_staged(PEERS) * 2u * a.rg);
  lds.fresh = lds.list + MQ_LIST_CAP;
  lds.tag = reinterpret_cast<uint8_t*>(lds.fresh + MQ_FRESH_CAP);
  lds.trust = reinterpret_cast<uint32_t*>(lds.tag + MQ_LIST_CAP);
  lds.sid = lds.trust + MQ_CHAIN;
  const uint32_t r0 = round - MQ_FIRST_ROUND;
  const uint32_t ci = r0 % 3u, co = (r0 + 1u) % 3u, cz = (r0 + 2u) % 3u;
  if (blockIdx.x == 0) {  // the counters the round after the next will fill; this round's total for the host
    const uint32_t l = lane_id();
    uint32_t mine = 0;
    for (uint32_t sg = l; sg < a.nseg; sg += WAVE) {
      a.qctr[((size_t)cz * a.nseg + sg) * 32u] = 0;
      a.qhead[((size_t)cz * a.nseg + sg) * 32u] = 0;
      const uint32_t n = a.qctr[((size_t)ci * a.nseg + sg) * 32u];
      mine += n < a.segcap ? n : a.segcap;
    }
    const uint32_t tot = qb_u32(mq_wave_scan(mine, MqAdd{}, 0u), WAVE - 1);
    if (l == 0) a.qtotal[ci] = tot;
  }
  const uint32_t seg = blockIdx.x & (a.nseg - 1u);
  uint32_t nq = a.qctr[((size_t)ci * a.nseg + seg) * 32u];
  nq = nq < a.segcap ? nq : a.segcap;  // (a counter overshoots when a push found the segment full and went elsewhere)
  const uint32_t* qin = a.queue[r0 & 1u] + (size_t)seg * a.segcap;
  uint32_t* qout = a.queue[(r0 + 1u) & 1u];
  uint32_t* cout = a.qctr + (size_t)co * a.nseg * 32u;
  // The workgroups of a segment draw its entries by ticket: activations differ in cost by an order of magnitude (a
  // confirm that finds its cell still asleep, a first activation of 500 points), and with a fixed stride the launch
  // lasts as long as its unluckiest workgroup.  The next ticket is requested before the current entry is worked on.
  uint32_t* head = a.qhead + ((size_t)ci * a.nseg + seg) * 32u;
  uint32_t i = blockIdx.x >> a.nseg_shift;  // the first entries go by position: no ticket needed
  const uint32_t wgs = gridDim.x >> a.nseg_shift;
  uint32_t entry = qin[i < a.segcap ? i : 0u];  // (requested together with the segment's count, not after it)
  while (i < nq) {
    uint32_t next = 0;
    if (lane_id() == 0) next = atomicAdd(head, 1u);  // (the result is first looked at after the activation)
    // the entry, then -- one after the other -- a chain of cells each woken by the one before: a dependency that this
    // wavefront resolves itself does not cost a round
    uint32_t cur = uni(entry), ntrust = 0;
    for (;;) {
      uint32_t woke = QNONE;
      mq_activate<U, PEERS>(a, round, cur, lds, qout, cout, seg, ntrust, ntrust + 1u < a.chain, woke);
      woke = uni(woke);
      if (woke == QNONE) break;
      if (lane_id() == 0) lds.trust[ntrust] = cur & ~MQ_WOKEN;
      ++ntrust;
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // what the cell has published has reached the L2 the next one reads from
      __builtin_amdgcn_wave_barrier();
      cur = woke | MQ_WOKEN;
    }
    i = wgs + qb_u32(next, 0);
    if (i < nq) entry = qin[i];
  }
}

// ---- dense cells
// A cell of thousands of points (a blob or a sheet of a clustered cloud) is walked by ONE wavefront, 256 points per
// memory round trip, and a launch lasts as long as its longest activation.  Almost all of those points are rejected by
// the handful of accepted points around them, so that part is taken out of the walk: a dense cell yields after it has
// accepted a point, every activation that publishes accepted points marks the cells around it, and between two launches
// one WORKGROUP per marked dense cell tests the cell's undecided points against the accepted points of the earlier
// adjacent cells (and its own) that are new since its last pass, and marks what they reject dead.  That is all it does
// -- a dead point is one that some published accepted earlier point rejects, which is what the state means anyway --, so
// the walk and the blocker scans of the others then jump over the killed stretches on the state bytes, 1024 points per
// look.  Pairs inside the band are left to the walk (it has the exact compare).
constexpr uint32_t MQ_DENSE_LIST = 256;  // accepted points a reject pass looks at (the rest waits for the walk)
__global__ __launch_bounds__(256) void mq_dense_reject_kernel(MqArgs a, uint32_t round) {
  __shared__ float4 lst[MQ_DENSE_LIST];
  __shared__ uint32_t cnt;
  const uint32_t c = a.dlist[blockIdx.x];
  if (!a.dirty[c]) return;  // (the same byte for the whole workgroup; cleared below, after everybody has read it)
  const uint32_t tid = threadIdx.x;
  const uint32_t rg = a.rg, rg2s = a.rg2_shift, cap = rg - 1u;
  const uint4* myrec = a.rec + ((size_t)c << rg2s);
  const uint4 h0 = myrec[0], h1 = myrec[rg];
  const uint4 mine = h1.z > h0.z ? h1 : h0;  // (no launch is running: both records are complete, the newer one counts)
  const uint32_t P = mine.x, e = a.cinfo[c].y;
  const uint32_t since = a.bulk_round[c];
  if (tid == 0) cnt = 0;
  __syncthreads();
  if (tid == 0) {
    a.dirty[c] = 0;
    a.bulk_round[c] = round + 1u;
  }
  if (P >= e) return;
  // the accepted points of the earlier adjacent cells and of the cell itself whose record is new since the last pass
  if (tid < 27u) {
    const uint32_t nb = a.qnbr[(size_t)c * 32 + tid];
    if (nb != QNONE && nb <= c) {
      const uint4* r = a.rec + ((size_t)nb << rg2s);
      const uint4 a0 = r[0], a1 = r[rg];
      const uint32_t pick = a1.z > a0.z ? 1u : 0u;
      const uint4 hd = pick ? a1 : a0;
      if (hd.z >= since && hd.y) {
        const uint32_t at = atomicAdd(&cnt, hd.y);
        for (uint32_t j = 0; j < hd.y && at + j < MQ_DENSE_LIST; ++j) {
          uint4 en;
          if (j < cap) en = r[pick * rg + 1u + j];
          else en = *reinterpret_cast<const uint4*>(a.ovf + (hd.w - 1u - (j - cap)));
          lst[at + j] = make_float4(__uint_as_float(en.x), __uint_as_float(en.y), __uint_as_float(en.z), 0.f);
        }
      }
    }
  }
  __syncthreads();
  const uint32_t n = cnt < MQ_DENSE_LIST ? cnt : MQ_DENSE_LIST;
  if (!n) return;
  for (uint32_t p = P + tid; p < e; p += 256u) {
    if (a.state[p] != QS_OPEN) continue;
    float x, y, z;
    mq_unpack(a.qpos[p], x, y, z);
    bool dead = false;
    for (uint32_t i = 0; i < n && !dead; ++i) dead = mq_d2(x, y, z, lst[i].x, lst[i].y, lst[i].z) < a.f_lo;
    if (dead) a.state[p] = QS_DEAD;
  }
}

// Sharded root: the round this shard's sweep is in, for the shards that read its records.  A launch of its own BETWEEN
// two rounds: when a reader sees round R here, every record stamped before R is complete (round R - 1 has finished and
// written back) and round R only ever writes the OLDER buffer of a cell -- a store from inside the sweep would become
// visible some time into the round, when that is no longer true.
__global__ void mq_round_word_kernel(uint32_t* word, uint32_t value) {
  __hip_atomic_store(word, value, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// A level whose taken bytes carry a code (LevelPlan::take_code): the sweep's own stores went to the state bytes (MqArgs::taken
// is the state array then, and 1 is QS_TAKEN), and this pass writes the level's code for every accepted point -- the bytes
// of points taken further up stay what they are.  Four points per thread.
__global__ __launch_bounds__(256) void mq_commit_kernel(const uint8_t* __restrict__ state, uint32_t m, uint8_t code, uint8_t* __restrict__ taken) {
  const uint64_t i0 = ((uint64_t)blockIdx.x * 256u + threadIdx.x) * 4u;
  if (i0 >= m) return;
  if (m - i0 >= 4u) {
    const uint32_t sw = *reinterpret_cast<const uint32_t*>(state + i0);
    uint32_t hit = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (((sw >> (8 * j)) & 0xFFu) == (uint32_t)QS_TAKEN) hit |= 0xFFu << (8 * j);
    if (!hit) return;
    uint32_t* w = reinterpret_cast<uint32_t*>(taken + i0);
    *w = (*w & ~hit) | ((0x01010101u * (uint32_t)code) & hit);
  } else {
    for (uint32_t j = 0; i0 + j < m; ++j)
      if (state[i0 + j] == QS_TAKEN) taken[i0 + j] = code;
  }
}

// after the last round: every cell must have reached its end (a protocol error would otherwise go unnoticed)
__global__ __launch_bounds__(256) void mq_verify_kernel(MqArgs a, uint32_t ncells, uint32_t* __restrict__ open_cells) {
  const uint32_t c = blockIdx.x * 256 + threadIdx.x;
  bool open = false;
  if (c < ncells) {
    const uint4* r = a.rec + ((size_t)c << a.rg2_shift);
    const uint4 h0 = r[0], h1 = r[a.rg];
    const uint4 h = h1.z > h0.z ? h1 : h0;
    open = h.x < h.w;
  }
  const uint64_t bm = __ballot(open);
  if (bm && lane_id() == 0) atomicAdd(open_cells, (uint32_t)__popcll(bm));
}

// ----------------------------------------------------------------------------- host
// The build of the sweep a level runs: four chunks per window for cells of hundreds of points, the peers' records at the
// joint root of a sharded batch.
using MqSweepFn = void (*)(MqArgs, uint32_t);
static MqSweepFn mq_sweep_fn(bool big_cells, bool peers) {
  if (peers) return big_cells ? mq_sweep_kernel<4, true> : mq_sweep_kernel<1, true>;
  return big_cells ? mq_sweep_kernel<4, false> : mq_sweep_kernel<1, false>;
}

// one wavefront per workgroup, as many as are resident at once (registers and LDS decide), a multiple of the segments
uint32_t mq_sweep_grid(swz_ctx* c, const MqLevel& q) {
  const MqArgs& a = q.a;
  int dev = 0, cus = 0, per_cu = 0;
  (void)hipGetDevice(&dev);
  (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
  // (The build WITHOUT peers is asked, with the LDS bytes of the one that runs: at the joint root of a sharded batch that is
  // not the kernel launched.  Kept as it is: the grid decides the schedule, and the schedule's numbers were measured so.)
  const hipError_t oe = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, mq_sweep_fn(q.big_cells, false), WAVE, mq_lds_bytes(a.rg, q.sharded));
  if (oe != hipSuccess || per_cu < 1) per_cu = 8;
  if (cus < 1) cus = 256;
  uint32_t cap = (uint32_t)cus * (uint32_t)per_cu;
  if (const char* e = c->opt("SWZ_MD_GRID")) cap = (uint32_t)std::max(1, atoi(e)) * 4u;
  return std::max(a.nseg, (std::min<uint32_t>(cap / q.groups, q.ncells) + a.nseg - 1u) / a.nseg * a.nseg);
}

// round q.round of node group g, on the group's stream
void mq_launch_round(const MqLevel& q, uint32_t g, uint32_t sweep_grid) {
  if (q.sharded) hipLaunchKernelGGL(mq_round_word_kernel, dim3(1), dim3(1), 0, q.gs[g], q.a.round_word, q.round);
  hipLaunchKernelGGL(mq_sweep_fn(q.big_cells, q.sharded), dim3(sweep_grid), dim3(WAVE), mq_lds_bytes(q.a.rg, q.sharded), q.gs[g], q.ga[g], q.round);
  if (q.ndense)  // (only a level of large cells in one group, not sharded, has any: mq_list_dense_cells)
    hipLaunchKernelGGL(mq_dense_reject_kernel, dim3(q.ndense), dim3(256), 0, q.gs[g], q.ga[g], q.round);
}

void mq_set_round_word(hipStream_t stream, uint32_t* word, uint32_t value) {
  hipLaunchKernelGGL(mq_round_word_kernel, dim3(1), dim3(1), 0, stream, word, value);
}

// every cell at its end, no queue segment ever full everywhere
int mq_verify(swz_ctx* c, MqLevel& q) {
  uint32_t* d_open = nullptr;
  SWZ_TRY(c->get("md_qopen", (size_t)4, &d_open));
  SWZ_HIP(c, hipMemsetAsync(d_open, 0, 4, c->stream));
  hipLaunchKernelGGL(mq_verify_kernel, dim3(div_up(q.ncells, 256)), dim3(256), 0, c->stream, q.a, q.ncells, d_open);
  SWZ_LAUNCH_CHECK(c);
  uint32_t open_cells = 0, err = 0;
  SWZ_HIP(c, hipMemcpyAsync(&open_cells, d_open, 4, hipMemcpyDeviceToHost, c->stream));
  for (uint32_t g = 0; g < q.groups; ++g) {
    uint32_t eg = 0;
    SWZ_HIP(c, hipMemcpyAsync(&eg, q.ga[g].counters + CTR_ERROR, 4, hipMemcpyDeviceToHost, c->stream));
    SWZ_HIP(c, hipStreamSynchronize(c->stream));
    err |= eg;
  }
  if (open_cells || err) {
    char msg[200];
    snprintf(msg, sizeof(msg), "MIN_DISTANCE sweep on keys ended with %u of %u cells undecided at level %d after %u rounds (queue overflow: %s)",
             open_cells, q.ncells, q.L.plan.level, q.round - MQ_FIRST_ROUND, err ? "yes" : "no");
    return c->fail(SWZ_ERR_INTERNAL, msg);
  }
  return SWZ_OK;
}

int mq_commit(swz_ctx* c, MqLevel& q) {
  if (!q.coded) return SWZ_OK;
  hipLaunchKernelGGL(mq_commit_kernel, dim3(div_up(q.a.m, 1024)), dim3(256), 0, c->stream, q.a.state, q.a.m, q.L.plan.take_code, q.L.lb.taken);
  SWZ_LAUNCH_CHECK(c);
  return SWZ_OK;
}

}  // namespace swz
