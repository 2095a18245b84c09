// swz_tstore.hip -- the node store and the pools of the multi-batch tiler (swz_tiler.h): where the files of a level lie,
// how a side or a pool grows -- on the device, or spilled to mapped host memory --, the node table, compaction.
#include <algorithm>
#include <cstring>

#include "swz_tiler.h"

namespace swz {

// ---------------------------------------------------------------------------------------------- kernels
struct HeadF {
  const uint64_t* key;
  uint32_t nsh;
  __device__ uint32_t operator()(uint32_t i) const { return (i == 0 || (key[i] >> nsh) != (key[i - 1] >> nsh)) ? 1u : 0u; }
};
struct HeadG {
  const uint64_t* key;
  uint32_t nsh;
  uint32_t* head_pos;
  uint64_t* head_key;
  __device__ void operator()(uint32_t i, uint32_t excl, uint32_t h) const {
    if (!h) return;
    head_pos[excl] = i;
    head_key[excl] = nsh >= 63 ? 0ull : ((key[i] >> nsh) << nsh);
  }
};

// ---- node table of a level store (log form)
__global__ __launch_bounds__(256) void tl_table_build_kernel(const uint64_t* __restrict__ hk, const uint32_t* __restrict__ hp,
                                                             uint32_t heads, uint32_t cnt, uint64_t* __restrict__ nkey,
                                                             uint64_t* __restrict__ noff, uint32_t* __restrict__ ncnt) {
  const uint32_t j = blockIdx.x * 256 + threadIdx.x;
  if (j >= heads) return;
  nkey[j] = hk[j];
  noff[j] = hp[j];
  ncnt[j] = (j + 1 < heads ? hp[j + 1] : cnt) - hp[j];
}
// segments j = 0 .. segs-1 of a source array, segment j = [psrc[j], +len_j) with len_j = poff[j+1] - poff[j]
// (poff[segs] = total), copied one behind the other: output element e belongs to the last segment that starts at or
// before e.  A workgroup's 256 consecutive outputs lie in consecutive segments: two searches over all of poff bracket
// them, every thread then searches the bracket (out of LDS when it is short).
constexpr uint32_t TL_SEG_LDS = 1024;
__device__ __forceinline__ uint32_t tl_upper_u32(const uint32_t* __restrict__ a, uint32_t lo, uint32_t hi, uint32_t k) {
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (a[mid] <= k) lo = mid + 1; else hi = mid;
  }
  return lo;
}
__global__ __launch_bounds__(256) void tl_gather_files_kernel(const uint32_t* __restrict__ poff, const uint64_t* __restrict__ psrc,
                                                              uint32_t segs, uint32_t total, const uint64_t* __restrict__ skey,
                                                              const uint32_t* __restrict__ sgid, uint64_t* __restrict__ okey,
                                                              uint32_t* __restrict__ ogid) {
  __shared__ uint32_t s_lo, s_hi;
  __shared__ uint32_t so[TL_SEG_LDS];
  const uint32_t tid = threadIdx.x;
  const uint32_t e0 = blockIdx.x * 256u, e = e0 + tid;
  const uint32_t last = (total - e0) > 256u ? e0 + 255u : total - 1u;
  if (tid < 2) {  // (two lanes of one wavefront: see tl_merge_rank_kernel)
    const uint32_t r = tl_upper_u32(poff, 0u, segs, tid ? last : e0) - 1u;
    if (tid) s_hi = r; else s_lo = r;
  }
  __syncthreads();
  const uint32_t lo = s_lo, span = s_hi - s_lo + 1u;
  const bool in_lds = span <= TL_SEG_LDS;
  if (in_lds)
    for (uint32_t j = tid; j < span; j += 256u) so[j] = poff[lo + j];
  __syncthreads();
  if (e >= total) return;
  const uint32_t j = in_lds ? lo + tl_upper_u32(so, 0u, span, e) - 1u : tl_upper_u32(poff, lo, lo + span, e) - 1u;
  const uint64_t src = psrc[j] + (e - poff[j]);
  okey[e] = skey[src];
  ogid[e] = sgid[src];
}
struct SegCntF {
  const uint32_t* cnt;
  __device__ uint32_t operator()(uint32_t i) const { return cnt[i]; }
};
struct SegMoveG {  // the files of a table, gathered one behind the other: where each goes, where it came from
  uint64_t* off;
  uint32_t* poff;
  uint64_t* psrc;
  __device__ void operator()(uint32_t i, uint32_t excl, uint32_t) const {
    poff[i] = excl;
    psrc[i] = off[i];
    off[i] = excl;
  }
};

// ---------------------------------------------------------------------------------------------- host
// Grows a named workspace buffer keeping its first `keep` bytes.  A POOL (spill == true) that finds no device memory
// -- hipMalloc out of memory, or the workspace above SWZ_TILER_DEVICE_BUDGET_MB -- moves to page-locked host memory mapped
// into the device's address space and stays there: the pools hold 24 bytes + the attribute rows of EVERY point of the
// data set, the bulk of a tiler's memory, and the tiling touches them lightly -- a batch's own points once, in order
// (clamp + index), the cached points a batch pulls in by id (re-key), MIN_DISTANCE's rare exact compares; the
// attribute columns not at all until the files are exported.  The kernels read and write them in place over the host
// link.  SWZ_TILER_SPILL: "auto" (default), "host" (pools on the host from the start), "off".
static int grow_preserving(swz_ctx* c, const char* name, size_t bytes, size_t keep, void** out, bool spill) {
  swz::DevBuf& b = c->bufs[name];
  if (b.cap < bytes) {
    void* np = nullptr;
    const size_t want = (bytes + 255) & ~size_t(255);
    int policy = 1;
    if (const char* e = c->opt("SWZ_TILER_SPILL")) policy = strcmp(e, "off") == 0 ? 0 : (strcmp(e, "host") == 0 ? 2 : 1);
    if (!spill) policy = 0;
    hipError_t e = hipErrorOutOfMemory;
    if (policy != 2 && !b.host) {  // (a pool that has moved to the host does not come back)
      bool over_budget = false;
      if (const char* bm = c->opt("SWZ_TILER_DEVICE_BUDGET_MB"))
        over_budget = policy != 0 && (c->held_bytes() + want) > (uint64_t)atoll(bm) * 1048576ull;
      if (!over_budget) e = hipMalloc(&np, want);
      if (const char* fa = c->opt("SWZ_FAIL_ALLOC"))
        if (e == hipSuccess && strcmp(fa, name) == 0) {
          (void)hipFree(np);
          np = nullptr;
          e = hipErrorOutOfMemory;
        }
    }
    bool host = false;
    if (e == hipErrorOutOfMemory && policy != 0) {
      (void)hipGetLastError();
      e = hipHostMalloc(&np, want, hipHostMallocMapped | hipHostMallocPortable);
      host = e == hipSuccess;
    }
    if (e != hipSuccess) return c->fail(SWZ_ERR_HIP, std::string("hipMalloc(") + name + "): " + hipGetErrorString(e));
    if (b.ptr && keep) SWZ_HIP(c, hipMemcpy(np, b.ptr, keep, hipMemcpyDefault));
    if (const char* e = c->opt("SWZ_POISON")) {  // (like swz_ctx::get: what nobody has written yet must not read as zeros)
      const char* only = c->opt("SWZ_POISON_ONLY");
      if (!only || strstr(name, only)) {
        if (host) {
          memset((char*)np + keep, atoi(e), want - keep);
        } else {  // (complete before anybody's stream writes into the buffer: hipMemset may return early)
          SWZ_HIP(c, hipMemset((char*)np + keep, atoi(e), want - keep));
          SWZ_HIP(c, hipDeviceSynchronize());
        }
      }
    }
    c->free_buf(b);
    b.ptr = np;
    b.cap = want;
    b.host = host;
  }
  *out = b.ptr;
  return SWZ_OK;
}

// The node store and the pools live in the context's grow-only workspace under fixed names, so a tiler created after
// another one on the same context reuses the memory (hipMalloc / hipFree of multi-GB blocks were measured to stall for
// seconds now and then).  One tiler per context at a time.
int store_reserve(swz_ctx* c, StoreLevel& s, int level_index, int which, size_t count) {
  if (s.cap[which] >= count && s.key[which]) return SWZ_OK;
  const size_t want = count + count / 4 + 1024;
  const std::string kn = "tiler_store_key_" + std::to_string(level_index) + "_" + std::to_string(which);
  const std::string gn = "tiler_store_gid_" + std::to_string(level_index) + "_" + std::to_string(which);
  // (the side being written holds nothing that is still needed: nothing is kept.  Like the pools, a store side that finds
  // no device memory -- or would push the workspace over SWZ_TILER_DEVICE_BUDGET_MB -- is placed in mapped pinned host
  // memory: the merges then stream through it over the host link, slowly, but a data set whose node store outgrows the
  // device still tiles.  The growth policy of the workspace (twice the old capacity) applies here as well.)
  const size_t old_k = c->bufs[kn].cap / sizeof(uint64_t);
  const size_t grown = std::max(want, std::min<size_t>(2 * old_k, want + (size_t(1) << 27)));
  void *pk = nullptr, *pg = nullptr;
  SWZ_TRY(grow_preserving(c, kn.c_str(), grown * sizeof(uint64_t), 0, &pk, true));
  SWZ_TRY(grow_preserving(c, gn.c_str(), grown * sizeof(uint32_t), 0, &pg, true));
  s.key[which] = static_cast<uint64_t*>(pk);
  s.gid[which] = static_cast<uint32_t*>(pg);
  s.cap[which] = std::min(c->bufs[kn].cap / sizeof(uint64_t), c->bufs[gn].cap / sizeof(uint32_t));
  return SWZ_OK;
}

// side `which` has just been written as a whole: `cnt` entries, node after node
void store_written_linear(StoreLevel& s, int which, uint32_t cnt, bool rekeyed) {
  s.cur = which;
  s.cnt = s.end = cnt;
  s.linear = true;
  s.table_valid = false;
  s.nn = 0;
  s.rekeyed = rekeyed || cnt == 0;
}

int table_reserve(swz_ctx* c, StoreLevel& s, int level_index, int which, size_t count) {
  // (part of the store: placed like its sides -- SWZ_TILER_SPILL=host leaves nothing of a tiler on the device)
  const std::string sfx = std::to_string(level_index) + "_" + std::to_string(which);
  auto one = [&](const std::string& name, size_t elem, void** out) -> int {
    const size_t have = c->bufs[name].cap / elem;
    const size_t want = have >= count && c->bufs[name].ptr ? have : count + count / 2 + 1024;
    return grow_preserving(c, name.c_str(), want * elem, 0, out, true);
  };
  void *pk = nullptr, *po = nullptr, *pc = nullptr;
  SWZ_TRY(one("tiler_store_tab_key_" + sfx, 8, &pk));
  SWZ_TRY(one("tiler_store_tab_off_" + sfx, 8, &po));
  SWZ_TRY(one("tiler_store_tab_cnt_" + sfx, 4, &pc));
  s.nkey[which] = static_cast<uint64_t*>(pk);
  s.noff[which] = static_cast<uint64_t*>(po);
  s.ncnt[which] = static_cast<uint32_t*>(pc);
  return SWZ_OK;
}

int node_heads_scan(swz_ctx* c, const uint64_t* keys, uint32_t n, uint32_t shift, uint32_t** hp, uint64_t** hk, uint32_t** d_heads) {
  uint32_t* counters = nullptr;
  SWZ_TRY(c->get("tl_counters", (size_t)4, &counters));
  SWZ_TRY(c->get("tl_head_pos", (size_t)n, hp));
  SWZ_TRY(c->get("tl_head_key", (size_t)n, hk));
  *d_heads = counters + 3;
  return fused_scan(c, HeadF{keys, shift}, HeadG{keys, shift, *hp, *hk}, n, *d_heads, "tl");
}
int node_heads(swz_ctx* c, const uint64_t* keys, uint32_t n, uint32_t shift, uint32_t** hp, uint64_t** hk, uint32_t* heads) {
  uint32_t* d_heads = nullptr;
  SWZ_TRY(node_heads_scan(c, keys, n, shift, hp, hk, &d_heads));
  return read_u32(c, d_heads, heads);
}

// the node table of a level in linear form: the runs of equal node prefix
int store_table(swz_ctx* c, StoreLevel& s, int level_index) {
  if (s.table_valid) return SWZ_OK;
  if (!s.linear) return c->fail(SWZ_ERR_INTERNAL, "node store: neither linear nor indexed");
  s.nn = 0;
  if (s.cnt) {
    uint32_t* hp = nullptr;
    uint64_t* hk = nullptr;
    uint32_t heads = 0;
    SWZ_TRY(node_heads(c, s.key[s.cur], s.cnt, store_shift(level_index), &hp, &hk, &heads));
    SWZ_TRY(table_reserve(c, s, level_index, s.ncur, heads));
    hipLaunchKernelGGL(tl_table_build_kernel, dim3(div_up(heads, 256)), dim3(256), 0, c->stream, hk, hp, heads, s.cnt,
                       s.nkey[s.ncur], s.noff[s.ncur], s.ncnt[s.ncur]);
    SWZ_LAUNCH_CHECK(c);
    s.nn = heads;
  }
  s.table_valid = true;
  return SWZ_OK;
}

int gather_files(swz_ctx* c, const uint32_t* poff, const uint64_t* psrc, uint32_t segs, uint32_t total, const uint64_t* skey,
                 const uint32_t* sgid, uint64_t* okey, uint32_t* ogid) {
  hipLaunchKernelGGL(tl_gather_files_kernel, dim3(div_up(total, 256)), dim3(256), 0, c->stream, poff, psrc, segs, total, skey, sgid,
                     okey, ogid);
  SWZ_LAUNCH_CHECK(c);
  return SWZ_OK;
}

uint32_t gather_lds() { return TL_SEG_LDS; }

// Gathers the files a table lists (ntab entries, `live` entries in all, in table order) into the other side, which gets
// room for `room` entries, and makes it the current one; off[] (device) is rewritten to the new places.
int store_compact(swz_ctx* c, StoreLevel& s, int level_index, uint64_t* off, const uint32_t* cnt, uint32_t ntab,
                  uint32_t live, size_t room) {
  const int dst = s.cur ^ 1;
  SWZ_TRY(store_reserve(c, s, level_index, dst, std::max<size_t>(room, live)));
  if (ntab && live) {
    uint32_t *poff = nullptr, *counters = nullptr;
    uint64_t* psrc = nullptr;
    SWZ_TRY(c->get("tl_counters", (size_t)4, &counters));
    SWZ_TRY(c->get("tl_poff", (size_t)ntab, &poff));
    SWZ_TRY(c->get("tl_psrc", (size_t)ntab, &psrc));
    SWZ_TRY(fused_scan(c, SegCntF{cnt}, SegMoveG{off, poff, psrc}, ntab, counters + 2, "tl"));
    SWZ_TRY(gather_files(c, poff, psrc, ntab, live, s.key[s.cur], s.gid[s.cur], s.key[dst], s.gid[dst]));
  }
  s.cur = dst;
  s.end = live;
  return SWZ_OK;
}
// log form -> linear form (the table stays valid)
int store_linearize(swz_tiler* t, StoreLevel& s, int level_index) {
  swz_ctx* c = t->c;
  if (s.linear) return SWZ_OK;
  if (!s.table_valid) return c->fail(SWZ_ERR_INTERNAL, "node store: log without a table");
  SWZ_TRY(store_compact(c, s, level_index, s.noff[s.ncur], s.ncnt[s.ncur], s.nn, s.cnt, s.cnt));
  s.linear = true;
  ++t->paths[TP_LINEARIZE_MOVED];
  return SWZ_OK;
}

// the taken entries (tkey, tgid) become the level's files as a whole: written to the other side, which becomes the current one
int store_write_linear(swz_ctx* c, StoreLevel& dst, int level_index, const uint64_t* tkey, const uint32_t* tgid, uint32_t nt) {
  const int w = dst.cur ^ 1;
  SWZ_TRY(store_reserve(c, dst, level_index, w, nt));
  SWZ_HIP(c, hipMemcpyAsync(dst.key[w], tkey, (size_t)nt * 8, hipMemcpyDeviceToDevice, c->stream));
  SWZ_HIP(c, hipMemcpyAsync(dst.gid[w], tgid, (size_t)nt * 4, hipMemcpyDeviceToDevice, c->stream));
  store_written_linear(dst, w, nt, false);
  return SWZ_OK;
}

// makes room for `points` points in the pools (positions and the attribute columns in use); keeps the content
int pool_reserve(swz_tiler* t, size_t points) {
  swz_ctx* c = t->c;
  if (points <= t->pool_cap && t->pool_xyz) return SWZ_OK;
  // nothing may still be writing into or reading from the old pools
  if (t->copy_stream) SWZ_HIP(c, hipStreamSynchronize(t->copy_stream));
  SWZ_HIP(c, hipStreamSynchronize(c->stream));
  size_t have = c->bufs["tiler_pool_xyz"].cap / 24;  // what an earlier tiler of this context left behind
  for (int a = 0; a < SWZ_ATTR_COUNT; ++a)
    if (t->attr_mask & (1u << a)) have = std::min(have, c->bufs["tiler_pool_attr" + std::to_string(a)].cap / TILER_ATTR_BYTES[a]);
  const size_t want = points <= have ? have : std::max(points, t->pool_cap + t->pool_cap / 2);
  const size_t used = t->staged_total;
  void* px = nullptr;
  SWZ_TRY(grow_preserving(c, "tiler_pool_xyz", want * 24, used * 24, &px, true));
  t->pool_xyz = static_cast<double*>(px);
  for (int a = 0; a < SWZ_ATTR_COUNT; ++a) {
    if (!(t->attr_mask & (1u << a))) continue;
    const std::string name = "tiler_pool_attr" + std::to_string(a);
    SWZ_TRY(grow_preserving(c, name.c_str(), want * TILER_ATTR_BYTES[a], used * TILER_ATTR_BYTES[a], &t->pool_attr[a], true));
  }
  t->pool_cap = want;
  return SWZ_OK;
}

}  // namespace swz
