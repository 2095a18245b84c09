// swz_tlevel.hip -- one level of a batch of the multi-batch tiler (tile_node, TilingAlgorithms.cpp:351-492): the files of the
// nodes the batch reaches are pulled out of the level's store, merged with the active set and sampled (level_step); the
// taken points become those nodes' new files, the rest goes down a level.  tiler_level is the entry point.
#include <algorithm>

#include "swz_tiler.h"

namespace swz {

// ---------------------------------------------------------------------------------------------- kernels
// read_pnts_from_disk, TilingAlgorithms.cpp:80-99: idx = node.morton_index; levels node.level+1 .. 20 are levels
// 0 .. of the index of the position inside node.bounds (bounds by descending octant by octant from the root).
// The result depends on the point's position and on the NODE (the top level+1 digits of `old`) only, not on the lower
// digits of `old`: re-keying a re-keyed entry of the same node changes nothing.
__device__ __forceinline__ uint64_t rekey_one(uint64_t old, const double* __restrict__ pool, size_t g, const Box& root, int level) {
  const Box nb = bounds_from_key(old, root, level + 1);
  const uint64_t rel = morton_in_box(pool[3 * g], pool[3 * g + 1], pool[3 * g + 2], nb);
  const uint32_t start_level = (uint32_t)(level + 1);
  const uint64_t prefix = start_level == 0 ? 0ull : ((old >> level_shift(level)) << level_shift(level));
  return prefix | (rel >> (3u * start_level));
}
__global__ __launch_bounds__(256) void tl_rekey_kernel(uint64_t* __restrict__ ckey, const uint32_t* __restrict__ cgid,
                                                       uint32_t nc, const double* __restrict__ pool, Box root,
                                                       int level) {
  const uint32_t j = blockIdx.x * 256 + threadIdx.x;
  if (j >= nc) return;
  ckey[j] = rekey_one(ckey[j], pool, cgid[j], root, level);
}

// pairs of neighbours inside one node (same prefix >> nsh) whose keys descend
__global__ __launch_bounds__(256) void tl_inversion_kernel(const uint64_t* __restrict__ key, uint32_t n, uint32_t nsh,
                                                           uint32_t* __restrict__ count) {
  const uint32_t j = blockIdx.x * 256 + threadIdx.x;
  const bool bad = j > 0 && j < n && (key[j] >> nsh) == (key[j - 1] >> nsh) && key[j] < key[j - 1];
  const uint64_t b = __ballot(bad);
  if (lane_id() == 0 && b) atomicAdd(count, (uint32_t)__popcll(b));
}

// point ids of the pulled points into the working pool, behind the batch's own points -- and their positions (SoA) when
// the working pool keeps positions (X != null; see work_need_positions)
__global__ __launch_bounds__(256) void tl_fill_kernel(const uint32_t* __restrict__ cgid, uint32_t nc,
                                                      const double* __restrict__ pool, double* __restrict__ X,
                                                      double* __restrict__ Y, double* __restrict__ Z,
                                                      uint32_t* __restrict__ wgid) {
  const uint32_t j = blockIdx.x * 256 + threadIdx.x;
  if (j >= nc) return;
  const size_t g = cgid[j];
  if (wgid) wgid[j] = (uint32_t)g;
  if (!X || g == 0xFFFFFFFFu) return;  // (the ghosts of a sharded root have no id: their positions were written with them)
  X[j] = pool[3 * g];
  Y[j] = pool[3 * g + 1];
  Z[j] = pool[3 * g + 2];
}

// std::merge(first, second, comp = key <): elements of `first` precede equal elements of `second`.
// Keys are compared after >> sh (sh = node shift merges by node only: merge_node_data_unsorted's "new ++ cached").
// Stable merge of two sorted runs by rank: an element's place is its own index plus the number of elements of the other
// run that go before it (first run: strictly smaller keys; second run: smaller or equal -- the first run wins ties, like
// std::merge).  The 256 consecutive elements of a workgroup are sorted, so the ranks of its first and last element bracket
// all others: two searches over the whole other run per workgroup, then every thread searches that bracket only -- out of
// LDS when it holds at most 1024 keys (runs of similar length interleave: a few hundred), instead of ~25 dependent probes
// all over a run of tens of millions of keys per element.
constexpr uint32_t TL_MERGE_LDS = 2048;
constexpr uint32_t TL_MERGE_IPT = 4;                    // elements per thread: the two searches over the whole other run that
constexpr uint32_t TL_MERGE_TILE = 256 * TL_MERGE_IPT;  // open a workgroup (~23 dependent loads each) serve 1024 elements
template <bool UPPER>
__device__ __forceinline__ uint32_t tl_rank(const uint64_t* __restrict__ k, uint32_t lo, uint32_t hi, uint64_t ks, uint32_t sh) {
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    const uint64_t v = k[mid] >> sh;
    if (UPPER ? (v <= ks) : (v < ks)) lo = mid + 1; else hi = mid;
  }
  return lo;
}
// run `a` (n_a elements, values va or `base + index`) against the other run `b`; UPPER: a is the second run
template <bool UPPER>
__global__ __launch_bounds__(256) void tl_merge_rank_kernel(const uint64_t* __restrict__ ka, const uint32_t* __restrict__ va, uint32_t na,
                                                            const uint64_t* __restrict__ kb, uint32_t nb, uint32_t sh, uint32_t base,
                                                            uint64_t* __restrict__ ok, uint32_t* __restrict__ ov) {
  __shared__ uint32_t s_lo, s_hi;
  __shared__ uint64_t sk[TL_MERGE_LDS];
  const uint32_t tid = threadIdx.x;
  const uint32_t i0 = blockIdx.x * TL_MERGE_TILE;
  const uint32_t last = (na - i0) > TL_MERGE_TILE ? i0 + TL_MERGE_TILE - 1u : na - 1u;
  // (both searches by two lanes of the first wavefront.  With the second one on thread 64 -- alone in its wavefront, so
  // hipcc 7.2 turns its search into scalar loads -- and more than one element per thread, the shift count of the loops
  // below came out of a register that only some wavefronts had set: wrong ranks for threads 128-255.  Found with a
  // stand-alone copy of this kernel against std::merge.)
  if (tid < 2) {
    const uint32_t r = tl_rank<UPPER>(kb, 0u, nb, ka[tid ? last : i0] >> sh, sh);
    if (tid) s_hi = r; else s_lo = r;
  }
  __syncthreads();
  const uint32_t lo = s_lo, hi = s_hi;
  const bool in_lds = hi - lo <= TL_MERGE_LDS;
  if (in_lds)
    for (uint32_t j = tid; j < hi - lo; j += 256u) sk[j] = kb[lo + j] >> sh;
  __syncthreads();
  for (uint32_t q = 0; q < TL_MERGE_IPT; ++q) {
    const uint32_t i = i0 + q * 256u + tid;
    if (i >= na) break;
    const uint64_t k = ka[i];
    const uint64_t ks = k >> sh;
    uint32_t r;
    if (in_lds) r = lo + tl_rank<UPPER>(sk, 0u, hi - lo, ks, 0u);
    else r = tl_rank<UPPER>(kb, lo, hi, ks, sh);
    ok[i + r] = k;
    ov[i + r] = va ? va[i] : base + i;
  }
}

// The level loop's store step: the taken points of the merged range become the new files of their nodes, written
// straight behind the files the side already holds.  An entry that did not come out of this level's files (a point of
// the batch, or one an ancestor handed down) gets the key the reference would compute when it reads the file back
// (rekey_one) -- once, here, instead of with every later batch that pulls the file; entries pulled from this level's
// files carry that key already.  The first `ghosts` taken entries are a sharded root's ghosts: not part of the file.
struct TakeStoreG {
  const uint64_t* mkey;
  const uint32_t* midx;
  const uint32_t* wgid;
  uint32_t pull_lo, pull_hi;  // working indices of what this level pulled
  uint32_t ghosts;
  const double* pool;
  Box root;
  int level;
  uint64_t* okey;
  uint32_t* ogid;
  uint32_t nsh;
  uint32_t* texcl;  // [i]: taken entries in front of merged entry i, written where a node starts (-> the heads of the new files)
  __device__ void operator()(uint32_t i, uint32_t excl, uint32_t t) const {
    if (i == 0 || (mkey[i] >> nsh) != (mkey[i - 1] >> nsh)) texcl[i] = excl;
    if (!t || excl < ghosts) return;
    const uint32_t w = midx ? midx[i] : i;
    const uint32_t g = wgid[w];
    uint64_t k = mkey[i];
    if ((w < pull_lo || w >= pull_hi) && g != 0xFFFFFFFFu) k = rekey_one(k, pool, g, root, level);
    okey[excl - ghosts] = k;
    ogid[excl - ghosts] = g;
  }
};

__device__ __forceinline__ uint32_t tl_lower_u64(const uint64_t* __restrict__ a, uint32_t n, uint64_t k) {
  uint32_t lo = 0, hi = n;
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (a[mid] < k) lo = mid + 1; else hi = mid;
  }
  return lo;
}
// the files of the nodes the active set reaches: head j of the active set -> its node's file (if it has one)
struct PullCntF {
  const uint64_t* hk;
  const uint64_t* nkey;
  const uint32_t* ncnt;
  uint32_t nn;
  __device__ uint32_t find(uint64_t k) const {
    const uint32_t r = tl_lower_u64(nkey, nn, k);
    return (r < nn && nkey[r] == k) ? r : 0xFFFFFFFFu;
  }
  __device__ uint32_t operator()(uint32_t j) const {
    const uint32_t r = find(hk[j]);
    return r == 0xFFFFFFFFu ? 0u : ncnt[r];
  }
};
struct PullSegG {
  PullCntF f;
  const uint64_t* noff;
  uint32_t* poff;
  uint64_t* psrc;
  uint8_t* touched;
  __device__ void operator()(uint32_t j, uint32_t excl, uint32_t) const {
    const uint32_t r = f.find(f.hk[j]);
    poff[j] = excl;
    psrc[j] = r == 0xFFFFFFFFu ? 0ull : noff[r];
    if (r != 0xFFFFFFFFu) touched[r] = 1;
  }
};
struct UntouchedF {
  const uint8_t* touched;  // null: every node counts
  __device__ uint32_t operator()(uint32_t i) const { return (touched && touched[i]) ? 0u : 1u; }
};
struct TableFilterG {
  const uint64_t* nkey;
  const uint64_t* noff;
  const uint32_t* ncnt;
  uint64_t* fkey;
  uint64_t* foff;
  uint32_t* fcnt;
  __device__ void operator()(uint32_t i, uint32_t excl, uint32_t keep) const {
    if (!keep) return;
    fkey[excl] = nkey[i];
    foff[excl] = noff[i];
    fcnt[excl] = ncnt[i];
  }
};
// the heads of the files a level step has just written: node j of the merged range starts at merged entry nstart[j], its
// file at the number of taken entries in front of that (texcl, TakeStoreG) -- no scan over the new files
__global__ __launch_bounds__(256) void tl_new_heads_kernel(const uint64_t* __restrict__ mkey, const uint32_t* __restrict__ nstart,
                                                           const uint32_t* __restrict__ texcl, uint32_t nodes, uint32_t nsh, uint32_t ghosts,
                                                           uint64_t* __restrict__ hk, uint32_t* __restrict__ hp) {
  const uint32_t j = blockIdx.x * 256 + threadIdx.x;
  if (j >= nodes) return;
  const uint32_t i = nstart[j];
  hk[j] = nsh >= 63u ? 0ull : ((mkey[i] >> nsh) << nsh);
  const uint32_t e = texcl[i];
  hp[j] = e > ghosts ? e - ghosts : 0u;
}
// two node tables with disjoint keys, both ascending, into one: the entries the batch left alone (f*) and the heads of
// the files it wrote (keys hk at positions hp of the `added` entries appended at `base`)
__global__ __launch_bounds__(256) void tl_table_merge_kernel(const uint64_t* __restrict__ fkey, const uint64_t* __restrict__ foff,
                                                             const uint32_t* __restrict__ fcnt, uint32_t nf,
                                                             const uint64_t* __restrict__ hk, const uint32_t* __restrict__ hp,
                                                             uint32_t heads, uint32_t added, uint64_t base,
                                                             uint64_t* __restrict__ okey, uint64_t* __restrict__ ooff,
                                                             uint32_t* __restrict__ ocnt) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i < nf) {
    const uint32_t o = i + tl_lower_u64(hk, heads, fkey[i]);
    okey[o] = fkey[i];
    ooff[o] = foff[i];
    ocnt[o] = fcnt[i];
  } else if (i < nf + heads) {
    const uint32_t j = i - nf;
    const uint32_t o = j + tl_lower_u64(fkey, nf, hk[j]);
    okey[o] = hk[j];
    ooff[o] = base + hp[j];
    ocnt[o] = (j + 1 < heads ? hp[j + 1] : added) - hp[j];
  }
}
__global__ __launch_bounds__(256) void tl_iota_base_kernel(uint32_t* __restrict__ out, uint32_t n, uint32_t base) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) out[i] = base + i;
}
__global__ __launch_bounds__(256) void tl_count_untaken_kernel(const uint8_t* __restrict__ taken, uint32_t n,
                                                               uint32_t* __restrict__ count) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  const uint64_t b = __ballot(i < n && !taken[i]);
  if (lane_id() == 0 && b) atomicAdd(count, (uint32_t)__popcll(b));
}

// ---------------------------------------------------------------------------------------------- host helpers
int fill_from_pool(swz_ctx* c, const uint32_t* gid, uint32_t n, const double* pool, double* wx, double* wy, double* wz,
                   uint32_t* wgid) {
  hipLaunchKernelGGL(tl_fill_kernel, dim3(div_up(n, 256)), dim3(256), 0, c->stream, gid, n, pool, wx, wy, wz, wgid);
  SWZ_LAUNCH_CHECK(c);
  return SWZ_OK;
}

int merge_pairs(swz_ctx* c, const uint64_t* k1, const uint32_t* v1, uint32_t n1, const uint64_t* k2,
                const uint32_t* v2, uint32_t n2, uint32_t sh, uint32_t base2, uint64_t* ok, uint32_t* ov) {
  if (n1) {
    hipLaunchKernelGGL(tl_merge_rank_kernel<false>, dim3(div_up(n1, TL_MERGE_TILE)), dim3(256), 0, c->stream, k1, v1, n1, k2, n2, sh, 0u, ok, ov);
    SWZ_LAUNCH_CHECK(c);
  }
  if (n2) {
    hipLaunchKernelGGL(tl_merge_rank_kernel<true>, dim3(div_up(n2, TL_MERGE_TILE)), dim3(256), 0, c->stream, k2, v2, n2, k1, n1, sh, base2, ok, ov);
    SWZ_LAUNCH_CHECK(c);
  }
  return SWZ_OK;
}
uint32_t merge_tile() { return TL_MERGE_TILE; }
uint32_t merge_lds() { return TL_MERGE_LDS; }

// (key, gid) ascending by key when the re-keyed order is not (the reference only sorts for a lossy persistence,
// :103-106 / :1690-1692; counted in rekey_inversions)
int sort_pairs_by_key(swz_ctx* c, uint64_t* key, uint32_t* gid, uint32_t n) {
  uint64_t* kb = nullptr;
  uint32_t* vb = nullptr;
  SWZ_TRY(c->get("tl_sort_k", (size_t)n, &kb));
  SWZ_TRY(c->get("tl_sort_v", (size_t)n, &vb));
  SWZ_HIP(c, hipMemcpyAsync(kb, key, (size_t)n * 8, hipMemcpyDeviceToDevice, c->stream));
  SWZ_HIP(c, hipMemcpyAsync(vb, gid, (size_t)n * 4, hipMemcpyDeviceToDevice, c->stream));
  SWZ_TRY(radix_sort_pairs(c, kb, vb, key, gid, n, false));
  return SWZ_OK;
}

// Re-sorts (key, gid) only if the order has an inversion inside a node (same key >> shift) -- one read-back
int resort_if_inverted(swz_tiler* t, uint64_t* key, uint32_t* gid, uint32_t n, uint32_t shift) {
  swz_ctx* c = t->c;
  uint32_t* counters = nullptr;
  SWZ_TRY(c->get("tl_counters", (size_t)4, &counters));
  SWZ_HIP(c, hipMemsetAsync(counters + 1, 0, 4, c->stream));
  hipLaunchKernelGGL(tl_inversion_kernel, dim3(div_up(n, 256)), dim3(256), 0, c->stream, key, n, shift, counters + 1);
  SWZ_LAUNCH_CHECK(c);
  uint32_t inv = 0;
  SWZ_TRY(read_u32(c, counters + 1, &inv));
  if (inv) {
    t->rekey_inversions += inv;
    ++t->paths[TP_RESORT];
    SWZ_TRY(sort_pairs_by_key(c, key, gid, n));
  }
  return SWZ_OK;
}

// The working pool keeps positions (SoA, by working index) only from the first level on that reads them: RANDOM_GRID never
// does, MIN_DISTANCE / GRID_CENTER / JITTERED decide on key coordinates and look up the position pool through the point ids
// (level_decides_on_keys) -- a batch of a usual data set never fills them.  Levels that do read them (bounds that are no
// cube, spacings of fewer than 64 key cells, re-rooted nodes, the ghosts of a sharded root) fill everything that is in the
// working pool by then, from the ids; entries pulled in later are filled as they come.
int work_need_positions(swz_tiler* t, BatchWork& w) {
  if (w.have_pos) return SWZ_OK;
  swz_ctx* c = t->c;
  // (24 bytes per working-pool entry -- batch + everything stored -- that most data sets never touch: allocated here, not
  // with the batch.  At 2.4 B stored points the three arrays were 78 of the 286 GB that ran the device out of memory.)
  SWZ_TRY(c->get("tl_wx", (size_t)w.wcap, &w.wx));
  SWZ_TRY(c->get("tl_wy", (size_t)w.wcap, &w.wy));
  SWZ_TRY(c->get("tl_wz", (size_t)w.wcap, &w.wz));
  if (w.wused) SWZ_TRY(fill_from_pool(c, w.wgid, w.wused, t->pool_xyz, w.wx, w.wy, w.wz, nullptr));
  w.have_pos = true;
  return SWZ_OK;
}

// ---------------------------------------------------------------------------------------------- the level's three steps
// what level_pull copied out of the level's files
struct LevelPull {
  uint64_t* ckey = nullptr;
  uint32_t* cgid = nullptr;
  uint32_t nc = 0;
  uint8_t* touched = nullptr;  // per node of the level's table: the batch rewrites its file
  bool all_touched = false;
  uint32_t pull_lo = 0;        // working indices of the pulled entries: [pull_lo, pull_lo + nc)
};

// ---- pull the files of the nodes this level's active set reaches
static int level_pull(swz_tiler* t, BatchWork& w, const LevelPlan& plan, const ActiveSet& as, const ShardRoot* sr, LevelPull* p) {
  swz_ctx* c = t->c;
  StoreLevel& st = t->lv[plan.level + 1];
  const uint32_t nsh = plan.node_shift;
  uint32_t* counters = nullptr;
  SWZ_TRY(c->get("tl_counters", (size_t)4, &counters));
  const int lvi = plan.level + 1;
  if (st.cnt && sr) {  // the root is reached by the batch as a whole: all of its local file
    SWZ_TRY(store_linearize(t, st, lvi));
    SWZ_TRY(store_table(c, st, lvi));
    SWZ_TRY(c->get("tl_ckey", (size_t)st.cnt, &p->ckey));
    SWZ_TRY(c->get("tl_cgid", (size_t)st.cnt, &p->cgid));
    SWZ_HIP(c, hipMemcpyAsync(p->ckey, st.key[st.cur], (size_t)st.cnt * 8, hipMemcpyDeviceToDevice, c->stream));
    SWZ_HIP(c, hipMemcpyAsync(p->cgid, st.gid[st.cur], (size_t)st.cnt * 4, hipMemcpyDeviceToDevice, c->stream));
    p->nc = st.cnt;
    p->all_touched = true;
  } else if (st.cnt) {
    // (profile class "tiler_pull": the nodes of the active set, their files looked up in the level's node table and
    // copied out -- what the batch reaches, not what the level holds)
    SWZ_TRY(store_table(c, st, lvi));
    uint32_t *hp = nullptr, *d_heads = nullptr;
    uint64_t* hk = nullptr;
    SWZ_TRY(c->get("tl_ntouch", (size_t)st.nn, &p->touched));
    uint32_t heads = 0;
    {
      ProfScope ps(c, "tiler_pull", (uint64_t)as.m * 8ull, 2);
      SWZ_TRY(node_heads_scan(c, as.akey, as.m, nsh, &hp, &hk, &d_heads));
      SWZ_HIP(c, hipMemsetAsync(p->touched, 0, (size_t)st.nn, c->stream));
    }
    SWZ_TRY(read_u32(c, d_heads, &heads));
    uint32_t* poff = nullptr;
    uint64_t* psrc = nullptr;
    SWZ_TRY(c->get("tl_poff", (size_t)heads, &poff));
    SWZ_TRY(c->get("tl_psrc", (size_t)heads, &psrc));
    const PullCntF pf{hk, st.nkey[st.ncur], st.ncnt[st.ncur], st.nn};
    SWZ_TRY(fused_scan(c, pf, PullSegG{pf, st.noff[st.ncur], poff, psrc, p->touched}, heads, counters, "tl"));
    SWZ_TRY(read_u32(c, counters, &p->nc));
    if (p->nc == st.cnt && st.linear) {
      // the batch reaches every node of the level and the side holds the files in node order (a batch cut out of the whole
      // cloud): what would be copied out is the side itself.  Everything on it is rewritten by this batch -- behind its end
      // or on the other side --, so the merge may read it in place (and a re-sort after an inversion may reorder it).
      p->ckey = st.key[st.cur];
      p->cgid = st.gid[st.cur];
      ++t->paths[TP_PULL_IN_PLACE];
    } else if (p->nc) {
      ++t->paths[TP_PULL_GATHERED];
      ProfScope ps(c, "tiler_pull", (uint64_t)p->nc * 24ull, 1);
      SWZ_TRY(c->get("tl_ckey", (size_t)p->nc, &p->ckey));
      SWZ_TRY(c->get("tl_cgid", (size_t)p->nc, &p->cgid));
      SWZ_TRY(gather_files(c, poff, psrc, heads, p->nc, st.key[st.cur], st.gid[st.cur], p->ckey, p->cgid));
    }
  } else {
    SWZ_TRY(store_table(c, st, lvi));  // (an empty level: an empty table)
  }
  p->pull_lo = w.wused;
  return SWZ_OK;
}

// ---- re-key and merge what was pulled with the active set (and the ghosts of a sharded root in front): *ms
static int level_merge(swz_tiler* t, BatchWork& w, const LevelPlan& plan, const ActiveSet& as, const ShardRoot* sr,
                       const LevelPull& p, ActiveSet* ms) {
  swz_ctx* c = t->c;
  StoreLevel& st = t->lv[plan.level + 1];
  const uint32_t nsh = plan.node_shift;
  const uint32_t ng = sr ? sr->ghosts : 0u;
  uint64_t* const ckey = p.ckey;
  uint32_t* const cgid = p.cgid;
  const uint32_t nc = p.nc;
  *ms = as;
  if (ng) SWZ_TRY(work_need_positions(t, w));  // (the ghosts bring their positions: the working pool holds them from here on)
  if (!nc && !ng) return SWZ_OK;
  if (nc && !st.rekeyed) {
    // ("tiler_rekey": the pulled points' keys against their NODE's bounds -- a random 24-byte read per point from the
    // pool; only for files the level loop did not write itself, see TakeStoreG)
    ProfScope ps(c, "tiler_rekey", (uint64_t)nc * 44ull, 1);
    hipLaunchKernelGGL(tl_rekey_kernel, dim3(div_up(nc, 256)), dim3(256), 0, c->stream, ckey, cgid, nc, t->pool_xyz,
                       root_box(t), plan.level);
    SWZ_LAUNCH_CHECK(c);
    ++t->paths[TP_REKEY];
  }
  // (needed for files the level loop wrote as well: TakeStoreG stores the key against the NODE's bounds, which may order two
  // points the other way round than the key they were sorted by -- tests/test_multibatch.py constructs such a pair)
  if (nc && !plan.terminal) SWZ_TRY(resort_if_inverted(t, ckey, cgid, nc, nsh));
  if (w.wused + nc + ng > w.wcap) return c->fail(SWZ_ERR_INTERNAL, "working pool overflow");
  if (nc)
    SWZ_TRY(fill_from_pool(c, cgid, nc, t->pool_xyz, w.have_pos ? w.wx + w.wused : nullptr, w.have_pos ? w.wy + w.wused : nullptr,
                           w.have_pos ? w.wz + w.wused : nullptr, w.wgid + w.wused));
  uint64_t* mkey = nullptr;
  uint32_t* midx = nullptr;
  SWZ_TRY(c->get("tl_mkey", (size_t)as.m + nc + ng, &mkey));
  SWZ_TRY(c->get("tl_midx", (size_t)as.m + nc + ng, &midx));
  // tile_node :421-442: terminal nodes append (new ++ cached), the others std::merge by key; ghosts lie in lower
  // octants, so their keys are smaller than every local key: sorted ghosts ++ merged locals is the merged whole
  {
    ProfScope ps(c, "tiler_merge", ((uint64_t)as.m + nc) * 24ull, 2);
    SWZ_TRY(merge_pairs(c, as.akey, as.aidx, as.m, ckey, nullptr, nc, plan.terminal ? nsh : 0u, w.wused, mkey + ng, midx + ng));
  }
  w.wused += nc;
  if (ng) {
    uint64_t *gk = nullptr, *gkb = nullptr;
    uint32_t *gp = nullptr, *gpb = nullptr;
    SWZ_TRY(c->get("tl_gkey", (size_t)ng, &gk));
    SWZ_TRY(c->get("tl_gkey_b", (size_t)ng, &gkb));
    SWZ_TRY(c->get("tl_gperm", (size_t)ng, &gp));
    SWZ_TRY(c->get("tl_gperm_b", (size_t)ng, &gpb));
    double* gx = const_cast<double*>(sr->ghost_xyz);  // inside the bounds already: the clamp of the encode is a no-op
    SWZ_TRY(index_and_sort(c, gx, ng, t->bmin, t->bmax, gkb, gpb, gk, gp));
    SWZ_TRY(gather_positions(c, sr->ghost_xyz, gp, ng, w.wx + w.wused, w.wy + w.wused, w.wz + w.wused));
    SWZ_HIP(c, hipMemsetAsync(w.wgid + w.wused, 0xFF, (size_t)ng * 4, c->stream));
    SWZ_HIP(c, hipMemcpyAsync(mkey, gk, (size_t)ng * 8, hipMemcpyDeviceToDevice, c->stream));
    hipLaunchKernelGGL(tl_iota_base_kernel, dim3(div_up(ng, 256)), dim3(256), 0, c->stream, midx, ng, w.wused);
    SWZ_LAUNCH_CHECK(c);
    w.wused += ng;
  }
  ms->akey = mkey;
  ms->aidx = midx;
  ms->m = as.m + nc + ng;
  ms->ckey = sr ? nullptr : ckey;  // a sharded root decides from the global counts
  ms->nc = sr ? 0u : nc;
  if (!sr && !ng && nc) {
    ms->old_lo = p.pull_lo;
    ms->old_hi = p.pull_lo + nc;
    ms->new_key = as.akey;
    ms->new_m = as.m;
    if (greedy_sampler(plan.sampler) && !plan.terminal && plan.level + 2 < 22) {
      StoreLevel& below = t->lv[plan.level + 2];
      if (below.cnt) {  // (the table this batch's next level asks for anyway)
        SWZ_TRY(store_table(c, below, plan.level + 2));
        ms->child_nkey = below.nkey[below.ncur];
        ms->child_nn = below.nn;
      }
    }
  }
  return SWZ_OK;
}

// ---- the nodes' new files: appended behind what the side holds, the node table points at them
static int level_store(swz_tiler* t, BatchWork& w, const LevelPlan& plan, const ActiveSet& ms, const LevelPull& p, uint32_t ng,
                       const LevelBuffers& lb, const LevelResult* res, ActiveSet& as) {
  swz_ctx* c = t->c;
  StoreLevel& st = t->lv[plan.level + 1];
  const uint32_t nsh = plan.node_shift;
  const int lvi = plan.level + 1;
  const uint32_t nc = p.nc;
  uint8_t* const touched = p.touched;
  const bool all_touched = p.all_touched;
  uint32_t* counters = nullptr;
  SWZ_TRY(c->get("tl_counters", (size_t)4, &counters));
  const uint32_t nt = ms.m - res->remaining - ng;  // (the ghosts lead the merged range and are all taken again)
  const uint32_t rest = st.cnt - nc;               // entries of the files the batch did not reach
  uint64_t *fkey = nullptr, *foff = nullptr;
  uint32_t* fcnt = nullptr;
  uint32_t nf = 0;
  bool nf_known = true;
  if (st.nn && !all_touched && rest) {
    ProfScope ps(c, "tiler_store", (uint64_t)st.nn * 21ull, 2);
    SWZ_TRY(c->get("tl_ftab_key", (size_t)st.nn, &fkey));
    SWZ_TRY(c->get("tl_ftab_off", (size_t)st.nn, &foff));
    SWZ_TRY(c->get("tl_ftab_cnt", (size_t)st.nn, &fcnt));
    SWZ_TRY(fused_scan(c, UntouchedF{touched}, TableFilterG{st.nkey[st.ncur], st.noff[st.ncur], st.ncnt[st.ncur], fkey, foff, fcnt},
                       st.nn, counters + 1, "tl"));
    nf_known = false;
  }
  if (!st.key[st.cur] || (uint64_t)st.end + nt > st.cap[st.cur]) {
    // the side is full: the files the batch left alone move to the other side, the old versions of the rest stay behind
    if (!nf_known) {
      SWZ_TRY(read_u32(c, counters + 1, &nf));
      nf_known = true;
    }
    if (st.key[st.cur]) ++t->paths[TP_COMPACT_FULL];  // (else the level's first file: there is no side yet)
    ProfScope ps(c, "tiler_store", (uint64_t)rest * 24ull, 2);
    const size_t room = (size_t)rest + nt;
    SWZ_TRY(store_compact(c, st, lvi, foff, fcnt, nf, rest, room + room / 4));
  }
  const uint32_t at = st.end;
  if (at) ++t->paths[TP_APPEND_BEHIND];
  uint32_t* texcl = nullptr;
  SWZ_TRY(c->get("tl_texcl", (size_t)ms.m, &texcl));
  {
    ProfScope ps(c, "tiler_store", (uint64_t)ms.m * 14ull + (uint64_t)nt * 12ull, 2);
    SWZ_TRY(fused_scan(c, TakenF{lb.taken},
                       TakeStoreG{ms.akey, ms.aidx, w.wgid, p.pull_lo, p.pull_lo + nc, ng, t->pool_xyz, root_box(t), plan.level,
                                  st.key[st.cur] + at, st.gid[st.cur] + at, nsh, texcl},
                       ms.m, counters + 2, "tl"));
  }
  if (ng) {  // the ghosts are not part of the local file
    SWZ_HIP(c, hipMemsetAsync(counters, 0, 4, c->stream));
    hipLaunchKernelGGL(tl_count_untaken_kernel, dim3(div_up(ng, 256)), dim3(256), 0, c->stream, lb.taken, ng, counters);
    SWZ_LAUNCH_CHECK(c);
    uint32_t lost = 0;
    SWZ_TRY(read_u32(c, counters, &lost));
    if (lost) return c->fail(SWZ_ERR_BAD_ARG, "swz_tiler: " + std::to_string(lost) + " ghost points were not taken again "
                                              "(they must be what the root took on LOWER shards in this batch)");
  }
  {
    ProfScope ps(c, "tiler_store", (uint64_t)nt * 8ull + (uint64_t)st.nn * 20ull, 2);
    // the nodes of the merged range are the nodes of the new files (every node takes at least one point; only a sharded
    // root whose local points all fell to the ghosts writes nothing): their number is the level step's, no read-back
    uint32_t* hp = nullptr;
    uint64_t* hk = nullptr;
    const uint32_t heads = nt ? res->num_nodes : 0u;
    if (heads) {
      SWZ_TRY(c->get("tl_head_pos", (size_t)heads, &hp));
      SWZ_TRY(c->get("tl_head_key", (size_t)heads, &hk));
      hipLaunchKernelGGL(tl_new_heads_kernel, dim3(div_up(heads, 256)), dim3(256), 0, c->stream, ms.akey, lb.nstart, texcl, heads, nsh, ng, hk, hp);
      SWZ_LAUNCH_CHECK(c);
    }
    if (!nf_known) SWZ_TRY(read_u32(c, counters + 1, &nf));
    const int nd = st.ncur ^ 1;
    SWZ_TRY(table_reserve(c, st, lvi, nd, (size_t)nf + heads));
    if (nf + heads) {
      hipLaunchKernelGGL(tl_table_merge_kernel, dim3(div_up(nf + heads, 256)), dim3(256), 0, c->stream, fkey, foff, fcnt, nf, hk, hp,
                         heads, nt, (uint64_t)at, st.nkey[nd], st.noff[nd], st.ncnt[nd]);
      SWZ_LAUNCH_CHECK(c);
      if (!nf) ++t->paths[TP_TABLE_MERGE_NF0];
      if (!heads) ++t->paths[TP_TABLE_MERGE_HEADS0];
    }
    st.ncur = nd;
    st.nn = nf + heads;
  }
  st.end = at + nt;
  st.cnt = rest + nt;
  st.linear = at == 0;  // (nothing in front of the new files: they are the level)
  if (rest == 0) st.rekeyed = true;

  as = ActiveSet{w.surv_key[w.which], w.surv_idx[w.which], res->remaining};
  as.parent_prefix = res->node_prefix;
  as.parents = res->node_prefix ? res->num_nodes : 0u;
  w.which ^= 1;
  return SWZ_OK;
}

// sr != nullptr: the ROOT level of a sharded batch (the node spans all shards: its take-all / sample decision is
// the global one, its whole local file takes part even without new local points, and for MIN_DISTANCE what the root
// took on lower shards in this batch sorts first as ghosts -- swz_tiler_shard_begin_device)
int tiler_level(swz_tiler* t, BatchWork& w, const LevelPlan& plan_in, ActiveSet& as, LevelResult* res, uint32_t* merged_out,
                const ShardRoot* sr) {
  swz_ctx* c = t->c;
  LevelPlan plan = plan_in;
  const uint32_t ng = sr ? sr->ghosts : 0u;
  if (sr) {
    if (sr->sample) plan.force_sample = true; else plan.max_points = ~0ull;
  }
  LevelPull p;
  ActiveSet ms;
  SWZ_TRY(level_pull(t, w, plan, as, sr, &p));
  SWZ_TRY(level_merge(t, w, plan, as, sr, p, &ms));
  if (ms.m == 0) {  // a shard without new points and without a root file
    res->remaining = 0;
    *merged_out = 0;
    return SWZ_OK;
  }
  *merged_out = ms.m;

  // ---- sample / take all, compact the survivors
  SWZ_TRY(c->get(w.which ? "tl_surv_key_1" : "tl_surv_key_0", (size_t)ms.m, &w.surv_key[w.which]));
  SWZ_TRY(c->get(w.which ? "tl_surv_idx_1" : "tl_surv_idx_0", (size_t)ms.m, &w.surv_idx[w.which]));
  LevelBuffers lb;
  SWZ_TRY(alloc_level_buffers(c, ms.m, &lb));
  // (exact positions for MIN_DISTANCE on key coordinates, swz_mqsweep.hip: working index -> point id -> position pool;
  // ghosts of a sharded root lie outside the pool)
  SortedPoints sp{nullptr, nullptr, nullptr, ng ? nullptr : t->pool_xyz, w.wgid};
  if (!level_decides_on_keys(c, plan, sp)) SWZ_TRY(work_need_positions(t, w));
  if (w.have_pos) {
    sp.X = w.wx;
    sp.Y = w.wy;
    sp.Z = w.wz;
  }
  SWZ_TRY(level_step(c, plan, ms, sp, lb, w.wlevel, w.surv_key[w.which], w.surv_idx[w.which], res));
  return level_store(t, w, plan, ms, p, ng, lb, res, as);
}

}  // namespace swz
