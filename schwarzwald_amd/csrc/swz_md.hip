// swz_md.hip -- MIN_DISTANCE: which algorithm samples a level, with which cells.
//
// min_distance_level surveys the level once (occupied cells per candidate cell size, typical cell populations, the
// numbering of the sampled nodes, the key metric) and then reads top to bottom as the ladder of algorithms:
//
//   joint root of a sharded batch      -> key sweep at the finest cells (swz_mdkeys.hip)
//   sparse level                       -> block kernel (swz_mdblock.hip), else thread per point (swz_mdsparse.hip)
//   property mode, key metric          -> rounds (swz_mdrounds.hip)
//   key metric                         -> key sweep (swz_mdkeys.hip)
//   positions in Morton order          -> position sweep (swz_mindist.hip); property mode: coloured phases (swz_mdprop.hip)
//
// Every rung may decline a level (*used / *done = false); the level then goes on to the next one.  The algorithms get
// the survey as an MdLevel (swz_md.h) and never call each other.
#include <algorithm>
#include <cmath>

#include "swz_md.h"
#include "swz_scan.h"

namespace swz {

// ----------------------------------------------------------------------------- survey
__global__ __launch_bounds__(256) void md_node_flag_kernel(const uint8_t* __restrict__ nmode, uint32_t nnodes,
                                                           uint32_t* __restrict__ out) {
  const uint32_t j = blockIdx.x * 256 + threadIdx.x;
  if (j < nnodes) out[j] = nmode[j] == MODE_SAMPLE ? 1u : 0u;
}

// How many cells are OCCUPIED at every candidate cell level: a point that is not the first of its node is a cell
// head at cell level cl exactly when its key differs from its predecessor's within the first cl digits below the
// node prefix.  hist[0] counts the firsts of the sampled nodes, hist[b] the points whose first differing digit is
// digit b (1-based); occupied(cl) = hist[0] + ... + hist[cl].
__global__ __launch_bounds__(256) void md_cell_hist_kernel(const uint64_t* __restrict__ akey, const uint32_t* __restrict__ nid,
                                                           const uint8_t* __restrict__ nmode, uint32_t m, uint32_t node_shift,
                                                           uint32_t cl_geo, uint32_t skip, uint32_t* __restrict__ hist) {
  __shared__ uint32_t lh[16];
  if (threadIdx.x < 16) lh[threadIdx.x] = 0;
  __syncthreads();
  uint32_t mine = 0;  // lane b accumulates the wavefront's count of bin b
  // every skip-th tile of 256 points (see MdLevel::occupied)
  for (uint64_t i0 = (uint64_t)blockIdx.x * skip * 256u; i0 < m; i0 += (uint64_t)gridDim.x * skip * 256u) {
    const uint32_t i = (uint32_t)i0 + threadIdx.x;
    uint32_t bin = 0xFFu;
    if (i0 + threadIdx.x < m && nmode[nid[i]] == MODE_SAMPLE) {
      if (i == 0 || nid[i - 1] != nid[i]) {
        bin = 0;
      } else if (cl_geo) {
        const uint64_t diff = ((akey[i] ^ akey[i - 1]) >> (node_shift - 3u * cl_geo)) & ((1ull << (3u * cl_geo)) - 1ull);
        if (diff) bin = cl_geo - (uint32_t)(63 - __clzll((unsigned long long)diff)) / 3u;  // 1 .. cl_geo
      }
    }
    for (uint32_t b = 0; b <= cl_geo; ++b) {
      const uint32_t cnt = (uint32_t)__popcll(__ballot(bin == b));
      if (lane_id() == b) mine += cnt;
    }
  }
  if (lane_id() <= cl_geo && mine) atomicAdd(&lh[lane_id()], mine);
  __syncthreads();
  if (threadIdx.x < 16 && lh[threadIdx.x]) atomicAdd(&hist[threadIdx.x], lh[threadIdx.x]);
}

// Points-weighted mean cell population at the cell levels cl_geo, cl_geo-1, -2, -3 (out[0..3] = sums over the
// samples, out[4] = samples): the population of the cell of every MD_POP_SAMPLES-th point, found by binary search for the
// cell's run in the sorted keys.  Tells whether the TYPICAL point would sit in an oversized cell after coarsening,
// which the plain average over cells does not (a dense blob in a sparse background).
constexpr uint32_t MD_POP_SAMPLES = 1u << 16;
__global__ __launch_bounds__(256) void md_cell_pop_kernel(const uint64_t* __restrict__ akey, const uint32_t* __restrict__ nid,
                                                          const uint8_t* __restrict__ nmode, uint32_t m, uint32_t node_shift,
                                                          uint32_t cl_geo, unsigned long long* __restrict__ out) {
  const uint32_t t = blockIdx.x * 256 + threadIdx.x;
  if (t >= MD_POP_SAMPLES) return;
  const uint32_t i = (uint32_t)(((uint64_t)t * m) / MD_POP_SAMPLES);
  if (i >= m || nmode[nid[i]] != MODE_SAMPLE) return;
  const uint64_t key = akey[i];
  for (uint32_t k = 0; k <= 3u && k <= cl_geo; ++k) {
    const uint32_t sh = node_shift - 3u * (cl_geo - k);
    const uint64_t pre = key >> sh;
    uint32_t lo = 0, hi = i;  // first index with prefix >= pre
    while (lo < hi) {
      const uint32_t mid = lo + (hi - lo) / 2u;
      if ((akey[mid] >> sh) < pre) lo = mid + 1u; else hi = mid;
    }
    const uint32_t first = lo;
    lo = i;
    hi = m;  // first index with prefix > pre
    while (lo < hi) {
      const uint32_t mid = lo + (hi - lo) / 2u;
      if ((akey[mid] >> sh) <= pre) lo = mid + 1u; else hi = mid;
    }
    atomicAdd(&out[k], (unsigned long long)(lo - first));
  }
  atomicAdd(&out[4], 1ull);
}

__global__ __launch_bounds__(256) void md_gather_active_kernel(const uint32_t* __restrict__ aidx, uint32_t m,
                                                               const double* __restrict__ X,
                                                               const double* __restrict__ Y,
                                                               const double* __restrict__ Z, double* __restrict__ ax,
                                                               double* __restrict__ ay, double* __restrict__ az) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= m) return;
  const uint32_t s = aidx[i];
  ax[i] = X[s];
  ay[i] = Y[s];
  az[i] = Z[s];
}

__global__ __launch_bounds__(256) void pm_clear_taken_kernel(const uint32_t* __restrict__ nid, const uint8_t* __restrict__ nmode,
                                                             uint32_t m, uint8_t* __restrict__ taken) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i < m && nmode[nid[i]] == MODE_SAMPLE) taken[i] = 0;
}

int md_clamp_cell_levels(uint32_t sample_nodes, int cl) {
  while (cl > 0 && (double)sample_nodes * std::pow(8.0, cl) > 2147483648.0) --cl;
  return cl;
}

// one pass over the keys, or over every skip-th tile of them (then the counts are scaled up)
static int count_cells(swz_ctx* c, const MdLevel& L, uint32_t skip, uint32_t occupied[12]) {
  const uint32_t m = L.as.m;
  uint32_t* d_hist = nullptr;
  SWZ_TRY(c->get("md_hist", (size_t)16, &d_hist));
  SWZ_HIP(c, hipMemsetAsync(d_hist, 0, 64, c->stream));
  const uint32_t tiles = div_up(m, 256);
  const uint32_t sampled_tiles = div_up(tiles, skip);
  hipLaunchKernelGGL(md_cell_hist_kernel, dim3(std::min<uint32_t>(sampled_tiles, 4096u)), dim3(256), 0, c->stream, L.as.akey,
                     L.lb.nid, L.lb.nmode, m, L.plan.node_shift, (uint32_t)L.plan.cell_levels_geo, skip, d_hist);
  SWZ_LAUNCH_CHECK(c);
  SWZ_STAGE(c, "md cell hist");
  uint32_t h[16];
  SWZ_HIP(c, hipMemcpyAsync(h, d_hist, 64, hipMemcpyDeviceToHost, c->stream));
  SWZ_HIP(c, hipStreamSynchronize(c->stream));
  const double scale = skip == 1 ? 1.0 : (double)m / (double)std::min<uint64_t>(m, (uint64_t)sampled_tiles * 256u);
  double run = 0;
  for (int b = 0; b < 12; ++b) {
    run += h[b];
    occupied[b] = (uint32_t)std::min<double>(run * scale, (double)m);
  }
  return SWZ_OK;
}
int md_count_cells_exact(swz_ctx* c, const MdLevel& L, uint32_t occupied[12]) { return count_cells(c, L, 1u, occupied); }

// L.pop, on first use (one kernel and one host synchronisation)
static int md_populations(swz_ctx* c, MdLevel& L) {
  if (L.have_pop) return SWZ_OK;
  unsigned long long* d_pop = nullptr;
  SWZ_TRY(c->get("md_pop", (size_t)8, &d_pop));
  SWZ_HIP(c, hipMemsetAsync(d_pop, 0, 64, c->stream));
  hipLaunchKernelGGL(md_cell_pop_kernel, dim3(MD_POP_SAMPLES / 256), dim3(256), 0, c->stream, L.as.akey, L.lb.nid, L.lb.nmode, L.as.m,
                     L.plan.node_shift, (uint32_t)L.plan.cell_levels_geo, d_pop);
  SWZ_LAUNCH_CHECK(c);
  SWZ_STAGE(c, "md cell pop");
  unsigned long long h[5];
  SWZ_HIP(c, hipMemcpyAsync(h, d_pop, 40, hipMemcpyDeviceToHost, c->stream));
  SWZ_HIP(c, hipStreamSynchronize(c->stream));
  for (int k = 0; k < 4; ++k) L.pop[k] = h[4] ? (double)h[k] / (double)h[4] : 1e30;
  L.have_pop = true;
  return SWZ_OK;
}

static int survey(swz_ctx* c, MdLevel& L) {
  const uint32_t skip = std::max(1u, L.as.m >> 23);  // about 8 M points are looked at
  L.sampled_hist = skip > 1u;
  SWZ_TRY(count_cells(c, L, skip, L.occupied));
  // (property mode asks for the populations only when a cell-size rule needs them: most of its levels never do)
  if (!L.plan.md_property) SWZ_TRY(md_populations(c, L));
  uint32_t* snode = nullptr;
  SWZ_TRY(c->get("md_snode", (size_t)L.num_nodes, &snode));
  hipLaunchKernelGGL(md_node_flag_kernel, dim3(div_up(L.num_nodes, 256)), dim3(256), 0, c->stream, L.lb.nmode, L.num_nodes, snode);
  SWZ_LAUNCH_CHECK(c);
  SWZ_TRY(scan_exclusive_u32(c, snode, snode, L.num_nodes, nullptr, "mdn"));
  L.snode_of = snode;
  L.km = key_metric(c, L.plan, L.sp);
  return SWZ_OK;
}

int md_active_positions(swz_ctx* c, const MdLevel& L, size_t per_point, const double** X, const double** Y, const double** Z) {
  *X = L.sp.X;
  *Y = L.sp.Y;
  *Z = L.sp.Z;
  if (!L.as.aidx) return SWZ_OK;
  const uint32_t m = L.as.m;
  // the two big per-point buffers are shared by the position sweep, the coloured phases and the thread-per-point path
  // (never live at the same time): "md_pos" = x[], y[], z[] here (24 B per point used), {x,y,z,key} records there
  // (32 B), "md_acc" the same sizes.  Each path asks for what it uses: at 1 B clustered points the 2 x 8 GB between them
  // decide whether a level with 226 M cells fits
  double* ax = nullptr;
  SWZ_TRY(c->get("md_pos", (size_t)m * per_point, &ax));
  hipLaunchKernelGGL(md_gather_active_kernel, dim3(div_up(m, 256)), dim3(256), 0, c->stream, L.as.aidx, m, L.sp.X, L.sp.Y, L.sp.Z, ax,
                     ax + m, ax + 2 * (size_t)m);
  SWZ_LAUNCH_CHECK(c);
  *X = ax;
  *Y = ax + m;
  *Z = ax + 2 * (size_t)m;
  return SWZ_OK;
}

// ----------------------------------------------------------------------------- cell-size rules
// The two frontier sweeps (on keys, on positions).  Cell size: as fine as the spacing allows, but coarse enough that an
// OCCUPIED cell holds >= 8 points on average (clustered data leaves most of a node empty: the average over the node's
// volume would make the cells of a dense sheet or blob far too large) and that the dense [node][cell] lookup table stays
// affordable
static int sweep_cell_levels(const swz_ctx* c, const MdLevel& L) {
  const LevelPlan& plan = L.plan;
  int cl = plan.cell_levels_geo;
  const double avg = (double)L.sample_points / (double)L.sample_nodes;
  const double per_cell = 8.0;
  // ... but only while the TYPICAL point would not end up in an oversized cell (points-weighted mean population
  // after the step <= 160): with mixed densities (a dense blob in a sparse background) the average over the cells
  // says little, and cells that are too large for the dense part cost far more (long serial activations) than
  // cells that are too small for the sparse part (more, cheap activations).  Measured on 100 M clustered points:
  // 11.4 s with the volume average, 0.66 s with this rule; uniform data choose the same cells as before.
  const double max_pop = 160.0;
  while (cl > 0 && plan.cell_levels_geo - cl < 3 && (double)L.sample_points / (double)std::max(1u, L.occupied[cl]) < per_cell &&
         L.pop[plan.cell_levels_geo - cl + 1] <= max_pop)
    --cl;
  cl = md_clamp_cell_levels(L.sample_nodes, cl);
  if (const long coarsen = c->opt_int("SWZ_MD_COARSEN", 0))
    if (avg / std::pow(8.0, cl) >= c->opt_num("SWZ_MD_COARSEN_MIN", 32.0)) cl = std::max(0, cl - (int)coarsen);
  return cl;
}

bool md_guess_chained_level(const swz_ctx* c, const LevelPlan& plan, const SortedPoints& sp, uint32_t points, MqPrebuild* want) {
  want->wanted = false;
  if (plan.node_shift >= 63u || plan.node_shift < 3u || plan.node_shift % 3u != 0u || plan.terminal || plan.reroot || plan.md_property) return false;
  const KeyMetric km = key_metric(c, plan, sp);
  if (!km.ok) return false;
  const uint32_t levels = (63u - plan.node_shift) / 3u;  // below the root: every one of the 8^levels nodes is assumed to exist
  if (levels > 6u) return false;
  const double nodes = std::ldexp(1.0, 3 * (int)levels);
  if (plan.force_sample ? points == 0u : (double)points / nodes <= (double)plan.max_points) return false;  // (the nodes would keep what they hold)
  // occupied cells at cell level cl of evenly spread points: a cell is empty with probability exp(-points / cells)
  auto occupied = [&](int cl) {
    const double cells = nodes * std::ldexp(1.0, 3 * cl);
    return std::max(1.0, cells * -std::expm1(-(double)points / cells));
  };
  const int cl_sparse = md_clamp_cell_levels((uint32_t)nodes, plan.cell_levels_geo);
  if ((double)points / occupied(cl_sparse) < c->opt_num("SWZ_MD_SPARSE_LIMIT", 2.0)) return false;
  int cl = plan.cell_levels_geo;  // sweep_cell_levels without its population test
  while (cl > 0 && plan.cell_levels_geo - cl < 3 && (double)points / occupied(cl) < 8.0) --cl;
  cl = md_clamp_cell_levels((uint32_t)nodes, cl);
  const double cells = nodes * std::ldexp(1.0, 3 * cl);
  if (cells > 2147483632.0 || occupied(cl) / cells < c->opt_num("SWZ_MD_DIRECT_MIN_OCCUPANCY", 0.5)) return false;
  const uint32_t cell_shift = plan.node_shift - 3u * (uint32_t)cl;
  if (cell_shift / 3u > 21u) return false;
  want->want_node_shift = plan.node_shift;
  want->want_cl = (uint32_t)cl;
  want->want_rg = key_sweep_record_granules(c, cell_shift / 3u, km.T);
  want->wanted = true;
  return true;
}

// The coloured phases: one wavefront per cell.  Coarser cells are better filled, but a cell of side r spacings can hold
// about 0.75 r^3 taken points (points that are pairwise a spacing apart, and never more than it has points) and every
// point is tested against those of 27 cells: go one level coarser only when the finest cells are poorly filled and the
// coarser ones still hold few taken points WHATEVER their population (real data is clustered: an average says nothing
// about the dense parts).
static int phases_cell_levels(swz_ctx* c, MdLevel& L, int* cl_out) {
  const LevelPlan& plan = L.plan;
  const double node_ext = (plan.root.maxx - plan.root.minx) / std::pow(2.0, plan.level + 1);
  const double r0 = node_ext / std::pow(2.0, plan.cell_levels_geo) / plan.spacing_node;  // finest cells, in spacings
  int cl = plan.cell_levels_geo;
  if (cl > 0 && (double)L.sample_points / (double)std::max(1u, L.occupied[cl]) < 24.0 && 0.75 * 8.0 * r0 * r0 * r0 <= 48.0) {
    // ... and only while the TYPICAL point would not sit in an oversized cell afterwards (points-weighted mean
    // population: a dense blob in a sparse background keeps the plain average low)
    SWZ_TRY(md_populations(c, L));
    if (L.pop[1] <= 1024.0) --cl;
  }
  *cl_out = md_clamp_cell_levels(L.sample_nodes, cl);
  return SWZ_OK;
}

// ----------------------------------------------------------------------------- the ladder
int min_distance_level(swz_ctx* c, const LevelPlan& plan, const ActiveSet& as, const SortedPoints& sp, const LevelBuffers& lb,
                       uint32_t num_nodes, uint32_t sample_nodes, uint32_t sample_points, uint32_t* rounds_out, bool* keys_direct,
                       bool* needs_flush) {
  bool direct = false;
  if (keys_direct) *keys_direct = false;
  if (needs_flush) *needs_flush = false;
  // A level inside a chain (as.gone: the arrays still hold the points taken further up, swz_level.h) is the key sweep's
  // with direct numbering or nobody's: every other rung hands it back before anything is decided, and the caller compacts.
  // (The survey counts the cells of those points as occupied -- a per cent or two of a dense level, in numbers that only
  // steer the choice of cell size.)
  const bool shared = as.gone != nullptr;
  if (shared && !needs_flush) return c->fail(SWZ_ERR_INTERNAL, "MIN_DISTANCE: a level on shared arrays needs a caller that can compact them");
  c->next_scratch_epoch();  // what the level before asked for ("md_*", "sp_*", "pm_*") may go if memory runs out
  MdLevel L{plan, as, sp, lb, num_nodes, sample_nodes, sample_points, sample_nodes == num_nodes};
  SWZ_TRY(survey(c, L));
  bool used = false;

  if (c->md_shard_root && plan.level == -1) {
    // The root of a batch sharded over the GPUs of one process (swz_group): every shard sweeps the cells of its own
    // octants, on keys, with the same cells everywhere (the finest ones: what a shard sees of the cloud must not decide).
    SWZ_TRY(min_distance_keys_level(c, L, plan.cell_levels_geo, rounds_out, &used, static_cast<const MdShardRoot*>(c->md_shard_root)));
    if (!used) return c->fail(SWZ_ERR_INTERNAL, "MIN_DISTANCE root of a sharded batch: the joint sweep needs a level that can be decided on keys");
    return SWZ_OK;
  }

  // Sparse levels (about one point per spacing-sized cell or fewer; points per OCCUPIED cell: clustered data fills a small
  // part of a node's volume): the Morton-order greedy needs only a few dependent rounds there.  Property mode takes the
  // exact set too: it has the property a fortiori, and one thread per point beats one wavefront per (nearly empty) cell.
  const int cl_sparse = md_clamp_cell_levels(sample_nodes, plan.cell_levels_geo);
  // (per occupied cell; a uniform level with 1.5 points per cell of volume has 1.93)
  const bool sparse = (double)sample_points / (double)std::max(1u, L.occupied[cl_sparse]) < c->opt_num("SWZ_MD_SPARSE_LIMIT", 2.0);
  // (not the root of a sharded batch with ghosts in front, decided on keys: the sweep looks up two position arrays, these paths one)
  if (sparse && shared) {
    *needs_flush = true;
    return SWZ_OK;
  }
  if (sparse && !(sp.ghosts && plan.level == -1 && !sp.X)) {
    // blocks of cells out of LDS, decisions in the same launch; levels it cannot take -- no key metric, a block that does
    // not fit its LDS capacity -- go on to one thread per point
    SWZ_TRY(min_distance_block_level(c, L, &used));
    if (used) {
      if (rounds_out) *rounds_out += 1;
      return SWZ_OK;
    }
    SWZ_TRY(min_distance_sparse_level(c, L, cl_sparse, rounds_out, &used));
    if (used) return SWZ_OK;
    // it gave up half way (locally dense data).  Exact mode: every decision taken so far is exact and will simply be taken
    // again.  Property mode: they are those of ANOTHER priority order than the rounds' or the phases'.
    if (plan.md_property) {
      hipLaunchKernelGGL(pm_clear_taken_kernel, dim3(div_up(as.m, 256)), dim3(256), 0, c->stream, lb.nid, lb.nmode, as.m, lb.taken);
      SWZ_LAUNCH_CHECK(c);
    }
  }

  if (plan.md_property && L.km.ok) {
    // On key coordinates (cubic bounds, as the Tiler's are): a maximal independent set grown in data-parallel rounds, no
    // positions in Morton order, no dependent phases.
    SWZ_TRY(min_distance_rounds_level(c, L, rounds_out, &used));
    if (used) return SWZ_OK;
  }

  // Dense levels whose spacing spans enough key cells: the frontier sweep on key coordinates.  Exact mode always; a
  // property level that the rounds did not take only when its positions were never gathered -- the exact set has the
  // property a fortiori and decides on the keys as well (with positions at hand it gets the coloured phases).
  int cl = 0;
  if (!plan.md_property || !sp.X) {
    SWZ_TRY(md_populations(c, L));
    cl = sweep_cell_levels(c, L);
    SWZ_TRY(min_distance_keys_level(c, L, cl, rounds_out, &used, nullptr, &direct));
    if (used) {
      if (keys_direct) *keys_direct = direct;
      return SWZ_OK;
    }
  }
  if (shared) {
    *needs_flush = true;
    return SWZ_OK;
  }

  if (!sp.X) return c->fail(SWZ_ERR_INTERNAL, "MIN_DISTANCE: this level needs the positions in Morton order and they were not gathered");
  if (!plan.md_property) return min_distance_sweep_level(c, L, cl, rounds_out);
  SWZ_TRY(phases_cell_levels(c, L, &cl));
  return min_distance_phases_level(c, L, cl, rounds_out);
}

}  // namespace swz
