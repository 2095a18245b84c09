// swz_query.hip -- the streaming query of a written data set: by box and depth (swz_dataset_query), by a region, the box cut
// by planes or by a polygon in x-y (swz_dataset_query_region), and with an attribute filter (swz_dataset_query_filtered).  The
// nodes that are read are the ones swz_qplan.hip leaves: the scan without the nodes whose widened boxes miss the query box or
// cannot hold a row of the region, and without those that the directory's node-summaries.swz shows the filter cannot reach.
// They are streamed chunk by chunk by SourceLoop::each_chunk (swz_source.hip); what is here is the body of that loop: every chunk's
// chunk-local positions and columns go through the selection kernel (swz_select.hip) into the caller's arrays at the running
// offset, and the selected rows get their nodes.  The readers of chunk j + 1 run while chunk j is selected.  With a filter the
// stream unpacks the caller's columns and the filter's, and the selection reads the latter.
#include <chrono>
#include <cstddef>
#include <string>
#include <vector>

#include "swz_convert.h"
#include "swz_hostio.h"
#include "swz_qplan.h"
#include "swz_select.h"

static_assert(sizeof(swz_query_params) == 72 && offsetof(swz_query_params, max_depth) == 48 && offsetof(swz_query_params, chunk_points) == 64 &&
                sizeof(swz_query_stats) == 88 && offsetof(swz_query_stats, read_ms) == 48,
              "the structs of the query as include/swz_gpu.h and the bindings lay them out");

namespace swz {

// per selected row of a chunk its node: the last node of the chunk whose first row is not behind the row (nodes without
// points share their first row with the node behind them); node_index: the chunk's nodes as indices of the query's table
__global__ __launch_bounds__(256) void query_row_nodes_kernel(const uint32_t* __restrict__ rows, uint32_t cnt, const uint32_t* __restrict__ node_first,
                                                              uint32_t nodes, const uint32_t* __restrict__ node_index,
                                                              uint32_t* __restrict__ node_out) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= cnt) return;
  const uint32_t r = rows[i];
  uint32_t lo = 0, hi = nodes;  // node_first[lo] <= r < node_first[hi] (node_first[nodes]: the chunk's rows)
  while (hi - lo > 1u) {
    const uint32_t mid = (lo + hi) >> 1;
    if (node_first[mid] <= r) lo = mid;
    else hi = mid;
  }
  node_out[i] = node_index[lo];
}

static int query(swz_ctx* c, const char* who, const char* dir, const swz_query_params* q, const swz_region* region, const swz_filter* filter,
                 uint64_t capacity, double* d_xyz_out, const swz_attribute_columns* d_out, uint32_t* d_node_out, uint64_t* count_out,
                 swz_query_stats* stats) {
  auto refuse = [&](const std::string& what) { return c->fail(SWZ_ERR_BAD_ARG, std::string(who) + ": " + what); };
  const auto t_wall = std::chrono::steady_clock::now();
  if (stats) *stats = swz_query_stats{};
  if (!count_out) return refuse("NULL argument");
  *count_out = 0;
  DatasetScan kept;
  uint64_t scanned = 0;
  RegionHost region_host;
  uint32_t fattrs = 0;  // the columns the filter reads: unpacked for it, handed to the caller only if the mask names them too
  SWZ_TRY(query_plan(c, who, dir, q, region, filter, &kept, &scanned, &region_host, &fattrs));
  const bool count_only = !d_xyz_out && capacity == 0;
  if (!d_xyz_out && !count_only) return refuse("NULL d_xyz_out with a capacity (count only: NULL and capacity 0)");
  uint32_t mask = q->attribute_mask == ~0u ? kept.info.attribute_mask : q->attribute_mask;
  if (mask & ~kept.info.attribute_mask) return refuse("the attribute_mask names a column the source does not hold");
  if (count_only) mask = 0;  // positions decide
  for (int a = 0; a < SWZ_ATTR_COUNT; ++a)
    if (((mask >> a) & 1u) && (!d_out || !d_out->column[a])) return refuse("a bit of the mask without an output column");
  SWZ_HIP(c, hipSetDevice(c->device));

  // ---- the nodes that are read: all of the kept table, or those the filter can reach by the directory's summaries; `index`
  // holds their places in the kept table, which d_node_out keeps indexing
  std::vector<uint32_t> index;
  {
    std::vector<uint8_t> read;
    SWZ_TRY(filter_reads(c, who, dir, kept, filter, &read));
    const uint64_t all = kept.count.size();
    for (uint64_t k = 0; k < all; ++k)
      if (read[k]) index.push_back((uint32_t)k);
    if (index.size() < all) kept = kept.subset(index);
  }

  // ---- the chunks, whole nodes of that table as the converter cuts its source; what a query sets up once, for a table with
  // points: the rows' array, and a polygon's vertices, which go up once, not per chunk
  SourceLoop loop{c, who, kept, mask | fattrs, q->chunk_points};
  uint32_t *d_rows = nullptr, *d_first = nullptr;
  RegionDev region_dev;
  if (loop.rows_max()) {
    if (d_node_out && !count_only) {
      SWZ_TRY(c->get("out_q_rows", (size_t)loop.rows_max(), &d_rows));
      SWZ_TRY(c->get("out_q_first", 2 * (size_t)loop.nodes_max() + 1, &d_first));  // the first rows, then the nodes' indices
    }
    SWZ_TRY(region_upload(c, region_host, &region_dev));
  }
  // ---- what is done with each chunk
  uint64_t total = 0;
  std::vector<uint32_t> node_first;
  const Selection sel{q->box_min, q->box_max, nullptr, &region_dev, filter};
  const SourceChunkBody body = [&](const SourceChunkView& ch) -> int {
    swz_attribute_columns at{};
    for (int a = 0; a < SWZ_ATTR_COUNT; ++a)
      if ((mask >> a) & 1u) at.column[a] = static_cast<uint8_t*>(d_out->column[a]) + total * ATTR_BYTES[a];
    const uint64_t room = count_only ? 0 : capacity - total;
    uint64_t cnt = 0;
    // (a chunk selects its rows at the most: the capacity the kernel's checks see ends with the chunk-local row array)
    const int status = region_select(c, who, ch.xyz, ch.rows, ch.cols, mask, sel, std::min(room, ch.rows),
                                     count_only ? nullptr : d_xyz_out + 3 * total, &at, d_rows, &cnt);
    if (status != SWZ_OK) {
      if (!count_only && cnt > room) {  // the stream stops after this chunk's count
        *count_out = total + cnt;
        return refuse("capacity " + std::to_string(capacity) + " is less than the " + std::to_string(total + cnt) +
                      " rows selected up to chunk " + std::to_string(ch.j));
      }
      return status;
    }
    if (d_rows && cnt) {
      const uint64_t nk = ch.k1 - ch.k0;
      node_first.assign(2 * nk + 1, 0);
      for (uint64_t k = ch.k0; k < ch.k1; ++k) {
        node_first[k - ch.k0 + 1] = node_first[k - ch.k0] + (uint32_t)kept.count[k];
        node_first[nk + 1 + (k - ch.k0)] = index[k];
      }
      SWZ_HIP(c, hipMemcpyAsync(d_first, node_first.data(), node_first.size() * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
      hipLaunchKernelGGL(query_row_nodes_kernel, dim3(div_up(cnt, 256)), dim3(256), 0, c->stream, d_rows, (uint32_t)cnt, d_first,
                         (uint32_t)nk, d_first + nk + 1, d_node_out + total);
      SWZ_LAUNCH_CHECK(c);
      SWZ_HIP(c, hipStreamSynchronize(c->stream));  // (node_first is the next chunk's)
    }
    total += cnt;
    return SWZ_OK;
  };
  SourceLoopStats ls;
  SWZ_TRY(loop.each_chunk(body, &ls));
  *count_out = total;
  if (stats) {
    stats->nodes_scanned = scanned;
    stats->nodes_read = kept.count.size();
    stats->points_read = kept.info.points;
    stats->points_out = total;
    stats->bytes_read = ls.bytes_read;
    stats->chunks = ls.chunks;
    stats->read_ms = ls.read_ms;
    stats->unpack_ms = ls.unpack_ms;
    stats->select_ms = ls.body_ms;
    stats->copy_ms = ls.copy_ms;
    stats->wall_ms = ms_since(t_wall);
  }
  return SWZ_OK;
}

}  // namespace swz

using namespace swz;

extern "C" {

int swz_dataset_query(swz_ctx* c, const char* dir, const swz_query_params* params, uint64_t capacity, double* d_xyz_out,
                      const swz_attribute_columns* d_out, uint32_t* d_node_out, uint64_t* count_out, swz_query_stats* stats) {
  if (!c) return SWZ_ERR_BAD_ARG;
  return query(c, "swz_dataset_query", dir, params, nullptr, nullptr, capacity, d_xyz_out, d_out, d_node_out, count_out, stats);
}

int swz_dataset_query_region(swz_ctx* c, const char* dir, const swz_query_params* params, const swz_region* region, uint64_t capacity,
                             double* d_xyz_out, const swz_attribute_columns* d_out, uint32_t* d_node_out, uint64_t* count_out,
                             swz_query_stats* stats) {
  if (!c) return SWZ_ERR_BAD_ARG;
  return query(c, "swz_dataset_query_region", dir, params, region, nullptr, capacity, d_xyz_out, d_out, d_node_out, count_out, stats);
}

int swz_dataset_query_filtered(swz_ctx* c, const char* dir, const swz_query_params* params, const swz_region* region,
                               const swz_filter* filter, uint64_t capacity, double* d_xyz_out, const swz_attribute_columns* d_out,
                               uint32_t* d_node_out, uint64_t* count_out, swz_query_stats* stats) {
  if (!c) return SWZ_ERR_BAD_ARG;
  return query(c, "swz_dataset_query_filtered", dir, params, region, filter, capacity, d_xyz_out, d_out, d_node_out, count_out, stats);
}

}  // extern "C"
