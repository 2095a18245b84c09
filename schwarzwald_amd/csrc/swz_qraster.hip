// swz_qraster.hip -- swz_dataset_rasterize: the raster (swz_raster.hip) as a chunk body of SourceLoop::each_chunk
// (swz_source.hip), beside the streaming query (swz_query.hip) and swz_dataset_summarize.  Planning is the query's
// (swz_qplan.hip): the nodes whose widened boxes meet the box and the region, less those the directory's node-summaries.swz
// shows the filter cannot reach.  The stream unpacks the filter's columns and the value's and nothing else.  A chunk of the box
// alone goes straight through the accumulate kernel, which tests the box itself; with a region or a filter the selection
// (region_select, swz_select.hip) compacts positions and the value column into the workspace first.  The cell table lives in
// the workspace for the call: preset before the first chunk, copied to the caller's host array behind the last.
#include <chrono>
#include <string>
#include <vector>

#include "swz_convert.h"
#include "swz_hostio.h"
#include "swz_qplan.h"
#include "swz_raster.h"
#include "swz_select.h"

namespace swz {

static int rasterize(swz_ctx* c, const char* who, const char* dir, const swz_query_params* q, const swz_region* region,
                     const swz_filter* filter, const swz_raster_grid* grid, swz_raster_cell* cells_out, swz_raster_frame* frame_out,
                     swz_query_stats* stats) {
  auto refuse = [&](const std::string& what) { return c->fail(SWZ_ERR_BAD_ARG, std::string(who) + ": " + what); };
  const auto t_wall = std::chrono::steady_clock::now();
  if (stats) *stats = swz_query_stats{};
  if (!dir || !q || !grid || !cells_out || !frame_out) return refuse("NULL argument");
  if (q->attribute_mask != 0 && q->attribute_mask != ~0u) return refuse("the attribute_mask of a raster must be 0 or ~0u (it is ignored: the value chooses the column)");
  swz_raster_frame frame;
  SWZ_TRY(raster_frame(c, who, q->box_min, q->box_max, grid, &frame));  // (before any file is read)
  DatasetScan kept;
  uint64_t scanned = 0;
  RegionHost region_host;
  uint32_t fattrs = 0;
  SWZ_TRY(query_plan(c, who, dir, q, region, filter, &kept, &scanned, &region_host, &fattrs));
  const int value = frame.value;
  const uint32_t vmask = value == SWZ_RASTER_VALUE_Z ? 0u : 1u << value;
  if (vmask) {
    if (kept.info.format == SWZ_OUT_3DTILES && value != SWZ_ATTR_INTENSITY)
      return refuse(std::string("the value is ") + attribute_name(value) + ", which .pnts files do not carry (a 3DTILES source holds RGB and intensity)");
    if (!(kept.info.attribute_mask & vmask)) {
      char hex[16];
      snprintf(hex, sizeof(hex), "0x%x", kept.info.attribute_mask);
      return refuse(std::string("the value is ") + attribute_name(value) + ", which the source does not hold (its attribute mask is " + hex + ")");
    }
  }
  {
    std::vector<uint8_t> read;
    SWZ_TRY(filter_reads(c, who, dir, kept, filter, &read));
    std::vector<uint32_t> index;
    const uint64_t all = kept.count.size();
    for (uint64_t k = 0; k < all; ++k)
      if (read[k]) index.push_back((uint32_t)k);
    if (index.size() < all) kept = kept.subset(index);
  }
  if (kept.info.points > 0xFFFFFFFFull)
    return refuse("the nodes to read hold " + std::to_string(kept.info.points) + " rows, more than the 2^32 - 1 a cell's sum has room for");

  const uint64_t ncells = (uint64_t)frame.nx * frame.ny;
  const bool box_alone = region_host.kind == SWZ_REGION_BOX && !(filter && filter->count);
  SourceLoop loop{c, who, kept, fattrs | vmask, q->chunk_points};
  SourceLoopStats ls;
  if (loop.rows_max()) {
    SWZ_HIP(c, hipSetDevice(c->device));
    // ---- what a call sets up once: the table, a polygon's vertices and, unless the box is alone, the compacted rows
    swz_raster_cell* d_cells = nullptr;
    SWZ_TRY(c->get("out_raster_cells", (size_t)ncells, &d_cells));
    double* d_sel_xyz = nullptr;
    uint8_t* d_sel_value = nullptr;
    RegionDev region_dev;
    if (!box_alone) {
      SWZ_TRY(c->get("out_raster_xyz", (size_t)loop.rows_max() * 3, &d_sel_xyz));
      if (vmask) SWZ_TRY(c->get("out_raster_value", (size_t)loop.rows_max() * ATTR_BYTES[value], &d_sel_value));
      SWZ_TRY(region_upload(c, region_host, &region_dev));
    }
    SWZ_TRY(raster_clear(c, who, &frame, d_cells));
    // ---- what is done with each chunk
    const Selection sel{q->box_min, q->box_max, nullptr, &region_dev, filter};
    const SourceChunkBody body = [&](const SourceChunkView& ch) -> int {
      if (box_alone)
        return raster_accumulate(c, who, ch.xyz, ch.rows, vmask ? ch.cols->column[value] : nullptr, q->box_min, q->box_max, &frame, d_cells);
      swz_attribute_columns at{};
      if (vmask) at.column[value] = d_sel_value;
      uint64_t cnt = 0;
      SWZ_TRY(region_select(c, who, ch.xyz, ch.rows, ch.cols, vmask, sel, ch.rows, d_sel_xyz, &at, nullptr, &cnt));
      return raster_accumulate(c, who, d_sel_xyz, cnt, d_sel_value, q->box_min, q->box_max, &frame, d_cells);
    };
    SWZ_TRY(loop.each_chunk(body, &ls));
    SWZ_HIP(c, hipMemcpyAsync(cells_out, d_cells, ncells * sizeof(swz_raster_cell), hipMemcpyDeviceToHost, c->stream));
    SWZ_HIP(c, hipStreamSynchronize(c->stream));
  } else {
    for (uint64_t i = 0; i < ncells; ++i) cells_out[i] = raster_empty_cell();  // no node with points: nothing is launched
  }
  *frame_out = frame;
  if (stats) {
    uint64_t total = 0;
    for (uint64_t i = 0; i < ncells; ++i) total += cells_out[i].count;
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

int swz_dataset_rasterize(swz_ctx* c, const char* dir, const swz_query_params* params, const swz_region* region, const swz_filter* filter,
                          const swz_raster_grid* grid, swz_raster_cell* cells_out, swz_raster_frame* frame_out, swz_query_stats* stats) {
  if (!c) return SWZ_ERR_BAD_ARG;
  return rasterize(c, "swz_dataset_rasterize", dir, params, region, filter, grid, cells_out, frame_out, stats);
}

}  // extern "C"
