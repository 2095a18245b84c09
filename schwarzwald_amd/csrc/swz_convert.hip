// swz_convert.hip -- a written data set converted to another format in one call (swz_convert_dataset): the reference's
// --converter mode (ConverterProcess::run, core/process/ConverterProcess.cpp).  The source is scanned (swz_dataset.hip), the
// target is planned with the parts of swz_tiler_write_output (swz_toutput.h), and the node table is streamed chunk by chunk:
// SourceStream (swz_source.hip, which the query shares) reads, copies and unpacks a chunk into chunk-local positions and
// columns (a .pnts source only with SWZ_CONVERT_LOSSY_SOURCE), and output_stream packs, copies back and writes them in the
// target format.  The readers of chunk k + 1 run while chunk k is packed and written.
//
// Size limit: row numbers are chunk-local, so a data set may hold more than 2^32 points; only a chunk, and therefore a
// node, is bound by 2^32 - 65536.  Device and host hold two raw images, one set of chunk-local arrays and two output images.
#include <sys/stat.h>

#include <climits>
#include <cstddef>
#include <cstdlib>

#include <algorithm>
#include <chrono>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "swz_convert.h"
#include "swz_hostio.h"
#include "swz_srs.h"
#include "swz_tinput.h"
#include "swz_toutput.h"

static_assert(sizeof(swz_convert_params) == 128 && offsetof(swz_convert_params, source_flags) == 116 && sizeof(swz_bin_segment) == 32 && sizeof(swz_dataset_info) == 88,
              "the structs of the converter as include/swz_gpu.h and the bindings lay them out");

namespace swz {

__global__ __launch_bounds__(256) void iota_kernel(uint32_t* out, uint32_t n) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i < n) out[i] = i;
}

static bool same_dir(const char* a, const char* b) {
  if (strcmp(a, b) == 0) return true;
  char ra[PATH_MAX], rb[PATH_MAX];
  return realpath(a, ra) && realpath(b, rb) && strcmp(ra, rb) == 0;
}

// swz_convert_dataset, and swz_convert_dataset_world (world: every chunk projected with srs, which may be null, between
// its unpack and its pack, the files relative to their nodes' origins, the tileset with oriented boxes)
static int convert(swz_ctx* c, const char* who, const char* src_dir, const char* dst_dir, const swz_convert_params* params, bool world,
                   const swz_srs* srs, swz_convert_stats* stats) {
  auto refuse = [&](const std::string& what) { return c->fail(SWZ_ERR_BAD_ARG, std::string(who) + ": " + what); };
  if (!src_dir || !dst_dir || !params) return refuse("NULL argument");
  const auto t_wall = std::chrono::steady_clock::now();
  if (stats) *stats = swz_convert_stats{};
  SWZ_HIP(c, hipSetDevice(c->device));

  // ---- the source, then everything that is refused before anything is written
  if (params->source_flags & ~(uint32_t)SWZ_CONVERT_LOSSY_SOURCE) return refuse("an unknown bit in source_flags");
  if (params->reserved[0] || params->reserved[1])
    return refuse(world ? "reserved must be 0 (--delete-source is not offered)"
                        : "reserved must be 0 (--delete-source and --source-projection are not offered: project while tiling)");
  DatasetScan scan;
  SWZ_TRY(source_open(c, who, src_dir, params->max_depth, params->source_flags, &scan, nullptr));
  if (same_dir(src_dir, dst_dir)) return refuse("dst_dir is src_dir");
  swz_output_params op = params->out;
  if (world) {
    if (op.format != SWZ_OUT_3DTILES) return refuse("only 3DTILES is written in the world frame (a LAS or BIN target keeps the source's coordinates: swz_convert_dataset)");
    if (op.global_offset[0] != 0.0 || op.global_offset[1] != 0.0 || op.global_offset[2] != 0.0)
      return refuse("global_offset must be 0: every file is relative to its own node's origin");
    if (srs && !srs_valid(srs)) return refuse("not a definition swz_srs_parse made");
  }
  if (op.attribute_mask == ~0u) op.attribute_mask = scan.info.attribute_mask;
  if (op.attribute_mask & ~scan.info.attribute_mask) return refuse("the attribute_mask names a column the source does not hold");
  double bmin[3], bmax[3];
  float spacing;
  if (params->root_given) {
    if (!finite3(params->root_min) || !finite3(params->root_max) || !std::isfinite(params->spacing_at_root))
      return refuse("the given root box or spacing is not finite");
    memcpy(bmin, params->root_min, sizeof(bmin));
    memcpy(bmax, params->root_max, sizeof(bmax));
    spacing = params->spacing_at_root;
  } else if (scan.info.root_source != SWZ_DATASET_ROOT_ABSENT) {
    memcpy(bmin, scan.info.root_min, sizeof(bmin));
    memcpy(bmax, scan.info.root_max, sizeof(bmax));
    spacing = scan.info.spacing_at_root;
  } else {
    return refuse("no root box and spacing: the source has neither properties.json nor ept.json, and the parameters give none");
  }
  const uint64_t nn = scan.count.size();
  OutputPlan p;
  p.level = scan.level;
  p.key = scan.key;
  p.count = scan.count;
  p.offset.assign(nn, 0);
  SWZ_TRY(output_plan(c, who, &op, scan.info.attribute_mask, bmin, bmax, spacing, dst_dir, &p));
  if (world) {
    p.world = true;
    p.world_srs = srs;
    p.world_min.assign(3 * nn, std::numeric_limits<double>::infinity());
    p.world_max.assign(3 * nn, -std::numeric_limits<double>::infinity());
  }
  SWZ_TRY(output_create_dirs(c, who, &p, dst_dir));

  // ---- the chunks; rows are chunk-local: a node's offset is what its chunk holds in front of it
  std::vector<uint64_t> first;
  uint64_t out_image_max = 0;
  output_cuts(c, p, 0, nn, op.chunk_points, &first, &out_image_max);
  const uint64_t num_chunks = first.empty() ? 0 : first.size() - 1;
  for (uint64_t j = 0; j < num_chunks; ++j) {
    uint64_t at = 0;
    for (uint64_t k = first[j]; k < first[j + 1]; ++k) {
      p.offset[k] = at;
      at += p.count[k];
    }
  }

  OutputStreamStats ss;
  OutputWorkspace ow{c};  // the chunk-local arrays ("out_*") are the call's part of the workspace
  SourceStream source;    // (swz_source.hip) the readers, the raw images and the unpack of every chunk
  source.plan(c, who, &scan, &first, op.attribute_mask);
  int status = SWZ_OK;
  if (out_image_max && source.rows_max) {
    // the identity ids and the images of the way out; the copy stream serves both directions
    OutputSource src;
    uint32_t* d_ids = nullptr;
    SWZ_TRY(c->get("out_cv_ids", (size_t)source.rows_max, &d_ids));
    hipLaunchKernelGGL(iota_kernel, dim3(div_up(source.rows_max, 256)), dim3(256), 0, c->stream, d_ids, (uint32_t)source.rows_max);
    SWZ_LAUNCH_CHECK(c);
    SWZ_HIP(c, hipStreamSynchronize(c->stream));
    OutputImages images;
    SWZ_TRY(images.reserve(c, out_image_max, num_chunks > 1));
    SWZ_TRY(source.start(images.copy));
    src.ids = d_ids;
    src.xyz = source.xyz;
    src.world_xyz = source.xyz;
    src.in = source.cols;
    // chunk j lies in the chunk-local arrays, the readers go on with chunk j + 1 while output_stream packs and writes chunk j
    const OutputChunkFeed feed = [&](uint64_t j, OutputSource*) -> int { return source.next(j); };
    status = output_stream(c, p, first, src, images, 0, &ss, &feed);
  }

  // ---- the metadata, and properties.json for whoever converts the result again
  uint64_t points = 0;
  for (uint64_t k = 0; k < nn; ++k) points += p.count[k];
  if (status == SWZ_OK) status = output_metadata(c, who, p, dst_dir, &op);
  if (status == SWZ_OK) status = swz_properties_json_write(c, dst_dir, bmin, bmax, spacing, points);
  if (stats) {
    stats->nodes = nn;
    stats->points = points;
    stats->bytes_read = source.bytes_read;
    stats->bytes_written = ss.bytes_written;
    stats->chunks = ss.chunks;
    stats->read_ms = source.read_ms;
    stats->unpack_ms = source.unpack_ms;
    stats->pack_ms = ss.pack_ms;
    stats->copy_ms = source.copy_ms + ss.copy_ms;
    stats->write_ms = ss.write_ms;
    stats->wall_ms = ms_since(t_wall);
  }
  return status;
}

}  // namespace swz

using namespace swz;

extern "C" {

int swz_convert_dataset(swz_ctx* c, const char* src_dir, const char* dst_dir, const swz_convert_params* params,
                        swz_convert_stats* stats) {
  if (!c) return SWZ_ERR_BAD_ARG;
  return convert(c, "swz_convert_dataset", src_dir, dst_dir, params, false, nullptr, stats);
}

int swz_convert_dataset_world(swz_ctx* c, const char* src_dir, const char* dst_dir, const swz_convert_params* params,
                              const swz_srs* srs, swz_convert_stats* stats) {
  if (!c) return SWZ_ERR_BAD_ARG;
  return convert(c, "swz_convert_dataset_world", src_dir, dst_dir, params, true, srs, stats);
}

}  // extern "C"
