// swz_toutput.hip -- the node files of a tiler written in one call (swz_tiler_write_output): the node table is cut into
// chunks of whole nodes, and while the writer threads write the files of chunk k out of one page-locked host buffer, chunk
// k + 1 is packed on the device (swz_bin_pack_device, swz_pnts_pack_device, swz_las_pack_device, straight from the pools) and
// copied into the other one.  File names, node boxes, LAS offsets and scales are what TilingAlgorithmGPU::finalize and the
// sinks of host/swz_tiling.hpp compute from the node table.  The call's three parts -- plan, stream a node range, metadata --
// are functions of their own (swz_toutput.h): swz_group_write_output (swz_goutput.hip) runs the middle one per shard and the
// other two once, on the table swz_merge_shard_node_tables (here) makes of the shards' tables.
#include <sys/stat.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstddef>
#include <limits>
#include <string>
#include <vector>

#include "swz_convert.h"
#include "swz_toutput.h"
#include "swz_hostio.h"

// `flags` took the four bytes of padding behind rgb_mapping: a caller built against the struct without it, which
// value-initialises the struct, passes 0 there and gets what it got before
static_assert(sizeof(swz_output_params) == 56 && offsetof(swz_output_params, format) == 0 &&
                offsetof(swz_output_params, attribute_mask) == 4 && offsetof(swz_output_params, rgb_mapping) == 8 &&
                offsetof(swz_output_params, flags) == 12 && offsetof(swz_output_params, global_offset) == 16 &&
                offsetof(swz_output_params, chunk_points) == 40 && offsetof(swz_output_params, ept) == 48,
              "swz_output_params: flags must sit in the former padding, every other member where it was");

namespace swz {

constexpr uint64_t OUTPUT_CHUNK_POINTS = 16ull << 20;  // TilingAlgorithmGPU's export chunk

static int plan_layout(swz_ctx* c, const char* who, OutputPlan& p) {
  const uint64_t nn = p.count.size();
  p.body_at.resize(nn);
  p.body_size.resize(nn);
  p.file_size.assign(nn, 0);
  int st = SWZ_OK;
  switch (p.format) {
    case SWZ_OUT_BIN:
    case SWZ_OUT_BINZ: st = swz_bin_layout(nn, p.count.data(), p.mask, p.body_at.data(), p.body_size.data(), p.file_size.data(), nullptr); break;
    case SWZ_OUT_3DTILES:
      st = swz_pnts_layout(nn, p.count.data(), p.mask, p.rgb_mapping, p.body_at.data(), p.body_size.data(), nullptr, nullptr, nullptr);
      break;
    default: st = swz_las_image_layout(nn, p.count.data(), p.mask, p.body_at.data(), p.body_size.data(), nullptr); break;
  }
  if (st != SWZ_OK) return c->fail(SWZ_ERR_BAD_ARG, std::string(who) + ": a node is too large for a file of this format");
  return SWZ_OK;
}

// the file of node k out of the host image of its chunk, whose first body lies at image_at of the whole table's image
static int write_node_file(const OutputPlan& p, uint64_t k, const unsigned char* image, uint64_t image_at, std::string* err) {
  if (p.count[k] == 0) return SWZ_OK;
  const unsigned char* body = image + (p.body_at[k] - image_at);
  char name[72];
  if (p.format == SWZ_OUT_ENTWINE_LAS) (void)swz_node_name_entwine(p.level[k], p.key[k], name);
  else (void)swz_node_name(p.level[k], p.key[k], name);
  const std::string stem = p.data_dir + "/" + name;
  int st = SWZ_OK;
  std::string path;
  switch (p.format) {
    case SWZ_OUT_BIN: return write_file(stem + ".bin", {{body, (size_t)p.file_size[k]}}, err);
    case SWZ_OUT_BINZ: return write_file_zlib(stem + ".binz", body, (size_t)p.file_size[k], err);
    case SWZ_OUT_3DTILES:
      path = stem + ".pnts";
      st = swz_pnts_write_node(nullptr, path.c_str(), p.count[k], body, p.body_size[k], p.mask, p.world ? &p.world_min[3 * k] : p.rtc);
      break;
    default:
      path = stem + ".las";
      if (p.tight) {  // the header's extent: the box of the stored records; offset, scale and records as without the flag
        double lo[3], hi[3];
        (void)swz_las_stored_box(&p.tight_min[3 * k], &p.tight_max[3 * k], &p.box_min[3 * k], p.scale[k], lo, hi);
        st = swz_las_write_node_extent(nullptr, path.c_str(), p.count[k], body, p.mask, &p.box_min[3 * k], &p.box_max[3 * k], p.scale[k], lo, hi);
        break;
      }
      st = swz_las_write_node(nullptr, path.c_str(), p.count[k], body, p.mask, &p.box_min[3 * k], &p.box_max[3 * k], p.scale[k]);
      break;
  }
  if (st != SWZ_OK) *err = "cannot write " + path;
  return st;
}

static int make_dir(const std::string& path) {
  if (mkdir(path.c_str(), 0777) == 0) return 0;
  struct stat st;
  return (stat(path.c_str(), &st) == 0 && S_ISDIR(st.st_mode)) ? 0 : -1;
}


OutputImages::~OutputImages() {
  for (int b = 0; b < 2; ++b) {
    if (host[b]) (void)hipHostFree(host[b]);
    if (begin[b]) (void)hipEventDestroy(begin[b]);
    if (end[b]) (void)hipEventDestroy(end[b]);
  }
  if (copy) (void)hipStreamDestroy(copy);
}

int OutputImages::reserve(swz_ctx* ctx, uint64_t image_bytes, bool two) {
  c = ctx;
  SWZ_TRY(c->get("out_image0", (size_t)image_bytes, &device[0]));
  if (two) SWZ_TRY(c->get("out_image1", (size_t)image_bytes, &device[1]));
  SWZ_HIP(c, hipStreamCreateWithFlags(&copy, hipStreamNonBlocking));
  for (int b = 0; b < (two ? 2 : 1); ++b) {
    SWZ_HIP(c, hipHostMalloc(&host[b], image_bytes, hipHostMallocDefault));
    SWZ_HIP(c, hipEventCreate(&begin[b]));
    SWZ_HIP(c, hipEventCreate(&end[b]));
  }
  return SWZ_OK;
}

OutputWorkspace::~OutputWorkspace() {
  for (auto it = c->bufs.begin(); it != c->bufs.end();) {
    if (it->first.compare(0, 4, "out_") != 0) {
      ++it;
      continue;
    }
    c->free_buf(it->second);
    it = c->bufs.erase(it);
  }
}

int output_tiler_table(swz_tiler* t, const char* who, OutputPlan* p, swz_tiler_info* info) {
  swz_ctx* c = t->c;
  SWZ_TRY(swz_tiler_get_info(t, info));  // (a poisoned tiler answers here)
  const uint64_t cap_nodes = std::max<uint64_t>(info->num_nodes, 1);
  p->level.resize(cap_nodes);
  p->key.resize(cap_nodes);
  p->offset.resize(cap_nodes);
  p->count.resize(cap_nodes);
  uint64_t nn = 0;
  SWZ_TRY(swz_tiler_node_table(t, cap_nodes, p->level.data(), p->key.data(), p->offset.data(), p->count.data(), &nn));
  p->level.resize(nn);
  p->key.resize(nn);
  p->offset.resize(nn);
  p->count.resize(nn);
  if (!t->staged_sizes.empty() || t->batch_open) return c->fail(SWZ_ERR_BAD_ARG, std::string(who) + ": a batch is staged or open");
  return SWZ_OK;
}

int output_plan(swz_ctx* c, const char* who, const swz_output_params* params, uint32_t attr_mask, const double bmin[3],
                const double bmax[3], float spacing_at_root, const char* dir, OutputPlan* plan) {
  OutputPlan& p = *plan;
  const std::string w = std::string(who) + ": ";
  const uint64_t nn = p.count.size();
  if (params->format < SWZ_OUT_BIN || params->format > SWZ_OUT_ENTWINE_LAS) return c->fail(SWZ_ERR_BAD_ARG, w + "unknown format");
  if (params->attribute_mask & ~attr_mask) return c->fail(SWZ_ERR_BAD_ARG, w + "the mask names a column the batches did not carry");
  const char* bad_flags = nullptr;
  if (swz_output_flags_check(params->format, params->flags, &bad_flags) != SWZ_OK) return c->fail(SWZ_ERR_BAD_ARG, w + bad_flags);
  p.tight = (params->flags & SWZ_OUT_TIGHT_BOUNDS) != 0;
  if (p.tight) {
    p.tight_min.assign(3 * nn, std::numeric_limits<double>::infinity());
    p.tight_max.assign(3 * nn, -std::numeric_limits<double>::infinity());
  }
  p.format = params->format;
  p.mask = params->attribute_mask;
  p.data_dir = dir;
  p.spacing_at_root = spacing_at_root;
  for (int a = 0; a < 3; ++a) {
    p.bmin[a] = bmin[a];
    p.bmax[a] = bmax[a];
  }
  if (p.format == SWZ_OUT_3DTILES) {
    const int m = params->rgb_mapping;
    if (m != SWZ_PNTS_RGB_FROM_COLOR && m != SWZ_PNTS_RGB_FROM_INTENSITY_LINEAR && m != SWZ_PNTS_RGB_FROM_INTENSITY_LOG)
      return c->fail(SWZ_ERR_BAD_ARG, w + "unknown rgb_mapping");
    const bool mapped = m != SWZ_PNTS_RGB_FROM_COLOR, has_intensity = (params->attribute_mask & SWZ_PNTS_INTENSITY) != 0;
    if (mapped && !has_intensity) return c->fail(SWZ_ERR_BAD_ARG, w + "an rgb_mapping needs the intensities in the mask");
    if (!finite3(params->global_offset)) return c->fail(SWZ_ERR_BAD_ARG, w + "global_offset is not finite");
    // (Cesium3DTilesSink::persist_rows: RGB and INTENSITY of what the rows carry, with a mapping RGB out of the intensity)
    p.mask = has_intensity ? SWZ_PNTS_INTENSITY : 0u;
    if (mapped ? has_intensity : (params->attribute_mask & SWZ_PNTS_RGB) != 0) p.mask |= SWZ_PNTS_RGB;
    p.rgb_mapping = m;
    for (int a = 0; a < 3; ++a) p.rtc[a] = params->global_offset[a];
  }
  SWZ_TRY(plan_layout(c, who, p));
  if (p.format == SWZ_OUT_LAS || p.format == SWZ_OUT_ENTWINE_LAS) {
    p.box_min.resize(3 * nn);
    p.box_max.resize(3 * nn);
    p.scale.resize(nn);
    for (uint64_t k = 0; k < nn; ++k) {
      if (swz_node_bounds(p.level[k], p.key[k], bmin, bmax, &p.box_min[3 * k], &p.box_max[3 * k]) != SWZ_OK)
        return c->fail(SWZ_ERR_INTERNAL, w + "bad node level");
      p.scale[k] = swz_las_scale_from_bounds(&p.box_min[3 * k], &p.box_max[3 * k]);
    }
  }
  return SWZ_OK;
}

int output_create_dirs(swz_ctx* c, const char* who, OutputPlan* p, const char* dir) {
  if (p->format == SWZ_OUT_ENTWINE_LAS) {
    if (swz_ept_create_dirs(nullptr, dir) != SWZ_OK)
      return c->fail(SWZ_ERR_BAD_ARG, std::string(who) + ": cannot create the ept directories under " + dir);
    p->data_dir = std::string(dir) + "/ept-data";
  } else if (make_dir(dir) != 0) {
    return c->fail(SWZ_ERR_BAD_ARG, std::string(who) + ": cannot create " + dir);
  }
  return SWZ_OK;
}

// where node `node`'s body begins in the image of the whole table (node == the table's size: where the image ends)
static uint64_t image_at(const OutputPlan& p, uint64_t node) {
  const uint64_t nn = p.count.size();
  return node < nn ? p.body_at[node] : (nn ? p.body_at[nn - 1] + p.body_size[nn - 1] : 0);
}

uint64_t output_chunk_points(swz_ctx* c, uint64_t chunk_points) {
  return chunk_points ? chunk_points : (uint64_t)std::max(1L, c->opt_int("SWZ_OUTPUT_CHUNK_POINTS", (long)OUTPUT_CHUNK_POINTS));
}

void output_cuts(swz_ctx* c, const OutputPlan& p, uint64_t k0, uint64_t k1, uint64_t chunk_points, std::vector<uint64_t>* first,
                 uint64_t* image_max) {
  source_cuts(c, p.count.data() + k0, k1 - k0, chunk_points, first);
  for (uint64_t& f : *first) f += k0;
  *image_max = 0;
  for (size_t j = 0; j + 1 < first->size(); ++j) *image_max = std::max(*image_max, image_at(p, (*first)[j + 1]) - image_at(p, (*first)[j]));
}

int output_stream(swz_ctx* c, OutputPlan& p, const std::vector<uint64_t>& first, const OutputSource& source, OutputImages& ob,
                  long writer_threads, OutputStreamStats* stats, const OutputChunkFeed* feed) {
  OutputSource src = source;
  const uint64_t num_chunks = first.empty() ? 0 : first.size() - 1;
  int status = SWZ_OK;
  std::string why;
  TicketRun writers;  // of the chunk before
  auto join_writers = [&]() {
    if (!writers.running()) return;
    double ms = 0;
    std::string err;
    const int st = writers.wait(&err, &ms);
    stats->write_ms += ms;
    if (st != SWZ_OK && status == SWZ_OK) {
      status = st;
      why = err;
    }
  };
  std::vector<uint64_t> rel_offset;
  for (uint64_t j = 0; j < num_chunks && status == SWZ_OK; ++j) {
    const int b = ob.device[1] ? (int)(j & 1) : 0;
    const uint64_t k0 = first[j], k1 = first[j + 1];
    const uint64_t at0 = image_at(p, k0), bytes = image_at(p, k1) - at0;
    if (feed && *feed) {
      const int st = (*feed)(j, &src);
      if (st != SWZ_OK) {
        status = st;
        why = c->err;
        break;
      }
    }
    const uint64_t row0 = p.offset[k0];
    const uint64_t rows = p.offset[k1 - 1] + p.count[k1 - 1] - row0;
    // buffer b, device and host: chunk j - 2 has been copied out of the one and written out of the other (with one buffer
    // only, the writers of the chunk before are joined before the copy)
    if (bytes) {
      rel_offset.resize(k1 - k0);
      for (uint64_t k = k0; k < k1; ++k) rel_offset[k - k0] = p.offset[k] - row0;
      const auto t_pack = std::chrono::steady_clock::now();
      int st = SWZ_OK;
      switch (p.format) {
        case SWZ_OUT_BIN:
        case SWZ_OUT_BINZ:
          st = swz_bin_pack_device(c, src.ids + row0, nullptr, rows, src.xyz, &src.in, k1 - k0, rel_offset.data(), &p.count[k0], p.mask,
                                   ob.device[b], bytes);
          break;
        case SWZ_OUT_3DTILES:
          if (p.world) {
            // the chunk's rows to ECEF in place and the boxes of its nodes' projected rows; their minima are the files' origins
            st = swz_srs_project_node_boxes_device(c, p.world_srs, src.world_xyz + 3 * row0, rows, k1 - k0, rel_offset.data(),
                                                   &p.count[k0], &p.world_min[3 * k0], &p.world_max[3 * k0]);
            if (st == SWZ_OK)
              st = swz_pnts_pack_origin_device(c, src.ids + row0, nullptr, rows, src.xyz, &src.in, k1 - k0, rel_offset.data(),
                                               &p.count[k0], p.mask, p.rgb_mapping, ob.device[b], bytes, &p.world_min[3 * k0]);
            break;
          }
          st = swz_pnts_pack_device(c, src.ids + row0, nullptr, rows, src.xyz, &src.in, k1 - k0, rel_offset.data(), &p.count[k0], p.mask,
                                    p.rgb_mapping, ob.device[b], bytes);
          break;
        default:
          st = swz_las_pack_device(c, src.ids + row0, nullptr, rows, src.xyz, &src.in, k1 - k0, rel_offset.data(), &p.count[k0],
                                   &p.box_min[3 * k0], &p.scale[k0], p.mask, ob.device[b], bytes);
          break;
      }
      // (the boxes of chunk j's nodes: the writers of chunk j - 1 read other entries, and chunk j's start after this)
      if (st == SWZ_OK && p.tight && !p.world)  // (a world plan has its boxes already)
        st = swz_node_boxes_device(c, src.ids + row0, nullptr, rows, src.xyz, k1 - k0, rel_offset.data(), &p.count[k0],
                                   &p.tight_min[3 * k0], &p.tight_max[3 * k0]);
      stats->pack_ms += ms_since(t_pack);
      if (!ob.device[1]) join_writers();  // one image: its files are written before it is overwritten
      hipError_t e = hipSuccess;
      if (st == SWZ_OK) e = hipEventRecord(ob.begin[b], ob.copy);
      if (st == SWZ_OK && e == hipSuccess) e = hipMemcpyAsync(ob.host[b], ob.device[b], bytes, hipMemcpyDeviceToHost, ob.copy);
      if (st == SWZ_OK && e == hipSuccess) e = hipEventRecord(ob.end[b], ob.copy);
      // the files of the chunk before are being written all the while; they end before the next ones begin
      join_writers();
      if (st == SWZ_OK && e == hipSuccess) e = hipEventSynchronize(ob.end[b]);
      if (st != SWZ_OK) {
        if (status == SWZ_OK) {
          status = st;
          why = c->err;
        }
        break;
      }
      if (e != hipSuccess) {
        if (status == SWZ_OK) {
          status = c->hip_fail(e, "the copy of a chunk image", __FILE__, __LINE__);
          why = c->err;
        }
        break;
      }
      float ms = 0.f;
      if (hipEventElapsedTime(&ms, ob.begin[b], ob.end[b]) == hipSuccess) stats->copy_ms += ms;
      if (status != SWZ_OK) break;  // a file of the chunk before could not be written
      const unsigned char* image = static_cast<const unsigned char*>(ob.host[b]);
      const OutputPlan* plan = &p;
      writers.start(c, k1 - k0, [plan, k0, image, at0](uint64_t i, std::string* err) { return write_node_file(*plan, k0 + i, image, at0, err); },
                    writer_threads);
      stats->bytes_written += bytes;
    }
    ++stats->chunks;
  }
  join_writers();
  (void)hipStreamSynchronize(ob.copy);
  return status == SWZ_OK ? SWZ_OK : c->fail(status, why);
}

int output_metadata(swz_ctx* c, const char* who, const OutputPlan& p, const char* dir, const swz_output_params* params) {
  const uint64_t nn = p.count.size();
  if (p.format == SWZ_OUT_3DTILES && nn && p.world) {
    // the tree on the SOURCE root box, its cubes as oriented boxes in the target; with tight bounds the entries that hold
    // points below them get the axis-aligned box of what the files hold instead: origin + the floats, evaluated in double
    // like a reader does (narrowing and the sum are monotonic, so the largest offset bounds every point's)
    uint64_t num = 0;
    int st = swz_tileset_build(nn, p.level.data(), p.key.data(), p.bmin, p.bmax, p.spacing_at_root, nullptr, 0, nullptr, &num);
    std::vector<swz_tileset_node> tiles(num);
    if (st == SWZ_OK) st = swz_tileset_build(nn, p.level.data(), p.key.data(), p.bmin, p.bmax, p.spacing_at_root, nullptr, num, tiles.data(), &num);
    std::vector<double> obb(12 * num);
    if (st == SWZ_OK) st = swz_tileset_oriented_boxes(p.world_srs, tiles.data(), num, obb.data());
    if (st == SWZ_OK && p.tight) {
      std::vector<double> hi(p.world_max);
      for (size_t i = 0; i < hi.size(); ++i)
        if (p.world_min[i] <= p.world_max[i]) hi[i] = p.world_min[i] + (double)(float)(p.world_max[i] - p.world_min[i]);
      st = swz_tileset_build_boxes(nn, p.level.data(), p.key.data(), p.world_min.data(), hi.data(), p.bmin, p.bmax, p.spacing_at_root,
                                   nullptr, num, tiles.data(), &num);
    }
    if (st != SWZ_OK) return c->fail(st, std::string(who) + ": swz_tileset_build failed");
    SWZ_TRY(swz_tileset_write_oriented(c, tiles.data(), num, obb.data(), dir));
  } else if (p.format == SWZ_OUT_3DTILES && nn) {
    uint64_t num = 0;
    std::vector<swz_tileset_node> tiles;
    int st = swz_tileset_build(nn, p.level.data(), p.key.data(), p.bmin, p.bmax, p.spacing_at_root, p.rtc, 0, nullptr, &num);
    if (st == SWZ_OK) {
      tiles.resize(num);
      if (p.tight) {
        // the box of what a .pnts file HOLDS: the floats the positions were narrowed to (narrowing is monotonic)
        std::vector<double> lo(p.tight_min), hi(p.tight_max);
        for (double& v : lo) v = (double)(float)v;
        for (double& v : hi) v = (double)(float)v;
        st = swz_tileset_build_boxes(nn, p.level.data(), p.key.data(), lo.data(), hi.data(), p.bmin, p.bmax, p.spacing_at_root, p.rtc,
                                     num, tiles.data(), &num);
      } else {
        st = swz_tileset_build(nn, p.level.data(), p.key.data(), p.bmin, p.bmax, p.spacing_at_root, p.rtc, num, tiles.data(), &num);
      }
    }
    if (st != SWZ_OK) return c->fail(st, std::string(who) + ": swz_tileset_build failed");
    SWZ_TRY(swz_tileset_write(c, tiles.data(), num, dir));
  }
  if (p.format == SWZ_OUT_ENTWINE_LAS) {
    SWZ_TRY(swz_ept_hierarchy_write(c, dir, nn, p.level.data(), p.key.data(), p.count.data()));
    if (params->ept) {
      swz_ept_json ept = *params->ept;
      if (p.tight) {  // boundsConforming: the union of the files' extents; without a point it stays the caller's
        double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
        for (uint64_t k = 0; k < nn; ++k) {
          if (p.count[k] == 0) continue;
          double a[3], b[3];
          (void)swz_las_stored_box(&p.tight_min[3 * k], &p.tight_max[3 * k], &p.box_min[3 * k], p.scale[k], a, b);
          for (int ax = 0; ax < 3; ++ax) {
            lo[ax] = std::min(lo[ax], a[ax]);
            hi[ax] = std::max(hi[ax], b[ax]);
          }
        }
        for (int ax = 0; ax < 3 && lo[0] <= hi[0]; ++ax) {
          ept.conforming_min[ax] = lo[ax];
          ept.conforming_max[ax] = hi[ax];
        }
      }
      SWZ_TRY(swz_ept_json_write(c, (std::string(dir) + "/ept.json").c_str(), &ept));
    }
  }
  return SWZ_OK;
}

}  // namespace swz

using namespace swz;

extern "C" {

int swz_output_chunks(uint64_t num_nodes, const uint64_t* node_count, uint64_t chunk_points, uint64_t max_chunks,
                      uint64_t* first_node_out, uint64_t* num_chunks_out) {
  if (!num_chunks_out || (num_nodes && !node_count)) return SWZ_ERR_BAD_ARG;
  uint64_t largest = 0;
  for (uint64_t j = 0; j < num_nodes; ++j) largest = std::max(largest, node_count[j]);
  const uint64_t cap = std::max(std::max<uint64_t>(chunk_points, 1), largest);  // a chunk is never smaller than the largest node
  uint64_t chunks = 0;
  for (uint64_t j0 = 0; j0 < num_nodes;) {
    uint64_t j1 = j0, cnt = 0;
    while (j1 < num_nodes && node_count[j1] <= cap - cnt) cnt += node_count[j1++];
    if (first_node_out) {
      if (chunks >= max_chunks) return SWZ_ERR_BAD_ARG;
      first_node_out[chunks] = j0;
    }
    ++chunks;
    j0 = j1;
  }
  if (first_node_out) first_node_out[chunks] = num_nodes;
  *num_chunks_out = chunks;
  return SWZ_OK;
}

int swz_tiler_write_output(swz_tiler* t, const char* dir, const swz_output_params* params, swz_output_stats* stats) {
  if (!t) return SWZ_ERR_BAD_ARG;
  swz_ctx* c = t->c;
  const char* who = "swz_tiler_write_output";
  if (!dir || !params) return c->fail(SWZ_ERR_BAD_ARG, "swz_tiler_write_output: NULL argument");
  const auto t_wall = std::chrono::steady_clock::now();
  SWZ_HIP(c, hipSetDevice(c->device));
  if (stats) *stats = swz_output_stats{};

  // ---- the node table (a poisoned tiler answers here), then everything that is refused before anything is written
  swz_tiler_info info{};
  OutputPlan p;
  SWZ_TRY(output_tiler_table(t, who, &p, &info));
  SWZ_TRY(output_plan(c, who, params, t->attr_mask, t->bmin, t->bmax, t->p.spacing_at_root, dir, &p));
  SWZ_TRY(output_create_dirs(c, who, &p, dir));

  // ---- the chunks, and the largest chunk image
  const uint64_t nn = p.count.size(), ns = info.num_stored;
  std::vector<uint64_t> first;
  uint64_t image_max = 0;
  output_cuts(c, p, 0, nn, params->chunk_points, &first, &image_max);
  OutputStreamStats ss;
  int status = SWZ_OK;
  if (image_max) {
    uint32_t* d_ids = nullptr;
    OutputWorkspace ow{c};
    SWZ_TRY(c->get("out_ids", (size_t)ns, &d_ids));
    OutputImages images;
    SWZ_TRY(images.reserve(c, image_max, first.size() > 2));
    SWZ_TRY(swz_tiler_export_device(t, nullptr, d_ids, nullptr));
    OutputSource src;
    src.ids = d_ids;
    src.xyz = t->pool_xyz;
    for (int a = 0; a < SWZ_ATTR_COUNT; ++a) src.in.column[a] = (t->attr_mask & (1u << a)) ? t->pool_attr[a] : nullptr;
    status = output_stream(c, p, first, src, images, 0, &ss);
  }
  // ---- the metadata
  if (status == SWZ_OK) status = output_metadata(c, who, p, dir, params);
  if (stats) {
    stats->nodes = nn;
    stats->stored_points = ns;
    stats->bytes_written = ss.bytes_written;
    stats->chunks = ss.chunks;
    stats->pack_ms = ss.pack_ms;
    stats->copy_ms = ss.copy_ms;
    stats->write_ms = ss.write_ms;
    stats->wall_ms = ms_since(t_wall);
  }
  return status;
}

int swz_output_flags_check(int format, uint32_t flags, const char** what_out) {
  const char* what = nullptr;
  if (flags & ~(uint32_t)SWZ_OUT_TIGHT_BOUNDS) what = "unknown flag bit";
  else if ((flags & SWZ_OUT_TIGHT_BOUNDS) && (format == SWZ_OUT_BIN || format == SWZ_OUT_BINZ))
    what = "SWZ_OUT_TIGHT_BOUNDS: BIN and BINZ files hold no box";
  if (what_out) *what_out = what;
  return what ? SWZ_ERR_BAD_ARG : SWZ_OK;
}

int swz_tiler_node_boxes(swz_tiler* t, uint64_t max_nodes, double* box_min_out, double* box_max_out, uint64_t* num_nodes_out) {
  if (!t) return SWZ_ERR_BAD_ARG;
  swz_ctx* c = t->c;
  const char* who = "swz_tiler_node_boxes";
  if (!num_nodes_out) return c->fail(SWZ_ERR_BAD_ARG, "swz_tiler_node_boxes: NULL argument");
  SWZ_HIP(c, hipSetDevice(c->device));
  swz_tiler_info info{};
  OutputPlan p;
  SWZ_TRY(output_tiler_table(t, who, &p, &info));
  const uint64_t nn = p.count.size(), ns = info.num_stored;
  *num_nodes_out = nn;
  if (nn > max_nodes || (nn && (!box_min_out || !box_max_out)))
    return c->fail(SWZ_ERR_BAD_ARG, "swz_tiler_node_boxes: max_nodes too small, or a NULL buffer");
  for (uint64_t i = 0; i < 3 * nn; ++i) {
    box_min_out[i] = std::numeric_limits<double>::infinity();
    box_max_out[i] = -std::numeric_limits<double>::infinity();
  }
  if (!ns) return SWZ_OK;
  // the chunks of swz_tiler_write_output (no image: only the rows count), the ids exported once
  p.body_at.assign(nn, 0);
  p.body_size.assign(nn, 0);
  std::vector<uint64_t> first;
  uint64_t image_max = 0;
  output_cuts(c, p, 0, nn, 0, &first, &image_max);
  uint32_t* d_ids = nullptr;
  OutputWorkspace ow{c};
  SWZ_TRY(c->get("out_ids", (size_t)ns, &d_ids));
  SWZ_TRY(swz_tiler_export_device(t, nullptr, d_ids, nullptr));
  std::vector<uint64_t> rel_offset;
  for (size_t j = 0; j + 1 < first.size(); ++j) {
    const uint64_t k0 = first[j], k1 = first[j + 1];
    if (k0 == k1) continue;
    const uint64_t row0 = p.offset[k0], rows = p.offset[k1 - 1] + p.count[k1 - 1] - row0;
    rel_offset.resize(k1 - k0);
    for (uint64_t k = k0; k < k1; ++k) rel_offset[k - k0] = p.offset[k] - row0;
    SWZ_TRY(swz_node_boxes_device(c, d_ids + row0, nullptr, rows, t->pool_xyz, k1 - k0, rel_offset.data(), &p.count[k0],
                                  box_min_out + 3 * k0, box_max_out + 3 * k0));
  }
  return SWZ_OK;
}

int swz_merge_shard_node_tables(int num_shards, const uint64_t* num_nodes, const int8_t* const* node_level,
                                const uint64_t* const* node_key, const uint64_t* const* node_count, uint64_t max_nodes,
                                int8_t* level_out, uint64_t* key_out, uint64_t* count_out, int32_t* shard_out,
                                uint64_t* num_nodes_out) {
  if (num_shards < 1 || !num_nodes || !node_level || !node_key || !node_count || !num_nodes_out) return SWZ_ERR_BAD_ARG;
  struct Entry {
    int8_t level;
    uint64_t key, count;
    int32_t shard;
  };
  std::vector<Entry> all;
  bool have_root = false;
  Entry root{-1, 0, 0, -1};
  for (int s = 0; s < num_shards; ++s) {
    if (num_nodes[s] && (!node_level[s] || !node_key[s] || !node_count[s])) return SWZ_ERR_BAD_ARG;
    for (uint64_t k = 0; k < num_nodes[s]; ++k) {
      if (node_level[s][k] < 0) {  // a part of the root's file
        have_root = true;
        root.count += node_count[s][k];
      } else {
        all.push_back(Entry{node_level[s][k], node_key[s][k], node_count[s][k], s});
      }
    }
  }
  // (level, node key): the order of swz_tiler_node_table, re-rooted subtrees included -- see the header
  std::stable_sort(all.begin(), all.end(), [](const Entry& a, const Entry& b) { return a.level != b.level ? a.level < b.level : a.key < b.key; });
  const uint64_t nn = all.size() + (have_root ? 1 : 0);
  *num_nodes_out = nn;
  for (size_t k = 1; k < all.size(); ++k)
    if (all[k].level == all[k - 1].level && all[k].key == all[k - 1].key) return SWZ_ERR_INTERNAL;  // a node below the root lives on one shard
  if (!level_out && !key_out && !count_out && !shard_out) return SWZ_OK;
  if (nn > max_nodes || !level_out || !key_out || !count_out) return SWZ_ERR_BAD_ARG;
  uint64_t at = 0;
  auto put = [&](const Entry& e) {
    level_out[at] = e.level;
    key_out[at] = e.key;
    count_out[at] = e.count;
    if (shard_out) shard_out[at] = e.shard;
    ++at;
  };
  if (have_root) put(root);
  for (const Entry& e : all) put(e);
  return SWZ_OK;
}
}  // extern "C"
