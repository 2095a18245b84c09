// swz_toutput.hip -- the node files of a tiler written in one call (swz_tiler_write_output): the node table is cut into
// chunks of whole nodes, and while the writer threads write the files of chunk k out of one page-locked host buffer, chunk
// k + 1 is packed on the device (swz_bin_pack_device, swz_pnts_pack_device, swz_las_pack_device, straight from the pools) and
// copied into the other one.  File names, node boxes, LAS offsets and scales are what TilingAlgorithmGPU::finalize and the
// sinks of host/swz_tiling.hpp compute from the node table.
#include <sys/stat.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <string>
#include <vector>

#include "swz_tiler.h"
#include "swz_hostio.h"

namespace swz {

constexpr uint64_t OUTPUT_CHUNK_POINTS = 16ull << 20;  // TilingAlgorithmGPU's export chunk

static double ms_since(std::chrono::steady_clock::time_point t0) {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// what a call holds besides the context's workspace; released however the call ends
struct OutputBuffers {
  void* host[2] = {nullptr, nullptr};
  hipStream_t copy = nullptr;
  hipEvent_t begin[2] = {nullptr, nullptr}, end[2] = {nullptr, nullptr};
  ~OutputBuffers() {
    for (int b = 0; b < 2; ++b) {
      if (host[b]) (void)hipHostFree(host[b]);
      if (begin[b]) (void)hipEventDestroy(begin[b]);
      if (end[b]) (void)hipEventDestroy(end[b]);
    }
    if (copy) (void)hipStreamDestroy(copy);
  }
};

// the call's part of the workspace goes back when it ends: two chunk images are the call's, not the data set's
struct OutputWorkspace {
  swz_ctx* c;
  ~OutputWorkspace() {
    for (const char* name : {"out_ids", "out_image0", "out_image1"}) {
      const auto it = c->bufs.find(name);
      if (it == c->bufs.end()) continue;
      c->free_buf(it->second);
      c->bufs.erase(it);
    }
  }
};

// the table of one output format: sizes of the bodies, the pack call and the file of a node
struct OutputPlan {
  int format = 0;
  uint32_t mask = 0;        // as the format's pack call takes it
  int rgb_mapping = SWZ_PNTS_RGB_FROM_COLOR;
  double rtc[3] = {0, 0, 0};
  std::string data_dir;     // where the node files go
  std::vector<int8_t> level;
  std::vector<uint64_t> key, offset, count;
  std::vector<uint64_t> body_at, body_size, file_size;  // per node, body_at relative to the image of the whole table
  std::vector<double> box_min, box_max, scale;           // LAS
};

static int plan_layout(swz_ctx* c, OutputPlan& p) {
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
  if (st != SWZ_OK) return c->fail(SWZ_ERR_BAD_ARG, "swz_tiler_write_output: a node is too large for a file of this format");
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
      st = swz_pnts_write_node(nullptr, path.c_str(), p.count[k], body, p.body_size[k], p.mask, p.rtc);
      break;
    default:
      path = stem + ".las";
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
  if (!dir || !params) return c->fail(SWZ_ERR_BAD_ARG, "swz_tiler_write_output: NULL argument");
  const auto t_wall = std::chrono::steady_clock::now();
  SWZ_HIP(c, hipSetDevice(c->device));
  if (stats) *stats = swz_output_stats{};

  // ---- the node table (a poisoned tiler answers here), then everything that is refused before anything is written
  swz_tiler_info info{};
  SWZ_TRY(swz_tiler_get_info(t, &info));
  OutputPlan p;
  const uint64_t cap_nodes = std::max<uint64_t>(info.num_nodes, 1);
  p.level.resize(cap_nodes);
  p.key.resize(cap_nodes);
  p.offset.resize(cap_nodes);
  p.count.resize(cap_nodes);
  uint64_t nn = 0;
  SWZ_TRY(swz_tiler_node_table(t, cap_nodes, p.level.data(), p.key.data(), p.offset.data(), p.count.data(), &nn));
  p.level.resize(nn);
  p.key.resize(nn);
  p.offset.resize(nn);
  p.count.resize(nn);
  if (!t->staged_sizes.empty() || t->batch_open)
    return c->fail(SWZ_ERR_BAD_ARG, "swz_tiler_write_output: a batch is staged or open");
  if (params->format < SWZ_OUT_BIN || params->format > SWZ_OUT_ENTWINE_LAS)
    return c->fail(SWZ_ERR_BAD_ARG, "swz_tiler_write_output: unknown format");
  if (params->attribute_mask & ~t->attr_mask)
    return c->fail(SWZ_ERR_BAD_ARG, "swz_tiler_write_output: the mask names a column the batches did not carry");
  p.format = params->format;
  p.mask = params->attribute_mask;
  p.data_dir = dir;
  if (p.format == SWZ_OUT_3DTILES) {
    const int m = params->rgb_mapping;
    if (m != SWZ_PNTS_RGB_FROM_COLOR && m != SWZ_PNTS_RGB_FROM_INTENSITY_LINEAR && m != SWZ_PNTS_RGB_FROM_INTENSITY_LOG)
      return c->fail(SWZ_ERR_BAD_ARG, "swz_tiler_write_output: unknown rgb_mapping");
    const bool mapped = m != SWZ_PNTS_RGB_FROM_COLOR, has_intensity = (params->attribute_mask & SWZ_PNTS_INTENSITY) != 0;
    if (mapped && !has_intensity) return c->fail(SWZ_ERR_BAD_ARG, "swz_tiler_write_output: an rgb_mapping needs the intensities in the mask");
    if (!finite3(params->global_offset)) return c->fail(SWZ_ERR_BAD_ARG, "swz_tiler_write_output: global_offset is not finite");
    // (Cesium3DTilesSink::persist_rows: RGB and INTENSITY of what the rows carry, with a mapping RGB out of the intensity)
    p.mask = has_intensity ? SWZ_PNTS_INTENSITY : 0u;
    if (mapped ? has_intensity : (params->attribute_mask & SWZ_PNTS_RGB) != 0) p.mask |= SWZ_PNTS_RGB;
    p.rgb_mapping = m;
    for (int a = 0; a < 3; ++a) p.rtc[a] = params->global_offset[a];
  }
  SWZ_TRY(plan_layout(c, p));
  if (p.format == SWZ_OUT_LAS || p.format == SWZ_OUT_ENTWINE_LAS) {
    p.box_min.resize(3 * nn);
    p.box_max.resize(3 * nn);
    p.scale.resize(nn);
    for (uint64_t k = 0; k < nn; ++k) {
      if (swz_node_bounds(p.level[k], p.key[k], t->bmin, t->bmax, &p.box_min[3 * k], &p.box_max[3 * k]) != SWZ_OK)
        return c->fail(SWZ_ERR_INTERNAL, "swz_tiler_write_output: bad node level");
      p.scale[k] = swz_las_scale_from_bounds(&p.box_min[3 * k], &p.box_max[3 * k]);
    }
  }
  if (p.format == SWZ_OUT_ENTWINE_LAS) {
    if (swz_ept_create_dirs(nullptr, dir) != SWZ_OK)
      return c->fail(SWZ_ERR_BAD_ARG, std::string("swz_tiler_write_output: cannot create the ept directories under ") + dir);
    p.data_dir = std::string(dir) + "/ept-data";
  } else if (make_dir(dir) != 0) {
    return c->fail(SWZ_ERR_BAD_ARG, std::string("swz_tiler_write_output: cannot create ") + dir);
  }

  // ---- the chunks, and the largest chunk image
  uint64_t chunk_points = params->chunk_points;
  if (!chunk_points) chunk_points = (uint64_t)std::max(1L, c->opt_int("SWZ_OUTPUT_CHUNK_POINTS", (long)OUTPUT_CHUNK_POINTS));
  uint64_t num_chunks = 0;
  (void)swz_output_chunks(nn, p.count.data(), chunk_points, 0, nullptr, &num_chunks);
  std::vector<uint64_t> first(num_chunks + 1, 0);
  (void)swz_output_chunks(nn, p.count.data(), chunk_points, num_chunks, first.data(), &num_chunks);
  auto image_at = [&](uint64_t node) { return node < nn ? p.body_at[node] : (nn ? p.body_at[nn - 1] + p.body_size[nn - 1] : 0); };
  uint64_t image_max = 0, bytes_written = 0;
  for (uint64_t j = 0; j < num_chunks; ++j) image_max = std::max(image_max, image_at(first[j + 1]) - image_at(first[j]));

  const uint64_t ns = info.num_stored;
  double pack_ms = 0, copy_ms = 0, write_ms = 0;
  uint64_t chunks_done = 0;
  int status = SWZ_OK;
  std::string why;
  if (image_max) {
    uint32_t* d_ids = nullptr;
    uint8_t* d_image[2] = {nullptr, nullptr};
    OutputWorkspace ow{c};
    SWZ_TRY(c->get("out_ids", (size_t)ns, &d_ids));
    SWZ_TRY(c->get("out_image0", (size_t)image_max, &d_image[0]));
    if (num_chunks > 1) SWZ_TRY(c->get("out_image1", (size_t)image_max, &d_image[1]));
    SWZ_TRY(swz_tiler_export_device(t, nullptr, d_ids, nullptr));
    OutputBuffers ob;
    SWZ_HIP(c, hipStreamCreateWithFlags(&ob.copy, hipStreamNonBlocking));
    for (int b = 0; b < (num_chunks > 1 ? 2 : 1); ++b) {
      SWZ_HIP(c, hipHostMalloc(&ob.host[b], image_max, hipHostMallocDefault));
      SWZ_HIP(c, hipEventCreate(&ob.begin[b]));
      SWZ_HIP(c, hipEventCreate(&ob.end[b]));
    }
    swz_attribute_columns d_in{};
    for (int a = 0; a < SWZ_ATTR_COUNT; ++a) d_in.column[a] = (t->attr_mask & (1u << a)) ? t->pool_attr[a] : nullptr;

    TicketRun writers;  // of the chunk before
    auto join_writers = [&]() {
      if (!writers.running()) return;
      double ms = 0;
      std::string err;
      const int st = writers.wait(&err, &ms);
      write_ms += ms;
      if (st != SWZ_OK && status == SWZ_OK) {
        status = st;
        why = err;
      }
    };
    std::vector<uint64_t> rel_offset;
    for (uint64_t j = 0; j < num_chunks && status == SWZ_OK; ++j) {
      const int b = (int)(j & 1);
      const uint64_t k0 = first[j], k1 = first[j + 1];
      const uint64_t at0 = image_at(k0), bytes = image_at(k1) - at0;
      const uint64_t row0 = p.offset[k0];
      const uint64_t rows = p.offset[k1 - 1] + p.count[k1 - 1] - row0;
      // buffer b, device and host: chunk j - 2 has been copied out of the one and written out of the other
      if (bytes) {
        rel_offset.resize(k1 - k0);
        for (uint64_t k = k0; k < k1; ++k) rel_offset[k - k0] = p.offset[k] - row0;
        const auto t_pack = std::chrono::steady_clock::now();
        int st = SWZ_OK;
        switch (p.format) {
          case SWZ_OUT_BIN:
          case SWZ_OUT_BINZ:
            st = swz_bin_pack_device(c, d_ids + row0, nullptr, rows, t->pool_xyz, &d_in, k1 - k0, rel_offset.data(), &p.count[k0], p.mask,
                                     d_image[b], bytes);
            break;
          case SWZ_OUT_3DTILES:
            st = swz_pnts_pack_device(c, d_ids + row0, nullptr, rows, t->pool_xyz, &d_in, k1 - k0, rel_offset.data(), &p.count[k0], p.mask,
                                      p.rgb_mapping, d_image[b], bytes);
            break;
          default:
            st = swz_las_pack_device(c, d_ids + row0, nullptr, rows, t->pool_xyz, &d_in, k1 - k0, rel_offset.data(), &p.count[k0],
                                     &p.box_min[3 * k0], &p.scale[k0], p.mask, d_image[b], bytes);
            break;
        }
        pack_ms += ms_since(t_pack);
        hipError_t e = hipSuccess;
        if (st == SWZ_OK) e = hipEventRecord(ob.begin[b], ob.copy);
        if (st == SWZ_OK && e == hipSuccess) e = hipMemcpyAsync(ob.host[b], d_image[b], bytes, hipMemcpyDeviceToHost, ob.copy);
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
        if (hipEventElapsedTime(&ms, ob.begin[b], ob.end[b]) == hipSuccess) copy_ms += ms;
        if (status != SWZ_OK) break;  // a file of the chunk before could not be written
        const unsigned char* image = static_cast<const unsigned char*>(ob.host[b]);
        const OutputPlan* plan = &p;
        writers.start(c, k1 - k0, [plan, k0, image, at0](uint64_t i, std::string* err) { return write_node_file(*plan, k0 + i, image, at0, err); });
        bytes_written += bytes;
      }
      ++chunks_done;
    }
    join_writers();
    (void)hipStreamSynchronize(ob.copy);
  }

  // ---- the metadata
  if (status == SWZ_OK && p.format == SWZ_OUT_3DTILES && nn) {
    uint64_t num = 0;
    std::vector<swz_tileset_node> tiles;
    int st = swz_tileset_build(nn, p.level.data(), p.key.data(), t->bmin, t->bmax, t->p.spacing_at_root, p.rtc, 0, nullptr, &num);
    if (st == SWZ_OK) {
      tiles.resize(num);
      st = swz_tileset_build(nn, p.level.data(), p.key.data(), t->bmin, t->bmax, t->p.spacing_at_root, p.rtc, num, tiles.data(), &num);
    }
    if (st != SWZ_OK) {
      status = st;
      why = "swz_tiler_write_output: swz_tileset_build failed";
    } else if ((st = swz_tileset_write(c, tiles.data(), num, dir)) != SWZ_OK) {
      status = st;
      why = c->err;
    }
  }
  if (status == SWZ_OK && p.format == SWZ_OUT_ENTWINE_LAS) {
    int st = swz_ept_hierarchy_write(c, dir, nn, p.level.data(), p.key.data(), p.count.data());
    if (st == SWZ_OK && params->ept) st = swz_ept_json_write(c, (std::string(dir) + "/ept.json").c_str(), params->ept);
    if (st != SWZ_OK) {
      status = st;
      why = c->err;
    }
  }
  if (stats) {
    stats->nodes = nn;
    stats->stored_points = ns;
    stats->bytes_written = bytes_written;
    stats->chunks = chunks_done;
    stats->pack_ms = pack_ms;
    stats->copy_ms = copy_ms;
    stats->write_ms = write_ms;
    stats->wall_ms = ms_since(t_wall);
  }
  return status == SWZ_OK ? SWZ_OK : c->fail(status, why);
}

}  // extern "C"
