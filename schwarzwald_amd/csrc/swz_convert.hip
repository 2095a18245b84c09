// swz_convert.hip -- a written data set converted to another format in one call (swz_convert_dataset): the reference's
// --converter mode (ConverterProcess::run, core/process/ConverterProcess.cpp).  The source is scanned (swz_dataset.hip), the
// target is planned with the parts of swz_tiler_write_output (swz_toutput.h), and the node table is streamed chunk by chunk:
// reader threads fill one of two page-locked images with the chunk's files (BINZ inflated, LAS as record ranges, .pnts whole),
// the copy stream moves it to the device, the unpack kernel (swz_binunpack.hip; LAS sources: the segment kernel of
// swz_tinput.hip; .pnts sources, which SWZ_CONVERT_LOSSY_SOURCE admits: swz_pntsunpack.hip) makes chunk-local positions and columns of it, and output_stream packs, copies back and writes them in the target format.
// The readers of chunk k + 1 run while chunk k is packed and written.
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

constexpr uint64_t CONVERT_READ_PIECE = 8ull << 20;  // bytes one reader thread takes at a time

static double ms_since(std::chrono::steady_clock::time_point t0) {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

__global__ __launch_bounds__(256) void iota_kernel(uint32_t* out, uint32_t n) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i < n) out[i] = i;
}

// the raw image of one chunk: the files of its nodes back to back, each at a multiple of 8, then the kernel's segment table
struct ConvertChunk {
  uint64_t rows = 0, raw_bytes = 0, table_at = 0, image_bytes = 0;
  InputBatch las;                  // LAS sources: segments and pieces as swz_tiler_add_las_files cuts them
  std::vector<BinUnpackSeg> segs;  // BIN, BINZ
  std::vector<ReadPiece> pieces;   // BIN: parts of files; BINZ: whole files (bytes: what the stream inflates to); 3DTILES: whole files
  std::vector<uint64_t> piece_row; // 3DTILES: the first row of a piece's file; its segment is filled by the piece's reader
};

static void build_chunk(const DatasetScan& scan, uint64_t k0, uint64_t k1, ConvertChunk* out) {
  ConvertChunk& ch = *out;
  ch = ConvertChunk{};
  const int format = scan.info.format;
  const bool las = format == SWZ_OUT_LAS || format == SWZ_OUT_ENTWINE_LAS;
  const bool pnts = format == SWZ_OUT_3DTILES;
  uint64_t at = 0;
  for (uint64_t k = k0; k < k1; ++k) {
    const uint64_t cnt = scan.count[k];
    if (!cnt) continue;
    uint64_t bytes;
    if (pnts) {
      bytes = scan.file_bytes[k];
      ch.pieces.push_back({k, 0, bytes, at});
      ch.piece_row.push_back(ch.rows);
    } else if (las) {
      bytes = cnt * scan.layout[k].record_bytes;
      swz_las_segment sg{};
      sg.first_row = ch.rows;
      sg.count = cnt;
      sg.byte_offset = at;
      sg.layout = scan.layout[k];
      ch.las.segs.push_back(sg);
      for (uint64_t done = 0; done < bytes; done += CONVERT_READ_PIECE)
        ch.las.pieces.push_back({k, scan.data_at[k] + done, std::min(CONVERT_READ_PIECE, bytes - done), at + done});
    } else {
      bytes = bin_image_bytes(cnt, scan.info.attribute_mask);
      ch.segs.push_back(bin_unpack_seg(at, ch.rows, cnt, scan.info.attribute_mask));
      if (format == SWZ_OUT_BINZ) {
        ch.pieces.push_back({k, 0, bytes, at});
      } else {
        for (uint64_t done = 0; done < bytes; done += CONVERT_READ_PIECE)
          ch.pieces.push_back({k, done, std::min(CONVERT_READ_PIECE, bytes - done), at + done});
      }
    }
    at = (at + bytes + 7) & ~7ull;
    ch.rows += cnt;
  }
  ch.raw_bytes = at;
  ch.table_at = (at + 15) & ~15ull;
  ch.image_bytes = ch.table_at + (las    ? ch.las.segs.size() * sizeof(swz_las_segment)
                                  : pnts ? ch.pieces.size() * sizeof(swz_pnts_segment)
                                         : ch.segs.size() * sizeof(BinUnpackSeg));
  ch.las.points = ch.rows;
  ch.las.raw_bytes = ch.raw_bytes;
  ch.las.table_at = ch.table_at;
  ch.las.image_bytes = ch.image_bytes;
}

// one .binz file inflated to exactly `bytes` bytes at dst
static bool inflate_file(const std::string& path, unsigned char* dst, uint64_t bytes) {
  std::vector<unsigned char> z;
  if (read_whole_file(nullptr, path.c_str(), &z) != SWZ_OK) return false;
  z_stream zs;
  memset(&zs, 0, sizeof(zs));
  if (inflateInit(&zs) != Z_OK) return false;
  uint64_t in_at = 0, out_at = 0;
  unsigned char spare;
  bool ok = false;
  for (;;) {  // (uInt counters: a gigabyte at a time)
    if (!zs.avail_in && in_at < z.size()) {
      zs.next_in = z.data() + in_at;
      zs.avail_in = (uInt)std::min<uint64_t>(z.size() - in_at, 1u << 30);
      in_at += zs.avail_in;
    }
    if (!zs.avail_out) {
      if (out_at < bytes) {
        zs.next_out = dst + out_at;
        zs.avail_out = (uInt)std::min<uint64_t>(bytes - out_at, 1u << 30);
        out_at += zs.avail_out;
      } else {  // room for one byte too many: only the end of the stream may follow
        zs.next_out = &spare;
        zs.avail_out = 1;
        out_at = bytes + 1;
      }
    }
    const int rc = inflate(&zs, Z_NO_FLUSH);
    if (rc == Z_STREAM_END) {
      ok = out_at - zs.avail_out == bytes;
      break;
    }
    if (rc != Z_OK) break;                       // corrupt, or cut short (Z_BUF_ERROR: no input is left)
    if (out_at > bytes && !zs.avail_out) break;  // more than the header promises
  }
  inflateEnd(&zs);
  return ok;
}

// the reader threads of a BIN / BINZ chunk: every piece into the image, the 12-byte headers checked against the scan
static void start_read(TicketRun& run, swz_ctx* c, const char* who, const DatasetScan* scan, const ConvertChunk* ch, unsigned char* image,
                       long threads) {
  memcpy(image + ch->table_at, ch->segs.data(), ch->segs.size() * sizeof(BinUnpackSeg));
  run.start(c, ch->pieces.size(), [who, scan, ch, image](uint64_t i, std::string* err) {
    const ReadPiece& p = ch->pieces[i];
    const std::string& path = scan->path[p.file];
    if (scan->info.format == SWZ_OUT_BINZ) {
      if (!inflate_file(path, image + p.image_at, p.bytes)) {
        *err = std::string(who) + ": cannot read " + path + ", or its zlib stream does not hold what its header says";
        return (int)SWZ_ERR_BAD_ARG;
      }
    } else {
      Fd f;
      f.fd = open(path.c_str(), O_RDONLY | O_CLOEXEC);
      if (f.fd < 0 || !pread_all(f.fd, image + p.image_at, p.bytes, p.file_at)) {
        *err = std::string(who) + ": cannot read the arrays of " + path + " (shorter than its header says?)";
        return (int)SWZ_ERR_BAD_ARG;
      }
    }
    if (p.file_at == 0) {
      uint32_t mask;
      uint64_t count;
      memcpy(&mask, image + p.image_at, 4);
      memcpy(&count, image + p.image_at + 4, 8);
      if (mask != scan->info.attribute_mask || count != scan->count[p.file]) {
        *err = std::string(who) + ": the header of " + path + " is not the one that was scanned";
        return (int)SWZ_ERR_BAD_ARG;
      }
    }
    return (int)SWZ_OK;
  }, threads);
}

// the reader threads of a 3DTILES chunk: every file whole into the image, parsed there and checked against the scan; piece i
// fills segment i of the table behind the files
static void start_read_pnts(TicketRun& run, swz_ctx* c, const char* who, const DatasetScan* scan, const ConvertChunk* ch,
                            unsigned char* image, long threads) {
  run.start(c, ch->pieces.size(), [who, scan, ch, image](uint64_t i, std::string* err) {
    const ReadPiece& p = ch->pieces[i];
    const std::string& path = scan->path[p.file];
    Fd f;
    f.fd = open(path.c_str(), O_RDONLY | O_CLOEXEC);
    struct stat sb;
    if (f.fd < 0 || fstat(f.fd, &sb) != 0 || (uint64_t)sb.st_size != p.bytes || !pread_all(f.fd, image + p.image_at, p.bytes, 0)) {
      *err = std::string(who) + ": cannot read " + path + ", or it is not the file that was scanned";
      return (int)SWZ_ERR_BAD_ARG;
    }
    PntsImage pi;
    std::string why;
    if (pnts_parse_image(image + p.image_at, p.bytes, &pi, &why) != SWZ_OK) {
      *err = std::string(who) + ": " + why + " in " + path;
      return (int)SWZ_ERR_BAD_ARG;
    }
    if (pi.mask != scan->info.attribute_mask || pi.count != scan->count[p.file]) {
      *err = std::string(who) + ": the header of " + path + " is not the one that was scanned";
      return (int)SWZ_ERR_BAD_ARG;
    }
    swz_pnts_segment sg{};
    sg.first_row = ch->piece_row[i];
    sg.count = pi.count;
    sg.position_offset = p.image_at + pi.position;
    sg.rgb_offset = p.image_at + pi.rgb;
    sg.intensity_offset = p.image_at + pi.intensity;
    sg.mask = pi.mask;
    memcpy(image + ch->table_at + i * sizeof(swz_pnts_segment), &sg, sizeof(sg));
    return (int)SWZ_OK;
  }, threads);
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
  SWZ_TRY(dataset_scan(c, who, src_dir, params->max_depth, &scan));
  const int src_format = scan.info.format;
  const bool pnts = src_format == SWZ_OUT_3DTILES;
  if (pnts && !(params->source_flags & SWZ_CONVERT_LOSSY_SOURCE))
    return refuse("a 3DTILES source is converted only with SWZ_CONVERT_LOSSY_SOURCE in source_flags: .pnts files hold float positions and no attribute beyond RGB and intensity");
  if (pnts) {
    // one frame for all files: a data set of swz_convert_dataset_world keeps every node relative to an origin of its own
    bool have = false;
    double rtc[3] = {0, 0, 0};
    scan.file_bytes.assign(scan.path.size(), 0);
    for (size_t k = 0; k < scan.path.size(); ++k) {
      PntsImage pi;
      std::string why;
      const int st = pnts_read_head(scan.path[k].c_str(), &pi, &why);
      if (st != SWZ_OK) return c->fail(st, std::string(who) + ": " + why);
      if (have && memcmp(rtc, pi.rtc, sizeof(rtc)) != 0)
        return refuse("the RTC_CENTER differs from the files before it (the positions of a data set of swz_convert_dataset_world are relative to an origin per node): " + scan.path[k]);
      have = true;
      memcpy(rtc, pi.rtc, sizeof(rtc));
      scan.file_bytes[k] = pi.file_bytes;
    }
  }
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
  uint64_t out_image_max = 0, in_image_max = 0, rows_max = 0;
  output_cuts(c, p, 0, nn, op.chunk_points, &first, &out_image_max);
  const uint64_t num_chunks = first.empty() ? 0 : first.size() - 1;
  ConvertChunk ch[2];
  for (uint64_t j = 0; j < num_chunks; ++j) {
    uint64_t at = 0;
    for (uint64_t k = first[j]; k < first[j + 1]; ++k) {
      p.offset[k] = at;
      at += p.count[k];
    }
    build_chunk(scan, first[j], first[j + 1], &ch[0]);
    in_image_max = std::max(in_image_max, ch[0].image_bytes);
    rows_max = std::max(rows_max, ch[0].rows);
  }

  OutputStreamStats ss;
  uint64_t bytes_read = 0;
  double read_ms = 0, unpack_ms = 0, in_copy_ms = 0;
  int status = SWZ_OK;
  if (out_image_max && rows_max) {
    const bool las = src_format == SWZ_OUT_LAS || src_format == SWZ_OUT_ENTWINE_LAS;
    const long threads =
      std::max(1L, c->opt_int("SWZ_INPUT_READER_THREADS", (long)std::min(32u, std::max(1u, std::thread::hardware_concurrency()))));
    std::vector<const char*> paths(nn);
    for (uint64_t k = 0; k < nn; ++k) paths[k] = scan.path[k].c_str();
    // the chunk-local arrays ("out_*": the call's part of the workspace), the identity ids, the images of both directions
    OutputWorkspace ow{c};
    OutputSource src;
    uint32_t* d_ids = nullptr;
    double* d_xyz = nullptr;
    SWZ_TRY(c->get("out_cv_ids", (size_t)rows_max, &d_ids));
    SWZ_TRY(c->get("out_cv_xyz", (size_t)rows_max * 3, &d_xyz));
    for (int a = 0; a < SWZ_ATTR_COUNT; ++a) {
      if (!((op.attribute_mask >> a) & 1u)) continue;
      const std::string name = "out_cv_col" + std::to_string(a);
      SWZ_TRY(c->get(name.c_str(), (size_t)rows_max * ATTR_BYTES[a], &src.in.column[a]));
    }
    src.ids = d_ids;
    src.xyz = d_xyz;
    src.world_xyz = d_xyz;
    hipLaunchKernelGGL(iota_kernel, dim3(div_up(rows_max, 256)), dim3(256), 0, c->stream, d_ids, (uint32_t)rows_max);
    SWZ_LAUNCH_CHECK(c);
    SWZ_HIP(c, hipStreamSynchronize(c->stream));
    TicketRun readers;
    InputBuffers ib;
    OutputImages images;
    struct JoinFirst {  // the readers write into ib's host images: they end before those are freed
      TicketRun& r;
      ~JoinFirst() { (void)r.wait(nullptr, nullptr); }
    } join_first{readers};
    SWZ_TRY(ib.reserve(c, in_image_max, num_chunks > 1));
    SWZ_TRY(images.reserve(c, out_image_max, num_chunks > 1));

    auto read_chunk = [&](uint64_t j) {
      ConvertChunk& cc = ch[j & 1];
      build_chunk(scan, first[j], first[j + 1], &cc);
      unsigned char* image = static_cast<unsigned char*>(ib.host[ib.host[1] ? (j & 1) : 0]);
      if (las) las_start_read(readers, c, who, &cc.las, image, paths.data(), threads);
      else if (pnts) start_read_pnts(readers, c, who, &scan, &cc, image, threads);
      else start_read(readers, c, who, &scan, &cc, image, threads);
    };
    // chunk j: its image is read -> to the device -> unpacked into the chunk-local arrays; then the readers go on with
    // chunk j + 1 while output_stream packs and writes chunk j
    const OutputChunkFeed feed = [&](uint64_t j, OutputSource*) -> int {
      const int b = ib.host[1] ? (int)(j & 1) : 0;
      const ConvertChunk& cc = ch[j & 1];
      double ms = 0;
      std::string err;
      const int st = readers.wait(&err, &ms);
      read_ms += ms;
      if (st != SWZ_OK) return c->fail(st, err);
      bytes_read += cc.raw_bytes;
      SWZ_HIP(c, hipEventRecord(ib.begin[b], images.copy));
      if (cc.image_bytes) SWZ_HIP(c, hipMemcpyAsync(ib.device[b], ib.host[b], cc.image_bytes, hipMemcpyHostToDevice, images.copy));
      SWZ_HIP(c, hipEventRecord(ib.copied[b], images.copy));
      if (las) {
        SWZ_TRY(las_launch_image(c, images.copy, ib.device[b], cc.las, nullptr, d_xyz, &src.in, op.attribute_mask, nullptr));
      } else if (pnts) {
        SWZ_TRY(pnts_unpack_launch(c, images.copy, ib.device[b], cc.raw_bytes, reinterpret_cast<const swz_pnts_segment*>(ib.device[b] + cc.table_at),
                                   (uint32_t)cc.pieces.size(), (uint32_t)cc.rows, d_xyz, &src.in));
      } else {
        SWZ_TRY(bin_unpack_launch(c, images.copy, ib.device[b], cc.raw_bytes, reinterpret_cast<const BinUnpackSeg*>(ib.device[b] + cc.table_at),
                                  (uint32_t)cc.segs.size(), (uint32_t)cc.rows, d_xyz, &src.in));
      }
      SWZ_HIP(c, hipEventRecord(ib.decoded[b], images.copy));
      SWZ_HIP(c, hipEventSynchronize(ib.decoded[b]));
      float t = 0.f;
      if (hipEventElapsedTime(&t, ib.begin[b], ib.copied[b]) == hipSuccess) in_copy_ms += t;
      if (hipEventElapsedTime(&t, ib.copied[b], ib.decoded[b]) == hipSuccess) unpack_ms += t;
      if (j + 1 < num_chunks) read_chunk(j + 1);  // (its host image: chunk j - 1's, whose copy has ended)
      return SWZ_OK;
    };
    read_chunk(0);
    status = output_stream(c, p, first, src, images, 0, &ss, &feed);
    (void)readers.wait(nullptr, nullptr);
  }

  // ---- the metadata, and properties.json for whoever converts the result again
  uint64_t points = 0;
  for (uint64_t k = 0; k < nn; ++k) points += p.count[k];
  if (status == SWZ_OK) status = output_metadata(c, who, p, dst_dir, &op);
  if (status == SWZ_OK) status = swz_properties_json_write(c, dst_dir, bmin, bmax, spacing, points);
  if (stats) {
    stats->nodes = nn;
    stats->points = points;
    stats->bytes_read = bytes_read;
    stats->bytes_written = ss.bytes_written;
    stats->chunks = ss.chunks;
    stats->read_ms = read_ms;
    stats->unpack_ms = unpack_ms;
    stats->pack_ms = ss.pack_ms;
    stats->copy_ms = in_copy_ms + ss.copy_ms;
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
