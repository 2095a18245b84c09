// swz_source.hip -- the source half of every reader of a written data set (swz_convert.h): a scanned data set opened with
// the refusals of a 3DTILES source (source_open) and streamed chunk by chunk onto the device (SourceStream).  Reader threads
// fill one of two page-locked images with the chunk's files (BINZ inflated, LAS as record ranges, .pnts whole), the copy
// stream moves it to the device, and the unpack kernel (swz_binunpack.hip; LAS sources: the segment kernel of
// swz_tinput.hip; .pnts sources: swz_pntsunpack.hip) makes chunk-local positions and columns of it.  The readers of chunk
// k + 1 run while the caller works on chunk k.  SourceLoop::each_chunk is the loop around it -- cuts, workspace, copy
// stream, plan, start, next, stats -- for the callers that only have something to do per chunk: swz_dataset_query*,
// swz_dataset_summarize and swz_dataset_rasterize.  swz_convert_dataset calls next() from output_stream's feed instead.
#include <sys/stat.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "swz_convert.h"
#include "swz_hostio.h"
#include "swz_tinput.h"
#include "swz_toutput.h"

namespace swz {

constexpr uint64_t SOURCE_READ_PIECE = 8ull << 20;  // bytes one reader thread takes at a time

static void build_chunk(const DatasetScan& scan, uint64_t k0, uint64_t k1, SourceChunk* out) {
  SourceChunk& ch = *out;
  ch = SourceChunk{};
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
      for (uint64_t done = 0; done < bytes; done += SOURCE_READ_PIECE)
        ch.las.pieces.push_back({k, scan.data_at[k] + done, std::min(SOURCE_READ_PIECE, bytes - done), at + done});
    } else {
      bytes = bin_image_bytes(cnt, scan.info.attribute_mask);
      ch.segs.push_back(bin_unpack_seg(at, ch.rows, cnt, scan.info.attribute_mask));
      if (format == SWZ_OUT_BINZ) {
        ch.pieces.push_back({k, 0, bytes, at});
      } else {
        for (uint64_t done = 0; done < bytes; done += SOURCE_READ_PIECE)
          ch.pieces.push_back({k, done, std::min(SOURCE_READ_PIECE, bytes - done), at + done});
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
static void start_read(TicketRun& run, swz_ctx* c, const char* who, const DatasetScan* scan, const SourceChunk* ch, unsigned char* image,
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
static void start_read_pnts(TicketRun& run, swz_ctx* c, const char* who, const DatasetScan* scan, const SourceChunk* ch,
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

int source_open(swz_ctx* c, const char* who, const char* dir, int32_t max_depth, uint32_t source_flags, DatasetScan* scan_out,
                double rtc_out[3]) {
  auto refuse = [&](const std::string& what) { return c->fail(SWZ_ERR_BAD_ARG, std::string(who) + ": " + what); };
  DatasetScan& scan = *scan_out;
  SWZ_TRY(dataset_scan(c, who, dir, max_depth, &scan));
  double rtc[3] = {0, 0, 0};
  if (scan.info.format == SWZ_OUT_3DTILES) {
    if (!(source_flags & SWZ_CONVERT_LOSSY_SOURCE))
      return refuse("a 3DTILES source is converted only with SWZ_CONVERT_LOSSY_SOURCE in source_flags: .pnts files hold float positions and no attribute beyond RGB and intensity");
    // one frame for all files: a data set of swz_convert_dataset_world keeps every node relative to an origin of its own
    bool have = false;
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
  if (rtc_out) memcpy(rtc_out, rtc, sizeof(rtc));
  return SWZ_OK;
}

void SourceStream::plan(swz_ctx* ctx, const char* who_c, const DatasetScan* s, const std::vector<uint64_t>* first_nodes,
                        uint32_t attribute_mask) {
  c = ctx;
  who = who_c;
  scan = s;
  first = first_nodes;
  mask = attribute_mask;
  num_chunks = first->empty() ? 0 : first->size() - 1;
  image_max = rows_max = 0;
  for (uint64_t j = 0; j < num_chunks; ++j) {
    build_chunk(*scan, (*first)[j], (*first)[j + 1], &ch_[0]);
    image_max = std::max(image_max, ch_[0].image_bytes);
    rows_max = std::max(rows_max, ch_[0].rows);
  }
}

int SourceStream::start(hipStream_t copy_stream) {
  copy = copy_stream;
  threads_ = std::max(1L, c->opt_int("SWZ_INPUT_READER_THREADS", (long)std::min(32u, std::max(1u, std::thread::hardware_concurrency()))));
  paths_.resize(scan->path.size());
  for (size_t k = 0; k < paths_.size(); ++k) paths_[k] = scan->path[k].c_str();
  SWZ_TRY(c->get("out_cv_xyz", (size_t)rows_max * 3, &xyz));
  for (int a = 0; a < SWZ_ATTR_COUNT; ++a) {
    if (!((mask >> a) & 1u)) continue;
    const std::string name = "out_cv_col" + std::to_string(a);
    SWZ_TRY(c->get(name.c_str(), (size_t)rows_max * ATTR_BYTES[a], &cols.column[a]));
  }
  SWZ_TRY(ib_.reserve(c, image_max, num_chunks > 1));
  read_chunk(0);
  return SWZ_OK;
}

void SourceStream::read_chunk(uint64_t j) {
  const int format = scan->info.format;
  SourceChunk& cc = ch_[j & 1];
  build_chunk(*scan, (*first)[j], (*first)[j + 1], &cc);
  unsigned char* image = static_cast<unsigned char*>(ib_.host[ib_.host[1] ? (j & 1) : 0]);
  if (format == SWZ_OUT_LAS || format == SWZ_OUT_ENTWINE_LAS) las_start_read(readers_, c, who, &cc.las, image, paths_.data(), threads_);
  else if (format == SWZ_OUT_3DTILES) start_read_pnts(readers_, c, who, scan, &cc, image, threads_);
  else start_read(readers_, c, who, scan, &cc, image, threads_);
}

// chunk j: its image is read -> to the device -> unpacked into the chunk-local arrays; then the readers go on with chunk j + 1
int SourceStream::next(uint64_t j) {
  const int format = scan->info.format;
  const int b = ib_.host[1] ? (int)(j & 1) : 0;
  const SourceChunk& cc = ch_[j & 1];
  double ms = 0;
  std::string err;
  const int st = readers_.wait(&err, &ms);
  read_ms += ms;
  if (st != SWZ_OK) return c->fail(st, err);
  bytes_read += cc.raw_bytes;
  SWZ_HIP(c, hipEventRecord(ib_.begin[b], copy));
  if (cc.image_bytes) SWZ_HIP(c, hipMemcpyAsync(ib_.device[b], ib_.host[b], cc.image_bytes, hipMemcpyHostToDevice, copy));
  SWZ_HIP(c, hipEventRecord(ib_.copied[b], copy));
  if (format == SWZ_OUT_LAS || format == SWZ_OUT_ENTWINE_LAS) {
    SWZ_TRY(las_launch_image(c, copy, ib_.device[b], cc.las, nullptr, xyz, &cols, mask, nullptr));
  } else if (format == SWZ_OUT_3DTILES) {
    SWZ_TRY(pnts_unpack_launch(c, copy, ib_.device[b], cc.raw_bytes, reinterpret_cast<const swz_pnts_segment*>(ib_.device[b] + cc.table_at),
                               (uint32_t)cc.pieces.size(), (uint32_t)cc.rows, xyz, &cols));
  } else {
    SWZ_TRY(bin_unpack_launch(c, copy, ib_.device[b], cc.raw_bytes, reinterpret_cast<const BinUnpackSeg*>(ib_.device[b] + cc.table_at),
                              (uint32_t)cc.segs.size(), (uint32_t)cc.rows, xyz, &cols));
  }
  SWZ_HIP(c, hipEventRecord(ib_.decoded[b], copy));
  SWZ_HIP(c, hipEventSynchronize(ib_.decoded[b]));
  float t = 0.f;
  if (hipEventElapsedTime(&t, ib_.begin[b], ib_.copied[b]) == hipSuccess) copy_ms += t;
  if (hipEventElapsedTime(&t, ib_.copied[b], ib_.decoded[b]) == hipSuccess) unpack_ms += t;
  if (j + 1 < num_chunks) read_chunk(j + 1);  // (its host image: chunk j - 1's, whose copy has ended)
  return SWZ_OK;
}

void source_cuts(swz_ctx* c, const uint64_t* counts, uint64_t n, uint64_t chunk_points, std::vector<uint64_t>* first) {
  chunk_points = output_chunk_points(c, chunk_points);
  uint64_t num_chunks = 0;
  (void)swz_output_chunks(n, counts, chunk_points, 0, nullptr, &num_chunks);
  first->assign(num_chunks + 1, 0);
  (void)swz_output_chunks(n, counts, chunk_points, num_chunks, first->data(), &num_chunks);
}

SourceLoop::SourceLoop(swz_ctx* c, const char* who, const DatasetScan& scan, uint32_t mask, uint64_t chunk_points) : ow_{c} {
  source_cuts(c, scan.count.data(), scan.count.size(), chunk_points, &first_);
  source_.plan(c, who, &scan, &first_, mask);
  for (uint64_t j = 0; j < source_.num_chunks; ++j) nodes_max_ = std::max(nodes_max_, first_[j + 1] - first_[j]);
}

int SourceLoop::each_chunk(const SourceChunkBody& body, SourceLoopStats* stats) {
  swz_ctx* c = ow_.c;
  SourceLoopStats st;
  if (source_.rows_max) {
    SWZ_HIP(c, hipStreamCreateWithFlags(&copy_.s, hipStreamNonBlocking));
    SWZ_TRY(source_.start(copy_.s));
    for (uint64_t j = 0; j < source_.num_chunks; ++j) {
      SWZ_TRY(source_.next(j));  // (a read error: the stream stops here, the file is named)
      ++st.chunks;
      const SourceChunkView v{j, first_[j], first_[j + 1], source_.rows(j), source_.xyz, &source_.cols};
      const auto t_body = std::chrono::steady_clock::now();
      SWZ_TRY(body(v));
      st.body_ms += ms_since(t_body);
    }
  }
  st.bytes_read = source_.bytes_read;
  st.read_ms = source_.read_ms;
  st.unpack_ms = source_.unpack_ms;
  st.copy_ms = source_.copy_ms;
  *stats = st;
  return SWZ_OK;
}

}  // namespace swz
