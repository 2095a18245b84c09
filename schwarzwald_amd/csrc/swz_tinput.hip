// swz_tinput.hip -- a data set of uncompressed LAS files read in one call (swz_tiler_add_las_files), the input side of
// swz_toutput.hip: the headers are scanned on the host (swz_las_scan_files: what TilerProcess::prepare and
// calculate_dataset_metadata do, core/process/TilerProcess.cpp:250-390), the concatenated files are cut into batches
// (swz_input_batches), and while batch k is tiled the reader threads pread the raw records of batch k + 1 into a page-locked
// buffer, the tiler's copy stream moves them to the device and ONE kernel decodes them straight into the pool rows of the
// batch (swz_las_decode_segments_device's kernel).  The loop is las_input_stream, which swz_group_add_las_files runs too.
//
// The kernel.  A batch is a run of points of the concatenated files, so its raw image holds SEGMENTS: records of several
// files, each with its own scale, offset, box, point format and record length, one behind the other.  The point data of a
// file starts at byte 227, 235 or 375 plus its VLRs and record lengths with extra bytes are odd, so neither a segment nor a
// record is 4-byte aligned.  One workgroup takes LASIN_TILE consecutive output rows, whatever segments they belong to:
// it finds the segment of its first row with one binary search in the table, puts the first rows of the LASIN_TILE segments
// from there on into LDS (a tile of one-point files spans that many), and every lane finds its own segment there.  The byte
// range the tile's records cover is loaded into LDS as the aligned dwords that cover it, consecutive lanes consecutive
// dwords; a dword that does not lie wholly inside [raw, raw + raw_bytes) is put together from the bytes that do.  The
// records are then unpacked at byte granularity from LDS (las_unpack, swz_lasrec.h).  A tile whose range is longer than the
// stage -- records of more than LASIN_MAX_RECORD bytes, or segments that do not lie back to back -- reads its records
// directly.
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <cerrno>
#include <chrono>
#include <cmath>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "swz_tinput.h"
#include "swz_lasrec.h"

namespace swz {

constexpr uint32_t LASIN_TILE = 256;                             // output rows per workgroup, one per thread
constexpr uint32_t LASIN_MAX_RECORD = 96;                        // a tile of records up to this length is staged
constexpr uint32_t LASIN_STAGE = LASIN_TILE * LASIN_MAX_RECORD;  // bytes of LDS the records pass through
constexpr uint64_t LASIN_MAX_POINTS = 0xFFFFFFFFull - 65535ull;  // the library's limit of points per batch (2^32 - 65536)
constexpr uint64_t INPUT_BATCH_POINTS = 10000000;                // --internal-cache-size, executable/main.cpp:233-236
constexpr uint64_t READ_PIECE = 8ull << 20;                      // bytes one reader thread takes at a time
constexpr uint32_t LAS_MASK_ALWAYS =
  (1u << SWZ_ATTR_INTENSITY) | (1u << SWZ_ATTR_CLASSIFICATION) | (1u << SWZ_ATTR_EDGE_OF_FLIGHT_LINE) |
  (1u << SWZ_ATTR_NUMBER_OF_RETURNS) | (1u << SWZ_ATTR_RETURN_NUMBER) | (1u << SWZ_ATTR_POINT_SOURCE_ID) |
  (1u << SWZ_ATTR_SCAN_DIRECTION_FLAG) | (1u << SWZ_ATTR_SCAN_ANGLE_RANK) | (1u << SWZ_ATTR_USER_DATA);

// ---------------------------------------------------------------------------------- the segment kernel
struct LasSegArgs {
  const uint8_t* raw;
  uint64_t raw_bytes;
  const swz_las_segment* segs;  // the segments that hold points; first_row ascends, every row belongs to exactly one
  uint32_t num_segs;
  uint32_t n;                   // rows
  double* xyz;
  void* col[SWZ_ATTR_COUNT];
  bool shift;
  double center[3];
};

// the kernel's arguments without and with a source projection: the first is LasSegArgs and nothing else
template <bool SRS>
struct LasSegArgsOf : LasSegArgs {};
template <>
struct LasSegArgsOf<true> : LasSegArgs {
  swz_srs srs;
};

// SRS: every position goes through the source projection to ECEF between clamp and shift (las_unpack<true>)
template <bool SRS>
__global__ __launch_bounds__(LASIN_TILE) void las_segments_kernel(LasSegArgsOf<SRS> a) {
  __shared__ uint32_t s_first[LASIN_TILE];  // first rows of the segments k0 .. k0 + LASIN_TILE - 1 (past the table: no row)
  __shared__ unsigned long long s_lo, s_hi;  // the byte range of the tile's records in raw
  __shared__ uint32_t s_stage[LASIN_STAGE / 4 + 2];
  const uint32_t t = threadIdx.x;
  const uint32_t r0 = blockIdx.x * LASIN_TILE;
  const uint32_t r1 = (uint32_t)min((uint64_t)r0 + LASIN_TILE, (uint64_t)a.n);

  // the segment of the tile's first row: the last one that begins at or before it (segment 0 begins at row 0)
  uint32_t k0 = 0;
  for (uint32_t hi = a.num_segs; hi - k0 > 1;) {
    const uint32_t mid = k0 + (hi - k0) / 2;
    if ((uint32_t)a.segs[mid].first_row <= r0) k0 = mid; else hi = mid;
  }
  s_first[t] = (k0 + t < a.num_segs) ? (uint32_t)a.segs[k0 + t].first_row : 0xFFFFFFFFu;
  if (t == 0) {
    s_lo = ~0ull;
    s_hi = 0ull;
  }
  __syncthreads();

  // this lane's row: its segment (every segment holds a point, so the tile's rows lie in the LASIN_TILE segments listed),
  // its record, and the layout it is unpacked with
  const uint32_t r = r0 + t;
  const bool live = r < r1;
  LasArgs la{};
  uint64_t start = 0;
  if (live) {
    uint32_t e = 0;
    for (uint32_t hi = LASIN_TILE; hi - e > 1;) {
      const uint32_t mid = e + (hi - e) / 2;
      if (s_first[mid] <= r) e = mid; else hi = mid;
    }
    const swz_las_segment* sg = a.segs + k0 + e;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      la.scale[k] = sg->layout.scale[k];
      la.offset[k] = sg->layout.offset[k];
      la.mn[k] = sg->layout.min[k];
      la.mx[k] = sg->layout.max[k];
      la.center[k] = a.center[k];
    }
    la.format = sg->layout.point_format;
    la.record_bytes = sg->layout.record_bytes;
    la.xyz = a.xyz;
#pragma unroll
    for (int k = 0; k < SWZ_ATTR_COUNT; ++k) la.col[k] = a.col[k];
    la.shift = a.shift;
    start = sg->byte_offset + (uint64_t)(r - s_first[e]) * la.record_bytes;
    atomicMin(&s_lo, (unsigned long long)start);
    atomicMax(&s_hi, (unsigned long long)(start + la.record_bytes));
  }
  __syncthreads();

  // The covering aligned dwords of [s_lo, s_hi): alignment is that of the ADDRESS, raw itself may lie anywhere.
  const uintptr_t raw_begin = (uintptr_t)a.raw, raw_end = raw_begin + a.raw_bytes;
  const uintptr_t word0 = (raw_begin + (uintptr_t)s_lo) & ~(uintptr_t)3;
  const uint64_t span = (raw_begin + (uintptr_t)s_hi) - word0;
  if (span <= (uint64_t)LASIN_STAGE + 4u) {  // (block-uniform)
    for (uint32_t w = t; 4ull * w < span; w += LASIN_TILE) {
      const uintptr_t at = word0 + 4u * (uintptr_t)w;
      uint32_t v;
      if (at >= raw_begin && at + 4u <= raw_end) {
        v = *reinterpret_cast<const uint32_t*>(at);
      } else {  // the first or the last dword of the buffer: only the bytes inside it
        v = 0;
        for (uint32_t b = 0; b < 4u; ++b)
          if (at + b >= raw_begin && at + b < raw_end) v |= (uint32_t)*reinterpret_cast<const uint8_t*>(at + b) << (8u * b);
      }
      s_stage[w] = v;
    }
    __syncthreads();
    if (live) {
      const uint8_t* rec = reinterpret_cast<const uint8_t*>(s_stage) + (size_t)((raw_begin + start) - word0);
      if constexpr (SRS) las_unpack<true>(la, rec, r, &a.srs);
      else las_unpack(la, rec, r);
    }
  } else if (live) {
    if constexpr (SRS) las_unpack<true>(la, a.raw + start, r, &a.srs);
    else las_unpack(la, a.raw + start, r);
  }
}

// ---------------------------------------------------------------------------------- what the two entry points share
// the segments that hold points, checked: rows contiguous from 0, records inside raw_bytes, formats and record lengths
static int check_segments(swz_ctx* c, const char* who, uint64_t raw_bytes, uint64_t num_segments, const swz_las_segment* segments,
                          std::vector<swz_las_segment>* kept, uint64_t* rows_out) {
  auto refuse = [&](const std::string& what) { return c->fail(SWZ_ERR_BAD_ARG, std::string(who) + ": " + what); };
  if (num_segments && !segments) return refuse("NULL segments");
  uint64_t rows = 0;
  for (uint64_t s = 0; s < num_segments; ++s) {
    const swz_las_segment& sg = segments[s];
    if (sg.first_row != rows) return refuse("the rows of the segments must ascend contiguously from 0");
    if (sg.layout.point_format > 10) return refuse("LAS point data record formats 0-10 are decoded");
    if (sg.layout.record_bytes < las_format_bytes(sg.layout.point_format)) return refuse("record length shorter than the point format");
    if (sg.count > LASIN_MAX_POINTS || rows + sg.count > LASIN_MAX_POINTS) return refuse("more than 2^32-65536 points");
    if (sg.byte_offset > raw_bytes || sg.count > (raw_bytes - sg.byte_offset) / sg.layout.record_bytes)
      return refuse("the records of a segment pass raw_bytes");
    rows += sg.count;
    if (sg.count) kept->push_back(sg);
  }
  *rows_out = rows;
  return SWZ_OK;
}

static uint64_t decode_bytes(const std::vector<swz_las_segment>& segs, const double* d_xyz, const swz_attribute_columns* d_out,
                             uint32_t mask) {
  uint64_t row = d_xyz ? 24 : 0, bytes = 0;
  for (int k = 0; k < SWZ_ATTR_COUNT; ++k)
    if (k != SWZ_ATTR_NORMAL && ((mask >> k) & 1u) && d_out && d_out->column[k]) row += ATTR_BYTES[k];
  for (const swz_las_segment& sg : segs) bytes += sg.count * (sg.layout.record_bytes + row);
  return bytes;
}

// launches the kernel on `stream`; d_table holds num_segs checked segments with points.  No synchronisation.
static int launch_segments(swz_ctx* c, hipStream_t stream, const uint8_t* d_raw, uint64_t raw_bytes, const swz_las_segment* d_table,
                           uint32_t num_segs, uint32_t rows, const double* shift_center, double* d_xyz_out,
                           const swz_attribute_columns* d_out, uint32_t mask, const swz_srs* srs) {
  LasSegArgs a{};
  a.raw = d_raw;
  a.raw_bytes = raw_bytes;
  a.segs = d_table;
  a.num_segs = num_segs;
  a.n = rows;
  a.xyz = d_xyz_out;
  for (int k = 0; k < SWZ_ATTR_COUNT; ++k)  // LAS points carry no normals
    a.col[k] = (d_out && k != SWZ_ATTR_NORMAL && ((mask >> k) & 1u)) ? d_out->column[k] : nullptr;
  a.shift = shift_center != nullptr;
  for (int k = 0; k < 3; ++k) a.center[k] = shift_center ? shift_center[k] : 0.0;
  if (srs) {
    LasSegArgsOf<true> as{};
    static_cast<LasSegArgs&>(as) = a;
    as.srs = *srs;
    hipLaunchKernelGGL(las_segments_kernel<true>, dim3(div_up(rows, LASIN_TILE)), dim3(LASIN_TILE), 0, stream, as);
  } else {
    LasSegArgsOf<false> an{};
    static_cast<LasSegArgs&>(an) = a;
    hipLaunchKernelGGL(las_segments_kernel<false>, dim3(div_up(rows, LASIN_TILE)), dim3(LASIN_TILE), 0, stream, an);
  }
  SWZ_LAUNCH_CHECK(c);
  return SWZ_OK;
}

// ---------------------------------------------------------------------------------- the headers
static uint32_t get_u16(const unsigned char* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }
static uint32_t get_u32(const unsigned char* p) { return get_u16(p) | (get_u16(p + 2) << 16); }
static uint64_t get_u64(const unsigned char* p) { return (uint64_t)get_u32(p) | ((uint64_t)get_u32(p + 4) << 32); }
static double get_f64(const unsigned char* p) {
  double v;
  memcpy(&v, p, 8);
  return v;
}

// the public header block of one file (LAS 1.0 - 1.4); SWZ_LAS_FILE_* and, unless OK, the reason
static int scan_one(const char* path, swz_las_file_info* info, std::string* why) {
  *info = swz_las_file_info{};
  Fd f;
  f.fd = open(path, O_RDONLY | O_CLOEXEC);
  struct stat st;
  if (f.fd < 0 || fstat(f.fd, &st) != 0 || !S_ISREG(st.st_mode)) {
    *why = "cannot open";
    return SWZ_LAS_FILE_UNREADABLE;
  }
  const uint64_t size = (uint64_t)st.st_size;
  unsigned char h[375];
  const uint64_t have = std::min<uint64_t>(size, sizeof(h));
  if (have < 227 || !pread_all(f.fd, h, have, 0)) {
    *why = "shorter than a LAS header";
    return SWZ_LAS_FILE_BAD_HEADER;
  }
  if (memcmp(h, "LASF", 4) != 0) {
    *why = "not a LAS file (signature)";
    return SWZ_LAS_FILE_BAD_HEADER;
  }
  const uint32_t major = h[24], minor = h[25];
  const uint64_t header_size = get_u16(h + 94), data_at = get_u32(h + 96);
  const uint64_t need = (major == 1 && minor >= 4) ? 375 : ((major == 1 && minor == 3) ? 235 : 227);
  if (header_size < need || header_size > size) {
    *why = "the header is shorter than its version's, or passes the file";
    return SWZ_LAS_FILE_BAD_HEADER;
  }
  if (data_at < header_size || data_at > size) {
    *why = "the offset to the point data passes the file";
    return SWZ_LAS_FILE_BAD_HEADER;
  }
  const uint32_t format = h[104], rb = get_u16(h + 105);
  if (format & 0x80u) {
    *why = "compressed point data (LAZ is not read)";
    return SWZ_LAS_FILE_COMPRESSED;
  }
  if (format > 10) {
    *why = "point data record format above 10";
    return SWZ_LAS_FILE_BAD_HEADER;
  }
  if (rb < las_format_bytes(format)) {
    *why = "the record length is below the format's";
    return SWZ_LAS_FILE_BAD_HEADER;
  }
  // the variable length records between the header and the point data: LASzip's marks a compressed file
  uint64_t at = header_size;
  for (uint32_t v = 0, num = get_u32(h + 100); v < num && at + 54 <= data_at; ++v) {
    unsigned char vlr[54];
    if (!pread_all(f.fd, vlr, sizeof(vlr), at)) break;
    if (memcmp(vlr + 2, "laszip encoded", 14) == 0 && get_u16(vlr + 18) == 22204) {
      *why = "a LASzip VLR (LAZ is not read)";
      return SWZ_LAS_FILE_COMPRESSED;
    }
    at += 54 + (uint64_t)get_u16(vlr + 20);
  }
  uint64_t count = get_u32(h + 107);
  if (major == 1 && minor >= 4 && (count == 0 || format >= 6)) count = get_u64(h + 247);
  if (count > (size - data_at) / rb) {
    *why = "the point records pass the end of the file";
    return SWZ_LAS_FILE_BAD_HEADER;
  }
  info->point_count = count;
  info->offset_to_point_data = data_at;
  for (int k = 0; k < 3; ++k) {
    info->layout.scale[k] = get_f64(h + 131 + 8 * k);
    info->layout.offset[k] = get_f64(h + 155 + 8 * k);
    info->layout.max[k] = get_f64(h + 179 + 16 * k);  // max x, min x, max y, min y, max z, min z
    info->layout.min[k] = get_f64(h + 187 + 16 * k);
  }
  info->layout.point_format = format;
  info->layout.record_bytes = rb;
  // las_file_has_attribute (LASFile.cpp:415-445), as written
  uint32_t mask = LAS_MASK_ALWAYS;
  if (format == 2 || format == 3 || format == 5 || format == 7 || format == 8 || format == 10) mask |= 1u << SWZ_ATTR_RGB;
  if (format == 1 || format == 3) mask |= 1u << SWZ_ATTR_GPS_TIME;
  info->attribute_mask = mask;
  return SWZ_LAS_FILE_OK;
}

// ---------------------------------------------------------------------------------- the parts of the streamed call
int InputBuffers::reserve(swz_ctx* ctx, uint64_t image_bytes, bool two) {
  c = ctx;
  SWZ_TRY(c->get("in_image0", (size_t)image_bytes, &device[0]));
  if (two) SWZ_TRY(c->get("in_image1", (size_t)image_bytes, &device[1]));
  for (int b = 0; b < (two ? 2 : 1); ++b) {
    SWZ_HIP(c, hipHostMalloc(&host[b], image_bytes, hipHostMallocDefault));
    SWZ_HIP(c, hipEventCreate(&begin[b]));
    SWZ_HIP(c, hipEventCreate(&copied[b]));
    SWZ_HIP(c, hipEventCreate(&decoded[b]));
  }
  return SWZ_OK;
}

InputBuffers::~InputBuffers() {
  for (int b = 0; b < 2; ++b) {
    if (host[b]) (void)hipHostFree(host[b]);
    for (hipEvent_t e : {begin[b], copied[b], decoded[b]})
      if (e) (void)hipEventDestroy(e);
  }
  if (!c) return;
  // two raw images are the call's, not the data set's
  for (const char* name : {"in_image0", "in_image1"}) {
    const auto it = c->bufs.find(name);
    if (it == c->bufs.end()) continue;
    c->free_buf(it->second);
    c->bufs.erase(it);
  }
}

int las_input_plan(swz_ctx* c, const char* who_c, const char* const* paths, uint64_t num_files, const swz_input_params* params,
                   const double bmin[3], const double bmax[3], const swz_tile_params& tp, bool mask_fixed, uint32_t mask_now,
                   uint64_t points_now, const swz_srs* srs, LasInputPlan* plan) {
  const std::string who = std::string(who_c) + ": ";
  // ---- the headers, and everything that is refused before a point is read
  plan->files.assign(std::max<uint64_t>(num_files, 1), swz_las_file_info{});
  swz_las_dataset& ds = plan->ds;
  SWZ_TRY(swz_las_scan_files_srs(c, paths, num_files, params->flags, srs, plan->files.data(), &ds));  // (ECEF boxes with srs)
  const uint32_t mask = params->attribute_mask == ~0u ? ds.attribute_mask : params->attribute_mask;
  if (mask & (1u << SWZ_ATTR_NORMAL)) return c->fail(SWZ_ERR_BAD_ARG, who + "LAS points carry no normals");
  if (mask & ~ds.attribute_mask) return c->fail(SWZ_ERR_BAD_ARG, who + "the mask names an attribute that not every file has");
  if (mask_fixed && mask != mask_now) return c->fail(SWZ_ERR_BAD_ARG, who + "every batch must carry the same attribute columns");
  // The (shifted) tight box inside the root box.  AABB::makeCubic's own box can miss the tight box it was made from by an ulp
  // of the coordinates (centre - half the extent need not round back to the minimum), so the comparison leaves that much
  // room; the shift is taken in double.  A position that lies outside by such a rounding, or that the narrowing to float
  // moves past the box, is clamped by the indexing, as in the reference.
  const bool shift = params->shift_to_center != 0;
  for (int k = 0; k < 3; ++k) {
    const double lo = shift ? ds.tight_min[k] - ds.center[k] : ds.tight_min[k];
    const double hi = shift ? ds.tight_max[k] - ds.center[k] : ds.tight_max[k];
    const double size = std::max(std::max(std::fabs(ds.tight_min[k]), std::fabs(ds.tight_max[k])), std::fabs(ds.center[k]));
    const double room = 4 * std::numeric_limits<double>::epsilon() * size;
    if (!(bmin[k] - room <= lo && hi <= bmax[k] + room))
      return c->fail(SWZ_ERR_BAD_ARG, who + "the tiler's root box does not contain the data set's box");
  }
  if (points_now + ds.total_points > 0xFFFF0000ull) return c->fail(SWZ_ERR_TOO_MANY_POINTS, "more than 2^32-65536 points per tiler");

  // ---- the batches
  const uint64_t batch_points = params->batch_points ? params->batch_points : INPUT_BATCH_POINTS;
  const uint64_t min_last = tp.strategy == SWZ_FAST ? tp.fast_concurrency : 0;
  if (batch_points < min_last) return c->fail(SWZ_ERR_BAD_ARG, "FAST: a batch needs at least fast_concurrency points");
  plan->counts.assign(plan->files.size(), 0);
  for (uint64_t i = 0; i < num_files; ++i) plan->counts[i] = plan->files[i].point_count;
  plan->file_first.assign(num_files + 1, 0);
  for (uint64_t i = 0; i < num_files; ++i) plan->file_first[i + 1] = plan->file_first[i] + plan->counts[i];
  uint64_t num_batches = 0;
  if (swz_input_batches(num_files, plan->counts.data(), batch_points, min_last, 0, nullptr, &num_batches) != SWZ_OK)
    return c->fail(SWZ_ERR_BAD_ARG, "FAST: a batch needs at least fast_concurrency points");
  plan->cuts.assign(num_batches + 1, 0);
  (void)swz_input_batches(num_files, plan->counts.data(), batch_points, min_last, num_batches, plan->cuts.data(), &num_batches);
  plan->mask = mask;
  plan->shift = shift;
  return SWZ_OK;
}

void las_input_image(const LasInputPlan& plan, uint64_t p0, uint64_t p1, InputBatch* out) {
  InputBatch& b = *out;
  b = InputBatch{};
  b.first_point = p0;
  b.points = p1 - p0;
  // the file the first point lies in: the last one that begins at or before it and holds a point
  uint64_t file = (uint64_t)(std::upper_bound(plan.file_first.begin(), plan.file_first.end(), p0) - plan.file_first.begin());
  file = file ? file - 1 : 0;
  for (uint64_t p = p0; p < p1;) {
    while (p >= plan.file_first[file + 1]) ++file;
    const swz_las_file_info& fi = plan.files[file];
    const uint64_t rec0 = p - plan.file_first[file], cnt = std::min(p1, plan.file_first[file + 1]) - p;
    const uint64_t rb = fi.layout.record_bytes;
    swz_las_segment sg{};
    sg.first_row = p - p0;
    sg.count = cnt;
    sg.byte_offset = b.raw_bytes;
    sg.layout = fi.layout;
    b.segs.push_back(sg);
    for (uint64_t done = 0; done < cnt * rb; done += READ_PIECE)
      b.pieces.push_back({file, fi.offset_to_point_data + rec0 * rb + done, std::min(READ_PIECE, cnt * rb - done), b.raw_bytes + done});
    b.raw_bytes += cnt * rb;
    p += cnt;
  }
  b.table_at = (b.raw_bytes + 15) & ~15ull;
  b.image_bytes = b.table_at + b.segs.size() * sizeof(swz_las_segment);
}

void las_start_read(TicketRun& run, swz_ctx* c, const char* who, const InputBatch* b, unsigned char* image, const char* const* paths,
                    long threads) {
  memcpy(image + b->table_at, b->segs.data(), b->segs.size() * sizeof(swz_las_segment));
  run.start(c, b->pieces.size(), [who, b, image, paths](uint64_t i, std::string* err) {
    const ReadPiece& p = b->pieces[i];
    Fd f;
    f.fd = open(paths[p.file], O_RDONLY | O_CLOEXEC);
    if (f.fd < 0 || !pread_all(f.fd, image + p.image_at, p.bytes, p.file_at)) {
      *err = std::string(who) + ": cannot read the point records of " + paths[p.file];
      return (int)SWZ_ERR_BAD_ARG;
    }
    return (int)SWZ_OK;
  }, threads);
}

int las_launch_image(swz_ctx* c, hipStream_t stream, const uint8_t* d_image, const InputBatch& b, const double* shift_center,
                     double* d_xyz_out, const swz_attribute_columns* d_out, uint32_t mask, const swz_srs* srs) {
  if (!b.points) return SWZ_OK;
  return launch_segments(c, stream, d_image, b.raw_bytes, reinterpret_cast<const swz_las_segment*>(d_image + b.table_at),
                         (uint32_t)b.segs.size(), (uint32_t)b.points, shift_center, d_xyz_out, d_out, mask, srs);
}

void InputLane::cut(const LasInputPlan& plan, int r, int of) {
  batches.assign(plan.num_batches(), InputBatch{});
  for (uint64_t j = 0; j < plan.num_batches(); ++j) {
    const uint64_t b0 = plan.cuts[j], pts = plan.cuts[j + 1] - b0;
    las_input_image(plan, b0 + pts * (uint64_t)r / of, b0 + pts * (uint64_t)(r + 1) / of, &batches[j]);
    image_max = std::max(image_max, batches[j].image_bytes);
    rows_max = std::max(rows_max, batches[j].points);
  }
}

void las_input_stream(const LasInputPlan& plan, const swz_srs* srs, const char* who, const char* const* paths, std::vector<InputLane>& lanes,
                      const InputStreamOps& ops, InputStreamResult* result) {
  InputStreamResult& o = *result;
  const int N = (int)lanes.size();
  const uint64_t num_batches = plan.num_batches();
  const long budget =
    std::max(1L, lanes[0].c->opt_int("SWZ_INPUT_READER_THREADS", (long)std::min(32u, std::max(1u, std::thread::hardware_concurrency()))));
  auto label = [&](int r) { return ops.lane_name ? std::string(ops.lane_name) + " " + std::to_string(r) + ": " : std::string(); };
  auto fail_stream = [&](int st, const std::string& text) {
    if (o.status == SWZ_OK) {
      o.status = st;
      o.why = text;
    }
  };
  auto start_read = [&](uint64_t j) {
    for (int r = 0; r < N; ++r)
      las_start_read(lanes[r].readers, lanes[r].c, who, &lanes[r].batches[j], static_cast<unsigned char*>(lanes[r].ib.host[j & 1]), paths,
                     std::max(1L, budget / N + (r < budget % N ? 1 : 0)));
  };
  // joins the readers of batch j; the time the call stood waiting for them counts as waiting for input
  auto wait_read = [&](uint64_t j) -> bool {
    const auto t0 = std::chrono::steady_clock::now();
    bool ok = true;
    for (InputLane& L : lanes) {
      double ms = 0;
      std::string err;
      const int st = L.readers.wait(&err, &ms);
      L.read_ms += ms;
      if (st != SWZ_OK) {
        fail_stream(st, err);
        ok = false;
      } else {
        o.bytes_read += L.batches[j].raw_bytes;
      }
    }
    o.wait_ms += ms_since(t0);
    return ok;
  };
  // batch j: every lane's image to its device and decoded to where the caller wants it (a lane with no point of the batch
  // copies and launches nothing, and records its events all the same), then the caller's commit
  auto enqueue = [&](uint64_t j) -> int {
    const int s = (int)(j & 1);
    std::string why;
    for (int r = 0; r < N && o.status == SWZ_OK; ++r) {
      InputLane& L = lanes[r];
      const InputBatch& b = L.batches[j];
      (void)hipSetDevice(L.c->device);
      const InputTarget to = ops.target(r);
      hipError_t e = hipEventRecord(L.ib.begin[s], L.copy);
      if (e == hipSuccess && b.image_bytes) e = hipMemcpyAsync(L.ib.device[s], L.ib.host[s], b.image_bytes, hipMemcpyHostToDevice, L.copy);
      if (e == hipSuccess) e = hipEventRecord(L.ib.copied[s], L.copy);
      if (e == hipSuccess) {
        const int st = las_launch_image(L.c, L.copy, L.ib.device[s], b, plan.shift ? plan.ds.center : nullptr, to.xyz, &to.cols, to.mask, srs);
        if (st != SWZ_OK) fail_stream(st, label(r) + L.c->err);
        else e = hipEventRecord(L.ib.decoded[s], L.copy);
      }
      if (e != hipSuccess) fail_stream(SWZ_ERR_HIP, label(r) + "the copy and decode of a batch image: " + hipGetErrorString(e));
    }
    if (o.status != SWZ_OK) return o.status;
    const int st = ops.commit(j, &why);
    if (st != SWZ_OK) fail_stream(st, why);
    return st;
  };

  start_read(0);
  if (wait_read(0)) {
    o.enqueued = true;
    if (enqueue(0) == SWZ_OK && num_batches > 1) start_read(1);
  }
  for (uint64_t j = 0; j < num_batches && o.status == SWZ_OK; ++j) {
    // (a read that failed: batch j, which is staged, is still tiled -- the stream stops after the running batch)
    if (j + 1 < num_batches && wait_read(j + 1) && enqueue(j + 1) == SWZ_OK && j + 2 < num_batches) {
      // the host images of batch j + 2 are batch j's: their copies have left them
      for (int r = 0; r < N && o.status == SWZ_OK; ++r) {
        (void)hipSetDevice(lanes[r].c->device);
        const hipError_t e = hipEventSynchronize(lanes[r].ib.copied[j & 1]);
        if (e != hipSuccess) fail_stream(SWZ_ERR_HIP, label(r) + "the copy of a batch image: " + hipGetErrorString(e));
      }
      if (o.status == SWZ_OK) start_read(j + 2);
    }
    const auto t_tile = std::chrono::steady_clock::now();
    double waited = 0;
    std::string why;
    o.tiled = true;
    const int st = ops.tile(&waited, &why);
    o.tile_ms += ms_since(t_tile) - waited;
    o.wait_ms += waited;
    if (st != SWZ_OK) {
      o.status = st;  // (the failure of the tiling comes first: its tiler is poisoned with that text)
      o.why = why;
      break;
    }
    for (InputLane& L : lanes) {  // batch j has been decoded: its tiling waited for the event behind it
      float ms = 0.f;
      if (hipEventElapsedTime(&ms, L.ib.begin[j & 1], L.ib.copied[j & 1]) == hipSuccess) L.copy_ms += ms;
      if (hipEventElapsedTime(&ms, L.ib.copied[j & 1], L.ib.decoded[j & 1]) == hipSuccess) L.decode_ms += ms;
    }
    ++o.batches;
    o.points += plan.cuts[j + 1] - plan.cuts[j];
  }
  for (InputLane& L : lanes) {
    if (L.readers.running()) (void)L.readers.wait(nullptr, nullptr);
    (void)hipSetDevice(L.c->device);
    if (L.copy) (void)hipStreamSynchronize(L.copy);
    o.read_ms = std::max(o.read_ms, L.read_ms);
    o.copy_ms = std::max(o.copy_ms, L.copy_ms);
    o.decode_ms = std::max(o.decode_ms, L.decode_ms);
  }
}

}  // namespace swz

using namespace swz;

extern "C" {

uint32_t swz_las_input_tile(void) { return LASIN_TILE; }

int swz_las_scan_files(swz_ctx* c, const char* const* paths, uint64_t num_files, uint32_t flags, swz_las_file_info* files_out,
                       swz_las_dataset* dataset_out) {
  return swz_las_scan_files_srs(c, paths, num_files, flags, nullptr, files_out, dataset_out);
}

// (the messages name swz_las_scan_files with and without a projection: it is that call)
int swz_las_scan_files_srs(swz_ctx* c, const char* const* paths, uint64_t num_files, uint32_t flags, const swz_srs* srs,
                           swz_las_file_info* files_out, swz_las_dataset* dataset_out) {
  if (!dataset_out || (num_files && !paths)) return fail(c, SWZ_ERR_BAD_ARG, "swz_las_scan_files: NULL argument");
  if (srs && !srs_valid(srs)) return fail(c, SWZ_ERR_BAD_ARG, "swz_las_scan_files_srs: not a definition swz_srs_parse made");
  if (flags & ~SWZ_LAS_SCAN_SKIP_UNREADABLE) return fail(c, SWZ_ERR_BAD_ARG, "swz_las_scan_files: unknown flag");
  swz_las_dataset ds{};
  ds.attribute_mask = LAS_MASK_ALWAYS | (1u << SWZ_ATTR_RGB) | (1u << SWZ_ATTR_GPS_TIME);
  // AABB(): min = the largest double, max = its negative; update() takes std::min / std::max per axis (AABB.h:15-48)
  for (int k = 0; k < 3; ++k) {
    ds.tight_min[k] = std::numeric_limits<double>::max();
    ds.tight_max[k] = -std::numeric_limits<double>::max();
  }
  for (uint64_t i = 0; i < num_files; ++i) {
    if (!paths[i]) return fail(c, SWZ_ERR_BAD_ARG, "swz_las_scan_files: NULL path");
    swz_las_file_info info;
    std::string why;
    const int status = scan_one(paths[i], &info, &why);
    if (status != SWZ_LAS_FILE_OK) {
      if (!(flags & SWZ_LAS_SCAN_SKIP_UNREADABLE)) return fail(c, SWZ_ERR_BAD_ARG, "swz_las_scan_files: " + why + ": " + paths[i]);
      info = swz_las_file_info{};
      info.status = status;
      if (files_out) files_out[i] = info;
      continue;
    }
    if (files_out) files_out[i] = info;
    ds.total_points += info.point_count;
    ++ds.readable_files;
    ds.attribute_mask &= info.attribute_mask;
    // with a projection the file's box joins the union as the box of its eight corners in ECEF (calculate_dataset_metadata,
    // TilerProcess.cpp:352-387); files_out keeps the header's own values
    double box_min[3], box_max[3];
    for (int k = 0; k < 3; ++k) {
      box_min[k] = info.layout.min[k];
      box_max[k] = info.layout.max[k];
    }
    if (srs && swz_srs_transform_box(srs, SWZ_SRS_ECEF, info.layout.min, info.layout.max, box_min, box_max) != SWZ_OK)
      return fail(c, SWZ_ERR_BAD_ARG, "swz_las_scan_files: the source projection could not map a header box");
    for (int k = 0; k < 3; ++k) {  // update(bounds.min), then update(bounds.max)
      for (const double v : {box_min[k], box_max[k]}) {
        ds.tight_min[k] = std::min(ds.tight_min[k], v);
        ds.tight_max[k] = std::max(ds.tight_max[k], v);
      }
    }
  }
  if (ds.total_points == 0) return fail(c, SWZ_ERR_BAD_ARG, "swz_las_scan_files: Found no points to process");
  // AABB::makeCubic (AABB.h:50-61) with getCenter = min + extent / 2 (:70)
  double extent[3];
  for (int k = 0; k < 3; ++k) extent[k] = ds.tight_max[k] - ds.tight_min[k];
  const double max_extent = std::max(extent[0], std::max(extent[1], extent[2]));
  const double half_length = max_extent / 2;
  for (int k = 0; k < 3; ++k) {
    const double center = ds.tight_min[k] + extent[k] / 2;
    ds.cubic_min[k] = center - half_length;
    ds.cubic_max[k] = center + half_length;
  }
  // total_bounds_cubic_at_origin (FileStats.cpp:30-37): minus the CUBIC box's centre
  for (int k = 0; k < 3; ++k) {
    ds.center[k] = ds.cubic_min[k] + (ds.cubic_max[k] - ds.cubic_min[k]) / 2;
    ds.origin_min[k] = ds.cubic_min[k] - ds.center[k];
    ds.origin_max[k] = ds.cubic_max[k] - ds.center[k];
  }
  *dataset_out = ds;
  return SWZ_OK;
}

int swz_input_batches(uint64_t num_files, const uint64_t* file_count, uint64_t batch_points, uint64_t min_last, uint64_t max_batches,
                      uint64_t* first_point_out, uint64_t* num_batches_out) {
  if (!num_batches_out || (num_files && !file_count) || batch_points == 0) return SWZ_ERR_BAD_ARG;
  uint64_t total = 0;
  for (uint64_t i = 0; i < num_files; ++i) {
    if (file_count[i] > ~0ull - total) return SWZ_ERR_BAD_ARG;
    total += file_count[i];
  }
  if (total < min_last) return SWZ_ERR_BAD_ARG;
  uint64_t batches = total / batch_points + (total % batch_points ? 1 : 0);
  // OURS: a tail shorter than min_last joins the batch before it
  if (batches > 1 && total - (batches - 1) * batch_points < min_last) --batches;
  if (first_point_out) {
    if (batches > max_batches) return SWZ_ERR_BAD_ARG;
    for (uint64_t j = 0; j < batches; ++j) first_point_out[j] = j * batch_points;
    first_point_out[batches] = total;
  }
  *num_batches_out = batches;
  return SWZ_OK;
}

int swz_las_decode_segments_device(swz_ctx* c, const uint8_t* d_raw, uint64_t raw_bytes, uint64_t num_segments,
                                   const swz_las_segment* segments, const double shift_center[3], double* d_xyz_out,
                                   const swz_attribute_columns* d_out) {
  return swz_las_decode_segments_srs_device(c, d_raw, raw_bytes, num_segments, segments, shift_center, d_xyz_out, d_out, nullptr);
}

int swz_las_decode_segments_srs_device(swz_ctx* c, const uint8_t* d_raw, uint64_t raw_bytes, uint64_t num_segments,
                                       const swz_las_segment* segments, const double shift_center[3], double* d_xyz_out,
                                       const swz_attribute_columns* d_out, const swz_srs* srs) {
  if (!c) return SWZ_ERR_BAD_ARG;
  if (srs && !srs_valid(srs)) return c->fail(SWZ_ERR_BAD_ARG, "swz_las_decode_segments_srs_device: not a definition swz_srs_parse made");
  SWZ_HIP(c, hipSetDevice(c->device));
  // everything is checked on the host before anything is launched
  std::vector<swz_las_segment> segs;
  uint64_t rows = 0;
  SWZ_TRY(check_segments(c, "swz_las_decode_segments_device", raw_bytes, num_segments, segments, &segs, &rows));
  if (shift_center && !finite3(shift_center)) return c->fail(SWZ_ERR_BAD_ARG, "swz_las_decode_segments_device: the centre is not finite");
  if (rows == 0) return SWZ_OK;
  if (!d_raw) return c->fail(SWZ_ERR_BAD_ARG, "swz_las_decode_segments_device: NULL records");
  swz_las_segment* d_table = nullptr;
  SWZ_TRY(c->get("las_segments", segs.size(), &d_table));
  SWZ_HIP(c, hipMemcpyAsync(d_table, segs.data(), segs.size() * sizeof(swz_las_segment), hipMemcpyHostToDevice, c->stream));
  {
    ProfScope ps(c, srs ? "las_decode_segments_srs" : "las_decode_segments", decode_bytes(segs, d_xyz_out, d_out, ~0u), 1);
    SWZ_TRY(launch_segments(c, c->stream, d_raw, raw_bytes, d_table, (uint32_t)segs.size(), (uint32_t)rows, shift_center, d_xyz_out, d_out,
                            ~0u, srs));
  }
  SWZ_HIP(c, hipStreamSynchronize(c->stream));  // (the table's host copy lives until here)
  return SWZ_OK;
}

int swz_tiler_add_las_files(swz_tiler* t, const char* const* paths, uint64_t num_files, const swz_input_params* params,
                            swz_input_stats* stats) {
  if (!t) return SWZ_ERR_BAD_ARG;
  swz_ctx* c = t->c;
  const char* who = "swz_tiler_add_las_files";
  const auto t_wall = std::chrono::steady_clock::now();
  if (stats) *stats = swz_input_stats{};
  SWZ_HIP(c, hipSetDevice(c->device));
  SWZ_TRY(tiler_guard(t));
  if (!params || (num_files && !paths)) return c->fail(SWZ_ERR_BAD_ARG, "swz_tiler_add_las_files: NULL argument");
  std::string refusal;
  if (const int st = tiler_refuses_input(t, who, &refusal)) return c->fail(st, refusal);

  // ---- the headers, everything that is refused before a point is read, the cuts and the images
  const bool first = tiler_empty(t);
  LasInputPlan plan;
  const swz_srs* const srs = t->has_srs ? &t->srs : nullptr;
  SWZ_TRY(las_input_plan(c, who, paths, num_files, params, t->bmin, t->bmax, t->p, !first, t->attr_mask, t->staged_total, srs, &plan));
  std::vector<InputLane> lanes(1);
  InputLane& lane = lanes[0];
  lane.c = c;
  lane.copy = t->copy_stream;
  lane.cut(plan, 0, 1);

  // ---- the pools, once for the total: nothing grows while a batch is in flight
  const uint32_t mask_before = t->attr_mask;
  auto prepare = [&]() -> int {
    if (first) {
      t->attr_mask = plan.mask;
      if (plan.mask && t->pool_cap) {  // the pools were presized before the columns were known
        const size_t cap = t->pool_cap;
        t->pool_cap = 0;
        t->pool_xyz = nullptr;
        SWZ_TRY(pool_reserve(t, cap));
      }
    }
    SWZ_TRY(pool_reserve(t, (size_t)t->staged_total + plan.ds.total_points));
    return lane.ib.reserve(c, lane.image_max, plan.num_batches() > 1);
  };
  if (const int st = prepare()) {
    t->attr_mask = mask_before;
    return st;
  }

  // ---- the stream: every batch into the pool rows behind what is staged, staged like a host batch
  InputStreamOps ops;
  ops.target = [&](int) {
    const size_t at = t->staged_total;
    InputTarget to{t->pool_xyz + at * 3, {}, t->attr_mask};
    for (int a = 0; a < SWZ_ATTR_COUNT; ++a)
      to.cols.column[a] = (t->attr_mask & (1u << a)) ? (void*)((char*)t->pool_attr[a] + at * TILER_ATTR_BYTES[a]) : nullptr;
    return to;
  };
  ops.commit = [&](uint64_t j, std::string* why) -> int {
    hipEvent_t ev = nullptr;
    hipError_t e = hipEventCreateWithFlags(&ev, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventRecord(ev, t->copy_stream);
    if (e != hipSuccess) {
      if (ev) (void)hipEventDestroy(ev);
      *why = std::string("the event behind a staged batch: ") + hipGetErrorString(e);
      return SWZ_ERR_HIP;
    }
    const InputBatch& b = lane.batches[j];
    t->staged_events.push_back(ev);
    t->staged_sizes.push_back((uint32_t)b.points);
    t->staged_total += (uint32_t)b.points;
    t->staged_bytes += b.image_bytes;
    return SWZ_OK;
  };
  ops.tile = [&](double* waited_ms, std::string* why) -> int {
    const double waited_before = t->staged_wait_ms;
    const int st = swz_tiler_tile_staged(t, nullptr);
    *waited_ms = t->staged_wait_ms - waited_before;
    if (st != SWZ_OK) *why = c->err;
    return st;
  };
  InputStreamResult res;
  las_input_stream(plan, srs, who, paths, lanes, ops, &res);
  // a failure once a batch has been enqueued: the pools are ahead of the ids, the store may be half merged
  if (res.status != SWZ_OK && res.enqueued) (void)swz_tiler_poison(t, res.why.c_str());
  else if (res.status != SWZ_OK) t->attr_mask = mask_before;
  if (stats) res.fill(stats, plan.ds.readable_files, ms_since(t_wall));
  return res.status == SWZ_OK ? SWZ_OK : c->fail(res.status, res.why);
}

int swz_tiler_set_source_srs(swz_tiler* t, const swz_srs* srs) {
  if (!t) return SWZ_ERR_BAD_ARG;
  swz_ctx* c = t->c;
  SWZ_TRY(tiler_guard(t));
  if (t->finalized || !tiler_empty(t))
    return c->fail(SWZ_ERR_BAD_ARG, "swz_tiler_set_source_srs: the tiler holds points, or a batch is staged or open");
  if (srs && !srs_valid(srs)) return c->fail(SWZ_ERR_BAD_ARG, "swz_tiler_set_source_srs: not a definition swz_srs_parse made");
  t->has_srs = srs != nullptr;
  if (srs) t->srs = *srs;
  return SWZ_OK;
}

}  // extern "C"
