// swz_convert.h -- what the readers of a written data set share: the scanned source (swz_dataset.hip), the launch of the BIN
// unpack kernel on a stream (swz_binunpack.hip) and the stream of a source's chunks onto the device (swz_source.hip).
// swz_dataset_query* (swz_query.hip), swz_dataset_summarize (swz_summary.hip) and swz_dataset_rasterize (swz_qraster.hip) are
// chunk bodies of SourceLoop::each_chunk, which owns the loop; swz_convert_dataset (swz_convert.hip) drives SourceStream's plan / start / next itself, from the feed of
// output_stream, because there the output side owns the loop.
#pragma once
#include <functional>
#include <string>
#include <vector>

#include "swz_internal.h"
#include "swz_tinput.h"
#include "swz_toutput.h"

namespace swz {

// a written data set as swz_dataset_scan finds it: the node table in (level, Morton index) order, and per node what the
// readers of swz_convert_dataset need
struct DatasetScan {
  swz_dataset_info info{};
  std::vector<int8_t> level;
  std::vector<uint64_t> key, count;
  std::vector<std::string> path;
  std::vector<swz_las_layout> layout;  // LAS sources
  std::vector<uint64_t> data_at;       // LAS sources: the offset to the point data
  std::vector<uint64_t> file_bytes;    // 3DTILES sources, filled by source_open: the size of the file
  // the scan of the nodes index[0], index[1], ... alone: every per-node array that is filled, info.points and
  // info.num_nodes counted anew, the rest of info as it is.  A new per-node array belongs in here, and nowhere else.
  DatasetScan subset(const std::vector<uint32_t>& index) const;
};
// `who` starts the messages; ctx may be NULL
int dataset_scan(swz_ctx* c, const char* who, const char* dir, int32_t max_depth, DatasetScan* out);

// an entry of the unpack kernel's table: a segment that holds points
struct BinUnpackSeg {
  uint64_t byte_offset;
  uint32_t first_row, count;
  uint32_t file_mask;  // bit j: the image holds the j-th attribute array of FILE_ORDER
  uint32_t pad;
};
BinUnpackSeg bin_unpack_seg(uint64_t byte_offset, uint64_t first_row, uint64_t count, uint32_t mask);
uint64_t bin_image_bytes(uint64_t count, uint32_t mask);  // 12 + count x the row of the mask
// the kernel on `stream` for a checked table that lies on the device: rows [0, rows) of d_xyz_out and of the columns of d_out.
// No synchronisation.
int bin_unpack_launch(swz_ctx* c, hipStream_t stream, const uint8_t* d_raw, uint64_t raw_bytes, const BinUnpackSeg* d_table,
                      uint32_t num_segs, uint32_t rows, double* d_xyz_out, const swz_attribute_columns* d_out);

// where the arrays of a .pnts file are (swz_pnts.hip): the offsets count from the first byte of the file
struct PntsImage {
  uint64_t count = 0;
  uint32_t mask = 0;  // SWZ_PNTS_RGB | SWZ_PNTS_INTENSITY: the arrays the file holds
  double rtc[3] = {0, 0, 0};
  uint64_t position = 0, rgb = 0, intensity = 0;
  uint64_t file_bytes = 0;  // the header's byteLength
};
// Every check of swz_pnts_read_header / swz_pnts_read_node on a file image; reads nothing outside [file, file + file_bytes).
// No context (reader threads call it): what is wrong goes to *why.
int pnts_parse_image(const unsigned char* file, uint64_t file_bytes, PntsImage* out, std::string* why);
// the same of a file's header and feature-table JSON alone; *why names the file
int pnts_read_head(const char* path, PntsImage* out, std::string* why);
// the .pnts unpack kernel (swz_pntsunpack.hip) on `stream` for a checked table on the device whose segments all hold points
int pnts_unpack_launch(swz_ctx* c, hipStream_t stream, const uint8_t* d_raw, uint64_t raw_bytes, const swz_pnts_segment* d_table,
                       uint32_t num_segs, uint32_t rows, double* d_xyz_out, const swz_attribute_columns* d_out);

// ---- the source half of swz_convert_dataset (swz_source.hip), shared with swz_dataset_query* and swz_dataset_summarize
// dataset_scan, then what is refused of a 3DTILES source: one without SWZ_CONVERT_LOSSY_SOURCE in source_flags, files whose
// RTC_CENTER differ.  Fills scan->file_bytes of such a source; rtc_out (may be NULL): the files' common RTC_CENTER, else 0.
int source_open(swz_ctx* c, const char* who, const char* dir, int32_t max_depth, uint32_t source_flags, DatasetScan* scan,
                double rtc_out[3]);

// the raw image of one chunk: the files of its nodes back to back, each at a multiple of 8, then the kernel's segment table
struct SourceChunk {
  uint64_t rows = 0, raw_bytes = 0, table_at = 0, image_bytes = 0;
  InputBatch las;                  // LAS sources: segments and pieces as swz_tiler_add_las_files cuts them
  std::vector<BinUnpackSeg> segs;  // BIN, BINZ
  std::vector<ReadPiece> pieces;   // BIN: parts of files; BINZ: whole files (bytes: what the stream inflates to); 3DTILES: whole files
  std::vector<uint64_t> piece_row; // 3DTILES: the first row of a piece's file; its segment is filled by the piece's reader
};

// Chunk after chunk of a scanned source as chunk-local positions and columns on the device: reader threads
// (SWZ_INPUT_READER_THREADS) fill one of two page-locked images with the chunk's files (BINZ inflated, LAS as record ranges,
// .pnts whole; headers checked against the scan), `copy` moves it to the device and the source format's unpack kernel runs
// behind it on the same stream.  next(j) returns when chunk j lies in xyz / cols and the readers of chunk j + 1 have been
// started: they run while the caller works on chunk j.  The arrays are "out_cv_*" of the workspace (an OutputWorkspace of
// the caller gives them back).  The scan, `first` and the stream outlive the object; its readers are joined when it ends.
struct SourceStream {
  swz_ctx* c = nullptr;
  const char* who = nullptr;
  const DatasetScan* scan = nullptr;
  const std::vector<uint64_t>* first = nullptr;  // chunk j: the nodes [first[j], first[j + 1]) of the scan
  hipStream_t copy = nullptr;
  uint32_t mask = 0;
  uint64_t num_chunks = 0, image_max = 0, rows_max = 0;
  double* xyz = nullptr;
  swz_attribute_columns cols{};
  uint64_t bytes_read = 0;
  double read_ms = 0, unpack_ms = 0, copy_ms = 0;

  // sizes the images and the arrays over all chunks; nothing is allocated
  void plan(swz_ctx* ctx, const char* who_c, const DatasetScan* s, const std::vector<uint64_t>* first_nodes, uint32_t attribute_mask);
  // the arrays and the images (a plan with rows); then the readers of chunk 0
  int start(hipStream_t copy_stream);
  int next(uint64_t j);
  uint64_t rows(uint64_t j) const { return ch_[j & 1].rows; }  // of the chunk next(j) delivered
  ~SourceStream() { (void)readers_.wait(nullptr, nullptr); }  // (they write into ib_'s host images)

private:
  void read_chunk(uint64_t j);
  TicketRun readers_;
  InputBuffers ib_;
  SourceChunk ch_[2];
  std::vector<const char*> paths_;
  long threads_ = 1;
};

// the chunks of a node table, whole nodes of chunk_points points at the most (0: the library's default, output_chunk_points;
// a node larger than that is a chunk of its own): first->at(j) .. first->at(j + 1) are chunk j's nodes, counted from 0
void source_cuts(swz_ctx* c, const uint64_t* counts, uint64_t n, uint64_t chunk_points, std::vector<uint64_t>* first);

// chunk j of SourceLoop::each_chunk as its body sees it: the nodes [k0, k1) of the scan, their rows back to back in the
// chunk-local arrays
struct SourceChunkView {
  uint64_t j, k0, k1, rows;
  const double* xyz;
  const swz_attribute_columns* cols;
};
using SourceChunkBody = std::function<int(const SourceChunkView&)>;
struct SourceLoopStats {
  uint64_t chunks = 0, bytes_read = 0;  // chunks: those next() delivered
  double read_ms = 0, unpack_ms = 0, copy_ms = 0;
  double body_ms = 0;  // host wall time of the bodies that returned SWZ_OK
};
// The chunk loop of a reader.  The constructor cuts the scan's nodes into chunks and sizes the stream for the columns of
// `mask` (host only, nothing is allocated); rows_max / nodes_max are the largest chunk's, for what a caller sets up once
// before the loop (rows_max 0: no points, no chunk comes).  each_chunk streams them: body(chunk) runs while the readers work
// on the next chunk.  A next() or a body that fails ends the loop with its status (c's error; *stats is then not written).
// The copy stream and the arrays exist only for a scan with points.  An object in the caller's frame and not a function:
// what it holds is given up when the CALL ends, however it ends, behind the caller's wall_ms -- freeing the page-locked
// images and the device arrays was never part of that figure, and a caller needs the sizes before the first chunk.
// The members' order is the order they end in, backwards: the stream's readers are joined first (they write into its
// page-locked images, and its unpack kernels run on the copy stream), then the copy stream is destroyed, and only then does
// the call's part of the workspace ("out_*": the chunk-local arrays those kernels write, and a caller's own) go back.
class SourceLoop {
public:
  SourceLoop(swz_ctx* c, const char* who, const DatasetScan& scan, uint32_t mask, uint64_t chunk_points);
  uint64_t rows_max() const { return source_.rows_max; }
  uint64_t nodes_max() const { return nodes_max_; }
  int each_chunk(const SourceChunkBody& body, SourceLoopStats* stats);

private:
  struct CopyStream {
    hipStream_t s = nullptr;
    ~CopyStream() {
      if (s) (void)hipStreamDestroy(s);
    }
  };
  OutputWorkspace ow_;
  CopyStream copy_;
  std::vector<uint64_t> first_;
  uint64_t nodes_max_ = 0;
  SourceStream source_;
};

}  // namespace swz
