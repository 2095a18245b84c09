// swz_toutput.h -- the three parts of swz_tiler_write_output (swz_toutput.hip), for the callers that run them apart:
// validate and plan (output_plan, output_create_dirs), stream the files of a node range of a plan (output_cuts,
// OutputImages, output_stream), write the metadata from a table (output_metadata).  swz_group_write_output
// (swz_goutput.hip) runs the middle part per shard and the other two once.
#pragma once
#include <functional>
#include <string>
#include <vector>

#include "swz_tiler.h"

namespace swz {

// the table of one output format: sizes of the bodies, the pack call and the file of a node
struct OutputPlan {
  int format = 0;
  uint32_t mask = 0;        // as the format's pack call takes it
  int rgb_mapping = SWZ_PNTS_RGB_FROM_COLOR;
  double rtc[3] = {0, 0, 0};
  double bmin[3] = {0, 0, 0}, bmax[3] = {0, 0, 0};  // the root box
  float spacing_at_root = 0.f;
  std::string data_dir;     // where the node files go
  std::vector<int8_t> level;
  std::vector<uint64_t> key, offset, count;              // offset: rows of the source's ids
  std::vector<uint64_t> body_at, body_size, file_size;  // per node, body_at relative to the image of the whole table
  std::vector<double> box_min, box_max, scale;           // LAS
  // SWZ_OUT_TIGHT_BOUNDS: the boxes of the nodes' points (3 per node; +inf / -inf until the node's chunk is reduced, and for
  // a node without points).  output_stream fills them chunk by chunk, before the chunk's files are written.
  bool tight = false;
  std::vector<double> tight_min, tight_max;
  // swz_convert_dataset_world (3DTILES): every chunk's positions are projected in place (world_srs, may be null: they stay)
  // and every file is relative to its node's own origin, the per-axis minimum of its projected rows: world_min, which
  // output_stream fills with world_max chunk by chunk like the tight boxes (3 per node; +inf / -inf for a node without points)
  bool world = false;
  const swz_srs* world_srs = nullptr;
  std::vector<double> world_min, world_max;
};

// where the rows of a plan's nodes come from: row i of a node = row ids[offset + i] of xyz and of the columns
struct OutputSource {
  const uint32_t* ids = nullptr;
  const double* xyz = nullptr;
  swz_attribute_columns in{};
  double* world_xyz = nullptr;  // a world plan: xyz, writable -- rows in stored order (ids the identity), projected in place
};

struct OutputStreamStats {
  uint64_t bytes_written = 0, chunks = 0;
  double pack_ms = 0, copy_ms = 0, write_ms = 0;
};

// Two chunk images on the device ("out_image0/1" of the workspace) and in page-locked host memory, the copy stream and
// its events; released however the call ends.  reserve() may be called once.
struct OutputImages {
  swz_ctx* c = nullptr;
  uint8_t* device[2] = {nullptr, nullptr};
  void* host[2] = {nullptr, nullptr};
  hipStream_t copy = nullptr;
  hipEvent_t begin[2] = {nullptr, nullptr}, end[2] = {nullptr, nullptr};
  int reserve(swz_ctx* ctx, uint64_t image_bytes, bool two);
  ~OutputImages();
};

// the call's part of the workspace ("out_*") goes back when it ends: it is the call's, not the data set's
struct OutputWorkspace {
  swz_ctx* c;
  ~OutputWorkspace();
};

// Everything that is refused before anything is written, except a dir that cannot be created; then the layout of the table
// that p->level / key / offset / count hold, and the LAS boxes.  `who` starts the messages.
int output_plan(swz_ctx* c, const char* who, const swz_output_params* params, uint32_t attr_mask, const double bmin[3],
                const double bmax[3], float spacing_at_root, const char* dir, OutputPlan* p);
int output_create_dirs(swz_ctx* c, const char* who, OutputPlan* p, const char* dir);
// chunk_points of swz_output_params as the cuts take it: 0 is the library's default (option SWZ_OUTPUT_CHUNK_POINTS)
uint64_t output_chunk_points(swz_ctx* c, uint64_t chunk_points);
// the chunks of the nodes [k0, k1) of a plan: first->at(j) .. first->at(j + 1) are chunk j's nodes; the largest chunk image
void output_cuts(swz_ctx* c, const OutputPlan& p, uint64_t k0, uint64_t k1, uint64_t chunk_points, std::vector<uint64_t>* first,
                 uint64_t* image_max);
// A source that exists chunk by chunk (swz_convert_dataset): called before chunk j is packed, while the files of chunk j - 1
// are being written; it may change *src.  A failure (c's error) stops the stream after the running chunk.
using OutputChunkFeed = std::function<int(uint64_t j, OutputSource* src)>;
// packs, copies and writes chunk after chunk; writer_threads 0: option SWZ_BIN_WRITER_THREADS.  A failure is c's error.
// A tight plan also gets its chunk's boxes (swz_node_boxes_device beside the pack call).  feed (may be NULL): see above.
int output_stream(swz_ctx* c, OutputPlan& p, const std::vector<uint64_t>& first, const OutputSource& src, OutputImages& img,
                  long writer_threads, OutputStreamStats* st, const OutputChunkFeed* feed = nullptr);
int output_metadata(swz_ctx* c, const char* who, const OutputPlan& p, const char* dir, const swz_output_params* params);

// the node table of a tiler into a plan; refuses a poisoned tiler and one with a batch staged or open
int output_tiler_table(swz_tiler* t, const char* who, OutputPlan* p, swz_tiler_info* info);

}  // namespace swz
