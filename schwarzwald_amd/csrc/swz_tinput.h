// swz_tinput.h -- the parts of swz_tiler_add_las_files (swz_tinput.hip), for the callers that run them apart: scan, refuse
// and cut (las_input_plan), the raw image of a run of points of the data set (las_input_image), its reader threads
// (las_start_read), the segment kernel on a stream (las_launch_segments), and the two images of a call (InputBuffers).
// swz_group_add_las_files (swz_group.hip) runs the first once and the others per shard.
#pragma once
#include <string>
#include <vector>

#include "swz_hostio.h"
#include "swz_tiler.h"

namespace swz {

// one piece of an image: `bytes` bytes at `file_at` of file `file` to `image_at` of the image
struct ReadPiece {
  uint64_t file, file_at, bytes, image_at;
};

// the raw image of a run of points of the concatenated files: a batch, or a shard's slice of one
struct InputBatch {
  uint64_t first_point = 0, points = 0;
  uint64_t raw_bytes = 0, table_at = 0, image_bytes = 0;  // the image: the records back to back, then the segment table
  std::vector<swz_las_segment> segs;
  std::vector<ReadPiece> pieces;
};

// what a call holds on one device besides the context's workspace; released however the call ends
struct InputBuffers {
  swz_ctx* c = nullptr;
  void* host[2] = {nullptr, nullptr};
  uint8_t* device[2] = {nullptr, nullptr};
  hipEvent_t begin[2] = {nullptr, nullptr}, copied[2] = {nullptr, nullptr}, decoded[2] = {nullptr, nullptr};
  // two images of image_bytes each (one when !two), on the device ("in_image0/1" of ctx's workspace) and page-locked
  int reserve(swz_ctx* ctx, uint64_t image_bytes, bool two);
  ~InputBuffers();
};

// the scanned data set and its cuts into batches
struct LasInputPlan {
  std::vector<swz_las_file_info> files;
  std::vector<uint64_t> counts, file_first;  // points of every file; the data set's point its first record is (one past the end too)
  swz_las_dataset ds{};
  uint32_t mask = 0;
  bool shift = false;
  std::vector<uint64_t> cuts;  // batch j: the points [cuts[j], cuts[j + 1])
  uint64_t num_batches() const { return cuts.size() - 1; }
};

// Scans the headers and refuses what is refused before a point is read: the mask rules (mask_fixed: a batch has fixed the
// columns to mask_now), the 4-ulp box check against [bmin, bmax], more than 2^32 - 65536 points with the points_now a tiler
// holds, FAST's fast_concurrency.  `who` starts the messages; a refusal is c's error.  srs (may be NULL): the source projection;
// the data set's boxes and the centre of the shift are then those of the files' boxes in ECEF (swz_las_scan_files_srs).
int las_input_plan(swz_ctx* c, const char* who, const char* const* paths, uint64_t num_files, const swz_input_params* params,
                   const double bmin[3], const double bmax[3], const swz_tile_params& tp, bool mask_fixed, uint32_t mask_now,
                   uint64_t points_now, const swz_srs* srs, LasInputPlan* plan);
// the image of the points [p0, p1) of the data set: segments with rows from 0, and the pieces the readers take
void las_input_image(const LasInputPlan& plan, uint64_t p0, uint64_t p1, InputBatch* b);
// puts the segment table into the image and starts `threads` reader threads on its pieces (run.wait joins them)
void las_start_read(TicketRun& run, swz_ctx* c, const char* who, const InputBatch* b, unsigned char* image, const char* const* paths,
                    long threads);
// the segment kernel on `stream` for an image that lies on the device (c's device is current); no synchronisation.  srs (may
// be NULL): the instantiation that projects every position to ECEF between clamp and shift
int las_launch_image(swz_ctx* c, hipStream_t stream, const uint8_t* d_image, const InputBatch& b, const double* shift_center,
                     double* d_xyz_out, const swz_attribute_columns* d_out, uint32_t mask, const swz_srs* srs);

}  // namespace swz
