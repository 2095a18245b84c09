// swz_tinput.h -- the parts of a data set of LAS files read in one call (swz_tinput.hip): scan, refuse and cut
// (las_input_plan), the raw image of a run of points of the data set (las_input_image), its reader threads
// (las_start_read), the segment kernel on a stream (las_launch_image), the two images of a call on one device
// (InputBuffers), and the loop that drives them (las_input_stream) over what every device contributes (InputLane).
// swz_tiler_add_las_files (swz_tinput.hip) runs the loop over one lane, swz_group_add_las_files (swz_gtiler.hip) over one
// lane per shard; what differs between them is an InputStreamOps.
#pragma once
#include <functional>

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

// What one device contributes to a streamed call: its context, the stream its images are copied and decoded on, its images
// and, per batch, the run of points it reads -- the whole batch, or a shard's slice of it.
struct InputLane {
  swz_ctx* c = nullptr;
  hipStream_t copy = nullptr;
  InputBuffers ib;
  std::vector<InputBatch> batches;
  uint64_t image_max = 0, rows_max = 0;  // the largest image and the most rows of a batch
  TicketRun readers;
  double read_ms = 0, copy_ms = 0, decode_ms = 0;
  // the r-th of `of` consecutive slices of every batch of the plan
  void cut(const LasInputPlan& plan, int r, int of);
};

// where a lane decodes a batch to: the rows of its positions and columns on the device, and the columns to fill
struct InputTarget { double* xyz; swz_attribute_columns cols; uint32_t mask; };
// What differs between the callers of las_input_stream.  A callback that fails returns its status and puts its text into *why.
struct InputStreamOps {
  const char* lane_name = nullptr;  // "shard": a failure on lane r reads "shard r: ..." (NULL: the lanes are not named)
  std::function<InputTarget(int r)> target;  // where lane r decodes the batch that is staged next
  // every lane's copy and decode of batch j are on their streams: the batch is staged
  std::function<int(uint64_t j, std::string* why)> commit;
  // tiles the oldest staged batch; *waited_ms: how much of the call stood waiting for the batch's copy
  std::function<int(double* waited_ms, std::string* why)> tile;
};

// How far a stream got and what it did; filled on failure as well.
struct InputStreamResult {
  int status = SWZ_OK;
  std::string why;
  bool enqueued = false;  // the first batch's copy and decode were attempted: `target` rows may have been written
  bool tiled = false;     // the first batch was handed to `tile`
  uint64_t batches = 0, points = 0, bytes_read = 0;     // batches tiled, their points; bytes read, summed over the lanes
  double read_ms = 0, copy_ms = 0, decode_ms = 0;       // the largest lane's
  double tile_ms = 0, wait_ms = 0;                      // tiling without, waiting with what `tile` reported as waited
  void fill(swz_input_stats* s, uint64_t files, double wall_ms) const {
    *s = swz_input_stats{files, points, batches, bytes_read, read_ms, copy_ms, decode_ms, tile_ms, wait_ms, wall_ms};
  }
};

// The streamed call, once: reads run two batches ahead of the tiling, copy + decode one.  While batch k is tiled, batch
// k + 1 is copied and decoded on every lane's stream and the readers fill the other host images with batch k + 2, whose read
// starts only when every lane's copy of batch k has left them.  The first failure wins and stops the stream after the batch
// that is staged (a read that fails for batch k + 1 still lets batch k be tiled); a failure of `tile` is reported in its
// place.  SWZ_INPUT_READER_THREADS (default: the host's threads, at most 32) is the budget of the whole call, shared out
// over the lanes, every lane at least one.  On every exit the readers are joined and the lanes' streams idle.
void las_input_stream(const LasInputPlan& plan, const swz_srs* srs, const char* who, const char* const* paths, std::vector<InputLane>& lanes,
                      const InputStreamOps& ops, InputStreamResult* result);

}  // namespace swz
