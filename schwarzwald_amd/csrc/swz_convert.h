// swz_convert.h -- what the parts of swz_convert_dataset share: the scanned source (swz_dataset.hip), the launch of the BIN
// unpack kernel on a stream (swz_binunpack.hip) and the call itself (swz_convert.hip).
#pragma once
#include <string>
#include <vector>

#include "swz_internal.h"

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
  std::vector<uint64_t> file_bytes;    // 3DTILES sources, filled by swz_convert_dataset: the size of the file
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

}  // namespace swz
