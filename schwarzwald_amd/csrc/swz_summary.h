// swz_summary.h -- per-node attribute summaries (swz_summary.hip) for the callers inside the library: the reduction of a
// chunk's columns, which swz_dataset_summarize runs chunk by chunk, and the sidecar file node-summaries.swz, which the node
// rule of the filtered query reads (swz_qplan.hip).
#pragma once
#include <limits>
#include <string>
#include <vector>

#include "swz_internal.h"

namespace swz {

constexpr uint32_t SUMMARY_MAX_COLS = 10;  // the scalar columns: popcount(SWZ_SUMMARY_SCALARS)

// an entry as the host presets it: no value yet
inline swz_attr_summary summary_empty() {
  swz_attr_summary e{};
  e.lo = std::numeric_limits<double>::infinity();
  e.hi = -std::numeric_limits<double>::infinity();
  return e;
}

// swz_node_summaries_device in `who`'s name.  Synchronises c's stream.
int node_summaries(swz_ctx* c, const char* who, uint64_t n, const swz_attribute_columns* d_in, uint32_t mask, uint64_t num_nodes,
                   const uint64_t* node_offset, const uint64_t* node_count, swz_attr_summary* out);

// node-summaries.swz of a directory as swz_dataset_summaries_read checks it
struct Sidecar {
  bool present = false;
  int32_t format = 0;
  uint32_t mask = 0, cols = 0;  // cols: popcount(mask)
  uint64_t points = 0;
  std::vector<int8_t> level;
  std::vector<uint64_t> key, count;
  std::vector<swz_attr_summary> entries;  // nodes x cols
};
// what is wrong goes to *why (no context: host only); a directory without the file is SWZ_OK with present == false
int sidecar_read(const std::string& dir, Sidecar* out, std::string* why);
int sidecar_write(const std::string& dir, int32_t format, uint32_t mask, uint64_t num_nodes, const int8_t* level, const uint64_t* key,
                  const uint64_t* count, const swz_attr_summary* entries, std::string* why);

}  // namespace swz
