// swz_qplan.h -- the node rules of a query (swz_qplan.hip, host only) for the streaming query (swz_query.hip)
#pragma once
#include <vector>

#include "swz_convert.h"
#include "swz_select.h"

namespace swz {

// The table a query reads: `kept` holds the nodes of the (depth-limited) scan whose widened boxes meet the query box and can
// hold a row of the region, in the scan's order; *scanned: the nodes of the scan; *region_out: the region, checked;
// *filter_attrs: the mask of the columns the filter (NULL: none) reads.  No node drops out for a filter here: filter_reads.
int query_plan(swz_ctx* c, const char* who, const char* dir, const swz_query_params* q, const swz_region* region, const swz_filter* filter,
               DatasetScan* kept, uint64_t* scanned, RegionHost* region_out, uint32_t* filter_attrs);

// read->at(k) = 0 for the nodes of `kept` the filter cannot reach; all 1 without a filter or without a sidecar in dir.  A
// sidecar that does not describe the scan is refused.
int filter_reads(swz_ctx* c, const char* who, const char* dir, const DatasetScan& kept, const swz_filter* filter,
                 std::vector<uint8_t>* read);

}  // namespace swz
