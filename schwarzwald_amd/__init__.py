"""schwarzwald_amd -- MI355X-native implementation of the Schwarzwald tiler hot path.

Morton encode -> radix sort by Morton key -> octree-node partition -> per-node LOD sampling
(RANDOM_GRID / GRID_CENTER / MIN_DISTANCE / JITTERED / MIN_DISTANCE_FAST), written as HIP kernels for gfx950 behind the
C ABI of include/swz_gpu.h.  This Python package is only the ctypes binding of that ABI plus the
multi-GPU sharding driver; there is no CPU implementation in the product.
"""
from .api import (ACCURATE, FLAG_MIN_DISTANCE_PROPERTY, ALWAYS_ADHERE_TO_MIN_SPACING, FAST, GRID_CENTER, JITTERED, MIN_DISTANCE, RANDOM_GRID,
                  SAMPLERS, ALL_SAMPLERS, MIN_DISTANCE_FAST, min_distance_fast_stride, TAKE_ALL_WHEN_COUNT_BELOW_MAX_POINTS, Context, SwzError, TileParams, TileResult,
                  ATTRIBUTES, bin_read_node, bin_write_node, bin_persist_nodes, library_path, load_library, node_bounds,
                  node_from_entwine_name, node_geometric_error, node_name, node_name_entwine,
                  spacing_from_diagonal, Tiler, pinned_empty, tileset_build, tileset_write, pnts_layout, pnts_write_node,
                  pnts_write_node_rows, pnts_read_node, pnts_rgb_from_intensity, PNTS_RGB, PNTS_INTENSITY, RGB_FROM_COLOR,
                  RGB_FROM_INTENSITY_LINEAR, RGB_FROM_INTENSITY_LOG, LAS_NAMING_POTREE, LAS_NAMING_ENTWINE, las_scale_from_bounds,
                  las_record_layout, las_pack_tile, las_image_layout, las_write_node, las_write_node_rows, las_persist_nodes,
                  las_read_header, las_read_node, ept_create_dirs, ept_hierarchy_write, ept_json_write, bin_layout, bin_pack_tile,
                  node_boxes_tile, las_stored_box, OUT_TIGHT_BOUNDS, properties_json_write, properties_json_read, dataset_scan,
                  bin_unpack_tile, pnts_unpack_tile, pnts_parse_image, CONVERT_LOSSY_SOURCE, convert_dataset, convert_dataset_world, box_select_tile, dataset_query_nodes, dataset_query, Region, REGION_BOX, REGION_PLANES, REGION_POLYGON, frustum_planes, dataset_query_region_nodes, dataset_query_region, Filter, FILTER_RANGE, FILTER_SET, FILTER_NOT, dataset_query_filtered, dataset_query_filtered_nodes, dataset_summarize, dataset_summaries_read, dataset_summaries_write, node_summaries_tile, SUMMARY_HAS_NAN, SUMMARY_SCALARS, SUMMARY_DTYPE, raster_tile, raster_frame_of, raster_finish, dataset_rasterize, RASTER_VALUE_Z, RASTER_MAX_CELLS, RASTER_CELL_DTYPE, tileset_oriented_boxes, tileset_write_oriented,
                  DATASET_ROOT_ABSENT, DATASET_ROOT_PROPERTIES, DATASET_ROOT_EPT,
                  bin_persist_nodes_image, output_chunks, merge_shard_node_tables, OUTPUT_FORMATS, las_scan_files, input_batches, las_input_tile,
                  attribute_names, Srs, srs_transform, srs_transform_box, srs_tile, SRS_ECEF, SRS_WGS84, SRS_LONGLAT, SRS_TMERC,
                  LAS_SCAN_SKIP_UNREADABLE, LAS_FILE_OK, LAS_FILE_UNREADABLE, LAS_FILE_BAD_HEADER, LAS_FILE_COMPRESSED)

__all__ = ["properties_json_write", "properties_json_read", "dataset_scan", "bin_unpack_tile", "pnts_unpack_tile", "pnts_parse_image", "CONVERT_LOSSY_SOURCE", "convert_dataset", "convert_dataset_world", "box_select_tile", "dataset_query_nodes", "dataset_query", "Region", "REGION_BOX", "REGION_PLANES", "REGION_POLYGON", "frustum_planes", "dataset_query_region_nodes", "dataset_query_region", "Filter", "FILTER_RANGE", "FILTER_SET", "FILTER_NOT", "dataset_query_filtered", "dataset_query_filtered_nodes", "dataset_summarize", "dataset_summaries_read", "dataset_summaries_write", "node_summaries_tile", "SUMMARY_HAS_NAN", "SUMMARY_SCALARS", "SUMMARY_DTYPE", "raster_tile", "raster_frame_of", "raster_finish", "dataset_rasterize", "RASTER_VALUE_Z", "RASTER_MAX_CELLS", "RASTER_CELL_DTYPE",
           "tileset_oriented_boxes", "tileset_write_oriented", "DATASET_ROOT_ABSENT",
           "DATASET_ROOT_PROPERTIES", "DATASET_ROOT_EPT", "node_boxes_tile", "las_stored_box", "OUT_TIGHT_BOUNDS", "Srs", "srs_transform", "srs_transform_box", "srs_tile", "SRS_ECEF", "SRS_WGS84", "SRS_LONGLAT", "SRS_TMERC", "merge_shard_node_tables", "las_scan_files", "input_batches", "las_input_tile", "attribute_names", "LAS_SCAN_SKIP_UNREADABLE", "LAS_FILE_OK",
           "LAS_FILE_UNREADABLE", "LAS_FILE_BAD_HEADER", "LAS_FILE_COMPRESSED", "bin_layout", "bin_pack_tile", "bin_persist_nodes_image", "output_chunks", "OUTPUT_FORMATS", "LAS_NAMING_POTREE", "LAS_NAMING_ENTWINE", "las_scale_from_bounds", "las_record_layout", "las_pack_tile", "las_image_layout",
           "las_write_node", "las_write_node_rows", "las_persist_nodes", "las_read_header", "las_read_node", "ept_create_dirs",
           "ept_hierarchy_write", "ept_json_write", "tileset_write", "pnts_layout", "pnts_write_node", "pnts_write_node_rows", "pnts_read_node", "pnts_rgb_from_intensity",
           "PNTS_RGB", "PNTS_INTENSITY", "RGB_FROM_COLOR", "RGB_FROM_INTENSITY_LINEAR", "RGB_FROM_INTENSITY_LOG",
           "tileset_build","FLAG_MIN_DISTANCE_PROPERTY", "Context", "Tiler", "pinned_empty", "SwzError", "TileParams", "TileResult", "load_library", "library_path", "SAMPLERS",
           "RANDOM_GRID", "GRID_CENTER", "MIN_DISTANCE", "JITTERED", "ACCURATE", "FAST",
           "MIN_DISTANCE_FAST", "ALL_SAMPLERS", "min_distance_fast_stride",
           "TAKE_ALL_WHEN_COUNT_BELOW_MAX_POINTS", "ALWAYS_ADHERE_TO_MIN_SPACING", "spacing_from_diagonal", "ATTRIBUTES", "bin_write_node", "bin_read_node", "bin_persist_nodes",
           "node_name", "node_name_entwine", "node_from_entwine_name", "node_bounds", "node_geometric_error"]
