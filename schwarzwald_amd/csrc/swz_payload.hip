// swz_payload.hip -- node lists on the device, the permuted payload gather, and BinaryPersistence node files
// (reference: core/io/BinaryPersistence.h:45-193, BinaryPersistence.cpp:200-375,
// core/tiling/TilingAlgorithms.cpp:139, 232-236).
#include <cmath>
#include <cstdio>
#include <cstring>
#include <algorithm>
#include <map>
#include <string>
#include <vector>

#include "swz_internal.h"
#include "swz_device.h"
#include "swz_hostio.h"

namespace swz {

// (ATTR_BYTES and FILE_ORDER, the attribute arrays of a node file: swz_hostio.h)
// ---------------------------------------------------------------------------------- node lists
__global__ __launch_bounds__(256) void level_key_kernel(const int8_t* __restrict__ level, uint32_t n, uint64_t* __restrict__ out,
                                                        uint32_t* __restrict__ bad) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int l = level[i];
  if (l < -1 || l > 20) atomicAdd(bad, 1u);
  out[i] = (uint64_t)(uint8_t)(l + 1) << 56;  // the stable partition looks at the top byte only
}

// position i of the level-grouped order starts a node: first of its level, or another key prefix
__global__ __launch_bounds__(256) void node_head_kernel(const uint32_t* __restrict__ order, const uint64_t* __restrict__ keys,
                                                        const int8_t* __restrict__ level, uint32_t n, uint32_t* __restrict__ flags) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const uint32_t p = order[i];
  const int l = level[p];
  bool head = i == 0;
  if (!head) {
    const uint32_t q = order[i - 1];
    head = level[q] != l || (l >= 0 && (keys[q] >> level_shift(l)) != (keys[p] >> level_shift(l)));
  }
  flags[i] = head ? 1u : 0u;
}

__global__ __launch_bounds__(256) void node_table_kernel(const uint32_t* __restrict__ order, const uint64_t* __restrict__ keys,
                                                         const int8_t* __restrict__ level, uint32_t n,
                                                         const uint32_t* __restrict__ excl, uint32_t max_nodes,
                                                         int8_t* __restrict__ nlevel, uint64_t* __restrict__ nkey,
                                                         uint64_t* __restrict__ noffset) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const uint32_t p = order[i];
  const int l = level[p];
  bool head = i == 0;
  if (!head) {
    const uint32_t q = order[i - 1];
    head = level[q] != l || (l >= 0 && (keys[q] >> level_shift(l)) != (keys[p] >> level_shift(l)));
  }
  if (!head) return;
  const uint32_t k = excl[i];
  if (k >= max_nodes) return;
  nlevel[k] = (int8_t)l;
  nkey[k] = l < 0 ? 0ull : ((keys[p] >> level_shift(l)) << level_shift(l));
  noffset[k] = i;
}

// ---------------------------------------------------------------------------------- payload gather
__global__ __launch_bounds__(256) void compose_kernel(const uint32_t* __restrict__ perm, const uint32_t* __restrict__ order,
                                                      uint32_t n, uint32_t* __restrict__ src) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) src[i] = perm[order ? order[i] : i];
}

// rows of K elements of T; one thread per row (rows are at most 24 bytes)
template <typename T, int K>
__global__ __launch_bounds__(256) void gather_rows_kernel(const T* __restrict__ in, const uint32_t* __restrict__ src, uint32_t n,
                                                          T* __restrict__ out) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const T* r = in + (size_t)src[i] * K;
  T v[K];
#pragma unroll
  for (int j = 0; j < K; ++j) v[j] = r[j];
#pragma unroll
  for (int j = 0; j < K; ++j) out[(size_t)i * K + j] = v[j];
}

template <typename T, int K>
static void launch_gather(swz_ctx* c, const void* in, const uint32_t* src, uint32_t n, void* out) {
  hipLaunchKernelGGL((gather_rows_kernel<T, K>), dim3(div_up(n, 256)), dim3(256), 0, c->stream, (const T*)in, src, n, (T*)out);
}

// ---------------------------------------------------------------------------------- node files
static int read_file(swz_ctx* c, const char* path, int compressed, std::vector<unsigned char>& out, size_t want_at_most) {
  std::vector<unsigned char> raw;
  SWZ_TRY(read_whole_file(c, path, &raw));
  if (!compressed) {
    out.swap(raw);
    return SWZ_OK;
  }
  unsigned char tmp[1 << 16];
  z_stream zs;
  memset(&zs, 0, sizeof(zs));
  if (inflateInit(&zs) != Z_OK) return fail(c, SWZ_ERR_INTERNAL, "inflateInit failed");
  zs.next_in = raw.data();
  zs.avail_in = (uInt)raw.size();
  int rc = Z_OK;
  out.clear();
  while (rc != Z_STREAM_END && out.size() < want_at_most) {
    zs.next_out = tmp;
    zs.avail_out = sizeof(tmp);
    rc = inflate(&zs, Z_NO_FLUSH);
    if (rc != Z_OK && rc != Z_STREAM_END) {
      inflateEnd(&zs);
      return fail(c, SWZ_ERR_BAD_ARG, std::string("corrupt zlib stream in ") + path);
    }
    out.insert(out.end(), tmp, tmp + (sizeof(tmp) - zs.avail_out));
  }
  inflateEnd(&zs);
  return SWZ_OK;
}

}  // namespace swz

using namespace swz;

extern "C" {

uint32_t swz_attribute_row_bytes(int attribute) {
  return (attribute >= 0 && attribute < SWZ_ATTR_COUNT) ? ATTR_BYTES[attribute] : 0u;
}

int swz_build_node_lists_device(swz_ctx* c, const uint64_t* d_keys_sorted, const int8_t* d_level, uint64_t n,
                                uint32_t* d_order_out, uint64_t max_nodes, int8_t* node_level_out, uint64_t* node_key_out,
                                uint64_t* node_offset_out, uint64_t* node_count_out, uint64_t* num_nodes_out) {
  if (!c || !num_nodes_out) return SWZ_ERR_BAD_ARG;
  SWZ_HIP(c, hipSetDevice(c->device));
  *num_nodes_out = 0;
  if (n == 0) return SWZ_OK;
  if (n > 0xFFFFFFFFull) return c->fail(SWZ_ERR_BAD_ARG, "more than 2^32-1 points in one batch");
  if (!d_keys_sorted || !d_level || !d_order_out) return c->fail(SWZ_ERR_BAD_ARG, "swz_build_node_lists_device: NULL buffer");
  const uint32_t m = (uint32_t)n;
  const uint32_t nb = div_up(m, 256);
  uint64_t* lkeys = nullptr;
  uint32_t *flags = nullptr, *cnt = nullptr;
  SWZ_TRY(c->get("nl_keys", (size_t)m, &lkeys));
  SWZ_TRY(c->get("nl_flags", (size_t)m, &flags));
  SWZ_TRY(c->get("nl_cnt", (size_t)2, &cnt));
  SWZ_HIP(c, hipMemsetAsync(cnt, 0, 8, c->stream));
  hipLaunchKernelGGL(level_key_kernel, dim3(nb), dim3(256), 0, c->stream, d_level, m, lkeys, cnt);
  SWZ_LAUNCH_CHECK(c);
  uint32_t starts[256];
  SWZ_TRY(partition_by_top_byte(c, lkeys, m, d_order_out, starts));
  hipLaunchKernelGGL(node_head_kernel, dim3(nb), dim3(256), 0, c->stream, d_order_out, d_keys_sorted, d_level, m, flags);
  SWZ_LAUNCH_CHECK(c);
  SWZ_TRY(scan_exclusive_u32(c, flags, flags, m, cnt + 1, "nl"));
  uint32_t h[2] = {0, 0};
  SWZ_HIP(c, hipMemcpyAsync(h, cnt, 8, hipMemcpyDeviceToHost, c->stream));
  SWZ_HIP(c, hipStreamSynchronize(c->stream));
  if (h[0]) return c->fail(SWZ_ERR_BAD_ARG, "level out of range");
  const uint64_t nn = h[1];
  *num_nodes_out = nn;
  if (nn > max_nodes) return c->fail(SWZ_ERR_BAD_ARG, "max_nodes too small");
  if (!node_level_out || !node_key_out || !node_offset_out || !node_count_out) return SWZ_OK;
  int8_t* dl = nullptr;
  uint64_t *dk = nullptr, *doff = nullptr;
  SWZ_TRY(c->get("nl_level", (size_t)nn, &dl));
  SWZ_TRY(c->get("nl_key", (size_t)nn, &dk));
  SWZ_TRY(c->get("nl_off", (size_t)nn, &doff));
  hipLaunchKernelGGL(node_table_kernel, dim3(nb), dim3(256), 0, c->stream, d_order_out, d_keys_sorted, d_level, m, flags,
                     (uint32_t)nn, dl, dk, doff);
  SWZ_LAUNCH_CHECK(c);
  SWZ_HIP(c, hipMemcpyAsync(node_level_out, dl, nn, hipMemcpyDeviceToHost, c->stream));
  SWZ_HIP(c, hipMemcpyAsync(node_key_out, dk, nn * 8, hipMemcpyDeviceToHost, c->stream));
  SWZ_HIP(c, hipMemcpyAsync(node_offset_out, doff, nn * 8, hipMemcpyDeviceToHost, c->stream));
  SWZ_HIP(c, hipStreamSynchronize(c->stream));
  for (uint64_t k = 0; k < nn; ++k) node_count_out[k] = (k + 1 < nn ? node_offset_out[k + 1] : n) - node_offset_out[k];
  return SWZ_OK;
}

int swz_gather_payload_device(swz_ctx* c, const uint32_t* d_perm, const uint32_t* d_order, uint64_t n, const double* d_xyz,
                              const swz_attribute_columns* d_in, double* d_xyz_out, const swz_attribute_columns* d_out) {
  if (!c) return SWZ_ERR_BAD_ARG;
  SWZ_HIP(c, hipSetDevice(c->device));
  if (n == 0) return SWZ_OK;
  if (n > 0xFFFFFFFFull) return c->fail(SWZ_ERR_BAD_ARG, "more than 2^32-1 points in one batch");
  if (!d_perm) return c->fail(SWZ_ERR_BAD_ARG, "swz_gather_payload_device: NULL perm");
  if ((d_xyz == nullptr) != (d_xyz_out == nullptr)) return c->fail(SWZ_ERR_BAD_ARG, "positions need input and output");
  const uint32_t m = (uint32_t)n;
  uint32_t* src = nullptr;
  SWZ_TRY(c->get("payload_src", (size_t)m, &src));
  uint64_t bytes = 12ull * n;  // perm + order read, composed index written
  hipLaunchKernelGGL(compose_kernel, dim3(div_up(m, 256)), dim3(256), 0, c->stream, d_perm, d_order, m, src);
  SWZ_LAUNCH_CHECK(c);
  {
    ProfScope ps(c, "payload_gather", 0, 1);
    if (d_xyz) {
      launch_gather<double, 3>(c, d_xyz, src, m, d_xyz_out);
      bytes += 52ull * n;
    }
    for (int a = 0; a < SWZ_ATTR_COUNT; ++a) {
      const void* in = d_in ? d_in->column[a] : nullptr;
      void* out = d_out ? d_out->column[a] : nullptr;
      if (!in || !out) continue;
      switch (ATTR_BYTES[a]) {
        case 3: launch_gather<uint8_t, 3>(c, in, src, m, out); break;
        case 12: launch_gather<float, 3>(c, in, src, m, out); break;
        case 2: launch_gather<uint16_t, 1>(c, in, src, m, out); break;
        case 8: launch_gather<double, 1>(c, in, src, m, out); break;
        default: launch_gather<uint8_t, 1>(c, in, src, m, out); break;
      }
      bytes += (4ull + 2ull * ATTR_BYTES[a]) * n;
    }
    SWZ_LAUNCH_CHECK(c);
    ps.bytes = bytes;
  }
  SWZ_HIP(c, hipStreamSynchronize(c->stream));
  return SWZ_OK;
}

int swz_node_name(int8_t node_level, uint64_t node_key, char* name_out) {
  if (!name_out || node_level < -1 || node_level > 20) return SWZ_ERR_BAD_ARG;
  int k = 0;
  name_out[k++] = 'r';
  for (int l = 0; l <= node_level; ++l) name_out[k++] = (char)('0' + ((node_key >> level_shift(l)) & 7u));
  name_out[k] = 0;
  return SWZ_OK;
}

int swz_node_name_entwine(int8_t node_level, uint64_t node_key, char* name_out) {
  if (!name_out || node_level < -1 || node_level > 20) return SWZ_ERR_BAD_ARG;
  uint64_t x = 0, y = 0, z = 0;
  for (int l = 0; l <= node_level; ++l) {
    const uint32_t o = (uint32_t)(node_key >> level_shift(l)) & 7u;
    x = (x << 1) | ((o >> 2) & 1u);
    y = (y << 1) | ((o >> 1) & 1u);
    z = (z << 1) | (o & 1u);
  }
  snprintf(name_out, 72, "%d-%llu-%llu-%llu", node_level + 1, (unsigned long long)x, (unsigned long long)y,
           (unsigned long long)z);
  return SWZ_OK;
}

int swz_node_from_entwine_name(const char* name, int8_t* node_level_out, uint64_t* node_key_out) {
  if (!name || !node_level_out || !node_key_out) return SWZ_ERR_BAD_ARG;
  unsigned long long d = 0, x = 0, y = 0, z = 0;
  char tail = 0;
  if (sscanf(name, "%llu-%llu-%llu-%llu%c", &d, &x, &y, &z, &tail) != 4) return SWZ_ERR_BAD_ARG;
  if (d > 21) return SWZ_ERR_BAD_ARG;  // more levels than a 64-bit index holds (OctreeNodeIndex64)
  if (d < 64 && ((x >> d) || (y >> d) || (z >> d))) return SWZ_ERR_BAD_ARG;
  uint64_t key = 0;
  for (unsigned l = 0; l < d; ++l) {
    const unsigned b = (unsigned)d - 1u - l;
    const uint64_t o = (((x >> b) & 1ull) << 2) | (((y >> b) & 1ull) << 1) | ((z >> b) & 1ull);
    key |= o << level_shift((int)l);
  }
  *node_level_out = (int8_t)((int)d - 1);
  *node_key_out = key;
  return SWZ_OK;
}

int swz_node_bounds(int8_t node_level, uint64_t node_key, const double root_min[3], const double root_max[3],
                    double min_out[3], double max_out[3]) {
  if (!root_min || !root_max || !min_out || !max_out || node_level < -1 || node_level > 20) return SWZ_ERR_BAD_ARG;
  double mn[3] = {root_min[0], root_min[1], root_min[2]}, mx[3] = {root_max[0], root_max[1], root_max[2]};
  for (int l = 0; l <= node_level; ++l) {
    const uint32_t o = (uint32_t)(node_key >> level_shift(l)) & 7u;
    const uint32_t bit[3] = {(o >> 2) & 1u, (o >> 1) & 1u, o & 1u};
    for (int ax = 0; ax < 3; ++ax) {  // get_octant_bounds: min (+ extent / 2), max = min + extent / 2
      const double e = mx[ax] - mn[ax];
      if (bit[ax]) mn[ax] = mn[ax] + e / 2;
      mx[ax] = mn[ax] + e / 2;
    }
  }
  for (int ax = 0; ax < 3; ++ax) {
    min_out[ax] = mn[ax];
    max_out[ax] = mx[ax];
  }
  return SWZ_OK;
}

double swz_node_geometric_error(int8_t node_level, float spacing_at_root) {
  return spacing_at_root / std::pow(2.0, (double)(node_level + 1));
}

// Cesium3DTilesPersistence::on_write_node (core/io/Cesium3DTilesPersistence.cpp:80-156): every written node makes a
// Tileset for itself and for every ancestor that has none yet; name, geometricError = spacing_at_root / 2^depth
// (:91-92), bounds by descending from the root box octant by octant (:100-112, 136) translated by the global offset
// (:88); write_tilesets (:175-199) starts a new tileset.json every MAX_DEPTH + 1 = 3 levels.  The reference keeps
// children in the order its worker threads happened to write them; here they are ordered by octant.
int swz_tileset_build(uint64_t num_nodes, const int8_t* node_level, const uint64_t* node_key, const double root_min[3],
                      const double root_max[3], float spacing_at_root, const double global_offset[3], uint64_t max_out,
                      swz_tileset_node* out, uint64_t* num_out) {
  if (!num_out || (num_nodes && (!node_level || !node_key)) || !root_min || !root_max) return SWZ_ERR_BAD_ARG;
  *num_out = 0;
  // all nodes and their ancestors, keyed by (level, prefix): std::map iterates in (level, key) order
  std::map<std::pair<int, uint64_t>, uint8_t> all;
  for (uint64_t j = 0; j < num_nodes; ++j) {
    const int lv = node_level[j];
    if (lv < -1 || lv > 20) return SWZ_ERR_BAD_ARG;
    for (int l = lv; l >= -1; --l) {
      const uint64_t key = l < 0 ? 0ull : ((node_key[j] >> level_shift(l)) << level_shift(l));
      uint8_t& flag = all[{l, key}];
      if (l == lv) {
        flag = 1;
      } else if (all.size() == 0) {
        break;
      }
    }
  }
  const uint64_t total = all.size();
  *num_out = total;
  if (!out) return SWZ_OK;
  if (total > max_out) return SWZ_ERR_BAD_ARG;
  std::map<std::pair<int, uint64_t>, uint64_t> index;
  uint64_t k = 0;
  for (const auto& kv : all) index[kv.first] = k++;
  k = 0;
  for (const auto& kv : all) {
    swz_tileset_node& t = out[k];
    std::memset(&t, 0, sizeof(t));
    const int lv = kv.first.first;
    t.level = (int8_t)lv;
    t.key = kv.first.second;
    t.has_content = kv.second;
    t.parent = -1;
    t.first_child = -1;
    if (lv >= 0) {
      const uint64_t pkey = lv == 0 ? 0ull : ((t.key >> level_shift(lv - 1)) << level_shift(lv - 1));
      const uint64_t p = index[{lv - 1, pkey}];
      t.parent = (int64_t)p;
      if (out[p].first_child < 0) out[p].first_child = (int64_t)k;  // (level, key) order: children are contiguous
      out[p].num_children += 1;
    }
    t.is_tileset_root = ((lv + 1) % 3 == 0) ? 1 : 0;
    t.geometric_error = swz_node_geometric_error((int8_t)lv, spacing_at_root);
    swz_node_bounds((int8_t)lv, t.key, root_min, root_max, t.bounds_min, t.bounds_max);
    for (int ax = 0; ax < 3; ++ax) {  // AABB::translate(_global_offset), :88
      const double off = global_offset ? global_offset[ax] : 0.0;
      t.bounds_min[ax] += off;
      t.bounds_max[ax] += off;
    }
    ++k;
  }
  return SWZ_OK;
}

}  // extern "C"

// one node file (BinaryPersistence::persist_points, BinaryPersistence.h:46-57 / .cpp): bitmask, count, positions, then the
// attribute columns in file order.  No context: the files of a batch are written by several threads (swz_bin_persist_nodes).
static int bin_write_node_impl(const char* path, uint64_t count, const double* xyz, const swz_attribute_columns* columns, int compressed,
                               std::string* err) {
  uint32_t bitmask = 0;
  for (int a = 0; a < SWZ_ATTR_COUNT; ++a)
    if (columns && columns->column[a]) bitmask |= 1u << a;
  // (the pieces go out as they lie in the caller's arrays: a node file is its header and slices of the columns)
  std::vector<FilePiece> pieces = {{&bitmask, 4}, {&count, 8}, {xyz, (size_t)count * 24}};
  for (int k = 0; k < SWZ_ATTR_COUNT; ++k) {
    const int a = FILE_ORDER[k];
    if (bitmask & (1u << a)) pieces.push_back({columns->column[a], (size_t)count * ATTR_BYTES[a]});
  }
  if (!compressed) return write_file(path, pieces, err);
  std::vector<unsigned char> plain;
  for (const FilePiece& p : pieces) plain.insert(plain.end(), (const unsigned char*)p.data, (const unsigned char*)p.data + p.bytes);
  return write_file_zlib(path, plain.data(), plain.size(), err);
}

extern "C" {

int swz_bin_write_node(swz_ctx* c, const char* path, uint64_t count, const double* xyz, const swz_attribute_columns* columns,
                       int compressed) {
  if (!path) return fail(c, SWZ_ERR_BAD_ARG, "swz_bin_write_node: NULL path");
  if (count == 0) return SWZ_OK;  // persist_points returns before opening the file
  if (!xyz) return fail(c, SWZ_ERR_BAD_ARG, "swz_bin_write_node: NULL positions");
  std::string err;
  const int st = bin_write_node_impl(path, count, xyz, columns, compressed, &err);
  return st == SWZ_OK ? SWZ_OK : fail(c, st, err);
}

int swz_bin_read_header(swz_ctx* c, const char* path, int compressed, uint32_t* bitmask_out, uint64_t* count_out) {
  if (!path || !bitmask_out || !count_out) return fail(c, SWZ_ERR_BAD_ARG, "swz_bin_read_header: NULL argument");
  std::vector<unsigned char> data;
  const int st = read_file(c, path, compressed, data, compressed ? 12 : (size_t)-1);
  if (st != SWZ_OK) return st;
  if (data.size() < 12) return fail(c, SWZ_ERR_BAD_ARG, std::string("truncated node file ") + path);
  memcpy(bitmask_out, data.data(), 4);
  memcpy(count_out, data.data() + 4, 8);
  return SWZ_OK;
}

int swz_bin_read_node(swz_ctx* c, const char* path, int compressed, double* xyz_out, const swz_attribute_columns* columns_out) {
  if (!path) return fail(c, SWZ_ERR_BAD_ARG, "swz_bin_read_node: NULL path");
  std::vector<unsigned char> data;
  const int st = read_file(c, path, compressed, data, (size_t)-1);
  if (st != SWZ_OK) return st;
  if (data.size() < 12) return fail(c, SWZ_ERR_BAD_ARG, std::string("truncated node file ") + path);
  uint32_t bitmask;
  uint64_t count;
  memcpy(&bitmask, data.data(), 4);
  memcpy(&count, data.data() + 4, 8);
  size_t need = 12 + (size_t)count * 24;
  for (int a = 0; a < SWZ_ATTR_COUNT; ++a)
    if (bitmask & (1u << a)) need += (size_t)count * ATTR_BYTES[a];
  if (data.size() < need) return fail(c, SWZ_ERR_BAD_ARG, std::string("truncated node file ") + path);
  size_t at = 12;
  if (xyz_out) memcpy(xyz_out, data.data() + at, (size_t)count * 24);
  at += (size_t)count * 24;
  for (int k = 0; k < SWZ_ATTR_COUNT; ++k) {
    const int a = FILE_ORDER[k];
    if (!(bitmask & (1u << a))) continue;
    if (columns_out && columns_out->column[a]) memcpy(columns_out->column[a], data.data() + at, (size_t)count * ATTR_BYTES[a]);
    at += (size_t)count * ATTR_BYTES[a];
  }
  return SWZ_OK;
}

int swz_bin_persist_nodes(swz_ctx* c, const char* dir, uint64_t num_nodes, const int8_t* node_level, const uint64_t* node_key,
                          const uint64_t* node_offset, const uint64_t* node_count, const double* xyz,
                          const swz_attribute_columns* columns, int compressed) {
  if (!dir || (num_nodes && (!node_level || !node_key || !node_offset || !node_count || !xyz)))
    return fail(c, SWZ_ERR_BAD_ARG, "swz_bin_persist_nodes: NULL argument");
  for (uint64_t k = 0; k < num_nodes; ++k) {
    char name[24];
    if (swz_node_name(node_level[k], node_key[k], name) != SWZ_OK) return fail(c, SWZ_ERR_BAD_ARG, "bad node level");
  }
  std::string first_err;
  const int st = run_tickets(c, num_nodes, [&](uint64_t k, std::string* err) {
    if (node_count[k] == 0) return (int)SWZ_OK;  // persist_points returns before opening the file
    char name[24];
    (void)swz_node_name(node_level[k], node_key[k], name);
    const std::string path = std::string(dir) + "/" + name + (compressed ? ".binz" : ".bin");
    swz_attribute_columns cols;
    for (int a = 0; a < SWZ_ATTR_COUNT; ++a)
      cols.column[a] = (columns && columns->column[a])
                         ? (void*)((unsigned char*)columns->column[a] + (size_t)node_offset[k] * ATTR_BYTES[a])
                         : nullptr;
    return bin_write_node_impl(path.c_str(), node_count[k], xyz + (size_t)node_offset[k] * 3, &cols, compressed, err);
  }, &first_err);
  return st == SWZ_OK ? SWZ_OK : fail(c, st, first_err);
}

}  // extern "C"

// ---------------------------------------------------------------------------------- LAS point records (F2)
#include "swz_lasrec.h"

namespace swz {

constexpr int LAS_POINTS_PER_BLOCK = 256;
constexpr int LAS_MAX_RECORD = 96;  // staged through LDS; longer records (many extra bytes) are read directly

// the field mapping of a record: las_unpack, swz_lasrec.h

__global__ __launch_bounds__(LAS_POINTS_PER_BLOCK) void las_decode_kernel(const uint8_t* __restrict__ rec, uint32_t n, LasArgs a) {
  __shared__ uint32_t stage[LAS_POINTS_PER_BLOCK * LAS_MAX_RECORD / 4];
  const uint32_t first = blockIdx.x * LAS_POINTS_PER_BLOCK;
  const uint32_t cnt = min((uint32_t)LAS_POINTS_PER_BLOCK, n - first);
  const uint32_t i = first + threadIdx.x;
  if (a.record_bytes <= (uint32_t)LAS_MAX_RECORD && (a.record_bytes & 1u) == 0) {
    // the block's records are one contiguous, 4-byte aligned run (256 x an even length): coalesced word loads
    const size_t byte0 = (size_t)first * a.record_bytes;
    const uint32_t bytes = cnt * a.record_bytes, words = bytes / 4u;
    const uint32_t* src = reinterpret_cast<const uint32_t*>(rec + byte0);
    for (uint32_t w = threadIdx.x; w < words; w += LAS_POINTS_PER_BLOCK) stage[w] = src[w];
    if (threadIdx.x < (bytes & 3u))  // the last block may end in a partial word: no read past the buffer
      reinterpret_cast<uint8_t*>(stage)[words * 4u + threadIdx.x] = rec[byte0 + words * 4u + threadIdx.x];
    __syncthreads();
    if (threadIdx.x < cnt) las_unpack(a, reinterpret_cast<const uint8_t*>(stage) + (size_t)threadIdx.x * a.record_bytes, i);
  } else if (threadIdx.x < cnt) {
    las_unpack(a, rec + (size_t)i * a.record_bytes, i);
  }
}

}  // namespace swz

extern "C" int swz_las_decode_device(swz_ctx* c, const uint8_t* d_records, uint64_t n, const swz_las_layout* layout,
                                     double* d_xyz_out, const swz_attribute_columns* d_out) {
  if (!c) return SWZ_ERR_BAD_ARG;
  SWZ_HIP(c, hipSetDevice(c->device));
  if (!layout) return c->fail(SWZ_ERR_BAD_ARG, "swz_las_decode_device: NULL layout");
  static const uint32_t kMinBytes[11] = {20, 28, 26, 34, 57, 63, 30, 36, 38, 59, 67};
  if (layout->point_format > 10) return c->fail(SWZ_ERR_BAD_ARG, "LAS point data record formats 0-10 are decoded");
  if (layout->record_bytes < kMinBytes[layout->point_format])
    return c->fail(SWZ_ERR_BAD_ARG, "record length shorter than the point format");
  if (n == 0) return SWZ_OK;
  if (n > 0xFFFFFFFFull) return c->fail(SWZ_ERR_BAD_ARG, "more than 2^32-1 points in one batch");
  if (!d_records) return c->fail(SWZ_ERR_BAD_ARG, "swz_las_decode_device: NULL records");
  if (((uintptr_t)d_records & 3u) != 0) return c->fail(SWZ_ERR_BAD_ARG, "records must be 4-byte aligned");
  swz::LasArgs a{};
  uint64_t out_bytes = d_xyz_out ? 24 : 0;
  for (int k = 0; k < 3; ++k) {
    a.scale[k] = layout->scale[k];
    a.offset[k] = layout->offset[k];
    a.mn[k] = layout->min[k];
    a.mx[k] = layout->max[k];
  }
  a.format = layout->point_format;
  a.record_bytes = layout->record_bytes;
  a.xyz = d_xyz_out;
  for (int k = 0; k < SWZ_ATTR_COUNT; ++k) {
    a.col[k] = (d_out && k != SWZ_ATTR_NORMAL) ? d_out->column[k] : nullptr;  // LAS points carry no normals
    if (a.col[k]) out_bytes += swz::ATTR_BYTES[k];
  }
  swz::ProfScope ps(c, "las_decode", (uint64_t)n * (layout->record_bytes + out_bytes), 1);
  hipLaunchKernelGGL(swz::las_decode_kernel, dim3(swz::div_up((uint32_t)n, swz::LAS_POINTS_PER_BLOCK)),
                     dim3(swz::LAS_POINTS_PER_BLOCK), 0, c->stream, d_records, (uint32_t)n, a);
  SWZ_LAUNCH_CHECK(c);
  SWZ_HIP(c, hipStreamSynchronize(c->stream));
  return SWZ_OK;
}
