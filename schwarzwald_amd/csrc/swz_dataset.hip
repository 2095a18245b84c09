// swz_dataset.hip -- a written data set found again (host only): properties.json as the reference writes and parses it
// (write_properties_json, core/process/TilerProcess.cpp:76-151; parse_properties_json / parse_ept_json,
// core/process/ConverterProcess.cpp:55-143) and the scan of a directory of node files (find_all_octree_node_files,
// :296-323): format, node table, counts, attribute mask, root box and spacing.  swz_convert_dataset (swz_convert.hip) starts
// from here.
#include <dirent.h>
#include <sys/stat.h>

#include <algorithm>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "swz_convert.h"
#include "swz_device.h"
#include "swz_hostio.h"
#include "swz_tiler.h"

namespace swz {

// ---------------------------------------------------------------------------------- the numbers of a JSON text
// Every number of the document under its path ("source_properties.bounds.min[0]"); strings, booleans and nulls are passed
// over.  false: not JSON.
struct JsonNumbers {
  const char* p;
  const char* end;
  std::map<std::string, double> numbers;
  int depth = 0;

  void space() {
    while (p < end && (*p == ' ' || *p == '\t' || *p == '\n' || *p == '\r')) ++p;
  }
  bool string(std::string* out) {
    if (p >= end || *p != '"') return false;
    for (++p; p < end && *p != '"'; ++p) {
      if (*p == '\\' && ++p >= end) return false;
      if (out) out->push_back(*p);
    }
    if (p >= end) return false;
    ++p;
    return true;
  }
  bool value(const std::string& path) {
    if (++depth > 64) return false;
    space();
    if (p >= end) return false;
    bool ok = true;
    if (*p == '{') {
      ++p;
      space();
      if (p < end && *p == '}') {
        ++p;
      } else {
        for (;;) {
          std::string name;
          space();
          if (!string(&name)) return false;
          space();
          if (p >= end || *p++ != ':') return false;
          if (!value(path.empty() ? name : path + "." + name)) return false;
          space();
          if (p < end && *p == ',') {
            ++p;
            continue;
          }
          if (p < end && *p == '}') {
            ++p;
            break;
          }
          return false;
        }
      }
    } else if (*p == '[') {
      ++p;
      space();
      if (p < end && *p == ']') {
        ++p;
      } else {
        for (int i = 0;; ++i) {
          if (!value(path + "[" + std::to_string(i) + "]")) return false;
          space();
          if (p < end && *p == ',') {
            ++p;
            continue;
          }
          if (p < end && *p == ']') {
            ++p;
            break;
          }
          return false;
        }
      }
    } else if (*p == '"') {
      ok = string(nullptr);
    } else if (*p == '-' || (*p >= '0' && *p <= '9')) {
      const char* q = p;
      while (q < end && (*q == '-' || *q == '+' || *q == '.' || *q == 'e' || *q == 'E' || (*q >= '0' && *q <= '9'))) ++q;
      double v = 0;
      const auto r = std::from_chars(p, q, v);
      if (r.ec != std::errc() || r.ptr != q) return false;
      numbers[path] = v;
      p = q;
    } else {
      const char* words[] = {"true", "false", "null"};
      ok = false;
      for (const char* w : words) {
        const size_t n = strlen(w);
        if ((size_t)(end - p) >= n && memcmp(p, w, n) == 0) {
          p += n;
          ok = true;
          break;
        }
      }
    }
    --depth;
    return ok;
  }
};

static bool json_numbers(const std::vector<unsigned char>& text, std::map<std::string, double>* out) {
  JsonNumbers j{reinterpret_cast<const char*>(text.data()), reinterpret_cast<const char*>(text.data()) + text.size(), {}};
  if (!j.value("")) return false;
  j.space();
  if (j.p != j.end) return false;
  out->swap(j.numbers);
  return true;
}

static bool file_exists(const std::string& path) {
  struct stat st;
  return stat(path.c_str(), &st) == 0 && S_ISREG(st.st_mode);
}

// the members named, all of them or false
static bool take(const std::map<std::string, double>& m, const std::string& prefix, int n, double* out) {
  for (int i = 0; i < n; ++i) {
    const auto it = m.find(n == 1 ? prefix : prefix + "[" + std::to_string(i) + "]");
    if (it == m.end()) return false;
    out[i] = it->second;
  }
  return true;
}

static int properties_read(swz_ctx* c, const std::string& path, double mn[3], double mx[3], float* spacing, uint64_t* points) {
  std::vector<unsigned char> text;
  SWZ_TRY(read_whole_file(c, path.c_str(), &text));
  std::map<std::string, double> m;
  double s = 0, n = 0;
  if (!json_numbers(text, &m)) return fail(c, SWZ_ERR_BAD_ARG, "cannot parse " + path);
  if (!take(m, "source_properties.bounds.min", 3, mn) || !take(m, "source_properties.bounds.max", 3, mx) ||
      !take(m, "source_properties.root_spacing", 1, &s))
    return fail(c, SWZ_ERR_BAD_ARG, path + " lacks source_properties.bounds or root_spacing");
  *spacing = (float)s;  // (parse_properties_json: static_cast<float>(GetDouble()))
  *points = take(m, "source_properties.processed_points", 1, &n) && n >= 0 ? (uint64_t)n : 0;
  return SWZ_OK;
}

// bounds and x extent / span (parse_ept_json, :125-134)
static int ept_read(swz_ctx* c, const std::string& path, double mn[3], double mx[3], float* spacing) {
  std::vector<unsigned char> text;
  SWZ_TRY(read_whole_file(c, path.c_str(), &text));
  std::map<std::string, double> m;
  double b[6], span = 0;
  if (!json_numbers(text, &m)) return fail(c, SWZ_ERR_BAD_ARG, "cannot parse " + path);
  if (!take(m, "bounds", 6, b) || !take(m, "span", 1, &span)) return fail(c, SWZ_ERR_BAD_ARG, path + " lacks bounds or span");
  for (int a = 0; a < 3; ++a) {
    mn[a] = b[a];
    mx[a] = b[3 + a];
  }
  *spacing = (float)((mx[0] - mn[0]) / (double)(int64_t)span);
  return SWZ_OK;
}

// ---------------------------------------------------------------------------------- the scan
static bool list_dir(const std::string& dir, std::vector<std::string>* names) {
  DIR* d = opendir(dir.c_str());
  if (!d) return false;
  while (const dirent* e = readdir(d)) {
    if (strcmp(e->d_name, ".") == 0 || strcmp(e->d_name, "..") == 0) continue;
    names->push_back(e->d_name);
  }
  closedir(d);
  std::sort(names->begin(), names->end());
  return true;
}

// "r" + octant digits -> (level, Morton index); false: no node name
static bool node_from_potree_name(const std::string& stem, int8_t* level, uint64_t* key) {
  if (stem.empty() || stem[0] != 'r' || stem.size() > 1 + MAX_LEVELS) return false;
  uint64_t k = 0;
  for (size_t l = 1; l < stem.size(); ++l) {
    if (stem[l] < '0' || stem[l] > '7') return false;
    k |= (uint64_t)(stem[l] - '0') << level_shift((int)l - 1);
  }
  *level = (int8_t)((int)stem.size() - 2);
  *key = k;
  return true;
}

// what a LAS node file's point format carries: everything but normals; colours and GPS times by the format
static uint32_t las_node_mask(uint32_t format) {
  uint32_t mask = ((1u << SWZ_ATTR_COUNT) - 1u) & ~((1u << SWZ_ATTR_NORMAL) | (1u << SWZ_ATTR_RGB) | (1u << SWZ_ATTR_GPS_TIME));
  if (format & 2u) mask |= 1u << SWZ_ATTR_RGB;
  if (format & 1u) mask |= 1u << SWZ_ATTR_GPS_TIME;
  return mask;
}

int dataset_scan(swz_ctx* c, const char* who_c, const char* dir_c, int32_t max_depth, DatasetScan* out) {
  const std::string who = std::string(who_c) + ": ", dir = dir_c;
  auto refuse = [&](const std::string& what) { return fail(c, SWZ_ERR_BAD_ARG, who + what); };
  *out = DatasetScan{};
  std::vector<std::string> top, ept;
  if (!list_dir(dir, &top)) return refuse("cannot read the directory " + dir);
  (void)list_dir(dir + "/ept-data", &ept);

  // ---- the format: the node files share one extension
  struct Found {
    int format;
    std::string dir, name;
  };
  std::vector<Found> files;
  std::string first_of[5];
  auto extension = [](const std::string& name) {
    const size_t dot = name.rfind('.');
    return dot == std::string::npos ? std::string() : name.substr(dot + 1);
  };
  for (const std::string& name : top) {
    const std::string ext = extension(name);
    if (ext == "laz") return refuse("LAZ is not read: " + dir + "/" + name);
    const int format = ext == "bin" ? SWZ_OUT_BIN : ext == "binz" ? SWZ_OUT_BINZ : ext == "pnts" ? SWZ_OUT_3DTILES : ext == "las" ? SWZ_OUT_LAS : -1;
    if (format < 0) continue;
    files.push_back({format, dir, name});
    if (first_of[format].empty()) first_of[format] = name;
  }
  for (const std::string& name : ept) {
    const std::string ext = extension(name);
    if (ext == "laz") return refuse("LAZ is not read: " + dir + "/ept-data/" + name);
    if (ext != "las") continue;
    files.push_back({SWZ_OUT_ENTWINE_LAS, dir + "/ept-data", name});
    if (first_of[SWZ_OUT_ENTWINE_LAS].empty()) first_of[SWZ_OUT_ENTWINE_LAS] = "ept-data/" + name;
  }
  int format = -1;
  for (int f = 0; f < 5; ++f) {
    if (first_of[f].empty()) continue;
    if (format >= 0) return refuse("node files of two kinds in " + dir + ": " + first_of[format] + " and " + first_of[f]);
    format = f;
  }
  if (format < 0) {
    if (file_exists(dir + "/cloud.js")) return refuse("a cloud.js data set is not read: " + dir + "/cloud.js");
    return refuse("no node files in " + dir);
  }

  // ---- the names: (level, Morton index), the depth limit, the table's order
  struct Node {
    int8_t level;
    uint64_t key;
    std::string path;
  };
  std::vector<Node> nodes;
  for (const Found& f : files) {
    const std::string stem = f.name.substr(0, f.name.rfind('.')), path = f.dir + "/" + f.name;
    Node nd{0, 0, path};
    bool ok;
    if (format == SWZ_OUT_ENTWINE_LAS) {
      char back[72];
      ok = swz_node_from_entwine_name(stem.c_str(), &nd.level, &nd.key) == SWZ_OK &&
           swz_node_name_entwine(nd.level, nd.key, back) == SWZ_OK && stem == back;
    } else {
      ok = node_from_potree_name(stem, &nd.level, &nd.key);
    }
    if (!ok) return refuse("not a node name: " + path);
    if (max_depth >= 0 && (int)nd.level + 1 > max_depth) continue;
    nodes.push_back(nd);
  }
  std::sort(nodes.begin(), nodes.end(), [](const Node& a, const Node& b) { return a.level != b.level ? a.level < b.level : a.key < b.key; });

  // ---- the headers: counts, and one mask for all
  swz_dataset_info& info = out->info;
  info.format = format;
  info.max_level = -1;
  bool have_mask = false;
  for (const Node& nd : nodes) {
    uint64_t count = 0;
    uint32_t mask = 0;
    swz_las_layout layout{};
    uint32_t data_at = 0;
    int st = SWZ_OK;
    if (format == SWZ_OUT_BIN || format == SWZ_OUT_BINZ) {
      if (format == SWZ_OUT_BIN) {  // the first 12 bytes, not the whole file
        Fd f;
        f.fd = open(nd.path.c_str(), O_RDONLY | O_CLOEXEC);
        unsigned char h[12];
        if (f.fd < 0) return refuse("cannot open " + nd.path);
        if (!pread_all(f.fd, h, 12, 0)) return refuse("truncated node file " + nd.path);
        memcpy(&mask, h, 4);
        memcpy(&count, h + 4, 8);
      } else {
        st = swz_bin_read_header(c, nd.path.c_str(), 1, &mask, &count);
      }
      if (st == SWZ_OK && (mask & ~((1u << SWZ_ATTR_COUNT) - 1u))) return refuse("a mask bit that does not exist in " + nd.path);
    } else if (format == SWZ_OUT_3DTILES) {
      double rtc[3];
      st = swz_pnts_read_header(c, nd.path.c_str(), &count, &mask, rtc);
    } else {
      uint32_t point_format = 0, record_bytes = 0;
      st = swz_las_read_header(c, nd.path.c_str(), &count, &point_format, &record_bytes, &data_at, &layout);
      mask = las_node_mask(point_format);
    }
    if (st != SWZ_OK) return c ? c->fail(st, who + c->err) : st;
    if (have_mask && mask != info.attribute_mask) return refuse("the attribute mask differs from the files before it: " + nd.path);
    have_mask = true;
    info.attribute_mask = mask;
    info.points += count;
    info.max_level = std::max<int32_t>(info.max_level, nd.level);
    out->level.push_back(nd.level);
    out->key.push_back(nd.key);
    out->count.push_back(count);
    out->path.push_back(nd.path);
    out->layout.push_back(layout);
    out->data_at.push_back(data_at);
  }
  info.num_nodes = nodes.size();

  // ---- the root box and the spacing
  uint64_t points = 0;
  if (file_exists(dir + "/properties.json")) {
    SWZ_TRY(properties_read(c, dir + "/properties.json", info.root_min, info.root_max, &info.spacing_at_root, &points));
    info.root_source = SWZ_DATASET_ROOT_PROPERTIES;
  } else if (file_exists(dir + "/ept.json")) {
    SWZ_TRY(ept_read(c, dir + "/ept.json", info.root_min, info.root_max, &info.spacing_at_root));
    info.root_source = SWZ_DATASET_ROOT_EPT;
  }
  return SWZ_OK;
}

DatasetScan DatasetScan::subset(const std::vector<uint32_t>& index) const {
  DatasetScan out;
  out.info = info;
  out.info.points = 0;
  auto take = [&index](const auto& from, auto* to) {
    if (from.empty()) return;
    to->reserve(index.size());
    for (uint32_t k : index) to->push_back(from[k]);
  };
  take(level, &out.level);
  take(key, &out.key);
  take(count, &out.count);
  take(path, &out.path);
  take(layout, &out.layout);
  take(data_at, &out.data_at);
  take(file_bytes, &out.file_bytes);
  for (uint64_t n : out.count) out.info.points += n;
  out.info.num_nodes = out.count.size();
  return out;
}

}  // namespace swz

using namespace swz;

extern "C" {

int swz_properties_json_write(swz_ctx* c, const char* dir, const double root_min[3], const double root_max[3], float spacing_at_root,
                              uint64_t processed_points) {
  if (!dir || !root_min || !root_max) return fail(c, SWZ_ERR_BAD_ARG, "swz_properties_json_write: NULL argument");
  if (!finite3(root_min) || !finite3(root_max) || !std::isfinite(spacing_at_root))
    return fail(c, SWZ_ERR_BAD_ARG, "swz_properties_json_write: a number is not finite");
  std::string s = "{\"source_properties\":{\"bounds\":{\"min\":[";
  for (int a = 0; a < 3; ++a) {
    if (a) s += ",";
    put_number(s, root_min[a]);
  }
  s += "],\"max\":[";
  for (int a = 0; a < 3; ++a) {
    if (a) s += ",";
    put_number(s, root_max[a]);
  }
  s += "]},\"root_spacing\":";
  put_number(s, (double)spacing_at_root);  // (rapidjson has no float: AddMember widens it)
  s += ",\"processed_points\":" + std::to_string(processed_points);
  s += "},\"performance_stats\":{\"prepare_duration\":0,\"indexing_duration\":0}}";
  std::string err;
  const int st = write_file(std::string(dir) + "/properties.json", {{s.data(), s.size()}}, &err);
  return st == SWZ_OK ? SWZ_OK : fail(c, st, err);
}

int swz_properties_json_read(swz_ctx* c, const char* dir, double root_min_out[3], double root_max_out[3], float* spacing_out,
                             uint64_t* points_out) {
  if (!dir) return fail(c, SWZ_ERR_BAD_ARG, "swz_properties_json_read: NULL argument");
  double mn[3], mx[3];
  float spacing = 0.f;
  uint64_t points = 0;
  SWZ_TRY(properties_read(c, std::string(dir) + "/properties.json", mn, mx, &spacing, &points));
  for (int a = 0; a < 3; ++a) {
    if (root_min_out) root_min_out[a] = mn[a];
    if (root_max_out) root_max_out[a] = mx[a];
  }
  if (spacing_out) *spacing_out = spacing;
  if (points_out) *points_out = points;
  return SWZ_OK;
}

int swz_tiler_write_properties(swz_tiler* t, const char* dir) {
  if (!t) return SWZ_ERR_BAD_ARG;
  swz_tiler_info info{};
  SWZ_TRY(swz_tiler_get_info(t, &info));
  return swz_properties_json_write(t->c, dir, t->bmin, t->bmax, t->p.spacing_at_root, info.num_points);
}

int swz_dataset_scan(swz_ctx* c, const char* dir, int32_t max_depth, swz_dataset_info* info_out, uint64_t max_nodes,
                     int8_t* node_level_out, uint64_t* node_key_out, uint64_t* node_count_out, uint64_t* num_nodes_out) {
  if (!dir || !num_nodes_out) return fail(c, SWZ_ERR_BAD_ARG, "swz_dataset_scan: NULL argument");
  DatasetScan scan;
  SWZ_TRY(dataset_scan(c, "swz_dataset_scan", dir, max_depth, &scan));
  const uint64_t nn = scan.count.size();
  *num_nodes_out = nn;
  if (info_out) *info_out = scan.info;
  if (!node_level_out && !node_key_out && !node_count_out) return SWZ_OK;
  if (nn > max_nodes) return fail(c, SWZ_ERR_BAD_ARG, "swz_dataset_scan: max_nodes too small");
  for (uint64_t k = 0; k < nn; ++k) {
    if (node_level_out) node_level_out[k] = scan.level[k];
    if (node_key_out) node_key_out[k] = scan.key[k];
    if (node_count_out) node_count_out[k] = scan.count[k];
  }
  return SWZ_OK;
}

int swz_dataset_scan_why(const char* dir, int32_t max_depth, swz_dataset_info* info_out, uint64_t max_nodes, int8_t* node_level_out,
                         uint64_t* node_key_out, uint64_t* node_count_out, uint64_t* num_nodes_out, char* why_out, uint64_t why_bytes) {
  swz_ctx text;  // (only its error text is used: no device is touched)
  const int st = swz_dataset_scan(&text, dir, max_depth, info_out, max_nodes, node_level_out, node_key_out, node_count_out, num_nodes_out);
  return why_text(st, text, why_out, why_bytes);
}

}  // extern "C"
