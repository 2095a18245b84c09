// swz_srs.hip -- a source projection without PROJ: the definition (swz_srs_parse), the map on the host (swz_srs_transform,
// swz_srs_transform_box) and in place on the device (swz_srs_transform_device).  The map itself is swz_srs.h; the decode of a
// data set of LAS files inlines it too (swz_tinput.hip).  Reference: Proj4Transform, core/util/Transformation.cpp:10-44, 74-211.
#include <charconv>
#include <cmath>
#include <cstring>
#include <limits>
#include <map>
#include <string>
#include <vector>

#include "swz_internal.h"
#include "swz_device.h"
#include "swz_hostio.h"
#include "swz_srs.h"

namespace swz {

constexpr uint32_t SRS_TILE = 256;                              // rows per workgroup and turn, one per thread
constexpr uint64_t SRS_MAX_POINTS = 0xFFFFFFFFull - 65535ull;   // the library's limit of points per batch (2^32 - 65536)

// In place on AoS rows of 24 bytes.  A workgroup takes tiles of SRS_TILE rows, grid-stride: the tile's 3 * SRS_TILE doubles go
// into LDS as consecutive lanes read consecutive doubles, every lane maps its own row there, and the tile leaves the same way.
__global__ __launch_bounds__(SRS_TILE) void srs_transform_kernel(swz_srs s, int target, double* xyz, uint64_t n) {
  __shared__ double s_row[3 * SRS_TILE];
  const uint32_t t = threadIdx.x;
  const uint64_t tiles = (n + SRS_TILE - 1) / SRS_TILE;
  for (uint64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const uint64_t r0 = tile * SRS_TILE;
    const uint32_t rows = (uint32_t)min((uint64_t)SRS_TILE, n - r0);
    double* const g = xyz + 3 * r0;
    for (uint32_t w = t; w < 3 * rows; w += SRS_TILE) s_row[w] = g[w];
    __syncthreads();
    if (t < rows) {
      double x = s_row[3 * t], y = s_row[3 * t + 1], z = s_row[3 * t + 2];
      srs_to_target(s, target, x, y, z);
      s_row[3 * t] = x;
      s_row[3 * t + 1] = y;
      s_row[3 * t + 2] = z;
    }
    __syncthreads();
    for (uint32_t w = t; w < 3 * rows; w += SRS_TILE) g[w] = s_row[w];
    __syncthreads();  // the next tile's loads write what these stores read
  }
}

// ---------------------------------------------------------------------------------- the definition
namespace {

struct Ellipsoid {
  double a, rf;  // rf = 0: a sphere
};
const Ellipsoid ELL_WGS84{6378137.0, 298.257223563}, ELL_GRS80{6378137.0, 298.257222101};

// a decimal number, the whole text: std::from_chars, which knows neither the process's locale nor hex forms; one leading '+'
// is allowed as strtod allows it.  "nan" and "inf" parse -- the callers refuse what is not finite, naming the token.
bool number(const std::string& text, double* out) {
  const char* first = text.c_str();
  const char* const last = first + text.size();
  if (first != last && *first == '+' && last - first > 1 && first[1] != '-' && first[1] != '+') ++first;
  if (first == last) return false;
  const std::from_chars_result r = std::from_chars(first, last, *out, std::chars_format::general);
  return r.ec == std::errc() && r.ptr == last;
}

// an EPSG code: decimal digits and nothing else
bool digits(const std::string& text, long* out) {
  if (text.empty() || text.size() > 9) return false;
  long v = 0;
  for (const char ch : text) {
    if (ch < '0' || ch > '9') return false;
    v = v * 10 + (ch - '0');
  }
  *out = v;
  return true;
}

std::string lower(std::string s) {
  for (char& ch : s) ch = (char)tolower((unsigned char)ch);
  return s;
}

// the series of tools/srs_series.py, evaluated once
void srs_series(swz_srs* s) {
  const double n = s->n, n2 = n * n, n3 = n2 * n, n4 = n3 * n, n5 = n4 * n, n6 = n5 * n;
  s->beta[0] = n / 2 - 2 * n2 / 3 + 37 * n3 / 96 - n4 / 360 - 81 * n5 / 512 + 96199 * n6 / 604800;
  s->beta[1] = n2 / 48 + n3 / 15 - 437 * n4 / 1440 + 46 * n5 / 105 - 1118711 * n6 / 3870720;
  s->beta[2] = 17 * n3 / 480 - 37 * n4 / 840 - 209 * n5 / 4480 + 5569 * n6 / 90720;
  s->beta[3] = 4397 * n4 / 161280 - 11 * n5 / 504 - 830251 * n6 / 7257600;
  s->beta[4] = 4583 * n5 / 161280 - 108847 * n6 / 3991680;
  s->beta[5] = 20648693 * n6 / 638668800;
  s->delta[0] = 2 * n - 2 * n2 / 3 - 2 * n3 + 116 * n4 / 45 + 26 * n5 / 45 - 2854 * n6 / 675;
  s->delta[1] = 7 * n2 / 3 - 8 * n3 / 5 - 227 * n4 / 45 + 2704 * n5 / 315 + 2323 * n6 / 945;
  s->delta[2] = 56 * n3 / 15 - 136 * n4 / 35 - 1262 * n5 / 105 + 73814 * n6 / 2835;
  s->delta[3] = 4279 * n4 / 630 - 332 * n5 / 35 - 399572 * n6 / 14175;
  s->delta[4] = 4174 * n5 / 315 - 144838 * n6 / 6237;
  s->delta[5] = 601676 * n6 / 22275;
  s->radius = s->k_0 * (s->a / (1 + n) * (1 + n2 / 4 + n4 / 64 + n6 / 256));
}

// The rectifying latitude of lat_0: the mu whose conformal latitude chi(mu) = mu - sum beta_j sin 2 j mu is lat_0's, by
// Newton's iteration on the series the map itself inverts (so northing y_0 is lat_0 to the series' accuracy).
double rectifying_of(const swz_srs& s, double phi) {
  if (phi == 0.0) return 0.0;
  const double e = std::sqrt(s.e2);
  const double chi = std::atan(std::sinh(std::asinh(std::tan(phi)) - e * std::atanh(e * std::sin(phi))));
  double mu = chi;
  for (int it = 0; it < 8; ++it) {
    double f = mu - chi, df = 1.0;
    for (int j = 0; j < 6; ++j) {
      f -= s.beta[j] * std::sin(2.0 * (j + 1) * mu);
      df -= 2.0 * (j + 1) * s.beta[j] * std::cos(2.0 * (j + 1) * mu);
    }
    mu -= f / df;
  }
  return mu;
}

int parse(const char* definition, swz_srs* out, std::string* why) {
  auto refuse = [&](const std::string& text) {
    *why = "swz_srs_parse: " + text;
    return (int)SWZ_ERR_BAD_ARG;
  };
  if (!definition || !out) return refuse("NULL argument");
  std::vector<std::string> tokens;
  {
    std::string cur;
    for (const char* p = definition;; ++p) {
      if (*p == 0 || isspace((unsigned char)*p)) {
        if (!cur.empty()) tokens.push_back(cur);
        cur.clear();
        if (*p == 0) break;
      } else {
        cur += *p;
      }
    }
  }
  if (tokens.empty()) return refuse("the definition is empty");
  const std::string whole = definition;
  if (whole.find('[') != std::string::npos || whole.find('{') != std::string::npos)
    return refuse("WKT and PROJJSON are not read: '" + tokens[0] + "'");

  std::map<std::string, std::string> kv;  // key -> value ("" for a flag)
  std::map<std::string, std::string> spelled;
  if (tokens.size() == 1 && tokens[0][0] != '+') {
    const std::string t = lower(tokens[0]);
    long code = 0;
    if (t.compare(0, 5, "epsg:") != 0 || !digits(t.substr(5), &code))
      return refuse("not a +proj definition and not an EPSG code: '" + tokens[0] + "'");
    int zone = 0;
    bool south = false, grs80 = false;
    if (code >= 32601 && code <= 32660) zone = (int)code - 32600;
    else if (code >= 32701 && code <= 32760) zone = (int)code - 32700, south = true;
    else if (code >= 25828 && code <= 25838) zone = (int)code - 25800, grs80 = true;
    else return refuse("unknown EPSG code '" + tokens[0] + "' (WGS 84 / UTM 326xx, 327xx and ETRS89 / UTM 25828-25838 are known)");
    kv["proj"] = "utm";
    kv["zone"] = std::to_string(zone);
    if (south) kv["south"] = "";
    kv["ellps"] = grs80 ? "GRS80" : "WGS84";
    for (const auto& e : kv) spelled[e.first] = tokens[0];
  } else {
    for (const std::string& tok : tokens) {
      if (tok[0] != '+' || tok.size() < 2) return refuse("not a +key[=value] token: '" + tok + "'");
      const size_t eq = tok.find('=');
      const std::string key = tok.substr(1, eq == std::string::npos ? std::string::npos : eq - 1);
      const std::string value = eq == std::string::npos ? "" : tok.substr(eq + 1);
      static const char* const known[] = {"proj", "zone", "south", "lat_0", "lon_0", "k", "k_0", "x_0", "y_0", "ellps", "datum",
                                          "a", "rf", "b", "units", "no_defs", "type"};
      bool ok = false;
      for (const char* k : known) ok = ok || key == k;
      if (!ok) return refuse("'" + tok + "' is not supported");
      const std::string canon = key == "k_0" ? "k" : key;
      if (kv.count(canon)) return refuse("'" + tok + "' is given twice");
      kv[canon] = value;
      spelled[canon] = tok;
    }
  }
  auto has = [&](const char* k) { return kv.count(k) != 0; };
  auto tok = [&](const char* k) { return "'" + spelled[k] + "'"; };
  if (!has("proj")) return refuse("no +proj in '" + whole + "'");
  if (has("units") && kv["units"] != "m") return refuse(tok("units") + ": only metres are read");
  if (has("type") && kv["type"] != "crs") return refuse(tok("type") + " is not supported");
  for (const char* flag : {"south", "no_defs"})
    if (has(flag) && !kv[flag].empty()) return refuse(tok(flag) + " takes no value");

  swz_srs s{};
  const std::string proj = kv["proj"];
  const bool utm = proj == "utm", tmerc = proj == "tmerc", longlat = proj == "longlat" || proj == "latlong";
  if (!utm && !tmerc && !longlat) return refuse(tok("proj") + ": utm, tmerc and longlat are read");
  s.kind = longlat ? SWZ_SRS_LONGLAT : SWZ_SRS_TMERC;
  // keys a projection does not take
  for (const char* k : {"zone", "south"})
    if (!utm && has(k)) return refuse(tok(k) + " belongs to +proj=utm");
  for (const char* k : {"lat_0", "lon_0", "k", "x_0", "y_0"})
    if (!tmerc && has(k)) return refuse(tok(k) + " belongs to +proj=tmerc");
  if (longlat && has("units")) return refuse(tok("units") + ": +proj=longlat is in degrees");

  // ---- the ellipsoid
  Ellipsoid ell{0, 0};
  bool have = false;
  if (has("ellps")) {
    if (kv["ellps"] == "WGS84") ell = ELL_WGS84;
    else if (kv["ellps"] == "GRS80") ell = ELL_GRS80;
    else return refuse(tok("ellps") + ": WGS84 and GRS80 are known");
    have = true;
  }
  if (has("datum")) {
    if (kv["datum"] != "WGS84") return refuse(tok("datum") + ": only WGS84 is known (no datum shifts)");
    if (have && ell.rf != ELL_WGS84.rf) return refuse(tok("ellps") + " contradicts " + tok("datum"));
    ell = ELL_WGS84;
    have = true;
  }
  if (has("a")) {
    if (have) return refuse(tok("a") + " beside +ellps or +datum");
    if (!number(kv["a"], &ell.a) || !std::isfinite(ell.a) || !(ell.a > 0)) return refuse(tok("a") + " is not finite and positive");
    if (has("rf") && has("b")) return refuse(tok("b") + " beside " + tok("rf"));
    if (has("rf")) {
      if (!number(kv["rf"], &ell.rf) || !std::isfinite(ell.rf) || !(ell.rf > 1)) return refuse(tok("rf") + " is not finite and above 1");
    } else if (has("b")) {
      double b = 0;
      if (!number(kv["b"], &b) || !std::isfinite(b) || !(b > 0) || b > ell.a) return refuse(tok("b") + " is not finite, positive and at most +a");
      ell.rf = b == ell.a ? 0.0 : ell.a / (ell.a - b);
    } else {
      return refuse(tok("a") + " needs +rf or +b");
    }
    have = true;
  } else {
    for (const char* k : {"rf", "b"})
      if (has(k)) return refuse(tok(k) + " without +a");
  }
  if (!have) return refuse("no ellipsoid in '" + whole + "' (+ellps, +datum or +a)");
  s.a = ell.a;
  s.f = ell.rf ? 1.0 / ell.rf : 0.0;
  s.e2 = s.f * (2.0 - s.f);
  s.n = s.f / (2.0 - s.f);

  // ---- the projection's constants
  const double rad = SRS_PI / 180.0;
  s.k_0 = 1.0;
  if (utm) {
    double zone = 0;
    if (!has("zone")) return refuse("+proj=utm without +zone in '" + whole + "'");
    if (!number(kv["zone"], &zone) || zone != std::floor(zone) || zone < 1 || zone > 60) return refuse(tok("zone") + ": zones 1 to 60");
    s.lon_0 = (zone * 6.0 - 183.0) * rad;
    s.k_0 = 0.9996;
    s.x_0 = 500000.0;
    s.y_0 = has("south") ? 10000000.0 : 0.0;
  } else if (tmerc) {
    struct Field {
      const char* key;
      double* to;
      double unit;
    };
    double lat = 0, lon = 0;
    for (const Field& fd : {Field{"lat_0", &lat, 1}, Field{"lon_0", &lon, 1}, Field{"k", &s.k_0, 1}, Field{"x_0", &s.x_0, 1}, Field{"y_0", &s.y_0, 1}}) {
      if (!has(fd.key)) continue;
      if (!number(kv[fd.key], fd.to) || !std::isfinite(*fd.to)) return refuse(tok(fd.key) + " is not a finite number");
    }
    if (!(s.k_0 > 0)) return refuse(tok("k") + " is not positive");
    if (std::fabs(lat) > 90) return refuse(tok("lat_0") + " is outside [-90, 90]");
    if (std::fabs(lon) > 360) return refuse(tok("lon_0") + " is outside [-360, 360]");
    s.lat_0 = lat * rad;
    s.lon_0 = lon * rad;
  }
  if (!longlat) {
    srs_series(&s);
    s.xi_0 = rectifying_of(s, s.lat_0);
  }
  *out = s;
  return SWZ_OK;
}

}  // namespace
}  // namespace swz

using namespace swz;

extern "C" {

int swz_srs_parse(swz_ctx* c, const char* definition, swz_srs* out) {
  std::string why;
  const int st = parse(definition, out, &why);
  return st == SWZ_OK ? SWZ_OK : fail(c, st, why);
}

int swz_srs_parse_why(const char* definition, swz_srs* out, char* why_out, uint64_t why_bytes) {
  std::string why;
  const int st = parse(definition, out, &why);
  if (why_out && why_bytes) {
    const size_t len = std::min<size_t>(why.size(), (size_t)why_bytes - 1);
    memcpy(why_out, why.data(), len);
    why_out[len] = 0;
  }
  return st;
}

int swz_srs_transform(const swz_srs* srs, int target, double* xyz, uint64_t n) {
  if (!srs_valid(srs) || (n && !xyz) || (target != SWZ_SRS_ECEF && target != SWZ_SRS_WGS84)) return SWZ_ERR_BAD_ARG;
  for (uint64_t i = 0; i < n; ++i) srs_to_target(*srs, target, xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]);
  return SWZ_OK;
}

int swz_srs_transform_box(const swz_srs* srs, int target, const double mn[3], const double mx[3], double out_min[3], double out_max[3]) {
  if (!srs_valid(srs) || !mn || !mx || !out_min || !out_max || (target != SWZ_SRS_ECEF && target != SWZ_SRS_WGS84)) return SWZ_ERR_BAD_ARG;
  double lo[3], hi[3];
  for (int k = 0; k < 3; ++k) {
    lo[k] = std::numeric_limits<double>::max();
    hi[k] = std::numeric_limits<double>::lowest();
  }
  for (int idx = 0; idx < 8; ++idx) {
    double p[3] = {(idx & 1) ? mx[0] : mn[0], (idx & 2) ? mx[1] : mn[1], (idx & 4) ? mx[2] : mn[2]};
    srs_to_target(*srs, target, p[0], p[1], p[2]);
    for (int k = 0; k < 3; ++k) {
      lo[k] = std::min(lo[k], p[k]);
      hi[k] = std::max(hi[k], p[k]);
    }
  }
  for (int k = 0; k < 3; ++k) {
    out_min[k] = lo[k];
    out_max[k] = hi[k];
  }
  return SWZ_OK;
}

uint32_t swz_srs_tile(void) { return SRS_TILE; }

int swz_srs_transform_device(swz_ctx* c, const swz_srs* srs, int target, double* d_xyz, uint64_t n) {
  if (!c) return SWZ_ERR_BAD_ARG;
  if (!srs_valid(srs)) return c->fail(SWZ_ERR_BAD_ARG, "swz_srs_transform_device: not a definition swz_srs_parse made");
  if (target != SWZ_SRS_ECEF && target != SWZ_SRS_WGS84) return c->fail(SWZ_ERR_BAD_ARG, "swz_srs_transform_device: unknown target");
  if (n > SRS_MAX_POINTS) return c->fail(SWZ_ERR_TOO_MANY_POINTS, "swz_srs_transform_device: more than 2^32-65536 points");
  if (n == 0) return SWZ_OK;
  if (!d_xyz) return c->fail(SWZ_ERR_BAD_ARG, "swz_srs_transform_device: NULL positions");
  SWZ_HIP(c, hipSetDevice(c->device));
  {
    ProfScope ps(c, "srs_transform", n * 48, 1);
    // grid-stride: enough workgroups to fill the device several times over, no more than there are tiles
    const uint64_t tiles = (n + SRS_TILE - 1) / SRS_TILE;
    const uint32_t grid = (uint32_t)std::min<uint64_t>(tiles, 256u * 32u);
    hipLaunchKernelGGL(srs_transform_kernel, dim3(grid), dim3(SRS_TILE), 0, c->stream, *srs, target, d_xyz, n);
    SWZ_LAUNCH_CHECK(c);
  }
  SWZ_HIP(c, hipStreamSynchronize(c->stream));
  return SWZ_OK;
}

}  // extern "C"
