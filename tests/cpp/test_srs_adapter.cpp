// swz_host::SourceProjection (schwarzwald_amd/host/swz_tiling.hpp) without a GPU: the constructor's refusal text, and
// transformPositionsTo / transformAABBsTo over the host calls of the C ABI.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>

#include "../../schwarzwald_amd/host/swz_tiling.hpp"

static int failures = 0;
#define CHECK(cond, what)                                   \
  do {                                                      \
    if (!(cond)) {                                          \
      std::fprintf(stderr, "FAIL: %s (%s)\n", what, #cond); \
      ++failures;                                           \
    }                                                       \
  } while (0)

int main() {
  using namespace swz_host;
  // refusals: the reference's sentence, and the token the library names
  const char* refused[][2] = {{"+proj=merc +datum=WGS84", "+proj=merc"}, {"EPSG:4326", "EPSG:4326"}, {"", "empty"},
                              {"+proj=utm +zone=32 +datum=WGS84 +towgs84=0,0,0", "+towgs84=0,0,0"}};
  for (const auto& r : refused) {
    bool threw = false;
    try {
      SourceProjection p{r[0]};
    } catch (const std::runtime_error& e) {
      threw = true;
      const std::string text = e.what();
      CHECK(text.rfind(std::string("Source projection ") + r[0] + " not recognized!", 0) == 0, text.c_str());
      CHECK(text.find(r[1]) != std::string::npos, text.c_str());
    }
    CHECK(threw, r[0]);
  }
  std::printf("refusals ok: %zu definitions\n", sizeof(refused) / sizeof(refused[0]));

  const SourceProjection utm{"+proj=utm +zone=32 +datum=WGS84"};
  AABB boxes[2];
  boxes[0].min = {499000.0, 5400000.0, 200.0};
  boxes[0].max = {501000.0, 5402000.0, 240.0};
  boxes[1].min = {412000.0, 5401000.0, 250.0};
  boxes[1].max = {412600.0, 5401600.0, 290.0};
  const AABB source[2] = {boxes[0], boxes[1]};
  utm.transformAABBsTo(SWZ_SRS_ECEF, boxes, 2);
  for (int b = 0; b < 2; ++b) {
    // the min / max of the eight corners sent through transformPositionsTo, bit for bit
    Vector3d corners[8];
    for (int i = 0; i < 8; ++i)
      corners[i] = {(i & 1) ? source[b].max.x : source[b].min.x, (i & 2) ? source[b].max.y : source[b].min.y,
                    (i & 4) ? source[b].max.z : source[b].min.z};
    utm.transformPositionsTo(SWZ_SRS_ECEF, corners, 8);
    Vector3d lo = corners[0], hi = corners[0];
    for (int i = 1; i < 8; ++i) {
      lo = {std::fmin(lo.x, corners[i].x), std::fmin(lo.y, corners[i].y), std::fmin(lo.z, corners[i].z)};
      hi = {std::fmax(hi.x, corners[i].x), std::fmax(hi.y, corners[i].y), std::fmax(hi.z, corners[i].z)};
    }
    CHECK(std::memcmp(&lo, &boxes[b].min, 24) == 0 && std::memcmp(&hi, &boxes[b].max, 24) == 0, "box == min / max of the corners");
    const double r = std::sqrt(lo.x * lo.x + lo.y * lo.y + lo.z * lo.z);
    CHECK(r > 6.3e6 && r < 6.4e6, "on the globe");
  }
  std::printf("transformAABBsTo ok: 2 boxes\n");

  // the WGS84 target: longitude and latitude in radians; the central meridian of zone 32 is 9 degrees east
  Vector3d p{500000.0, 5400000.0, 123.0};
  utm.transformPositionsTo(SWZ_SRS_WGS84, &p, 1);
  CHECK(std::fabs(p.x - 9.0 * 3.14159265358979323846 / 180.0) < 1e-15 && p.y > 0.84 && p.y < 0.86 && p.z == 123.0, "WGS84 target");
  bool threw = false;
  try {
    utm.transformPositionsTo(7, &p, 1);
  } catch (const std::runtime_error&) {
    threw = true;
  }
  CHECK(threw, "an unknown target throws");
  utm.transformPositionsTo(SWZ_SRS_ECEF, nullptr, 0);
  std::printf("transformPositionsTo ok\n");
  return failures ? 1 : 0;
}
