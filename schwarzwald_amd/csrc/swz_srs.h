// swz_srs.h -- the map of a source projection (swz_srs, include/swz_gpu.h) onto WGS84: one inline function for the host
// (swz_srs_transform, swz_srs_transform_box) and for every kernel that projects (swz_srs.hip: in place; swz_tinput.hip: fused
// into the segment decode).  What the reference asks of PROJ per point (Proj4Transform::transformPointsTo,
// core/util/Transformation.cpp:118-178), for the projections swz_srs_parse accepts.
//
// Inverse transverse Mercator: the Krueger series in the third flattening n to order n^6 (Karney 2011).  With xi = (y - y_0) /
// (k_0 A) + xi_0 and eta = (x - x_0) / (k_0 A), zeta' = zeta - sum beta_j sin 2 j zeta is summed by a complex Clenshaw
// recurrence that needs sin / cos of 2 xi and sinh / cosh of 2 eta once; longitude = lon_0 + atan2(sinh eta', cos xi'); the
// conformal latitude chi has sin chi = sin xi' / cosh eta', and the geodetic latitude is chi + sum delta_j sin 2 j chi, a
// real Clenshaw sum on sin / cos 2 chi, which are products of what is there already.  No loop depends on the data.
//
// Contraction is off inside the function: for given input bits the device result does not depend on the kernel the function
// was inlined into (tests compare the fused decode with decode -> swz_srs_transform_device bit for bit).
#pragma once
#include <math.h>

#include "swz_internal.h"

namespace swz {

constexpr double SRS_WGS84_A = 6378137.0;
constexpr double SRS_WGS84_F = 1.0 / 298.257223563;
constexpr double SRS_PI = 3.14159265358979323846;

// what every entry point that takes a swz_srs checks: a struct swz_srs_parse made -- not a zeroed or an unset one, which would
// otherwise pass for longlat and yield a plausible box
inline bool srs_valid(const swz_srs* s) {
  if (!s || (s->kind != SWZ_SRS_LONGLAT && s->kind != SWZ_SRS_TMERC)) return false;
  if (!(s->a > 0) || !isfinite(s->a) || !(s->f >= 0 && s->f < 1)) return false;
  if (s->kind == SWZ_SRS_LONGLAT) return true;
  return s->radius > 0 && isfinite(s->radius) && s->k_0 > 0 && isfinite(s->x_0) && isfinite(s->y_0) && isfinite(s->lon_0) &&
         isfinite(s->xi_0);
}

__host__ __device__ inline void srs_to_target(const swz_srs& s, int target, double& x, double& y, double& z) {
#pragma clang fp contract(off)
  double lam, sin_phi, cos_phi;
  if (s.kind == SWZ_SRS_TMERC) {
    const double xi = (y - s.y_0) / s.radius + s.xi_0;
    const double eta = (x - s.x_0) / s.radius;
    // a = 2 cos 2 zeta, zeta = xi + i eta
    const double s2 = sin(2.0 * xi), c2 = cos(2.0 * xi);
    const double sh2 = sinh(2.0 * eta), ch2 = cosh(2.0 * eta);
    const double ar = 2.0 * (c2 * ch2), ai = -2.0 * (s2 * sh2);
    // y_k = a y_{k+1} - y_{k+2} + beta_k, k = 6 .. 1; the sum is y_1 sin 2 zeta
    double y1r = 0.0, y1i = 0.0, y2r = 0.0, y2i = 0.0;
#pragma unroll
    for (int k = 5; k >= 0; --k) {
      const double tr = (ar * y1r - ai * y1i) - y2r + s.beta[k];
      const double ti = (ar * y1i + ai * y1r) - y2i;
      y2r = y1r;
      y2i = y1i;
      y1r = tr;
      y1i = ti;
    }
    const double zr = s2 * ch2, zi = c2 * sh2;  // sin 2 zeta
    const double xi_p = xi - (y1r * zr - y1i * zi);
    const double eta_p = eta - (y1r * zi + y1i * zr);
    const double sx = sin(xi_p), cx = cos(xi_p);
    const double sh = sinh(eta_p), ch = cosh(eta_p);
    lam = s.lon_0 + atan2(sh, cx);
    const double sin_chi = sx / ch;
    const double cos_chi = sqrt(sh * sh + cx * cx) / ch;
    // phi = chi + d, d = sum delta_j sin 2 j chi
    const double s2c = 2.0 * (sin_chi * cos_chi), c2c = (cos_chi - sin_chi) * (cos_chi + sin_chi);
    const double b = 2.0 * c2c;
    double d1 = 0.0, d2 = 0.0;
#pragma unroll
    for (int k = 5; k >= 0; --k) {
      const double t = b * d1 - d2 + s.delta[k];
      d2 = d1;
      d1 = t;
    }
    const double d = d1 * s2c;
    const double sd = sin(d), cd = cos(d);
    sin_phi = sin_chi * cd + cos_chi * sd;
    cos_phi = cos_chi * cd - sin_chi * sd;
  } else {
    const double rad = SRS_PI / 180.0;
    lam = x * rad;
    const double phi = y * rad;
    sin_phi = sin(phi);
    cos_phi = cos(phi);
  }
  if (target == SWZ_SRS_WGS84) {
    if (lam > SRS_PI) lam -= 2.0 * SRS_PI;
    if (lam < -SRS_PI) lam += 2.0 * SRS_PI;
    x = lam;
    y = atan2(sin_phi, cos_phi);
    return;  // the height stays
  }
  // geodetic -> geocentric on WGS84
  const double e2 = SRS_WGS84_F * (2.0 - SRS_WGS84_F);
  const double N = SRS_WGS84_A / sqrt(1.0 - e2 * (sin_phi * sin_phi));
  const double r = (N + z) * cos_phi;
  x = r * cos(lam);
  y = r * sin(lam);
  z = (N * (1.0 - e2) + z) * sin_phi;
}

}  // namespace swz
