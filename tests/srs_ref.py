"""The yardstick of the source projection tests: transverse Mercator and geocentric coordinates in mpmath at 40 digits, with
no series anywhere.

Forward, (phi, lam) -> (easting, northing):
  1. geodetic -> conformal latitude by the closed form (tau' = tau sqrt(1 + sigma^2) - sigma sqrt(1 + tau^2));
  2. the Gauss-Schreiber coordinates zeta' = xi' + i eta' by the closed spherical formulas -- zeta' = gd(psi + i lam), psi the
     isometric latitude;
  3. zeta = mu(zeta') by analytic continuation: the complex geodetic latitude Phi solves psi(Phi) = psi + i lam
     (mpmath.findroot, started at zeta'), the meridian-arc integrand (1 - e^2 sin^2 t)^(-3/2) is integrated along the straight
     path from 0 to Phi (mpmath.quad) and divided by the quarter meridian;
  4. easting = x_0 + k_0 A Im zeta, northing = y_0 + k_0 A (Re zeta - mu(lat_0)), A = a (1 - e^2) M(pi / 2) / (pi / 2).
Inverse, for the image of ROUNDED coordinates: the same equations solved the other way round (Newton on mu(Phi) = zeta with
the integrand as derivative, then psi(Phi) = psi + i lam read off, then the real psi(phi) = psi by findroot).
ECEF from (phi, lam, h) is the closed form on WGS84, whatever the source ellipsoid (no datum shift)."""
import functools
import os

import mpmath as mp
import numpy as np

mp.mp.dps = 40

WGS84 = (mp.mpf(6378137), 1 / mp.mpf("298.257223563"))
GRS80 = (mp.mpf(6378137), 1 / mp.mpf("298.257222101"))
AIRY = (mp.mpf("6377563.396"), 1 / mp.mpf("299.3249646"))


class TMerc:
    """a transverse Mercator: ellipsoid (a, f), lat_0 and lon_0 in degrees, k_0, x_0, y_0; values as strings or numbers"""

    def __init__(self, ell, lat_0=0, lon_0=0, k_0=1, x_0=0, y_0=0):
        self.a, self.f = ell
        self.e2 = self.f * (2 - self.f)
        self.e = mp.sqrt(self.e2)
        self.lat_0, self.lon_0 = mp.radians(mp.mpf(lat_0)), mp.radians(mp.mpf(lon_0))
        self.k_0, self.x_0, self.y_0 = mp.mpf(k_0), mp.mpf(x_0), mp.mpf(y_0)
        self.quarter = self.arc(mp.pi / 2)
        self.A = self.a * (1 - self.e2) * self.quarter / (mp.pi / 2)
        self.mu_0 = self.mu(self.lat_0)

    @staticmethod
    def utm(zone, south=False, ell=WGS84):
        return TMerc(ell, 0, 6 * zone - 183, "0.9996", 500000, 10000000 if south else 0)

    def integrand(self, t):
        return (1 - self.e2 * mp.sin(t) ** 2) ** mp.mpf(-1.5)

    def arc(self, Phi):
        """the integral of the meridian-arc integrand along the straight path from 0 to Phi (complex)"""
        if Phi == 0:
            return mp.mpf(0)
        return mp.quad(lambda s: self.integrand(s * Phi), [0, 1]) * Phi

    def mu(self, Phi):
        return self.arc(Phi) / self.quarter * (mp.pi / 2)

    def psi(self, Phi):
        """the isometric latitude, analytic in Phi"""
        return mp.asinh(mp.tan(Phi)) - self.e * mp.atanh(self.e * mp.sin(Phi))

    def conformal(self, phi):
        tau = mp.tan(phi)
        sigma = mp.sinh(self.e * mp.atanh(self.e * tau / mp.sqrt(1 + tau * tau)))
        return mp.atan(tau * mp.sqrt(1 + sigma * sigma) - sigma * mp.sqrt(1 + tau * tau))

    def forward(self, phi, lam):
        """(phi, lam) in radians -> (easting, northing)"""
        phi, dl = mp.mpf(phi), mp.mpf(lam) - self.lon_0
        taup = mp.tan(self.conformal(phi))
        xi_p = mp.atan2(taup, mp.cos(dl))
        eta_p = mp.asinh(mp.sin(dl) / mp.sqrt(taup * taup + mp.cos(dl) ** 2))
        target = self.psi(phi) + 1j * dl
        if dl == 0:
            Phi = mp.mpc(phi)
        else:
            Phi = mp.findroot(lambda P: self.psi(P) - target, mp.mpc(xi_p, eta_p))
        zeta = self.mu(Phi)
        return self.x_0 + self.k_0 * self.A * mp.im(zeta), self.y_0 + self.k_0 * self.A * (mp.re(zeta) - self.mu_0)

    def inverse(self, easting, northing):
        """(easting, northing), exact mpf or doubles -> (phi, lam) in radians"""
        zeta = mp.mpc((mp.mpf(northing) - self.y_0) / (self.k_0 * self.A) + self.mu_0, (mp.mpf(easting) - self.x_0) / (self.k_0 * self.A))
        Phi = zeta
        for _ in range(12):  # Newton; quadratic from a start within 3e-3
            step = (self.mu(Phi) - zeta) / (self.integrand(Phi) / self.quarter * (mp.pi / 2))
            Phi -= step
            if abs(step) < mp.mpf(10) ** -36:
                break
        else:
            raise ArithmeticError("the inverse did not converge")
        w = self.psi(Phi)
        psi_real, dl = mp.re(w), mp.im(w)
        phi = mp.findroot(lambda p: mp.re(self.psi(p)) - psi_real, mp.atan(mp.sinh(psi_real)))
        return phi, self.lon_0 + dl


def ecef(phi, lam, h):
    """WGS84 geocentric coordinates of (phi, lam) in radians and the ellipsoidal height"""
    a, f = WGS84
    e2 = f * (2 - f)
    N = a / mp.sqrt(1 - e2 * mp.sin(phi) ** 2)
    return ((N + h) * mp.cos(phi) * mp.cos(lam), (N + h) * mp.cos(phi) * mp.sin(lam), (N * (1 - e2) + h) * mp.sin(phi))


def wrap(lam):
    """longitude into [-pi, pi]"""
    if lam > mp.pi:
        return lam - 2 * mp.pi
    if lam < -mp.pi:
        return lam + 2 * mp.pi
    return lam


def image(proj, x, y, z):
    """the exact image of the DOUBLES (x, y, z): (ecef, (lam, phi, h)), as mpf.  proj: a TMerc, or None for longlat degrees"""
    x, y, z = mp.mpf(float(x)), mp.mpf(float(y)), mp.mpf(float(z))
    if proj is None:
        lam, phi = mp.radians(x), mp.radians(y)
    else:
        phi, lam = proj.inverse(x, y)
    return ecef(phi, lam, z), (wrap(lam), phi, z)


# ---------------------------------------------------------------------------------- the test points
UTM_CASES = [(zone, south) for zone in (1, 31, 32, 60) for south in (False, True)]
OSGB_LIKE = dict(definition="+proj=tmerc +lat_0=49 +lon_0=-2 +k=0.9996012717 +x_0=400000 +y_0=-100000 +a=6377563.396 +rf=299.3249646",
                 proj=lambda: TMerc(AIRY, 49, -2, "0.9996012717", 400000, -100000))
LONGLAT = "+proj=longlat +datum=WGS84"
HEIGHTS = (-500.0, 0.0, 9000.0)
ARCSEC = 1.0 / 3600.0


def utm_definition(zone, south):
    return "+proj=utm +zone=%d%s +datum=WGS84" % (zone, " +south" if south else "")


def group_rows():
    """the (phi, lam, h) of every group, in degrees: a list of (definition, projection factory, rows)"""
    out = []
    k = 0
    for zone, south in UTM_CASES:
        lats = (0.0, -0.5 * ARCSEC, -30.0, -55.0, -80.0) if south else (0.0, 0.5 * ARCSEC, 30.0, 55.0, 84.0)
        all_heights = (zone, south) == (32, False)
        rows = []
        for lat in lats:
            for dlon in (0.0, -3.0, 3.0, -4.0, 4.0):
                for h in (HEIGHTS if all_heights else (HEIGHTS[k % 3],)):
                    rows.append((lat, 6 * zone - 183 + dlon, h))
                k += 1
        out.append((utm_definition(zone, south), functools.partial(TMerc.utm, zone, south), rows))
    out.append((OSGB_LIKE["definition"], OSGB_LIKE["proj"],
                [(lat, lon, h) for lat in (50.0, 54.5, 58.0) for lon in (-2.0, -6.0, 1.5) for h in HEIGHTS]))
    out.append((LONGLAT, None, [(lat, lon, h) for lon in (-180.0, 0.0, 180.0) for lat in (-90.0, 0.0, 90.0) for h in HEIGHTS]))
    return out


def split(values):
    """a list of triples of mpf -> (hi, lo) float64 arrays whose sum is the value to about 32 digits"""
    hi = np.array([[float(v) for v in row] for row in values], dtype=np.float64)
    lo = np.array([[float(v - mp.mpf(float(v))) for v in row] for row in values], dtype=np.float64)
    return hi, lo


def make_group(definition, factory, rows):
    """One group, made forwards: (phi, lam, h) -> exact easting and northing -> rounded to double: those doubles are the
    input.  The expected values are the exact image of the ROUNDED input (re-solved), kept as hi + lo doubles."""
    proj = factory() if factory else None
    if proj is None:
        xyz = np.array([(lon, lat, h) for lat, lon, h in rows], dtype=np.float64)
    else:
        xyz = np.array([tuple(float(v) for v in proj.forward(mp.radians(mp.mpf(lat)), mp.radians(mp.mpf(lon)))) + (h,)
                        for lat, lon, h in rows], dtype=np.float64)
    images = [image(proj, x, y, z) for x, y, z in xyz]
    ecef_hi, ecef_lo = split([im[0] for im in images])
    geo_hi, geo_lo = split([im[1] for im in images])
    return dict(definition=definition, xyz=xyz, ecef_hi=ecef_hi, ecef_lo=ecef_lo, wgs84_hi=geo_hi, wgs84_lo=geo_lo)


FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "srs_points.npz")


@functools.lru_cache(maxsize=None)
def points():
    """The about 300 points of the accuracy tests, as make_group made them (python tests/srs_ref.py writes the fixture; a
    CPU test makes a sample of the groups again and compares).  A list of groups: definition, xyz (n, 3), and the expected
    ECEF and WGS84 (longitude, latitude in radians, height) as hi + lo."""
    with np.load(FIXTURE) as z:
        first = z["first"]
        out = []
        for g, definition in enumerate(z["definitions"]):
            rows = slice(int(first[g]), int(first[g + 1]))
            out.append(dict(definition=str(definition), **{k: z[k][rows] for k in ("xyz", "ecef_hi", "ecef_lo", "wgs84_hi", "wgs84_lo")}))
    return out




def errors(got, hi, lo, angles=()):
    """|got - (hi + lo)| per element; the columns in `angles` are compared on the circle (-pi and pi are one meridian)"""
    d = np.abs((np.asarray(got, dtype=np.float64) - hi) - lo)
    for c in angles:
        d[:, c] = np.minimum(d[:, c], np.abs(2 * np.pi - d[:, c]))
    return d


def write_fixture():
    groups = [make_group(*g) for g in group_rows()]
    first = np.cumsum([0] + [len(g["xyz"]) for g in groups])
    np.savez(FIXTURE, definitions=np.array([g["definition"] for g in groups]), first=first,
             **{k: np.concatenate([g[k] for g in groups]) for k in ("xyz", "ecef_hi", "ecef_lo", "wgs84_hi", "wgs84_lo")})


if __name__ == "__main__":
    write_fixture()
