"""The source projection on the host: swz_srs_parse, swz_srs_transform, swz_srs_transform_box and swz_las_scan_files_srs.

The numbers come from srs_ref.py (mpmath at 40 digits, no series).  ACCURACY CONDITION: every output coordinate within 1 um of
the reference (1 um / 6.4e6 m in angle for the WGS84 target) -- two orders below the finest LAS scale in use, far above double
rounding at 6.4e6 m.  Measured on the host build: 2.6e-9 m."""
import math
import os

import numpy as np
import pytest

import srs_ref as R
from las_input_util import LasTile, make_cubic

ERR_BAD_ARG = 2
TOL_M = 1e-6
TOL_RAD = 1e-6 / 6.4e6
UTM32 = "+proj=utm +zone=32 +datum=WGS84"


def _fields(definition):
    import schwarzwald_amd as swz
    return swz.Srs(definition).fields()


# ---------------------------------------------------------------------------------------------------------- the reference
def test_reference_premises():
    """On the central meridian the reference's northing is k_0 times the meridian arc, and its map is conformal: the
    Cauchy-Riemann equations hold for (easting, northing) as functions of (lam, psi), psi the isometric latitude."""
    mp = R.mp
    proj = R.TMerc.utm(32)
    for lat in (0.25, 33.0, 71.5):
        phi = mp.radians(mp.mpf(lat))
        arc = proj.a * (1 - proj.e2) * mp.quad(proj.integrand, [0, phi])
        e, n = proj.forward(phi, proj.lon_0)
        assert abs(e - 500000) < mp.mpf(10) ** -30 and abs(n - proj.k_0 * arc) < mp.mpf(10) ** -28
    h = mp.mpf(10) ** -12
    for lat, dlon in ((10.0, 2.5), (48.0, -3.0), (80.0, 4.0)):
        phi, lam = mp.radians(mp.mpf(lat)), proj.lon_0 + mp.radians(mp.mpf(dlon))
        dpsi_dphi = (1 - proj.e2) / ((1 - proj.e2 * mp.sin(phi) ** 2) * mp.cos(phi))
        e_lam = (proj.forward(phi, lam + h)[0] - proj.forward(phi, lam - h)[0]) / (2 * h)
        n_lam = (proj.forward(phi, lam + h)[1] - proj.forward(phi, lam - h)[1]) / (2 * h)
        e_psi = (proj.forward(phi + h, lam)[0] - proj.forward(phi - h, lam)[0]) / (2 * h) / dpsi_dphi
        n_psi = (proj.forward(phi + h, lam)[1] - proj.forward(phi - h, lam)[1]) / (2 * h) / dpsi_dphi
        # central differences with h = 1e-12 at 40 digits: the truncation is h^2 f''' ~ 1e-17 m
        assert abs(e_lam - n_psi) < mp.mpf(10) ** -12 and abs(e_psi + n_lam) < mp.mpf(10) ** -12
    # forward and inverse are each other's inverse
    phi, lam = proj.inverse(*proj.forward(mp.radians(47), proj.lon_0 + mp.radians(3)))
    assert abs(phi - mp.radians(47)) < mp.mpf(10) ** -30 and abs(lam - proj.lon_0 - mp.radians(3)) < mp.mpf(10) ** -30


def test_fixture_is_what_the_reference_makes():
    """tests/golden/srs_points.npz is the output of srs_ref.make_group: three rows of EVERY group made again (the first,
    one from the middle, the last), the OSGB-like tmerc with lat_0 != 0 on an +a +rf ellipsoid among them"""
    have = {g["definition"]: g for g in R.points()}
    assert sum(len(g["xyz"]) for g in have.values()) == 304
    made = 0
    for definition, factory, rows in R.group_rows():
        assert len(rows) == len(have[definition]["xyz"])
        pick = [0, len(rows) // 2 + 1, len(rows) - 1]
        again = R.make_group(definition, factory, [rows[i] for i in pick])
        for k in ("xyz", "ecef_hi", "ecef_lo", "wgs84_hi", "wgs84_lo"):
            assert np.array_equal(again[k], have[definition][k][pick]), (definition, k)
        made += 1
    assert made == 10 and R.OSGB_LIKE["definition"] in have
    # the near-equator rows are within 1" of it, zones 1 and 60 reach across the antimeridian
    g = have[R.utm_definition(32, False)]
    assert ((np.abs(g["wgs84_hi"][:, 1]) > 0) & (np.abs(g["wgs84_hi"][:, 1]) < math.radians(1 / 3600))).any()


# ---------------------------------------------------------------------------------------------------------- the definition
def test_parse_accepts():
    import schwarzwald_amd as swz
    utm = _fields(UTM32)
    assert utm["kind"] == swz.SRS_TMERC and utm["a"] == 6378137.0 and utm["f"] == 1 / 298.257223563
    assert utm["k_0"] == 0.9996 and utm["x_0"] == 500000.0 and utm["y_0"] == 0.0 and utm["lat_0"] == 0.0 and utm["xi_0"] == 0.0
    assert utm["lon_0"] == 9.0 * (math.pi / 180.0)
    n = utm["n"]
    assert n == utm["f"] / (2 - utm["f"]) and utm["e2"] == utm["f"] * (2 - utm["f"])
    # the terms everyone knows
    assert abs(utm["beta"][0] - (n / 2 - 2 * n ** 2 / 3 + 37 * n ** 3 / 96)) < 2 * n ** 4
    assert abs(utm["radius"] / utm["k_0"] - 6378137.0 / (1 + n) * (1 + n ** 2 / 4 + n ** 4 / 64 + n ** 6 / 256)) < 1e-8
    assert abs(utm["radius"] / utm["k_0"] - 6367449.145823) < 1e-5                # the WGS84 rectifying radius
    same = ["+proj=tmerc +lat_0=0 +lon_0=9 +k=0.9996 +x_0=500000 +y_0=0 +datum=WGS84",
            "+proj=tmerc +lon_0=9 +k_0=0.9996 +x_0=500000 +ellps=WGS84 +units=m +no_defs +type=crs",
            "  +proj=utm\t+zone=32 +ellps=WGS84 +datum=WGS84 +units=m +no_defs ", "EPSG:32632", "epsg:32632",
            "+proj=utm +zone=32 +a=6378137 +rf=298.257223563"]
    for d in same:
        assert _fields(d) == utm, d
    assert _fields("EPSG:25832") == _fields("+proj=utm +zone=32 +ellps=GRS80") != utm
    assert _fields("EPSG:25832")["f"] == 1 / 298.257222101
    south = _fields("+proj=utm +zone=32 +south +datum=WGS84")
    assert south["y_0"] == 1e7 and _fields("EPSG:32732") == south and {**south, "y_0": 0.0} == utm
    assert _fields("EPSG:32601")["lon_0"] == -177.0 * (math.pi / 180.0) and _fields("EPSG:32660")["lon_0"] == 177.0 * (math.pi / 180.0)
    assert _fields("EPSG:25828")["lon_0"] == -15.0 * (math.pi / 180.0) and _fields("EPSG:25838")["lon_0"] == 45.0 * (math.pi / 180.0)
    ll = _fields("+proj=longlat +datum=WGS84")
    assert ll["kind"] == swz.SRS_LONGLAT and _fields("+proj=latlong +ellps=WGS84 +no_defs") == ll
    osgb = _fields(R.OSGB_LIKE["definition"])
    assert osgb["a"] == 6377563.396 and osgb["f"] == 1 / 299.3249646 and osgb["k_0"] == 0.9996012717 and osgb["y_0"] == -100000.0
    assert abs(osgb["xi_0"] * osgb["radius"] - float(R.OSGB_LIKE["proj"]().mu_0 * R.OSGB_LIKE["proj"]().A * R.mp.mpf("0.9996012717"))) < 1e-8
    b = _fields("+proj=tmerc +a=6378137 +b=6356752.314245179 +lon_0=9 +k=0.9996 +x_0=500000")
    assert abs(b["f"] - utm["f"]) < 1e-15 and _fields("+proj=tmerc +a=6371000 +b=6371000")["n"] == 0.0


@pytest.mark.parametrize("definition,token", [
    ("+proj=merc +datum=WGS84", "+proj=merc"), ("+proj=lcc +lat_1=49 +datum=WGS84", "+lat_1=49"), ("+proj=geocent +datum=WGS84", "+proj=geocent"),
    (UTM32 + " +towgs84=0,0,0,0,0,0,0", "+towgs84=0,0,0,0,0,0,0"), (UTM32 + " +nadgrids=@null", "+nadgrids=@null"),
    (UTM32 + " +geoidgrids=egm96_15.gtx", "+geoidgrids=egm96_15.gtx"), (UTM32 + " +vunits=ft", "+vunits=ft"),
    (UTM32 + " +units=us-ft", "+units=us-ft"), (UTM32 + " +units=km", "+units=km"), (UTM32 + " +axis=neu", "+axis=neu"),
    (UTM32 + " +pm=paris", "+pm=paris"), (UTM32 + " +approx", "+approx"), ("EPSG:4326", "EPSG:4326"), ("EPSG:3857", "EPSG:3857"),
    ("EPSG:32661", "EPSG:32661"), ("EPSG:25839", "EPSG:25839"), ("EPSG:32600", "EPSG:32600"), ("EPSG:326x2", "EPSG:326x2"),
    ("EPSG:32632.0", "EPSG:32632.0"), ("EPSG:+32632", "EPSG:+32632"), ("EPSG:0x7F78", "EPSG:0x7F78"), ("EPSG:", "EPSG:"),
    ("+proj=utm +zone=0x20 +datum=WGS84", "+zone=0x20"), ("+proj=tmerc +k=0x1p0 +datum=WGS84", "+k=0x1p0"),
    ("+proj=tmerc +k=0,9996 +datum=WGS84", "+k=0,9996"), ("+proj=tmerc +lon_0=+-9 +datum=WGS84", "+lon_0=+-9"),
    ('PROJCS["WGS 84 / UTM zone 32N",GEOGCS["WGS 84"]]', "WKT"), ('GEOGCRS["WGS 84"]', "WKT"),
    ("+proj=utm +zone=0 +datum=WGS84", "+zone=0"), ("+proj=utm +zone=61 +datum=WGS84", "+zone=61"),
    ("+proj=utm +zone=32.5 +datum=WGS84", "+zone=32.5"), ("+proj=utm +zone=abc +datum=WGS84", "+zone=abc"),
    ("+proj=utm +datum=WGS84", "+zone"), ("+proj=utm +zone=32", "ellipsoid"), ("+proj=utm +zone=32 +ellps=bessel", "+ellps=bessel"),
    ("+proj=utm +zone=32 +datum=NAD27", "+datum=NAD27"), ("+proj=utm +zone=32 +ellps=GRS80 +datum=WGS84", "+ellps=GRS80"),
    ("+proj=utm +zone=32 +a=nan +rf=298", "+a=nan"), ("+proj=utm +zone=32 +a=inf +rf=298", "+a=inf"),
    ("+proj=utm +zone=32 +a=-6378137 +rf=298", "+a=-6378137"), ("+proj=utm +zone=32 +a=0 +rf=298", "+a=0"),
    ("+proj=utm +zone=32 +a=6378137 +rf=0", "+rf=0"), ("+proj=utm +zone=32 +a=6378137 +rf=nan", "+rf=nan"),
    ("+proj=utm +zone=32 +a=6378137 +b=-1", "+b=-1"), ("+proj=utm +zone=32 +a=6378137 +b=inf", "+b=inf"),
    ("+proj=utm +zone=32 +a=6378137", "+a=6378137"), ("+proj=utm +zone=32 +rf=298.2", "+rf=298.2"),
    ("+proj=utm +zone=32 +datum=WGS84 +a=6378137 +rf=298", "+a=6378137"),
    ("+proj=tmerc +zone=32 +datum=WGS84", "+zone=32"), ("+proj=tmerc +south +datum=WGS84", "+south"),
    ("+proj=utm +zone=32 +lon_0=9 +datum=WGS84", "+lon_0=9"), ("+proj=longlat +lon_0=9 +datum=WGS84", "+lon_0=9"),
    ("+proj=tmerc +lon_0=9x +datum=WGS84", "+lon_0=9x"), ("+proj=tmerc +k=0 +datum=WGS84", "+k=0"), ("+proj=tmerc +k=nan +datum=WGS84", "+k=nan"),
    ("+proj=tmerc +lat_0=91 +datum=WGS84", "+lat_0=91"), ("+proj=utm +zone=32 +zone=33 +datum=WGS84", "+zone=33"),
    ("+proj=utm +zone=32 +type=bound +datum=WGS84", "+type=bound"), ("proj=utm zone=32", "proj=utm"), ("+datum=WGS84 +zone=32", "+proj"),
    ("utm32", "utm32"), ("", "empty"), ("   \t ", "empty")])
def test_parse_refuses_by_name(definition, token):
    import schwarzwald_amd as swz
    with pytest.raises(swz.SwzError) as e:
        swz.Srs(definition)
    assert e.value.code == ERR_BAD_ARG and token in str(e.value), str(e.value)
    # ... and the call with a context's place for the text, given none, returns the same status
    out = swz.api._Srs()
    assert swz.load_library().swz_srs_parse(None, definition.encode(), out) == ERR_BAD_ARG


# ---------------------------------------------------------------------------------------------------------- the map
def test_host_map_within_a_micrometre_of_the_reference(capsys):
    import schwarzwald_amd as swz
    worst_m, worst_rad = 0.0, 0.0
    for g in R.points():
        got = swz.srs_transform(g["definition"], g["xyz"], swz.SRS_ECEF)
        worst_m = max(worst_m, R.errors(got, g["ecef_hi"], g["ecef_lo"]).max())
        geo = swz.srs_transform(swz.Srs(g["definition"]), g["xyz"], swz.SRS_WGS84)
        assert np.array_equal(geo[:, 2], g["xyz"][:, 2])                          # the height stays
        assert (np.abs(geo[:, 0]) <= math.pi).all()
        worst_rad = max(worst_rad, R.errors(geo, g["wgs84_hi"], g["wgs84_lo"], angles=(0,))[:, :2].max())
    with capsys.disabled():
        print("\nsrs host map: max |error| %.3g m (ECEF), %.3g rad (WGS84)" % (worst_m, worst_rad))
    assert worst_m <= TOL_M and worst_rad <= TOL_RAD


def test_nonfinite_and_far_outside():
    import schwarzwald_amd as swz
    for definition in (UTM32, R.LONGLAT):
        for target in (swz.SRS_ECEF, swz.SRS_WGS84):
            for bad in (float("nan"), float("inf"), float("-inf")):
                for col in (0, 1):
                    p = np.array([[500000.0, 5300000.0, 100.0]]) if definition == UTM32 else np.array([[9.0, 48.0, 100.0]])
                    p[0, col] = bad
                    out = swz.srs_transform(definition, p, target)
                    assert not np.isfinite(out[0, :2]).all(), (definition, target, bad, col, out)
        p = np.array([[500000.0, 5300000.0, float("nan")]]) if definition == UTM32 else np.array([[9.0, 48.0, float("nan")]])
        assert np.isnan(swz.srs_transform(definition, p)).all()
    # 5 000 km off the central meridian, and absurd coordinates: the call returns; the values are unspecified
    far = np.array([[5500000.0, 5300000.0, 0.0], [-4500000.0, 100.0, 0.0], [1e300, -1e300, 0.0], [1e18, 1e18, 1e18], [0.0, 1e9, 0.0]])
    assert swz.srs_transform(UTM32, far).shape == (5, 3) and swz.srs_transform(UTM32, far, swz.SRS_WGS84).shape == (5, 3)
    assert swz.srs_transform(UTM32, np.empty((0, 3))).shape == (0, 3)
    with pytest.raises(ValueError):
        swz.srs_transform(UTM32, far, 2)


# ---------------------------------------------------------------------------------------------------------- the box
def _corners(mn, mx):
    return np.array([[(mx if i & 1 else mn)[0], (mx if i & 2 else mn)[1], (mx if i & 4 else mn)[2]] for i in range(8)])


def test_box_is_the_min_max_of_eight_corners():
    import schwarzwald_amd as swz
    for definition, mn, mx in ((UTM32, [412000.0, 5401000.0, 200.0], [414000.0, 5403000.0, 900.0]),
                               ("EPSG:32733", [200000.0, 7000000.0, -30.0], [200600.0, 7000600.0, 10.0]),
                               (R.LONGLAT, [8.0, 47.0, 0.0], [9.0, 48.0, 100.0])):
        for target in (swz.SRS_ECEF, swz.SRS_WGS84):
            c = swz.srs_transform(definition, _corners(mn, mx), target)
            lo, hi = swz.srs_transform_box(definition, mn, mx, target)
            assert np.array_equal(lo, c.min(axis=0)) and np.array_equal(hi, c.max(axis=0))


def test_premise_a_flat_tile_bulges():
    """By the reference alone: the mid-point of the top edge (y and z at their maxima) of a 2 km UTM tile lies outside the box
    of its eight corners in ECEF, by centimetres -- (1 km)^2 / (2 R) = 8 cm along the local vertical."""
    proj = R.TMerc.utm(32)
    mn, mx = [499000.0, 5400000.0, 200.0], [501000.0, 5402000.0, 240.0]   # astride the central meridian
    corners = np.array([[float(v) for v in R.image(proj, *c)[0]] for c in _corners(mn, mx)])
    mid = np.array([float(v) for v in R.image(proj, 500000.0, mx[1], mx[2])[0]])
    outside = np.maximum(mid - corners.max(axis=0), corners.min(axis=0) - mid).max()
    assert 0.01 < outside < 0.2
    import schwarzwald_amd as swz
    lo, hi = swz.srs_transform_box(UTM32, mn, mx)
    got = swz.srs_transform(UTM32, [[500000.0, mx[1], mx[2]]])[0]
    assert abs(np.maximum(got - hi, lo - got).max() - outside) < 1e-5          # the library neither widens the box nor refuses


# ---------------------------------------------------------------------------------------------------------- the scan
def test_scan_with_a_projection(tmp_path):
    import schwarzwald_amd as swz
    rng = np.random.default_rng(5)
    a = LasTile(rng, 50, 3, offset=(412000.0, 5401000.0, 250.0), lo=0, hi=2 ** 19)
    b = LasTile(rng, 70, 7, offset=(415000.0, 5404000.0, 300.0), lo=0, hi=2 ** 19, clamp=True)
    paths = [a.write(tmp_path / "a.las"), b.write(tmp_path / "b.las")]
    assert a.bmax[0] < b.bmin[0] and a.bmax[1] < b.bmin[1]                        # disjoint boxes
    plain_files, plain = swz.las_scan_files(paths)
    again_files, again = swz.las_scan_files(paths, srs=None)
    assert plain_files == again_files and all(np.array_equal(np.concatenate(plain[k]), np.concatenate(again[k])) for k in ("tight", "cubic", "origin"))
    files, ds = swz.las_scan_files(paths, srs=UTM32)
    assert files == plain_files and files[0]["min"] == a.bmin and files[1]["max"] == b.bmax     # the layouts are untransformed
    boxes = [swz.srs_transform_box(UTM32, t.bmin, t.bmax) for t in (a, b)]
    tmin, tmax = np.minimum(boxes[0][0], boxes[1][0]), np.maximum(boxes[0][1], boxes[1][1])
    assert np.array_equal(ds["tight"][0], tmin) and np.array_equal(ds["tight"][1], tmax)
    union = swz.srs_transform_box(UTM32, plain["tight"][0], plain["tight"][1])
    assert not (np.array_equal(union[0], tmin) and np.array_equal(union[1], tmax))   # transform, then union -- not the reverse
    cubic, origin, center = make_cubic(tmin, tmax)
    for got, want in ((ds["cubic"], cubic), (ds["origin"], origin)):
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert np.array_equal(ds["center"], center) and ds["total_points"] == 120 and ds["attrs"] == plain["attrs"]
    assert 6.3e6 < np.linalg.norm(ds["center"]) < 6.4e6                            # on the globe
    # an Srs object, and the skip flag, go the same way
    assert np.array_equal(swz.las_scan_files(paths + [str(tmp_path / "none.las")], skip_unreadable=True, srs=swz.Srs(UTM32))[1]["center"], center)


def test_numbers_do_not_depend_on_the_locale_and_structs_are_checked():
    """a comma-decimal LC_NUMERIC in the process leaves +k=0.9996 what it is; a zeroed or unset swz_srs is refused by every
    host entry point instead of passing for longlat"""
    import ctypes as C
    import locale
    import schwarzwald_amd as swz
    want = _fields("+proj=tmerc +lon_0=9.5 +k=0.9996 +x_0=500000.25 +datum=WGS84")
    old = locale.setlocale(locale.LC_NUMERIC)
    tried = 0
    try:
        for name in ("de_DE.UTF-8", "de_DE.utf8", "fr_FR.UTF-8", "de_DE"):
            try:
                locale.setlocale(locale.LC_NUMERIC, name)
            except locale.Error:
                continue
            tried += 1
            assert _fields("+proj=tmerc +lon_0=9.5 +k=0.9996 +x_0=500000.25 +datum=WGS84") == want
            assert _fields("+proj=tmerc +lon_0=+9.5 +k=9996e-4 +x_0=5.0000025e5 +datum=WGS84") == want
    finally:
        locale.setlocale(locale.LC_NUMERIC, old)
    assert _fields("+proj=tmerc +lon_0=+9.5 +k=9996e-4 +x_0=5.0000025e5 +datum=WGS84") == want   # (whether or not such a locale exists here)
    L = swz.load_library()
    p = np.array([[9.0, 48.0, 0.0]])
    dp = C.POINTER(C.c_double)
    box = [(C.c_double * 3)() for _ in range(4)]
    for bad in (swz.api._Srs(), swz.api._Srs(kind=7, a=6378137.0), swz.api._Srs(kind=swz.SRS_TMERC, a=6378137.0, f=0.003)):
        assert L.swz_srs_transform(C.byref(bad), swz.SRS_ECEF, p.ctypes.data_as(dp), 1) == ERR_BAD_ARG
        assert L.swz_srs_transform_box(C.byref(bad), swz.SRS_ECEF, *box) == ERR_BAD_ARG
        ds = swz.api._LasDataset()
        assert L.swz_las_scan_files_srs(None, None, 0, 0, C.byref(bad), None, C.byref(ds)) == ERR_BAD_ARG
    assert np.array_equal(p, [[9.0, 48.0, 0.0]])
