"""The region predicates of include/swz_gpu.h restated in numpy, operation for operation: every *, + and - below is one rounded
double operation on arrays, in the order the header writes them.  Test infrastructure only: never the thing under test."""
import numpy as np


def box_mask(xyz, box):
    lo, hi = np.asarray(box[0], dtype=np.float64), np.asarray(box[1], dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return ((xyz >= lo) & (xyz <= hi)).all(axis=1)


def planes_mask(xyz, planes):
    """every plane: ((a*x + b*y) + c*z) + d >= 0"""
    x, y, z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    m = np.ones(len(xyz), bool)
    for a, b, c, d in np.asarray(planes, dtype=np.float64).reshape(-1, 4):
        m &= ((a * x + b * y) + c * z) + d >= 0.0
    return m


def polygon_mask(xyz, vertices):
    """even-odd: edge i counts iff (y0 > py) != (y1 > py) and (t > 0) == (y1 > y0), t = (x1 - x0)*(py - y0) - (px - x0)*(y1 - y0)"""
    v = np.asarray(vertices, dtype=np.float64).reshape(-1, 2)
    px, py = xyz[:, 0], xyz[:, 1]
    odd = np.zeros(len(xyz), bool)
    for i in range(len(v)):
        (x0, y0), (x1, y1) = v[i], v[(i + 1) % len(v)]
        t = (x1 - x0) * (py - y0) - (px - x0) * (y1 - y0)
        odd ^= ((y0 > py) != (y1 > py)) & ((t > 0.0) == (y1 > y0))
    return odd


def region_mask(xyz, box, region):
    """region: None, ("box",), ("planes", k x 4) or ("polygon", m x 2).  The box test first: it keeps NaN out of the kind tests."""
    xyz = np.asarray(xyz, dtype=np.float64).reshape(-1, 3)
    m = box_mask(xyz, box)
    if region is None or region[0] == "box":
        return m
    rows = np.flatnonzero(m)
    kind = planes_mask if region[0] == "planes" else polygon_mask
    m[rows] = kind(xyz[rows], region[1])
    return m


def as_region(swz, region):
    """the library's Region of a region given as above"""
    if region is None:
        return None
    if region[0] == "box":
        return swz.Region.box()
    return swz.Region.planes(region[1]) if region[0] == "planes" else swz.Region.polygon(region[1])


def look_at_view_proj(eye, target, up=(0.0, 0.0, 1.0), fovy_deg=40.0, aspect=1.25, near=0.1, far=3.0):
    """a row-major OpenGL-style view-projection matrix (clip = M (x, y, z, 1)) of a fixed camera"""
    eye, target, up = (np.asarray(v, dtype=np.float64) for v in (eye, target, up))
    f = target - eye
    f /= np.linalg.norm(f)
    s = np.cross(f, up)
    s /= np.linalg.norm(s)
    u = np.cross(s, f)
    view = np.eye(4)
    view[0, :3], view[1, :3], view[2, :3] = s, u, -f
    view[:3, 3] = -view[:3, :3] @ eye
    t = 1.0 / np.tan(np.radians(fovy_deg) / 2)
    proj = np.array([[t / aspect, 0, 0, 0], [0, t, 0, 0], [0, 0, (far + near) / (near - far), 2 * far * near / (near - far)], [0, 0, -1, 0]])
    return proj @ view


SQUARE = np.array([[16, 16], [48, 16], [48, 48], [16, 48]]) / 64.0
L_SHAPE = np.array([[16, 16], [48, 16], [48, 32], [32, 32], [32, 48], [16, 48]]) / 64.0          # notch: x, y in (1/2, 3/4)
U_SHAPE = np.array([[16, 16], [48, 16], [48, 48], [40, 48], [40, 24], [24, 24], [24, 48], [16, 48]]) / 64.0
BOW_TIE = np.array([[16, 16], [48, 48], [48, 16], [16, 48]]) / 64.0                              # self-intersecting at the centre


def circle(m=1024, centre=(0.5, 0.5), radius=0.25):
    a = 2 * np.pi * np.arange(m) / m
    return np.stack([centre[0] + radius * np.cos(a), centre[1] + radius * np.sin(a)], axis=1)
