"""The raster contract of include/swz_gpu.h restated in numpy: the frame of a grid, the cell of a row, q, the table and its
decode.  Every -, / and floor below is one rounded double operation on arrays, in the order the header writes them.  min and max
are taken on the values themselves (np.minimum.at), never on codes.  Test infrastructure only: never the thing under test."""
import math

import numpy as np

import region_ref as R

VALUE_Z = "z"
SIGNED = ("scan_angle_rank",)
ONE_OR_TWO_BYTES = ("intensity", "classification", "edge_of_flight_line", "number_of_returns", "return_number", "point_source_id",
                    "scan_direction_flag", "scan_angle_rank", "user_data")


def frame_of(box_min, box_max, nx, ny, value=VALUE_Z):
    lo, hi = np.asarray(box_min, dtype=np.float64), np.asarray(box_max, dtype=np.float64)
    f = dict(x0=float(lo[0]), y0=float(lo[1]), cw=float((hi[0] - lo[0]) / np.float64(nx)), ch=float((hi[1] - lo[1]) / np.float64(ny)),
             v0=0.0, scale=1.0, nx=int(nx), ny=int(ny), value=value)
    if value == VALUE_Z:
        rng = float(hi[2] - lo[2])
        k = 0 if rng == 0.0 else min(900, max(-900, 30 - (math.frexp(rng)[1] - 1)))   # ilogb(x) = frexp's exponent - 1
        f["v0"], f["scale"] = float(lo[2]), math.ldexp(1.0, k)
    return f


def _axis(p, p0, side, cells):
    if cells == 1:
        return np.zeros(len(p), dtype=np.int64)
    return np.minimum(np.floor((p - np.float64(p0)) / np.float64(side)), np.float64(cells - 1)).astype(np.int64)


def cell_index(frame, xyz):
    """of rows inside the box"""
    return _axis(xyz[:, 1], frame["y0"], frame["ch"], frame["ny"]) * frame["nx"] + _axis(xyz[:, 0], frame["x0"], frame["cw"], frame["nx"])


def values_of(frame, xyz, column=None):
    """v as doubles, q as int64"""
    if frame["value"] == VALUE_Z:
        v = xyz[:, 2].astype(np.float64)
        return v, np.rint((v - np.float64(frame["v0"])) * np.float64(frame["scale"])).astype(np.int64)   # rint: ties to even, as llrint
    col = np.asarray(column)
    return col.astype(np.float64), col.astype(np.int64)


def empty_table(frame):
    n = frame["nx"] * frame["ny"]
    return dict(count=np.zeros(n, dtype=np.uint64), sum=np.zeros(n, dtype=np.int64), min=np.full(n, np.inf), max=np.full(n, -np.inf))


def accumulate(frame, table, xyz, box, column=None, keep=None):
    """adds the rows of the closed box (and of `keep`, a mask, where given) to the table"""
    xyz = np.asarray(xyz, dtype=np.float64).reshape(-1, 3)
    m = R.box_mask(xyz, box)
    if keep is not None:
        m &= keep
    rows = xyz[m]
    v, q = values_of(frame, rows, None if column is None else np.asarray(column)[m])
    cell = cell_index(frame, rows)
    np.add.at(table["count"], cell, np.uint64(1))
    np.add.at(table["sum"], cell, q)
    np.minimum.at(table["min"], cell, v)
    np.maximum.at(table["max"], cell, v)
    return table


def raster(box, nx, ny, xyz, value=VALUE_Z, column=None, keep=None):
    frame = frame_of(box[0], box[1], nx, ny, value)
    return frame, accumulate(frame, empty_table(frame), xyz, box, column, keep)


def finish(frame, table):
    """dict(count, min, max, mean) of shape (ny, nx): mean = v0 + (sum / count) / scale, three rounded operations"""
    shape = (frame["ny"], frame["nx"])
    count = table["count"]
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = np.float64(frame["v0"]) + (table["sum"].astype(np.float64) / count.astype(np.float64)) / np.float64(frame["scale"])
    mean = np.where(count == 0, np.nan, mean)
    return dict(count=count.reshape(shape), min=table["min"].reshape(shape), max=table["max"].reshape(shape), mean=mean.reshape(shape))


def same_table(got, frame, table):
    """a result of the library (dict with count, sum, min, max of shape (ny, nx)) against a table of this file: the integer
    fields exactly, min and max by value (+0.0 equals -0.0)"""
    shape = (frame["ny"], frame["nx"])
    return (np.array_equal(got["count"], table["count"].reshape(shape)) and np.array_equal(got["sum"], table["sum"].reshape(shape))
            and np.array_equal(got["min"], table["min"].reshape(shape)) and np.array_equal(got["max"], table["max"].reshape(shape)))
