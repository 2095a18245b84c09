"""The filter contract of include/swz_gpu.h restated in numpy.  A filter is a list of clauses (None or []: no filter):
    ("range", name, lo, hi)      lo <= (double)v && (double)v <= hi, closed; a NaN fails both compares
    ("not_range", name, lo, hi)  the same, inverted: a NaN passes
    ("any_of", name, values)     bit (uint8)v of the 256-bit map is set
    ("none_of", name, values)    the same, inverted
A row passes iff it passes every clause.  Test infrastructure only: never the thing under test."""
import numpy as np

import region_ref as R

SCALARS = ("intensity", "classification", "edge_of_flight_line", "gps_time", "number_of_returns", "return_number", "point_source_id",
           "scan_direction_flag", "scan_angle_rank", "user_data")
ONE_BYTE = tuple(k for k in SCALARS if k not in ("intensity", "gps_time", "point_source_id"))


def clause_mask(col, clause):
    kind = clause[0]
    if kind in ("range", "not_range"):
        v = np.asarray(col).astype(np.float64)             # exact for uint8, int8, uint16 and double
        with np.errstate(invalid="ignore"):
            m = (np.float64(clause[2]) <= v) & (v <= np.float64(clause[3]))
        return ~m if kind == "not_range" else m
    bits = np.zeros(256, bool)
    for x in clause[2]:
        bits[int(x) & 255] = True                          # the stored byte read as unsigned: -1 is bit 255
    m = bits[np.asarray(col).view(np.uint8)]
    return ~m if kind == "none_of" else m


def filter_mask(cols, filter):
    n = len(next(iter(cols.values()))) if cols else 0
    m = np.ones(n, bool)
    for clause in filter or ():
        m &= clause_mask(cols[clause[1]], clause)
    return m


def select_mask(xyz, cols, box, region, filter):
    """region_mask & filter_mask"""
    m = R.region_mask(xyz, box, region)
    return m & filter_mask(cols, filter) if filter else m


def filter_names(filter):
    return tuple(dict.fromkeys(c[1] for c in filter or ()))


def as_filter(swz, filter):
    """the binding's Filter of a filter given as above"""
    if filter is None:
        return None
    f = swz.Filter()
    for c in filter:
        if c[0] == "range":
            f.range(c[1], c[2], c[3])
        elif c[0] == "not_range":
            f.clause(c[1], swz.FILTER_RANGE | swz.FILTER_NOT, c[2], c[3])
        elif c[0] == "any_of":
            f.any_of(c[1], c[2])
        else:
            f.none_of(c[1], c[2])
    return f
