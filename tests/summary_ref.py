"""Per-node attribute summaries and the node rule of a filtered query, as include/swz_gpu.h states them, in numpy.

An entry is one record of DTYPE (swz_attr_summary): for a one-byte column the 256-bit set of the stored bytes and lo / hi
derived from it (scan_angle_rank read as signed); for intensity, point_source_id and gps_time the exact min and max as doubles,
NaN left out and flagged.  A node without values has lo = +inf, hi = -inf.  Filters are filter_ref's clause lists.  Test
infrastructure only: never the thing under test."""
import numpy as np

import filter_ref as F

DTYPE = np.dtype([("lo", "<f8"), ("hi", "<f8"), ("set", "<u8", (4,)), ("flags", "<u4"), ("reserved", "<u4")])
HAS_NAN = 1
INDEX = {"intensity": 2, "classification": 3, "edge_of_flight_line": 4, "gps_time": 5, "number_of_returns": 6, "return_number": 7,
         "point_source_id": 8, "scan_direction_flag": 9, "scan_angle_rank": 10, "user_data": 11}
assert tuple(INDEX) == F.SCALARS


def ordered(names):
    """the columns of a mask in the order of its entries: ascending attribute index"""
    return sorted(names, key=INDEX.__getitem__)


def _byte_value(name, b):
    return float(np.int8(np.uint8(b))) if name == "scan_angle_rank" else float(b)


def entry(name, values):
    """the summary of one node's values of one column"""
    e = np.zeros((), dtype=DTYPE)
    e["lo"], e["hi"] = np.inf, -np.inf
    v = np.asarray(values)
    if name in F.ONE_BYTE:
        words = [0, 0, 0, 0]
        for b in np.unique(v.view(np.uint8)):
            words[int(b) >> 6] |= 1 << (int(b) & 63)
        e["set"] = np.array(words, dtype=np.uint64)
        held = [_byte_value(name, b) for b in range(256) if (words[b >> 6] >> (b & 63)) & 1]
        if held:
            e["lo"], e["hi"] = min(held), max(held)
        return e
    d = v.astype(np.float64)
    nan = np.isnan(d)
    if nan.any():
        e["flags"] = HAS_NAN
    if (~nan).any():
        e["lo"], e["hi"] = d[~nan].min(), d[~nan].max()
    return e


def summaries(cols, names, offset, count):
    """entries[k, j]: node k (rows offset[k] .. offset[k] + count[k]) and the j-th of ordered(names)"""
    names = ordered(names)
    out = np.zeros((len(offset), len(names)), dtype=DTYPE)
    for k, (o, c) in enumerate(zip(offset, count)):
        for j, name in enumerate(names):
            out[k, j] = entry(name, cols[name][int(o):int(o) + int(c)])
    return out


def same(a, b):
    """do two arrays of entries say the same?  +0.0 and -0.0 are one value; everything else compares exactly"""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool((a["lo"] == b["lo"]).all() and (a["hi"] == b["hi"]).all() and (a["set"] == b["set"]).all() and
                                       (a["flags"] == b["flags"]).all() and (a["reserved"] == b["reserved"]).all())


def clause_unreachable(e, clause):
    """the rule: has the node of entry e no row that could pass the clause?"""
    kind, name = clause[0], clause[1]
    negate = kind in ("not_range", "none_of")
    if name in F.ONE_BYTE:
        words = [int(w) for w in e["set"]]
        for b in range(256):
            if not (words[b >> 6] >> (b & 63)) & 1:
                continue
            if kind in ("any_of", "none_of"):
                ok = b in {int(x) & 255 for x in clause[2]}
            else:
                ok = np.float64(clause[2]) <= _byte_value(name, b) <= np.float64(clause[3])
            if ok != negate:
                return False
        return True
    lo, hi = np.float64(clause[2]), np.float64(clause[3])
    if not negate:
        return bool(e["hi"] < lo or e["lo"] > hi)
    return bool(not (int(e["flags"]) & HAS_NAN) and lo <= e["lo"] and e["hi"] <= hi)


def reads(entries, names, filter):
    """per node: does the rule read it?  A clause on a column outside names drops nothing."""
    names = ordered(names)
    out = np.ones(len(entries), bool)
    for k in range(len(entries)):
        for clause in filter or ():
            if clause[1] in names and clause_unreachable(entries[k, names.index(clause[1])], clause):
                out[k] = False
    return out


def node_passes(cols, offset, count, clause):
    """ground truth per node: does some row of the node pass the clause? (filter_ref's clause_mask over the node's rows)"""
    return np.array([bool(F.clause_mask(cols[clause[1]][int(o):int(o) + int(c)], clause).any()) for o, c in zip(offset, count)])


def node_passes_filter(cols, offset, count, filter):
    """... and: does some row of the node pass every clause?"""
    return np.array([bool(F.filter_mask({k: v[int(o):int(o) + int(c)] for k, v in cols.items()}, filter).any()) for o, c in zip(offset, count)])
