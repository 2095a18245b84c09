"""swz_filter_check: the one place the rules of a swz_filter live (host only, no GPU), and the bytes the binding's Filter
builder produces."""
import ctypes as C

import numpy as np
import pytest

ERR_BAD_ARG = 2
INF = float("inf")
NAN = float("nan")


def _swz():
    import schwarzwald_amd as swz
    return swz


def _refused(f, clause, word):
    swz = _swz()
    with pytest.raises(swz.SwzError) as e:
        f.check()
    text = str(e.value)
    assert e.value.code == ERR_BAD_ARG and "swz_filter_check" in text and word in text, text
    if clause is not None:
        assert "clause %d" % clause in text, text


def test_refusals_name_the_clause():
    swz = _swz()
    F, A = swz.Filter, swz.ATTRIBUTES
    ok = lambda: F().range("intensity", 0, 10)                       # clause 0 in order; the bad one is clause 1
    f = F()
    f.count = 9
    _refused(f, None, "8 clauses")
    _refused(F(reserved=1), None, "reserved")
    _refused(ok().clause(12, swz.FILTER_RANGE, 0, 1), 1, "outside the table")
    _refused(ok().clause(-1, swz.FILTER_RANGE, 0, 1), 1, "outside the table")
    _refused(ok().range("rgb", 0, 1), 1, ": SWZ_ATTR_RGB is not a scalar")
    _refused(ok().range("normal", 0, 1), 1, ": SWZ_ATTR_NORMAL is not a scalar")
    _refused(F().any_of("rgb", [1]), 0, ": SWZ_ATTR_RGB is not a scalar")
    _refused(ok().clause("intensity", 2, 0, 1), 1, "unknown kind")
    _refused(ok().clause("intensity", swz.FILTER_RANGE | 0x200, 0, 1), 1, "flag bit")
    _refused(ok().clause("classification", swz.FILTER_SET | 0x80000000, bits=(1, 0, 0, 0)), 1, "flag bit")
    for name in ("intensity", "point_source_id", "gps_time"):
        _refused(ok().any_of(name, [1]), 1, "wider than a byte")
        _refused(ok().none_of(name, [1]), 1, "a SET on SWZ_ATTR_%s," % name.upper())
    _refused(ok().range("gps_time", 2.0, 1.0), 1, "lo > hi")
    _refused(ok().range("gps_time", INF, -INF), 1, "lo > hi")
    _refused(ok().range("gps_time", NAN, 1.0), 1, "NaN")
    _refused(ok().range("gps_time", 0.0, NAN), 1, "NaN")
    _refused(ok().range("gps_time", 0.0, NAN, negate=True), 1, "NaN")
    _refused(ok().clause("classification", swz.FILTER_SET, lo=1.0, bits=(1, 0, 0, 0)), 1, "lo or hi")
    _refused(ok().clause("classification", swz.FILTER_SET, hi=-1.0, bits=(1, 0, 0, 0)), 1, "lo or hi")
    _refused(ok().clause("classification", swz.FILTER_SET, lo=NAN, bits=(1, 0, 0, 0)), 1, "lo or hi")
    _refused(ok().clause("classification", swz.FILTER_RANGE, 0, 1, bits=(0, 0, 0, 1)), 1, "set that is not 0")
    # the clause named is the first bad one, counted from 0
    seven = F()
    for _ in range(7):
        seven.range("user_data", 0, 1)
    _refused(seven.range("normal", 0, 1), 7, ": SWZ_ATTR_NORMAL is not a scalar")
    assert A["rgb"][0] == 0 and A["normal"][0] == 1


def test_what_is_in_order():
    swz = _swz()
    F = swz.Filter
    F().range("gps_time", -INF, INF).check()
    F().range("gps_time", -INF, 5.0).range("intensity", 3.5, INF).check()
    F().range("intensity", 7, 7).check()                             # lo == hi
    F().range("scan_angle_rank", -128, -1).range("scan_angle_rank", 0.5, 0.5).check()
    eight = F()
    for name in ("intensity", "classification", "edge_of_flight_line", "gps_time", "number_of_returns", "return_number", "point_source_id",
                 "scan_direction_flag"):
        eight.range(name, 0, 1)
    eight.check()
    F().range("classification", 2, 2).none_of("classification", [2]).check()   # two clauses on one attribute
    F().any_of("user_data", []).check()                              # an empty set: every field 0
    F().check()                                                      # count == 0
    L = swz.load_library()
    assert L.swz_filter_check(None, None, 0) == 0                    # NULL: no filter
    why = C.create_string_buffer(8)                                  # a short buffer is cut, and closed
    bad = F().range("rgb", 0, 1)._struct()
    assert L.swz_filter_check(C.byref(bad), why, len(why)) == ERR_BAD_ARG and why.value == b"swz_fil"
    assert L.swz_filter_check(C.byref(bad), None, 0) == ERR_BAD_ARG
    ok = F().range("intensity", 0, 1)._struct()
    why.value = b"x"
    assert L.swz_filter_check(C.byref(ok), why, len(why)) == 0 and why.value == b""


def test_the_builder_writes_the_struct():
    swz = _swz()
    from schwarzwald_amd import api
    assert C.sizeof(api._FilterClause) == 56 and C.sizeof(api._Filter) == 456
    f = swz.Filter().range("gps_time", -1.5, INF).any_of("scan_angle_rank", [-1, 0, 127]).none_of("classification", [7, 18]).any_of(
        "user_data", [255, 64, 128])
    raw = np.frombuffer(bytes(f._struct()), dtype=np.uint8)
    assert raw[:8].view(np.uint32).tolist() == [4, 0]

    def clause(k):
        b = raw[8 + 56 * k: 8 + 56 * (k + 1)]
        return (int(b[:4].view(np.int32)[0]), int(b[4:8].view(np.uint32)[0]), b[8:24].view(np.float64).tolist(), b[24:56].view(np.uint64).tolist())
    A = swz.ATTRIBUTES
    assert clause(0) == (A["gps_time"][0], swz.FILTER_RANGE, [-1.5, INF], [0, 0, 0, 0])
    assert clause(1) == (A["scan_angle_rank"][0], swz.FILTER_SET, [0.0, 0.0], [1, (1 << 63), 0, 1 << 63])      # -1 is bit 255, 127 bit 127
    assert clause(2) == (A["classification"][0], swz.FILTER_SET | swz.FILTER_NOT, [0.0, 0.0], [(1 << 7) | (1 << 18), 0, 0, 0])
    assert swz.FILTER_NOT == 0x100 and swz.FILTER_SET == 1 and swz.FILTER_RANGE == 0
    assert clause(3) == (A["user_data"][0], swz.FILTER_SET, [0.0, 0.0], [0, 1, 1, 1 << 63])
    assert not raw[8 + 56 * 4:].any()                                # the clauses not used are 0
    assert f.attributes() == sum(1 << A[k][0] for k in ("gps_time", "scan_angle_rank", "classification", "user_data"))
    with pytest.raises(ValueError):
        swz.Filter().any_of("classification", [256])
    nine = swz.Filter()
    for _ in range(8):
        nine.range("intensity", 0, 1)
    with pytest.raises(ValueError):
        nine.range("intensity", 0, 1)
