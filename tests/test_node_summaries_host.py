"""node-summaries.swz and the node rule of a filtered query, on the host (no GPU): swz_dataset_summaries_write / _read and
swz_dataset_query_filtered_nodes against tests/summary_ref.py.

The data set is BIN node files written with the host writers: the root, its eight octants and the eight children of one
octant.  The columns follow the positions (strip and intensity grow with x, GPS time and the edge flag with y, ground lies
below z = 0.35), so a filter takes and leaves whole nodes; one node's GPS times are all NaN, one holds a few NaN beside times
that all lie in a range, one node's scan angles are -128 and -1 only."""
import itertools
import os
import shutil

import numpy as np
import pytest

import filter_ref as F
import summary_ref as S
import schwarzwald_amd as swz

UNIT = ([0.0, 0.0, 0.0], [1.0, 1.0, 1.0])
ERR_BAD_ARG = 2
INF = float("inf")
FILE = "node-summaries.swz"


def _key(digits):
    k = 0
    for l, d in enumerate(digits):
        k |= d << (3 * (20 - l))
    return k


def _dataset():
    """nodes in scan order with their rows: dict(level, key, offset, count), cols, xyz, and the nodes named for their part"""
    rng = np.random.default_rng(577)
    digits = [()] + [(d,) for d in range(8)]
    lows = {d: tuple(swz.node_bounds(0, _key(d), *UNIT)[0]) for d in digits[1:]}
    parent = next(d for d, lo in lows.items() if lo == (0.0, 0.0, 0.0))
    digits += [parent + (d,) for d in range(8)]
    digits.sort(key=lambda d: (len(d), _key(d)))
    named = {"all_nan": next(d for d, lo in lows.items() if lo == (0.5, 0.5, 0.5)), "some_nan": next(d for d, lo in lows.items() if lo == (0.5, 0.0, 0.0)),
             "angles": next(d for d, lo in lows.items() if lo == (0.0, 0.5, 0.0))}
    xyz, cols, off, cnt = [], {k: [] for k in F.SCALARS}, [], []
    at = 0
    for d in digits:
        lo, hi = (np.asarray(v) for v in swz.node_bounds(len(d) - 1, _key(d), *UNIT))
        n = 60 if not d else 31
        p = lo + rng.random((n, 3)) * (hi - lo) * 0.999
        x, y, z = p[:, 0], p[:, 1], p[:, 2]
        gps = 1e5 * y
        angle = np.floor(x * 90).astype(np.int8)
        if d == named["all_nan"]:
            gps = np.full(n, np.nan)
        if d == named["some_nan"]:
            gps[:3] = np.nan
        if d == named["angles"]:
            angle = np.where(np.arange(n) % 2 == 0, -128, -1).astype(np.int8)
        if not d:
            angle[:4] = [127, -128, -1, -64]
        c = {"intensity": np.floor(x * 50000).astype(np.uint16), "classification": np.where(z < 0.35, 2, rng.choice([3, 4, 5, 6, 9], n)).astype(np.uint8),
             "edge_of_flight_line": (y >= 0.5).astype(np.uint8), "gps_time": gps, "number_of_returns": rng.integers(3, 5, n, endpoint=True).astype(np.uint8),
             "return_number": rng.integers(1, 3, n, endpoint=True).astype(np.uint8), "point_source_id": (1 + np.floor(x * 4)).astype(np.uint16),
             "scan_direction_flag": (x >= 0.5).astype(np.uint8), "scan_angle_rank": angle, "user_data": rng.integers(0, 255, n, endpoint=True).astype(np.uint8)}
        xyz.append(p)
        for k in cols:
            cols[k].append(c[k])
        off.append(at)
        cnt.append(n)
        at += n
    nodes = dict(level=np.array([len(d) - 1 for d in digits], dtype=np.int8), key=np.array([_key(d) for d in digits], dtype=np.uint64),
                 offset=np.array(off, dtype=np.uint64), count=np.array(cnt, dtype=np.uint64))
    return dict(nodes=nodes, xyz=np.concatenate(xyz), cols={k: np.concatenate(v) for k, v in cols.items()},
                named={k: digits.index(v) for k, v in named.items()})


def _write(directory, D, skip=()):
    os.makedirs(directory)
    nd = D["nodes"]
    for k in range(len(nd["count"])):
        o, c = int(nd["offset"][k]), int(nd["count"][k])
        swz.bin_write_node(os.path.join(directory, swz.node_name(int(nd["level"][k]), int(nd["key"][k])) + ".bin"), D["xyz"][o:o + c],
                           {name: v[o:o + c] for name, v in D["cols"].items()})
    swz.properties_json_write(directory, UNIT[0], UNIT[1], 0.05, len(D["xyz"]))


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    D = _dataset()
    root = tmp_path_factory.mktemp("node_summaries")
    plain, summed = str(root / "plain"), str(root / "summed")
    _write(plain, D)
    _write(summed, D)
    nd = D["nodes"]
    entries = S.summaries(D["cols"], F.SCALARS, nd["offset"], nd["count"])       # computed once, shared, never changed
    swz.dataset_summaries_write(summed, "BIN", F.SCALARS, nd, entries)
    return dict(D, plain=plain, summed=summed, entries=entries, root=root)


def _copy(data, name):
    dst = str(data["root"] / name)
    shutil.copytree(data["summed"], dst)
    return dst


def test_the_sidecar_round_trips_and_the_scan_ignores_it(data):
    got = swz.dataset_summaries_read(data["summed"])
    nd = data["nodes"]
    assert got["format"] == "BIN" and got["attribute_mask"] == swz.SUMMARY_SCALARS and sorted(got["attrs"]) == sorted(F.SCALARS)
    assert got["points"] == int(nd["count"].sum())
    for k in ("level", "key", "count"):
        assert np.array_equal(got["nodes"][k], nd[k])
    assert got["entries"].tobytes() == data["entries"].tobytes()
    size = os.path.getsize(os.path.join(data["summed"], FILE))
    assert size == 48 + len(nd["count"]) * (24 + 10 * 56)
    assert not [f for f in os.listdir(data["summed"]) if f.endswith(".tmp")]
    # a directory without the file is not an error; a scan does not see the file
    assert swz.dataset_summaries_read(data["plain"]) is None
    a, b = swz.dataset_scan(data["plain"]), swz.dataset_scan(data["summed"])
    assert a["format"] == b["format"] == "BIN" and np.array_equal(a["nodes"]["key"], b["nodes"]["key"]) and a["points"] == b["points"]
    # a subset of the columns, no columns, no nodes
    sub = ("gps_time", "classification")
    d = _copy(data, "subset")
    swz.dataset_summaries_write(d, "LAS", sub, nd, S.summaries(data["cols"], sub, nd["offset"], nd["count"]))
    got = swz.dataset_summaries_read(d)
    assert got["format"] == "LAS" and got["attrs"] == S.ordered(sub) and got["entries"].shape == (len(nd["count"]), 2)
    assert S.same(got["entries"], S.summaries(data["cols"], sub, nd["offset"], nd["count"]))
    swz.dataset_summaries_write(d, "BIN", 0, nd, np.zeros((len(nd["count"]), 0), dtype=S.DTYPE))
    assert swz.dataset_summaries_read(d)["entries"].shape == (len(nd["count"]), 0)
    empty = {k: v[:0] for k, v in nd.items()}
    swz.dataset_summaries_write(d, "BIN", F.SCALARS, empty, np.zeros((0, 10), dtype=S.DTYPE))
    assert swz.dataset_summaries_read(d)["points"] == 0


def test_what_the_writer_refuses(data):
    nd = data["nodes"]
    d = _copy(data, "writer")
    swapped = {k: v.copy() for k, v in nd.items()}
    for k in ("level", "key", "count"):
        swapped[k][[1, 2]] = swapped[k][[2, 1]]
    for words, args in ((("(level, Morton index) order",), ("BIN", F.SCALARS, swapped, data["entries"])),
                        (("no scalar column",), ("BIN", 1, nd, np.zeros((len(nd["count"]), 1), dtype=S.DTYPE))),
                        (("unknown format",), (9, F.SCALARS, nd, data["entries"]))):
        with pytest.raises(swz.SwzError) as e:
            swz.dataset_summaries_write(d, *args)
        assert e.value.code == ERR_BAD_ARG and all(w in str(e.value) for w in ("swz_dataset_summaries_write",) + words), str(e.value)
    assert swz.dataset_summaries_read(d)["entries"].tobytes() == data["entries"].tobytes()   # the file it had is still there


def test_every_read_refusal_is_named(data):
    d = _copy(data, "damaged")
    path = os.path.join(d, FILE)
    good = open(path, "rb").read()
    nodes = len(data["nodes"]["count"])
    at_nodes, at_entries = 48, 48 + 24 * nodes

    def with_bytes(at, new):
        return good[:at] + bytes(new) + good[at + len(new):]

    rec = lambda k: good[at_nodes + 24 * k: at_nodes + 24 * (k + 1)]  # noqa: E731
    cases = {"a wrong magic": with_bytes(0, b"SWZNSUX\0"),
             "a wrong version": with_bytes(8, (2).to_bytes(4, "little")),
             "a wrong entry size": with_bytes(20, (48).to_bytes(4, "little")),
             "a wrong file size": good[:-1],
             "a wrong file size: ": good + b"\0" * 56,
             "a wrong file size: shorter than its header": good[:40],
             "nodes out of order": with_bytes(at_nodes + 24, rec(2) + rec(1)),
             "is there twice": with_bytes(at_nodes + 48, rec(1)),
             "a nonzero reserved field in the header": with_bytes(40, b"\1"),
             "a nonzero reserved field in node 3": with_bytes(at_nodes + 3 * 24 + 20, b"\1"),
             "a nonzero reserved field in entry 5": with_bytes(at_entries + 5 * 56 + 52, b"\1")}
    for words, image in cases.items():
        open(path, "wb").write(image)
        with pytest.raises(swz.SwzError) as e:
            swz.dataset_summaries_read(d)
        assert e.value.code == ERR_BAD_ARG and "swz_dataset_summaries_read" in str(e.value) and FILE in str(e.value) and words in str(e.value), \
            (words, str(e.value))
        # ... and the query that would use it is refused the same way
        with pytest.raises(swz.SwzError) as e:
            swz.dataset_query_filtered_nodes(d, UNIT[0], UNIT[1], None, swz.Filter().any_of("classification", [2]))
        assert "swz_dataset_query_filtered_nodes" in str(e.value) and words in str(e.value) and "run swz_dataset_summarize again" in str(e.value)
    open(path, "wb").write(good)
    assert swz.dataset_summaries_read(d)["points"] == len(data["xyz"])


# every kind on byte, uint16 and GPS columns; scan angles -128 / -1; NaN times; two clauses on one attribute
SINGLE_BYTE = [[("any_of", "classification", [2])], [("none_of", "classification", [2])], [("range", "classification", 3, 9)],
               [("not_range", "classification", 2, 2)], [("range", "edge_of_flight_line", 1, 1)], [("none_of", "scan_direction_flag", [0])],
               [("range", "scan_angle_rank", -128, -1)], [("not_range", "scan_angle_rank", 0, 127)], [("any_of", "scan_angle_rank", [-1])],
               [("any_of", "scan_angle_rank", [-128])], [("none_of", "scan_angle_rank", [-128, -1])], [("range", "scan_angle_rank", -127, 44)]]
OTHERS = [[("range", "point_source_id", 1, 1)], [("not_range", "point_source_id", 1, 2)], [("range", "intensity", 0, 10000)],
          [("not_range", "intensity", 0, 24999)], [("range", "intensity", 49000, INF)], [("range", "gps_time", -INF, 2e4)],
          [("not_range", "gps_time", 0, 5e4)], [("range", "gps_time", 7.5e4, INF)],
          [("range", "gps_time", 0, 6e4), ("not_range", "gps_time", 2e4, 1e5)],
          [("any_of", "classification", [2, 3]), ("none_of", "classification", [2])],
          [("range", "point_source_id", 1, 2), ("any_of", "classification", [2])],
          [("range", "point_source_id", 3, 4), ("range", "edge_of_flight_line", 0, 0), ("not_range", "gps_time", -INF, INF)]]


@pytest.mark.parametrize("filter", SINGLE_BYTE + OTHERS, ids=lambda f: " & ".join("%s %s" % (c[0], c[1]) for c in f))
def test_the_node_rule_is_the_reference_rule_and_never_drops_a_passing_row(data, filter):
    nd = data["nodes"]
    want = S.reads(data["entries"], F.SCALARS, filter)
    passing = S.node_passes_filter(data["cols"], nd["offset"], nd["count"], filter)
    # the numpy side first
    assert not want.all() and want.any(), "the filter drops no node, or every node"
    assert not (passing & ~want).any(), "the reference rule drops a node that holds a passing row"
    if filter in SINGLE_BYTE:
        assert np.array_equal(want, S.node_passes(data["cols"], nd["offset"], nd["count"], filter[0])), "a single byte clause is exact"
    table = swz.dataset_query_region_nodes(data["summed"], UNIT[0], UNIT[1], None)
    got = swz.dataset_query_filtered_nodes(data["summed"], UNIT[0], UNIT[1], None, F.as_filter(swz, filter))
    for k in ("level", "key", "count"):
        assert np.array_equal(got[k], table[k]) and np.array_equal(got[k], nd[k])
    assert np.array_equal(got["read"], want), (got["read"], want)
    assert not (passing & ~got["read"]).any()
    assert got["points_bound"] == int(nd["count"][want].sum()) < table["points_bound"]


def test_the_special_nodes_are_judged_as_the_header_says(data):
    named, d = data["named"], data["summed"]
    read = lambda *clauses: swz.dataset_query_filtered_nodes(d, UNIT[0], UNIT[1], None, F.as_filter(swz, list(clauses)))["read"]  # noqa: E731
    # a node whose times are all NaN is dropped by a RANGE with a finite bound (with both ends open the rule, judging by lo and hi
    # alone, reads it) and passes every NOT RANGE; NaN beside times inside the range keeps a node
    assert not read(("range", "gps_time", -1e300, INF))[named["all_nan"]] and not read(("range", "gps_time", -INF, 1e300))[named["all_nan"]]
    assert read(("range", "gps_time", -INF, INF)).all() and read(("not_range", "gps_time", -INF, INF))[named["all_nan"]]
    r = read(("not_range", "gps_time", 0, 5e4))
    assert r[named["some_nan"]] and r[named["all_nan"]] and not r.all()
    assert int(read(("not_range", "gps_time", -INF, INF)).sum()) == 2
    # scan angles are signed: -128 and -1 lie below 0
    r = read(("range", "scan_angle_rank", -128, -1))
    assert r[named["angles"]] and r[0] and int(r.sum()) == 2
    assert not read(("range", "scan_angle_rank", 128, 255)).any()
    assert not read(("none_of", "scan_angle_rank", [255, 128]))[named["angles"]]
    # a region narrows the table; the flags follow it
    half = ([0.0, 0.0, 0.0], [0.4, 1.0, 1.0])
    table = swz.dataset_query_region_nodes(d, *half, None)
    got = swz.dataset_query_filtered_nodes(d, *half, None, swz.Filter().range("point_source_id", 2, 2))
    assert np.array_equal(got["key"], table["key"]) and len(got["key"]) < len(data["nodes"]["key"]) and 0 < got["read"].sum() < len(got["read"])


def test_a_column_outside_the_sidecars_mask_drops_nothing(data):
    nd = data["nodes"]
    d = _copy(data, "few_columns")
    sub = ("classification",)
    swz.dataset_summaries_write(d, "BIN", sub, nd, S.summaries(data["cols"], sub, nd["offset"], nd["count"]))
    assert swz.dataset_query_filtered_nodes(d, UNIT[0], UNIT[1], None, swz.Filter().range("point_source_id", 1, 1))["read"].all()
    filter = [("range", "point_source_id", 1, 1), ("any_of", "classification", [2])]
    want = S.reads(S.summaries(data["cols"], sub, nd["offset"], nd["count"]), sub, filter)
    assert not want.all() and np.array_equal(swz.dataset_query_filtered_nodes(d, UNIT[0], UNIT[1], None, F.as_filter(swz, filter))["read"], want)


def _refused(directory, *words):
    with pytest.raises(swz.SwzError) as e:
        swz.dataset_query_filtered_nodes(directory, UNIT[0], UNIT[1], None, swz.Filter().any_of("classification", [2]))
    assert e.value.code == ERR_BAD_ARG
    for w in ("swz_dataset_query_filtered_nodes", "node-summaries.swz is stale", "run swz_dataset_summarize again") + words:
        assert w in str(e.value), str(e.value)


def test_a_stale_sidecar_is_refused_by_name(data):
    nd = data["nodes"]
    d = _copy(data, "stale")
    # another count in one node file
    k = 4
    name = swz.node_name(int(nd["level"][k]), int(nd["key"][k]))
    o, c = int(nd["offset"][k]), int(nd["count"][k]) - 2
    swz.bin_write_node(os.path.join(d, name + ".bin"), data["xyz"][o:o + c], {n: v[o:o + c] for n, v in data["cols"].items()})
    _refused(d, "node %s holds %d points, the summary %d" % (name, c, c + 2))
    # a node the summary does not know
    d = _copy(data, "missing")
    keep = np.arange(len(nd["count"])) != 6
    swz.dataset_summaries_write(d, "BIN", F.SCALARS, {k: v[keep] for k, v in nd.items()}, data["entries"][keep])
    _refused(d, "node %s is not in the summary" % swz.node_name(int(nd["level"][6]), int(nd["key"][6])))
    # another format
    swz.dataset_summaries_write(d, "LAS", F.SCALARS, nd, data["entries"])
    _refused(d, "format")
    # the region and box tables do not look at the file
    assert len(swz.dataset_query_region_nodes(d, UNIT[0], UNIT[1], None)["key"]) == len(nd["key"])
    assert swz.dataset_query_filtered_nodes(d, UNIT[0], UNIT[1], None, None)["read"].all()


def test_without_a_sidecar_or_without_a_filter_every_node_is_read(data):
    box = ([0.0, 0.0, 0.0], [0.6, 0.3, 1.0])
    for directory, filter in itertools.product((data["plain"], data["summed"]), (None, swz.Filter(), swz.Filter().any_of("classification", [2]))):
        if directory == data["summed"] and filter is not None and filter.clauses:
            continue
        for region in (None, swz.Region.planes([[1.0, 0.0, 0.0, -0.2]])):
            want = swz.dataset_query_region_nodes(directory, box[0], box[1], region)
            got = swz.dataset_query_filtered_nodes(directory, box[0], box[1], region, filter)
            assert all(np.array_equal(got[k], want[k]) for k in ("level", "key", "count")) and got["points_bound"] == want["points_bound"]
            assert got["read"].all() and 0 < len(got["read"]) < len(data["nodes"]["key"])


def test_what_the_region_call_refuses_is_refused_in_this_calls_name(data):
    for kwargs, words in ((dict(reserved=1), "reserved must be 0"), (dict(source_flags=2), "an unknown bit in source_flags")):
        with pytest.raises(swz.SwzError) as e:
            swz.dataset_query_filtered_nodes(data["summed"], UNIT[0], UNIT[1], None, None, **kwargs)
        assert "swz_dataset_query_filtered_nodes" in str(e.value) and words in str(e.value)
    with pytest.raises(swz.SwzError) as e:
        swz.dataset_query_filtered_nodes(data["summed"], UNIT[0], UNIT[1], None, swz.Filter().range("intensity", 2, 1))
    assert "clause 0: a RANGE with lo > hi" in str(e.value)
