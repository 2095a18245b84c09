#!/usr/bin/env python3
"""Times swz_dataset_query beside the host recipe it replaces.  A multi-batch tiler (uniform points with RGB + intensity)
writes a BIN data set with write_output + write_properties, as tools/convert_probe.py does; then three boxes are queried:
  whole:  the root box -- every node is read, every point comes back;
  eighth: the octant [0, 0.5]^3;
  slab:   0.5 <= z <= 0.5 + 2^-10, thinner than the deepest node.
Per box: the stats of dataset_query (nodes read of nodes scanned, points read and returned, read / unpack / select / copy /
wall), and the host recipe -- bin_read_node of EVERY node file plus a numpy mask (--host-nodes N: only the first N nodes, the
time scaled to the whole table by points; 0: all).  The times are printed, none is asserted; the counts of the two must agree
when the host recipe ran over all nodes.  Everything goes into a fresh directory under --dir (default: the system's temporary
directory).  The work runs in one child process under `timeout`.
--polygon M: every box is cut by the regular M-gon inscribed in its x-y rectangle (dataset_query_region); --planes: by the
frustum of a fixed camera above the corner (-0.6, -0.4, 1.2) looking at (0.5, 0.5, 0.3).  Per box then: the stats of the region
query, beside them those of the box query of the region's bounding box (`box_query`), and the host recipe with the region's
formula in numpy.
--filter NAME=V[,V...] or NAME=LO..HI, any number of times (e.g. --filter classification=2 --filter return_number=1..1): the
data set also carries classification (0..15) and return_number (1..4), and every box -- or region -- is queried with the
filter (dataset_query_filtered; a list of values is a set on a one-byte column, LO..HI a closed range).  Per box then:
`filtered`, the stats of that call; `query`, the same region without the filter; and `filter_recipe`, what a caller did
before: the unfiltered query with the filtered columns added, copied to the host, and a numpy mask.  The counts of the first
and the last must agree.
--summaries (with one or more --filter): the data set also carries point_source_id, 16 flight strips along x
(point_source_id=3..3 is a filter few nodes can pass, intensity=0..65535 one that every node passes).  Every --filter is taken
as a filter of its own over the whole box: the filtered query (`without`), then dataset_summarize (`summarize`: its stats),
then the same query again (`with`: fewer nodes_read and bytes_read where the summaries let nodes drop), and `count_only`, the
unfiltered count-only query, which streams what dataset_summarize streams.  The counts of the two filtered runs must agree.
usage: query_probe.py [points] [--batches K] [--dir DIR] [--host-nodes N] [--json FILE] [--polygon M | --planes] [--filter SPEC]...
       [--summaries]"""
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
NAMES = ("rgb", "intensity")
BOXES = dict(whole=([0.0] * 3, [1.0] * 3), eighth=([0.0] * 3, [0.5] * 3), slab=([0.0, 0.0, 0.5], [1.0, 1.0, 0.5 + 2.0 ** -10]))


def camera_planes(swz, np):
    """the six planes of the fixed camera: an OpenGL-style look-at and perspective, through frustum_planes"""
    eye, target, up = np.array([-0.6, -0.4, 1.2]), np.array([0.5, 0.5, 0.3]), np.array([0.0, 0.0, 1.0])
    f = (target - eye) / np.linalg.norm(target - eye)
    s = np.cross(f, up) / np.linalg.norm(np.cross(f, up))
    view = np.eye(4)
    view[0, :3], view[1, :3], view[2, :3] = s, np.cross(s, f), -f
    view[:3, 3] = -view[:3, :3] @ eye
    t, aspect, near, far = 1.0 / np.tan(np.radians(40.0) / 2), 1.25, 0.1, 3.0
    proj = np.array([[t / aspect, 0, 0, 0], [0, t, 0, 0], [0, 0, (far + near) / (near - far), 2 * far * near / (near - far)], [0, 0, -1, 0]])
    return swz.frustum_planes(proj @ view)


def make_region(swz, np, spec, box):
    """spec: "", "planes" or "polygon:M" -> (Region or None, the region's bounding box, its mask over rows already in the box)"""
    if not spec:
        return None, box, lambda xyz: np.ones(len(xyz), bool)
    if spec == "planes":
        planes = camera_planes(swz, np)

        def inside(xyz):
            m = np.ones(len(xyz), bool)
            for a, b, c, d in planes:
                m &= ((a * xyz[:, 0] + b * xyz[:, 1]) + c * xyz[:, 2]) + d >= 0.0
            return m
        return swz.Region.planes(planes), box, inside
    m = int(spec.split(":")[1])
    ang = 2 * np.pi * np.arange(m) / m
    cx, cy = (box[0][0] + box[1][0]) / 2, (box[0][1] + box[1][1]) / 2
    v = np.stack([cx + (box[1][0] - box[0][0]) / 2 * np.cos(ang), cy + (box[1][1] - box[0][1]) / 2 * np.sin(ang)], axis=1)

    def inside(xyz):
        px, py = xyz[:, 0], xyz[:, 1]
        odd = np.zeros(len(xyz), bool)
        for i in range(m):
            (x0, y0), (x1, y1) = v[i], v[(i + 1) % m]
            t = (x1 - x0) * (py - y0) - (px - x0) * (y1 - y0)
            odd ^= ((y0 > py) != (y1 > py)) & ((t > 0.0) == (y1 > y0))
        return odd
    bound = ([max(box[0][0], v[:, 0].min()), max(box[0][1], v[:, 1].min()), box[0][2]],
             [min(box[1][0], v[:, 0].max()), min(box[1][1], v[:, 1].max()), box[1][2]])
    return swz.Region.polygon(v), bound, inside


def host_recipe(swz, np, src, nodes, box, limit, region_mask=None):
    """bin_read_node of the first `limit` nodes (0: all) and a numpy mask; seconds, points read, points inside"""
    lo, hi = np.asarray(box[0]), np.asarray(box[1])
    done = inside = 0
    t0 = time.perf_counter()
    for k in range(len(nodes["count"]) if not limit else min(limit, len(nodes["count"]))):
        xyz, cols = swz.bin_read_node(os.path.join(src, swz.node_name(int(nodes["level"][k]), int(nodes["key"][k])) + ".bin"))
        sel = ((xyz >= lo) & (xyz <= hi)).all(axis=1)
        if region_mask is not None:
            at = np.flatnonzero(sel)
            sel[at] = region_mask(xyz[at])
        kept = (xyz[sel], {name: v[sel] for name, v in cols.items()})
        done += len(xyz)
        inside += len(kept[0])
    return time.perf_counter() - t0, done, inside


FILTER_COLUMNS = ("classification", "return_number")


def make_filter(swz, np, specs):
    """["classification=2", "return_number=1..1"] -> (Filter, the names it reads, its mask over a dict of host columns)"""
    f, tests = swz.Filter(), []
    for spec in specs:
        name, _, value = spec.partition("=")
        if ".." in value:
            lo, hi = (float(v) for v in value.split(".."))
            f.range(name, lo, hi)
            tests.append((name, lambda v, lo=lo, hi=hi: (v.astype(np.float64) >= lo) & (v.astype(np.float64) <= hi)))
        else:
            values = [int(v) for v in value.split(",")]
            f.any_of(name, values)
            tests.append((name, lambda v, values=values: np.isin(v, values)))

    def mask(cols):
        m = None
        for name, test in tests:
            m = test(cols[name]) if m is None else m & test(cols[name])
        return m
    return f.check(), tuple(dict.fromkeys(name for name, _ in tests)), mask


def filter_recipe(swz, np, ctx, src, box, region, names, mask):
    """the unfiltered query with the filter's columns, copied out, and a numpy mask: seconds, rows moved, rows kept"""
    t0 = time.perf_counter()
    got = swz.dataset_query_region(ctx, src, box[0], box[1], region, attrs=NAMES + tuple(k for k in names if k not in NAMES))
    host = {k: got[k].cpu().numpy() for k in ("xyz",) + NAMES + names}
    sel = mask(host)
    kept = {k: host[k][sel] for k in ("xyz",) + NAMES}
    return time.perf_counter() - t0, got["count"], len(kept["xyz"])


def step(n, batches, base, host_nodes, spec="", filters=(), summaries=False):
    import numpy as np
    import schwarzwald_amd as swz
    ctx = swz.Context(0)
    bmin, bmax = [0.0] * 3, [1.0] * 3
    params = swz.TileParams(sampler=swz.GRID_CENTER, max_points_per_node=20000, spacing_at_root=swz.spacing_from_diagonal(bmin, bmax, 250))
    t = swz.Tiler(ctx, bmin, bmax, params, capacity_hint=n)
    rng = np.random.default_rng(1)
    per = n // batches
    for b in range(batches):
        m = per if b + 1 < batches else n - per * (batches - 1)
        cols = {"rgb": rng.integers(0, 256, (m, 3), dtype=np.uint8), "intensity": rng.integers(0, 65536, m, dtype=np.uint16)}
        if filters:
            cols.update(classification=rng.integers(0, 16, m, dtype=np.uint8), return_number=rng.integers(1, 5, m, dtype=np.uint8))
        xyz = rng.random((m, 3))
        if summaries:
            cols.update(point_source_id=(1 + np.floor(xyz[:, 0] * 16)).astype(np.uint16))
        t.add_batch(xyz, cols)
    t.finalize()
    info, nodes = t.info(), t.node_table()
    stored = int(info["num_stored"])
    work = tempfile.mkdtemp(prefix="swz_query_probe_", dir=base)
    src = os.path.join(work, "src_bin")
    out = dict(points=n, batches=batches, stored=stored, nodes=int(info["num_nodes"]), write_bin=t.write_output(src, "BIN", attrs=NAMES + (FILTER_COLUMNS if filters else ()) + (("point_source_id",) if summaries else ())))
    t.write_properties(src)
    t.close()
    print("QUERY_PROBE " + json.dumps(dict(source=out)), flush=True)
    if summaries:
        import ctypes
        from schwarzwald_amd import api
        box = BOXES["whole"]
        region, _, _ = make_region(swz, np, spec, box)
        rows = [dict(filter=f, region=spec or "box") for f in filters]
        for when in ("without", "with"):
            for row in rows:
                flt, _, _ = make_filter(swz, np, [row["filter"]])
                for rep in ("warm", "timed"):
                    got = swz.dataset_query_filtered(ctx, src, box[0], box[1], region, flt, attrs=NAMES)
                    row[when] = dict(got["stats"], count=got["count"])
                    del got
            if when == "without":
                for rep in ("warm", "timed"):   # (the unfiltered query never looks at the sidecar the first round leaves)
                    p = api._query_params(box[0], box[1], None, (), False, 0)
                    count, stats = ctypes.c_uint64(), api._QueryStats()
                    ctx._check(ctx._lib.swz_dataset_query(ctx._ctx, os.fsencode(src), ctypes.byref(p), 0, None, None, None, ctypes.byref(count),
                                                          ctypes.byref(stats)))
                    count_only = dict({k: getattr(stats, k) for k, _ in api._QueryStats._fields_}, count=int(count.value))
                    summarize = swz.dataset_summarize(ctx, src)
        for row in rows:
            assert row["with"]["count"] == row["without"]["count"], row
            print("QUERY_PROBE " + json.dumps(dict(row, summarize=summarize, count_only=count_only)), flush=True)
        shutil.rmtree(work, ignore_errors=True)
        ctx.close()
        return
    for name, box in BOXES.items():
        row = dict(box=name, region=spec or "box")
        region, bound, mask = make_region(swz, np, spec, box)
        if filters:
            flt, names, fmask = make_filter(swz, np, filters)
            row["filter"] = list(filters)
            for rep in ("warm", "timed"):
                got = swz.dataset_query_filtered(ctx, src, box[0], box[1], region, flt, attrs=NAMES)
                row["filtered"] = dict(got["stats"], count=got["count"])
                del got
                got = swz.dataset_query_region(ctx, src, box[0], box[1], region, attrs=NAMES)
                row["query"] = dict(got["stats"], count=got["count"])
                del got
                secs, moved, kept = filter_recipe(swz, np, ctx, src, box, region, names, fmask)
            row["filter_recipe"] = dict(wall_ms=secs * 1e3, rows_moved=moved, count=kept)
            row["recipe_over_filtered"] = secs * 1e3 / row["filtered"]["wall_ms"]
            assert kept == row["filtered"]["count"], (kept, row["filtered"]["count"])
            print("QUERY_PROBE " + json.dumps(row), flush=True)
            continue
        for rep in ("warm", "timed"):   # the first run pays allocations and the page cache
            got = swz.dataset_query_region(ctx, src, box[0], box[1], region, attrs=NAMES) if region is not None else \
                swz.dataset_query(ctx, src, box[0], box[1], attrs=NAMES)
            row["query"] = dict(got["stats"], count=got["count"])
            del got
            if region is not None:   # beside it: what the caller asked for before, the region's bounding box
                got = swz.dataset_query(ctx, src, bound[0], bound[1], attrs=NAMES)
                row["box_query"] = dict(got["stats"], count=got["count"])
                del got
        secs, done, inside = host_recipe(swz, np, src, nodes, box, host_nodes, mask if region is not None else None)
        row["host_recipe"] = dict(measured_s=secs, points=done, inside=inside, scaled_to_all_s=secs * stored / max(done, 1))
        row["host_over_query"] = row["host_recipe"]["scaled_to_all_s"] * 1e3 / row["query"]["wall_ms"]
        if done == stored:
            assert inside == row["query"]["count"], (inside, row["query"]["count"])
        print("QUERY_PROBE " + json.dumps(row), flush=True)
    shutil.rmtree(work, ignore_errors=True)
    ctx.close()


def main():
    args = sys.argv[1:]
    if args and args[0] == "--step":
        return step(int(args[1]), int(args[2]), args[3] or None, int(args[4]), args[5] if len(args) > 5 else "",
                    tuple(v for v in (args[6] if len(args) > 6 else "").split(";") if v), len(args) > 7 and args[7] == "summaries")

    def option(name, default):
        return args[args.index(name) + 1] if name in args else default
    n = int(args[0]) if args and not args[0].startswith("--") else 100_000_000
    limit = str(max(300, n // 50_000))
    spec = "planes" if "--planes" in args else "polygon:" + option("--polygon", "0") if "--polygon" in args else ""
    # one child under its own time limit; check=True: a failure ends the script here
    r = subprocess.run(["timeout", "-k", "10", limit, sys.executable, os.path.abspath(__file__), "--step", str(n), option("--batches", "10"),
                        option("--dir", ""), option("--host-nodes", "0"), spec,
                        ";".join(args[i + 1] for i, a in enumerate(args) if a == "--filter"), "summaries" if "--summaries" in args else ""],
                       check=True, stdout=subprocess.PIPE, text=True)
    results = [json.loads(l[len("QUERY_PROBE "):]) for l in r.stdout.splitlines() if l.startswith("QUERY_PROBE ")]
    for row in results:
        print(json.dumps(row), flush=True)
    if "--json" in args:
        with open(option("--json", None), "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
