#!/usr/bin/env python3
"""Times swz_dataset_rasterize beside the host recipe it replaces.  A multi-batch tiler (uniform points with RGB, intensity,
classification and return_number) writes a BIN data set with write_output + write_properties, by the recipe of
tools/query_probe.py; then two boxes are rastered on a --grid N x N grid (default 1024), z per cell:
  whole:  the root box -- every node is read, every point lands in a cell;
  eighth: the octant [0, 0.5]^3.
Per box: `raster`, the stats of dataset_rasterize (nodes read, points read and rastered, read / unpack / select / copy / wall;
select_ms is the time of the chunks' bodies: the accumulate kernel, behind the selection where there is one), and
`host_recipe`, what a caller did before: dataset_query_filtered of the same selection with no column, the positions copied to
the host (`query_ms`, `to_host_ms`), and numpy -- the cell of every row, np.add.at for count and sum, np.minimum.at and
np.maximum.at (`numpy_ms`).  The counts per cell of the two must agree.  Both run twice; the second run is reported (the first
pays allocations and fills the page cache: the figures are for a WARM page cache).
--polygon M: every box is cut by the regular M-gon inscribed in its x-y rectangle; --filter NAME=V[,V...] or NAME=LO..HI, any
number of times, as in tools/query_probe.py (e.g. --filter classification=2 --filter return_number=1..1).  Both send the
chunks through the selection before the accumulate kernel.
The times are printed, none is asserted.  Everything goes into a fresh directory under --dir (default: the system's temporary
directory).  The work runs in one child process under `timeout`.
usage: raster_probe.py [points] [--batches K] [--dir DIR] [--grid N] [--json FILE] [--polygon M] [--filter SPEC]..."""
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, HERE)
NAMES = ("rgb", "intensity", "classification", "return_number")
BOXES = dict(whole=([0.0] * 3, [1.0] * 3), eighth=([0.0] * 3, [0.5] * 3))


def host_recipe(swz, np, ctx, src, box, region, flt, grid, frame):
    """the filtered query without a column, its positions on the host, and a numpy raster"""
    t0 = time.perf_counter()
    got = swz.dataset_query_filtered(ctx, src, box[0], box[1], region, flt, attrs=[])
    t1 = time.perf_counter()
    xyz = got["xyz"].cpu().numpy()
    t2 = time.perf_counter()
    ix = np.minimum(np.floor((xyz[:, 0] - frame["x0"]) / frame["cw"]), grid - 1).astype(np.int64)
    iy = np.minimum(np.floor((xyz[:, 1] - frame["y0"]) / frame["ch"]), grid - 1).astype(np.int64)
    cell = iy * grid + ix
    count = np.zeros(grid * grid, dtype=np.int64)
    total = np.zeros(grid * grid, dtype=np.float64)
    lo, hi = np.full(grid * grid, np.inf), np.full(grid * grid, -np.inf)
    np.add.at(count, cell, 1)
    np.add.at(total, cell, xyz[:, 2])
    np.minimum.at(lo, cell, xyz[:, 2])
    np.maximum.at(hi, cell, xyz[:, 2])
    t3 = time.perf_counter()
    return dict(query_ms=(t1 - t0) * 1e3, to_host_ms=(t2 - t1) * 1e3, numpy_ms=(t3 - t2) * 1e3, wall_ms=(t3 - t0) * 1e3, rows=got["count"],
                query_output_bytes=24 * got["count"]), count, lo, hi


def step(n, batches, base, grid, spec="", filters=()):
    import numpy as np
    import query_probe as Q
    import schwarzwald_amd as swz
    ctx = swz.Context(0)
    bmin, bmax = [0.0] * 3, [1.0] * 3
    params = swz.TileParams(sampler=swz.GRID_CENTER, max_points_per_node=20000, spacing_at_root=swz.spacing_from_diagonal(bmin, bmax, 250))
    t = swz.Tiler(ctx, bmin, bmax, params, capacity_hint=n)
    rng = np.random.default_rng(1)
    per = n // batches
    for b in range(batches):
        m = per if b + 1 < batches else n - per * (batches - 1)
        t.add_batch(rng.random((m, 3)), {"rgb": rng.integers(0, 256, (m, 3), dtype=np.uint8), "intensity": rng.integers(0, 65536, m, dtype=np.uint16),
                                         "classification": rng.integers(0, 16, m, dtype=np.uint8), "return_number": rng.integers(1, 5, m, dtype=np.uint8)})
    t.finalize()
    info = t.info()
    work = tempfile.mkdtemp(prefix="swz_raster_probe_", dir=base)
    src = os.path.join(work, "src_bin")
    out = dict(points=n, batches=batches, stored=int(info["num_stored"]), nodes=int(info["num_nodes"]), format="BIN", grid=grid,
               page_cache="warm (second run of each call)", write_bin=t.write_output(src, "BIN", attrs=NAMES))
    t.write_properties(src)
    t.close()
    print("RASTER_PROBE " + json.dumps(dict(source=out)), flush=True)
    for name, box in BOXES.items():
        row = dict(box=name, region=spec or "box", filter=list(filters))
        region, _, _ = Q.make_region(swz, np, spec, box)
        flt = Q.make_filter(swz, np, filters)[0] if filters else None
        for rep in ("warm", "timed"):
            got = swz.dataset_rasterize(ctx, src, box[0], box[1], grid, grid, region=region, filter=flt)
            row["raster"] = dict(got["stats"], table_bytes=int(got["cells"].nbytes))
            recipe, count, lo, hi = host_recipe(swz, np, ctx, src, box, region, flt, grid, got["frame"])
            row["host_recipe"] = recipe
        assert np.array_equal(count.reshape(grid, grid), got["count"].astype(np.int64)), "the counts per cell differ"
        assert np.array_equal(lo.reshape(grid, grid), got["min"]) and np.array_equal(hi.reshape(grid, grid), got["max"]), "min / max differ"
        row["recipe_over_raster"] = recipe["wall_ms"] / row["raster"]["wall_ms"]
        print("RASTER_PROBE " + json.dumps(row), flush=True)
    shutil.rmtree(work, ignore_errors=True)
    ctx.close()


def main():
    args = sys.argv[1:]
    if args and args[0] == "--step":
        return step(int(args[1]), int(args[2]), args[3] or None, int(args[4]), args[5], tuple(v for v in args[6].split(";") if v))

    def option(name, default):
        return args[args.index(name) + 1] if name in args else default
    n = int(args[0]) if args and not args[0].startswith("--") else 100_000_000
    limit = str(max(300, n // 50_000))
    spec = "polygon:" + option("--polygon", "0") if "--polygon" in args else ""
    # one child under its own time limit; check=True: a failure ends the script here
    r = subprocess.run(["timeout", "-k", "10", limit, sys.executable, os.path.abspath(__file__), "--step", str(n), option("--batches", "10"),
                        option("--dir", ""), option("--grid", "1024"), spec, ";".join(args[i + 1] for i, a in enumerate(args) if a == "--filter")],
                       check=True, stdout=subprocess.PIPE, text=True)
    results = [json.loads(l[len("RASTER_PROBE "):]) for l in r.stdout.splitlines() if l.startswith("RASTER_PROBE ")]
    for row in results:
        print(json.dumps(row), flush=True)
    if "--json" in args:
        with open(option("--json", None), "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
