#!/usr/bin/env python3
"""Times swz_convert_dataset against the two things it stands between.  A multi-batch tiler (uniform points with RGB +
intensity) writes a BIN data set with write_output + write_properties; then, per target format:
  (c) convert_dataset(BIN -> format): the stats of the call (read, unpack, pack, copy, write, wall);
  (w) Tiler.write_output of the same format from the live tiler: the ceiling -- conversion adds the read and the unpack;
  (h) the host recipe: bin_read_node of every source file, then the format's *_write_node_rows writer, node by node
      (--host-nodes N: only the first N nodes, and the time scaled to the whole table by points; 0: all).
--source-projection DEF: the 3DTILES leg is also timed through convert_dataset_world (positions mapped to ECEF with DEF, files
relative to their nodes' origins, oriented boxes), beside the existing call: row["convert_world"].  The unit cube is read as
coordinates of DEF (for a UTM zone: a metre beside the false origin, on the equator); the map costs what it costs anywhere.
--source-format 3DTILES: the tiler also writes a 3DTILES data set, and every target is converted from it as well
(convert_dataset(..., lossy_source=True)), timed beside the BIN source: row["convert_from_3DTILES"].
Everything goes into fresh directories under --dir (default: the system's temporary directory).  The work runs in one child
process under `timeout`.
usage: convert_probe.py [points] [--batches K] [--formats BIN,LAS,...] [--dir DIR] [--host-nodes N] [--json FILE]
                        [--source-projection DEF] [--source-format 3DTILES]"""
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
FORMATS = ("BIN", "BINZ", "3DTILES", "LAS", "ENTWINE_LAS")


def host_recipe(swz, src, dst, fmt, nodes, bmin, bmax, limit):
    """bin_read_node + the host writer of fmt for the first `limit` nodes (0: all); seconds, points done"""
    data = dst
    if fmt == "ENTWINE_LAS":
        swz.ept_create_dirs(dst)
        data = os.path.join(dst, "ept-data")
    else:
        os.mkdir(dst)
    done = 0
    t0 = time.perf_counter()
    for k in range(len(nodes["count"]) if not limit else min(limit, len(nodes["count"]))):
        level, key = int(nodes["level"][k]), int(nodes["key"][k])
        name = swz.node_name(level, key)
        xyz, cols = swz.bin_read_node(os.path.join(src, name + ".bin"))
        if fmt in ("BIN", "BINZ"):
            swz.bin_write_node(os.path.join(data, name + (".binz" if fmt == "BINZ" else ".bin")), xyz, cols, compressed=fmt == "BINZ")
        elif fmt == "3DTILES":
            swz.pnts_write_node_rows(os.path.join(data, name + ".pnts"), xyz, cols)
        else:
            mn, mx = swz.node_bounds(level, key, bmin, bmax)
            if fmt == "ENTWINE_LAS":
                name = swz.node_name_entwine(level, key)
            swz.las_write_node_rows(os.path.join(data, name + ".las"), xyz, cols, mn, mx, swz.las_scale_from_bounds(mn, mx))
        done += len(xyz)
    return time.perf_counter() - t0, done


def step(n, batches, formats, base, host_nodes, projection, source_format=None):
    import numpy as np
    import schwarzwald_amd as swz
    ctx = swz.Context(0)
    bmin, bmax = [0.0] * 3, [1.0] * 3
    params = swz.TileParams(sampler=swz.GRID_CENTER, max_points_per_node=20000, spacing_at_root=swz.spacing_from_diagonal(bmin, bmax, 250))
    t = swz.Tiler(ctx, bmin, bmax, params, capacity_hint=n)
    rng = np.random.default_rng(1)
    per = n // batches
    t0 = time.perf_counter()
    for b in range(batches):
        m = per if b + 1 < batches else n - per * (batches - 1)
        t.add_batch(rng.random((m, 3)), {"rgb": rng.integers(0, 256, (m, 3), dtype=np.uint8),
                                         "intensity": rng.integers(0, 65536, m, dtype=np.uint16)})
    t.finalize()
    info, nodes = t.info(), t.node_table()
    stored = int(info["num_stored"])
    work = tempfile.mkdtemp(prefix="swz_convert_probe_", dir=base)
    src = os.path.join(work, "src_bin")
    out = dict(points=n, batches=batches, stored=stored, nodes=int(info["num_nodes"]), tile_s=time.perf_counter() - t0,
               write_bin=t.write_output(src, "BIN", attrs=NAMES))
    t.write_properties(src)
    src_tiles = os.path.join(work, "src_tiles")
    if source_format == "3DTILES":
        out["write_3dtiles"] = t.write_output(src_tiles, "3DTILES", attrs=NAMES)
        t.write_properties(src_tiles)
    elif source_format:
        raise SystemExit("--source-format: only 3DTILES is timed beside the BIN source")
    print("CONVERT_PROBE " + json.dumps(dict(source=out)), flush=True)
    for fmt in formats:
        row = dict(format=fmt)
        legs = [("convert", lambda d: swz.convert_dataset(ctx, src, d, fmt, attrs=NAMES)),
                ("write_output", lambda d: t.write_output(d, fmt, attrs=NAMES))]
        if projection and fmt == "3DTILES":
            legs.append(("convert_world", lambda d: swz.convert_dataset_world(ctx, src, d, projection, attrs=NAMES)))
        if source_format == "3DTILES":
            legs.append(("convert_from_3DTILES", lambda d: swz.convert_dataset(ctx, src_tiles, d, fmt, attrs=NAMES, lossy_source=True)))
        for name, fn in legs:
            for rep in ("warm", "timed"):   # the first run pays allocations and the page cache
                d = os.path.join(work, name + "_" + fmt)
                shutil.rmtree(d, ignore_errors=True)
                row[name] = fn(d)
            shutil.rmtree(d, ignore_errors=True)
        d = os.path.join(work, "host_" + fmt)
        secs, done = host_recipe(swz, src, d, fmt, nodes, bmin, bmax, host_nodes)
        shutil.rmtree(d, ignore_errors=True)
        row["host_recipe"] = dict(measured_s=secs, points=done, scaled_to_all_s=secs * stored / max(done, 1))
        row["convert_over_write_output"] = row["convert"]["wall_ms"] / row["write_output"]["wall_ms"]
        row["host_over_convert"] = row["host_recipe"]["scaled_to_all_s"] * 1e3 / row["convert"]["wall_ms"]
        if "convert_from_3DTILES" in row:
            row["from_3dtiles_over_from_bin"] = row["convert_from_3DTILES"]["wall_ms"] / row["convert"]["wall_ms"]
        if "convert_world" in row:
            row["world_over_convert"] = row["convert_world"]["wall_ms"] / row["convert"]["wall_ms"]
        print("CONVERT_PROBE " + json.dumps(row), flush=True)
    shutil.rmtree(work, ignore_errors=True)
    t.close()
    ctx.close()


def main():
    args = sys.argv[1:]
    if args and args[0] == "--step":
        return step(int(args[1]), int(args[2]), args[3].split(","), args[4] or None, int(args[5]), args[6] or None,
                    (args[7] if len(args) > 7 else "") or None)

    def option(name, default):
        return args[args.index(name) + 1] if name in args else default
    n = int(args[0]) if args and not args[0].startswith("--") else 100_000_000
    limit = str(max(300, n // 50_000))
    # one child under its own time limit; check=True: a failure ends the script here
    r = subprocess.run(["timeout", "-k", "10", limit, sys.executable, os.path.abspath(__file__), "--step", str(n), option("--batches", "10"),
                        option("--formats", ",".join(FORMATS)), option("--dir", ""), option("--host-nodes", "0"), option("--source-projection", ""),
                        option("--source-format", "")], check=True,
                       stdout=subprocess.PIPE, text=True)
    results = [json.loads(l[len("CONVERT_PROBE "):]) for l in r.stdout.splitlines() if l.startswith("CONVERT_PROBE ")]
    for row in results:
        print(json.dumps(row), flush=True)
    if "--json" in args:
        with open(option("--json", None), "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
