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
usage: query_probe.py [points] [--batches K] [--dir DIR] [--host-nodes N] [--json FILE]"""
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


def host_recipe(swz, np, src, nodes, box, limit):
    """bin_read_node of the first `limit` nodes (0: all) and a numpy mask; seconds, points read, points inside"""
    lo, hi = np.asarray(box[0]), np.asarray(box[1])
    done = inside = 0
    t0 = time.perf_counter()
    for k in range(len(nodes["count"]) if not limit else min(limit, len(nodes["count"]))):
        xyz, cols = swz.bin_read_node(os.path.join(src, swz.node_name(int(nodes["level"][k]), int(nodes["key"][k])) + ".bin"))
        sel = ((xyz >= lo) & (xyz <= hi)).all(axis=1)
        kept = (xyz[sel], {name: v[sel] for name, v in cols.items()})
        done += len(xyz)
        inside += len(kept[0])
    return time.perf_counter() - t0, done, inside


def step(n, batches, base, host_nodes):
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
        t.add_batch(rng.random((m, 3)), {"rgb": rng.integers(0, 256, (m, 3), dtype=np.uint8),
                                         "intensity": rng.integers(0, 65536, m, dtype=np.uint16)})
    t.finalize()
    info, nodes = t.info(), t.node_table()
    stored = int(info["num_stored"])
    work = tempfile.mkdtemp(prefix="swz_query_probe_", dir=base)
    src = os.path.join(work, "src_bin")
    out = dict(points=n, batches=batches, stored=stored, nodes=int(info["num_nodes"]), write_bin=t.write_output(src, "BIN", attrs=NAMES))
    t.write_properties(src)
    t.close()
    print("QUERY_PROBE " + json.dumps(dict(source=out)), flush=True)
    for name, box in BOXES.items():
        row = dict(box=name)
        for rep in ("warm", "timed"):   # the first run pays allocations and the page cache
            got = swz.dataset_query(ctx, src, box[0], box[1], attrs=NAMES)
            row["query"] = dict(got["stats"], count=got["count"])
            del got
        secs, done, inside = host_recipe(swz, np, src, nodes, box, host_nodes)
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
        return step(int(args[1]), int(args[2]), args[3] or None, int(args[4]))

    def option(name, default):
        return args[args.index(name) + 1] if name in args else default
    n = int(args[0]) if args and not args[0].startswith("--") else 100_000_000
    limit = str(max(300, n // 50_000))
    # one child under its own time limit; check=True: a failure ends the script here
    r = subprocess.run(["timeout", "-k", "10", limit, sys.executable, os.path.abspath(__file__), "--step", str(n), option("--batches", "10"),
                        option("--dir", ""), option("--host-nodes", "0")], check=True, stdout=subprocess.PIPE, text=True)
    results = [json.loads(l[len("QUERY_PROBE "):]) for l in r.stdout.splitlines() if l.startswith("QUERY_PROBE ")]
    for row in results:
        print(json.dumps(row), flush=True)
    if "--json" in args:
        with open(option("--json", None), "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
