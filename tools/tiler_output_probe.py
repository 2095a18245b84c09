#!/usr/bin/env python3
"""Times the two ways from a finished multi-batch tiler (uniform points with RGB + intensity) to its node files on disk:
  (s) Tiler.write_output: streamed -- chunks packed from the pools, copied and written while the next one is packed;
  (w) the whole-image recipe by hand: export ids, node table, pools, ONE pack of the whole data set (BIN / BINZ: the gather of
      every column), ONE copy to the host, then *_persist_nodes.
Both write into a fresh directory under --dir (default: the system's temporary directory), per format, `--reps` times after
one warm-up; the medians and the spread (min .. max) are reported.  Each format runs in a child process of its own under
`timeout`; the first one that fails ends the script.
--tight-bounds adds, for the formats that hold a box (3DTILES, LAS, ENTWINE_LAS), a third series: (s) with tight_bounds=True,
and the node-box kernel alone over the whole data set (its time and the bytes per second it reaches).
usage: tiler_output_probe.py [points] [--batches K] [--reps R] [--formats BIN,LAS,...] [--dir DIR] [--json FILE] [--tight-bounds]"""
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
NAMES = ("rgb", "intensity")
FORMATS = ("BIN", "BINZ", "3DTILES", "LAS", "ENTWINE_LAS")


def step(fmt, n, batches, reps, base, tight=False):
    import numpy as np
    import torch
    import schwarzwald_amd as swz
    dev = torch.device("cuda", 0)
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
    info = t.info()
    out = dict(format=fmt, points=n, batches=batches, stored=int(info["num_stored"]), nodes=int(info["num_nodes"]),
               tile_s=time.perf_counter() - t0)
    ns = out["stored"]
    work = tempfile.mkdtemp(prefix="swz_output_probe_", dir=base)

    def fresh(name):
        d = os.path.join(work, name)
        shutil.rmtree(d, ignore_errors=True)
        return d

    def streamed():
        s = t.write_output(fresh("streamed"), fmt, attrs=NAMES)
        return s["wall_ms"], s

    def streamed_tight():
        s = t.write_output(fresh("streamed_tight"), fmt, attrs=NAMES, tight_bounds=True)
        return s["wall_ms"], s

    def whole():
        d = fresh("whole")
        torch.cuda.synchronize()
        w0 = time.perf_counter()
        if fmt == "ENTWINE_LAS":
            swz.ept_create_dirs(d)
        else:
            os.mkdir(d)
        nodes = t.node_table()
        d_ids = torch.empty(ns, dtype=torch.int32, device=dev)
        t.export_device(None, d_ids.data_ptr(), None)
        pool_xyz, pool = t.pools_device()
        parts = {}
        if fmt in ("BIN", "BINZ"):
            g_xyz = torch.empty((ns, 3), dtype=torch.float64, device=dev)
            g_rgb = torch.empty((ns, 3), dtype=torch.uint8, device=dev)
            g_int = torch.empty(ns, dtype=torch.int16, device=dev)
            p0 = time.perf_counter()
            ctx.gather_payload_device(d_ids.data_ptr(), None, ns, pool_xyz, pool, g_xyz.data_ptr(),
                                      {"rgb": g_rgb.data_ptr(), "intensity": g_int.data_ptr()})
            torch.cuda.synchronize()
            parts["pack_ms"] = (time.perf_counter() - p0) * 1e3
            p0 = time.perf_counter()
            h_xyz, h_rgb, h_int = g_xyz.cpu().numpy(), g_rgb.cpu().numpy(), g_int.cpu().numpy().view(np.uint16)
            parts["copy_ms"] = (time.perf_counter() - p0) * 1e3
            p0 = time.perf_counter()
            ctx.bin_persist_nodes(d, nodes, h_xyz, {"rgb": h_rgb, "intensity": h_int}, compressed=fmt == "BINZ")
            parts["write_ms"] = (time.perf_counter() - p0) * 1e3
        else:
            if fmt == "3DTILES":
                total = swz.pnts_layout(nodes["count"], NAMES)["total"]
            else:
                total = swz.las_image_layout(nodes["count"], NAMES)["total"]
                boxes = [swz.node_bounds(int(l), int(k), bmin, bmax) for l, k in zip(nodes["level"], nodes["key"])]
                mn, mx = np.array([b[0] for b in boxes]), np.array([b[1] for b in boxes])
                scales = np.array([swz.las_scale_from_bounds(a, b) for a, b in zip(mn, mx)])
            image = torch.empty(total, dtype=torch.uint8, device=dev)
            p0 = time.perf_counter()
            if fmt == "3DTILES":
                ctx.pnts_pack_device(d_ids.data_ptr(), None, ns, pool_xyz, pool, nodes, image.data_ptr(), total, attrs=NAMES)
            else:
                ctx.las_pack_device(d_ids.data_ptr(), None, ns, pool_xyz, pool, nodes, mn, scales, image.data_ptr(), total, attrs=NAMES)
            torch.cuda.synchronize()
            parts["pack_ms"] = (time.perf_counter() - p0) * 1e3
            p0 = time.perf_counter()
            h_image = image.cpu().numpy()
            parts["copy_ms"] = (time.perf_counter() - p0) * 1e3
            p0 = time.perf_counter()
            if fmt == "3DTILES":
                ctx.pnts_persist_nodes(d, nodes, h_image, NAMES)
                swz.tileset_write(swz.tileset_build(nodes["level"], nodes["key"], bmin, bmax, params.spacing_at_root), d)
            else:
                entwine = fmt == "ENTWINE_LAS"
                ctx.las_persist_nodes(os.path.join(d, "ept-data") if entwine else d, nodes, h_image, NAMES, mn, mx, scales,
                                      swz.LAS_NAMING_ENTWINE if entwine else swz.LAS_NAMING_POTREE)
                if entwine:
                    swz.ept_hierarchy_write(d, nodes)
            parts["write_ms"] = (time.perf_counter() - p0) * 1e3
        return (time.perf_counter() - w0) * 1e3, parts

    def series(fn):
        fn()  # warm-up: allocations, page cache, the file system's directory
        runs = [fn() for _ in range(reps)]
        walls = [r[0] for r in runs]
        mid = runs[sorted(range(reps), key=lambda i: walls[i])[reps // 2]]
        return dict(wall_ms=statistics.median(walls), wall_min_ms=min(walls), wall_max_ms=max(walls), parts=mid[1])

    out["streamed"] = series(streamed)
    out["whole"] = series(whole)
    if tight and fmt not in ("BIN", "BINZ"):
        out["streamed_tight"] = series(streamed_tight)
        # the kernel alone: the boxes of all nodes in one call, timed by the library's own events
        d_ids = torch.empty(ns, dtype=torch.int32, device=dev)
        t.export_device(None, d_ids.data_ptr(), None)
        pool_xyz, _ = t.pools_device()
        nodes = t.node_table()
        ctx.node_boxes_device(d_ids.data_ptr(), None, ns, pool_xyz, nodes)  # warm-up
        ctx.profile_enable(True)
        ctx.profile_reset()
        for _ in range(reps):
            ctx.node_boxes_device(d_ids.data_ptr(), None, ns, pool_xyz, nodes)
        k = ctx.profile_get()["node_boxes"]
        ctx.profile_enable(False)
        out["node_boxes_kernel_ms"] = k["total_ms"] / reps
        out["node_boxes_GBps"] = k["algorithmic_bytes"] / reps / (k["total_ms"] / reps * 1e-3) / 1e9
    if fmt == "BIN":  # the kernels alone, on the same rows: bin_pack_kernel against the gather of the same columns
        d_ids = torch.empty(ns, dtype=torch.int32, device=dev)
        t.export_device(None, d_ids.data_ptr(), None)
        pool_xyz, pool = t.pools_device()
        nodes = t.node_table()
        total = swz.bin_layout(nodes["count"], NAMES)["total"]
        image = torch.empty(total, dtype=torch.uint8, device=dev)
        g_xyz = torch.empty((ns, 3), dtype=torch.float64, device=dev)
        g_rgb = torch.empty((ns, 3), dtype=torch.uint8, device=dev)
        g_int = torch.empty(ns, dtype=torch.int16, device=dev)

        def timed(fn):
            ms = []
            for _ in range(reps + 1):
                torch.cuda.synchronize()
                p0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                ms.append((time.perf_counter() - p0) * 1e3)
            return statistics.median(ms[1:])
        out["bin_pack_kernel_ms"] = timed(lambda: ctx.bin_pack_device(d_ids.data_ptr(), None, ns, pool_xyz, pool, nodes, image.data_ptr(),
                                                                      total, attrs=NAMES))
        out["gather_ms"] = timed(lambda: ctx.gather_payload_device(d_ids.data_ptr(), None, ns, pool_xyz, pool, g_xyz.data_ptr(),
                                                                   {"rgb": g_rgb.data_ptr(), "intensity": g_int.data_ptr()}))
    shutil.rmtree(work, ignore_errors=True)
    t.close()
    ctx.close()
    print("OUTPUT_PROBE " + json.dumps(out), flush=True)


def main():
    args = sys.argv[1:]
    if args and args[0] == "--step":
        return step(args[1], int(args[2]), int(args[3]), int(args[4]), args[5] if len(args) > 5 and args[5] else None,
                    len(args) > 6 and args[6] == "tight")

    def option(name, default):
        return args[args.index(name) + 1] if name in args else default
    n = int(args[0]) if args and not args[0].startswith("--") else 100_000_000
    batches, reps = int(option("--batches", 10)), int(option("--reps", 3))
    formats = option("--formats", ",".join(FORMATS)).split(",")
    limit = str(max(180, n // 100_000))
    results = []
    for fmt in formats:
        # one child per format, each under its own time limit; check=True: a failure ends the script here
        r = subprocess.run(["timeout", "-k", "10", limit, sys.executable, os.path.abspath(__file__), "--step", fmt, str(n), str(batches),
                            str(reps), option("--dir", ""), "tight" if "--tight-bounds" in args else ""], check=True,
                           stdout=subprocess.PIPE, text=True)
        line = [l for l in r.stdout.splitlines() if l.startswith("OUTPUT_PROBE ")][-1]
        print(line[len("OUTPUT_PROBE "):], flush=True)
        results.append(json.loads(line[len("OUTPUT_PROBE "):]))
    if "--json" in args:
        with open(option("--json", None), "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
