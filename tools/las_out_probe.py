#!/usr/bin/env python3
"""Times the two ways from a tiled batch to the LAS point records of its nodes in host memory, for each of the four record
lengths (20, 28, 26, 34 bytes: intensity always, gps time and colour in turn):
  (a) swz_gather_payload_device of the same columns, the copies of the gathered rows to the host, and the conversion of
      las_write_node_rows node by node on one host thread (files go to /dev/null) -- what persist_rows gives a user today;
  (b) swz_las_pack_device (the image of all bodies) and one copy of the image.
Both run in the same child process on the same node table, one child per mask under `timeout`; the first one that fails
ends the script.  The first nodes of the table are also written both ways and compared.
usage: las_out_probe.py [points] [--json FILE]"""
import json
import os
import subprocess
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
MASKS = {"20": ("intensity",), "28": ("intensity", "gps_time"), "26": ("rgb", "intensity"), "34": ("rgb", "intensity", "gps_time")}


def step(which, n):
    import numpy as np
    import torch
    import schwarzwald_amd as swz
    names = MASKS[which]
    dev = torch.device("cuda", 0)
    ctx = swz.Context(0)
    bmin, bmax = [0.0] * 3, [1.0] * 3
    torch.manual_seed(1)
    xyz = torch.rand((n, 3), dtype=torch.float64, device=dev)
    cols = {"intensity": torch.randint(-32768, 32767, (n,), dtype=torch.int16, device=dev)}
    if "rgb" in names:
        cols["rgb"] = torch.randint(0, 256, (n, 3), dtype=torch.uint8, device=dev)
    if "gps_time" in names:
        cols["gps_time"] = torch.rand((n,), dtype=torch.float64, device=dev)
    params = swz.TileParams(sampler=swz.GRID_CENTER, max_points_per_node=20000, spacing_at_root=swz.spacing_from_diagonal(bmin, bmax, 250))
    keys = torch.empty(n, dtype=torch.int64, device=dev)
    perm = torch.empty(n, dtype=torch.int32, device=dev)
    level = torch.empty(n, dtype=torch.int8, device=dev)
    order = torch.empty(n, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    ctx.tile_device(xyz.data_ptr(), n, bmin, bmax, params, keys.data_ptr(), perm.data_ptr(), level.data_ptr())
    nodes = ctx.build_node_lists_device(keys.data_ptr(), level.data_ptr(), n, order.data_ptr())
    del keys, level
    boxes = [swz.node_bounds(int(l), int(k), bmin, bmax) for l, k in zip(nodes["level"], nodes["key"])]
    mn, mx = np.array([b[0] for b in boxes]), np.array([b[1] for b in boxes])
    scales = np.array([swz.las_scale_from_bounds(a, b) for a, b in zip(mn, mx)])
    lay = swz.las_image_layout(nodes["count"], names)
    total = lay["total"]
    attrs = {k: v.data_ptr() for k, v in cols.items()}
    row = 24 + sum(v.element_size() * (3 if k == "rgb" else 1) for k, v in cols.items())
    out = dict(record_bytes=int(which), points=n, nodes=len(nodes["count"]), image_bytes=total, row_bytes=row)

    def timed(fn, repeat=1):
        best = None
        for _ in range(repeat):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) * 1e3
            best = ms if best is None else min(best, ms)
        return best

    # (a) gather, copy the rows, convert on the host
    out_xyz = torch.empty_like(xyz)
    out_cols = {k: torch.empty_like(v) for k, v in cols.items()}
    out["gather_ms"] = timed(lambda: ctx.gather_payload_device(perm.data_ptr(), order.data_ptr(), n, xyz.data_ptr(), attrs, out_xyz.data_ptr(),
                                                              {k: v.data_ptr() for k, v in out_cols.items()}), repeat=3)
    np_dtype = {"intensity": np.uint16, "rgb": np.uint8, "gps_time": np.float64}
    h_xyz = swz.pinned_empty((n, 3), np.float64)
    h_cols = {k: swz.pinned_empty(tuple(v.shape), np_dtype[k]) for k, v in cols.items()}

    def copy_rows():
        for h, d in [(h_xyz, out_xyz)] + [(h_cols[k], out_cols[k]) for k in cols]:
            torch.from_numpy(h.view(np.uint8).reshape(-1)).copy_(d.view(torch.uint8).reshape(-1), non_blocking=True)
    out["rows_copy_ms"] = timed(copy_rows, repeat=2)
    out["rows_copied_bytes"] = n * row
    listed = np.flatnonzero(nodes["count"])

    def convert(where, which_nodes):
        for k in which_nodes:
            o, c = int(nodes["offset"][k]), int(nodes["count"][k])
            swz.las_write_node_rows(where(k), h_xyz[o:o + c], {a: h[o:o + c] for a, h in h_cols.items()}, mn[k], mx[k], scales[k])
    out["host_convert_ms"] = timed(lambda: convert(lambda k: "/dev/null", listed))
    out["rows_total_ms"] = out["gather_ms"] + out["rows_copy_ms"] + out["host_convert_ms"]
    del out_xyz, out_cols

    # (b) pack, copy the image
    image = torch.empty(total, dtype=torch.uint8, device=dev)
    out["pack_ms"] = timed(lambda: ctx.las_pack_device(perm.data_ptr(), order.data_ptr(), n, xyz.data_ptr(), attrs, nodes, mn, scales,
                                                       image.data_ptr(), total, attrs=names), repeat=3)
    out["pack_over_gather"] = out["pack_ms"] / out["gather_ms"]
    # what each kernel has to move: order + perm and the source row, then the rows again / the image
    out["gather_bytes"] = n * (8 + 2 * row)
    out["pack_bytes"] = n * (8 + row) + total
    out["gather_GBps"] = out["gather_bytes"] / out["gather_ms"] / 1e6
    out["pack_GBps"] = out["pack_bytes"] / out["pack_ms"] / 1e6
    h_image = swz.pinned_empty((total,), np.uint8)
    out["image_copy_ms"] = timed(lambda: torch.from_numpy(h_image).copy_(image, non_blocking=True), repeat=2)
    out["pack_total_ms"] = out["pack_ms"] + out["image_copy_ms"]

    # the first nodes both ways: the files must agree
    some = listed[:8]
    with tempfile.TemporaryDirectory() as tmp:
        convert(lambda k: os.path.join(tmp, "rows%d.las" % k), some)
        for k in some:
            at, c = int(lay["offset"][k]), int(nodes["count"][k])
            swz.las_write_node(os.path.join(tmp, "pack%d.las" % k), c, h_image[at:at + int(lay["size"][k])], names, mn[k], mx[k], scales[k])
        out["files_agree"] = all(open(os.path.join(tmp, "rows%d.las" % k), "rb").read() == open(os.path.join(tmp, "pack%d.las" % k), "rb").read()
                                 for k in some)
    ctx.close()
    print("LAS_OUT_PROBE " + json.dumps(out), flush=True)


def main():
    args = sys.argv[1:]
    if args and args[0] == "--step":
        return step(args[1], int(args[2]))
    n = int(args[0]) if args and not args[0].startswith("--") else 100_000_000
    limit = str(max(120, n // 250_000))
    results = {}
    for which in MASKS:
        # one child per mask, each under its own time limit; check=True: a failure ends the script here
        r = subprocess.run(["timeout", "-k", "10", limit, sys.executable, os.path.abspath(__file__), "--step", which, str(n)],
                           check=True, stdout=subprocess.PIPE, text=True)
        line = [l for l in r.stdout.splitlines() if l.startswith("LAS_OUT_PROBE ")][-1]
        o = results[which] = json.loads(line[len("LAS_OUT_PROBE "):])
        print("%2d-byte records, %d points, %d nodes, image %.3f GB" % (o["record_bytes"], n, o["nodes"], o["image_bytes"] / 1e9))
        print("  (a) gather %.2f ms (%.0f GB/s) + copy of %.3f GB %.1f ms + host conversion %.1f ms = %.1f ms"
              % (o["gather_ms"], o["gather_GBps"], o["rows_copied_bytes"] / 1e9, o["rows_copy_ms"], o["host_convert_ms"], o["rows_total_ms"]))
        print("  (b) pack %.2f ms (%.0f GB/s, %.2f x the gather) + copy of %.3f GB %.1f ms = %.1f ms; files agree: %s"
              % (o["pack_ms"], o["pack_GBps"], o["pack_over_gather"], o["image_bytes"] / 1e9, o["image_copy_ms"], o["pack_total_ms"],
                 o["files_agree"]), flush=True)
    if "--json" in args:
        with open(args[args.index("--json") + 1], "w") as f:
            json.dump(results, f, indent=1)
    if not all(o["files_agree"] for o in results.values()):
        sys.exit("the two paths wrote different files")


if __name__ == "__main__":
    main()
