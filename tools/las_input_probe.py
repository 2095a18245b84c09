#!/usr/bin/env python3
"""Times Tiler.add_las_files (swz_tiler_add_las_files) beside the recipe out of the calls that existed before it, on the same
synthetic LAS tiles, in one process.

  python tools/las_input_probe.py [--tiles 16] [--points 1000000] [--batch 2000000] [--format 3]

The tiles (LAS 1.2, one point format, uniform coordinates inside a tile of a square mosaic) are written to a temporary
directory and read once before anything is timed, so both sides read them from the page cache: the numbers say what the
read path costs when the disk is not the limit.
  recipe: per file -- read the file, copy the records to the device (4-byte aligned: the point data is cut out on the host),
          swz_las_decode_device, copy positions and columns back into pinned host memory, stage_batch / tile_staged.
  stream: add_las_files with batch_points = --batch.
Both tile the same points with the same parameters; the recipe's batches are the files, the stream's are cut by --batch.
Prints one JSON line: wall times, the stream's stats (read / copy / decode / tile / wait), decode GB/s of both kernels."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SIZES = {0: 20, 1: 28, 2: 26, 3: 34}


def write_tile(path, rng, n, fmt, ox, oy):
    import struct
    rb = SIZES[fmt]
    rec = rng.integers(0, 255, (n, rb), dtype=np.uint8, endpoint=True)
    xyz = rng.integers(0, 1_000_000, (n, 3)).astype("<i4")
    rec[:, :12] = xyz.view(np.uint8).reshape(n, 12)
    h = bytearray(227)
    h[0:4] = b"LASF"
    h[24], h[25] = 1, 2
    struct.pack_into("<H", h, 94, 227)
    struct.pack_into("<I", h, 96, 227)
    h[104] = fmt
    struct.pack_into("<H", h, 105, rb)
    struct.pack_into("<I", h, 107, n)
    struct.pack_into("<3d", h, 131, 1e-3, 1e-3, 1e-3)
    struct.pack_into("<3d", h, 155, ox, oy, 0.0)
    struct.pack_into("<6d", h, 179, ox + 1000.0, ox, oy + 1000.0, oy, 1000.0, 0.0)
    with open(path, "wb") as f:
        f.write(bytes(h))
        f.write(rec.tobytes())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tiles", type=int, default=16)
    ap.add_argument("--points", type=int, default=1_000_000)
    ap.add_argument("--batch", type=int, default=2_000_000)
    ap.add_argument("--format", type=int, default=3, choices=sorted(SIZES))
    args = ap.parse_args()
    import torch
    import schwarzwald_amd as swz

    rng = np.random.default_rng(1)
    side = int(np.ceil(np.sqrt(args.tiles)))
    with tempfile.TemporaryDirectory() as d:
        paths = []
        for i in range(args.tiles):
            paths.append(os.path.join(d, "tile_%03d.las" % i))
            write_tile(paths[-1], rng, args.points, args.format, 400000.0 + 1000.0 * (i % side), 5400000.0 + 1000.0 * (i // side))
        for p in paths:  # into the page cache
            with open(p, "rb") as f:
                while f.read(1 << 24):
                    pass
        files, ds = swz.las_scan_files(paths)
        names = ds["attrs"]
        bounds = ds["cubic"]
        params = swz.TileParams(sampler=swz.RANDOM_GRID, max_points_per_node=20000,
                                spacing_at_root=swz.spacing_from_diagonal(bounds[0], bounds[1], 250), strategy=swz.FAST)
        n_total = ds["total_points"]
        rb = SIZES[args.format]
        dev = torch.device("cuda:0")
        out = dict(tiles=args.tiles, points=n_total, record_bytes=rb, batch_points=args.batch, columns=len(names))

        # ---- the stream
        with swz.Context(0) as ctx:
            with swz.Tiler(ctx, bounds[0], bounds[1], params) as t:
                t.reserve(n_total)
                t0 = time.perf_counter()
                st = t.add_las_files(paths, batch_points=args.batch)
                t.finalize()
                out["stream_wall_ms"] = (time.perf_counter() - t0) * 1e3
                out["stream"] = {k: (round(v, 3) if isinstance(v, float) else v) for k, v in st.items()}
                out["stream_nodes"] = int(t.info()["num_nodes"])
        row = 24 + sum(np.dtype(swz.ATTRIBUTES[k][1]).itemsize * swz.ATTRIBUTES[k][2] for k in names)
        out["stream_decode_GBps"] = n_total * (rb + row) / (st["decode_ms"] * 1e-3) / 1e9 if st["decode_ms"] else None

        # ---- the recipe out of the earlier calls
        with swz.Context(0) as ctx:
            ctx.set_stream(torch.cuda.current_stream(dev).cuda_stream)
            with swz.Tiler(ctx, bounds[0], bounds[1], params) as t:
                t.reserve(n_total)
                d_xyz = torch.empty((args.points, 3), dtype=torch.float64, device=dev)
                d_cols = {}
                for k in names:
                    _, dt, width = swz.ATTRIBUTES[k]
                    d_cols[k] = torch.empty((args.points, width) if width > 1 else (args.points,), dtype=getattr(torch, np.dtype(dt).name),
                                            device=dev)
                host = [dict(xyz=swz.pinned_empty((args.points, 3), np.float64),
                             **{k: swz.pinned_empty(tuple(d_cols[k].shape), swz.ATTRIBUTES[k][1]) for k in names}) for _ in range(2)]
                decode_ms = 0.0
                t0 = time.perf_counter()
                staged = 0
                for i, (p, f) in enumerate(zip(paths, files)):
                    raw = np.fromfile(p, dtype=np.uint8, offset=f["offset_to_point_data"])       # read, aligned by the cut
                    d_raw = torch.from_numpy(raw).to(dev)
                    torch.cuda.synchronize()
                    t1 = time.perf_counter()
                    ctx.las_decode_device(d_raw.data_ptr(), f["count"], f["scale"], f["offset"], f["min"], f["max"], f["point_format"],
                                          f["record_bytes"], d_xyz.data_ptr(), {k: v.data_ptr() for k, v in d_cols.items()})
                    decode_ms += (time.perf_counter() - t1) * 1e3
                    if staged == 2:
                        t.tile_staged()
                        staged -= 1
                    h = host[i & 1]
                    torch.from_numpy(h["xyz"]).copy_(d_xyz)
                    for k in names:
                        torch.from_numpy(h[k]).copy_(d_cols[k])
                    t.stage_batch(h["xyz"], {k: h[k] for k in names})
                    staged += 1
                while staged:
                    t.tile_staged()
                    staged -= 1
                t.finalize()
                out["recipe_wall_ms"] = (time.perf_counter() - t0) * 1e3
                out["recipe_decode_ms"] = decode_ms
                out["recipe_decode_GBps"] = n_total * (rb + row) / (decode_ms * 1e-3) / 1e9
                out["recipe_nodes"] = int(t.info()["num_nodes"])
        out["speedup"] = out["recipe_wall_ms"] / out["stream_wall_ms"]
        print(json.dumps(out))


if __name__ == "__main__":
    main()
