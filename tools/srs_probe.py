#!/usr/bin/env python3
"""Times the source projection on the device: las_decode_segments_device without and with an srs (the two instantiations of
the segment kernel) and srs_transform_device alone, on generated format-3 records of one UTM 32N tile.  Prints points per
second and the bandwidth of each (decode: record + 24 position bytes + the attribute columns per point; transform: 48 bytes).

    python tools/srs_probe.py [--points 100000000] [--repeats 7] [--plain-only]

Every figure is the median of --repeats timed launches after one warm-up, taken with device events around the call (the
call's own synchronisation of the stream included).  The in-place map is timed on fresh source coordinates every repeat: they
are restored OUTSIDE the pair of events.  --plain-only times the decode without a projection and nothing else: it runs on a
library that has no projection, for the comparison with an earlier commit."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=100_000_000)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--plain-only", action="store_true")
    args = ap.parse_args()
    import torch
    import schwarzwald_amd as swz

    n, rb = args.points, 34
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    # format 3 records: X, Y, Z in [0, 2^20) mm, everything else random bytes
    raw = torch.randint(0, 256, (n, rb), dtype=torch.uint8, device=dev, generator=g)
    xyz_i = torch.randint(0, 2 ** 20, (n, 3), dtype=torch.int32, device=dev, generator=g)
    raw[:, :12] = xyz_i.view(torch.uint8).reshape(n, 12)
    del xyz_i
    seg = dict(first_row=0, count=n, byte_offset=0, scale=[1e-3] * 3, offset=[412000.0, 5401000.0, 250.0],
               min=[412000.0, 5401000.0, 250.0], max=[413048.576, 5402048.576, 1298.576], point_format=3, record_bytes=rb)
    srs = None if args.plain_only else swz.Srs("+proj=utm +zone=32 +datum=WGS84")
    center = [4170000.0, 650000.0, 4760000.0]
    xyz = torch.empty((n, 3), dtype=torch.float64, device=dev)
    names = ["rgb", "intensity", "classification", "gps_time"]
    widths = {"rgb": 3, "intensity": 2, "classification": 1, "gps_time": 8}
    cols = {k: torch.empty(n * widths[k], dtype=torch.uint8, device=dev) for k in names}
    ptrs = {k: v.data_ptr() for k, v in cols.items()}
    decode_bytes = rb + 24 + sum(widths.values())

    def timed(fn, before=None):
        if before:
            before()
        fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.repeats):
            if before:
                before()
                torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        return float(np.median(ms)), float(np.min(ms)), float(np.max(ms))

    with swz.Context(0) as ctx:
        ctx.set_stream(torch.cuda.current_stream(dev).cuda_stream)
        plain = lambda: ctx.las_decode_segments_device(raw.data_ptr(), n * rb, [seg], xyz.data_ptr(), ptrs, shift_center=center)
        rows = [("decode", decode_bytes, plain)]
        if not args.plain_only:
            rows += [("decode + srs", decode_bytes, lambda: ctx.las_decode_segments_device(raw.data_ptr(), n * rb, [seg], xyz.data_ptr(), ptrs, shift_center=center, srs=srs)),
                     ("decode", decode_bytes, plain)]
        for name, bytes_per_point, fn in rows:
            med, lo, hi = timed(fn)
            print("%-14s %8.3f ms (min %.3f, max %.3f)  %7.2f G points/s  %7.1f GB/s" % (name, med, lo, hi, n / med / 1e6, n * bytes_per_point / med / 1e6))
        if args.plain_only:
            return
        ctx.las_decode_segments_device(raw.data_ptr(), n * rb, [seg], xyz.data_ptr(), ptrs)   # source coordinates
        keep = xyz.clone()
        med, lo, hi = timed(lambda: ctx.srs_transform_device(srs, xyz), before=lambda: xyz.copy_(keep))
        print("%-14s %8.3f ms (min %.3f, max %.3f)  %7.2f G points/s  %7.1f GB/s" % ("srs_transform", med, lo, hi, n / med / 1e6, n * 48 / med / 1e6))


if __name__ == "__main__":
    main()
