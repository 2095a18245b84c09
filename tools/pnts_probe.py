#!/usr/bin/env python3
"""Times the two ways from a tiled batch with RGB and intensity to the .pnts bodies of its nodes in host memory:
  (a) swz_gather_payload_device (double positions + columns, 29 B/point), copy to the host, narrow and lay out on the host;
  (b) swz_pnts_pack_device (the image of all bodies, 17 B/point + padding), copy of the image.
Each path runs in a child process of its own under `timeout`; the first one that fails ends the script.
usage: pnts_probe.py [points] [--json FILE]"""
import json
import os
import subprocess
import sys
import time
import zlib

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
NAMES = ("rgb", "intensity")


def step(which, n):
    import numpy as np
    import torch
    import schwarzwald_amd as swz
    dev = torch.device("cuda", 0)
    ctx = swz.Context(0)
    bmin, bmax = [0.0] * 3, [1.0] * 3
    torch.manual_seed(1)
    xyz = torch.rand((n, 3), dtype=torch.float64, device=dev)
    rgb = torch.randint(0, 256, (n, 3), dtype=torch.uint8, device=dev)
    inten = torch.randint(-32768, 32767, (n,), dtype=torch.int16, device=dev)
    params = swz.TileParams(sampler=swz.GRID_CENTER, max_points_per_node=20000, spacing_at_root=swz.spacing_from_diagonal(bmin, bmax, 250))
    keys = torch.empty(n, dtype=torch.int64, device=dev)
    perm = torch.empty(n, dtype=torch.int32, device=dev)
    level = torch.empty(n, dtype=torch.int8, device=dev)
    order = torch.empty(n, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    ctx.tile_device(xyz.data_ptr(), n, bmin, bmax, params, keys.data_ptr(), perm.data_ptr(), level.data_ptr())
    nodes = ctx.build_node_lists_device(keys.data_ptr(), level.data_ptr(), n, order.data_ptr())
    del keys, level
    lay = swz.pnts_layout(nodes["count"], NAMES)
    total = lay["total"]
    attrs = {"rgb": rgb.data_ptr(), "intensity": inten.data_ptr()}
    out = dict(path=which, points=n, nodes=len(nodes["count"]), image_bytes=total)

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

    h_image = swz.pinned_empty((total,), np.uint8)
    if which == "a":
        out_xyz, out_rgb, out_int = torch.empty_like(xyz), torch.empty_like(rgb), torch.empty_like(inten)
        out_attrs = {"rgb": out_rgb.data_ptr(), "intensity": out_int.data_ptr()}
        out["gather_ms"] = timed(lambda: ctx.gather_payload_device(perm.data_ptr(), order.data_ptr(), n, xyz.data_ptr(), attrs,
                                                                  out_xyz.data_ptr(), out_attrs), repeat=3)
        h_xyz, h_rgb, h_int = swz.pinned_empty((n, 3), np.float64), swz.pinned_empty((n, 3), np.uint8), swz.pinned_empty((n,), np.uint16)

        def copy():
            for h, d in ((h_xyz, out_xyz), (h_rgb, out_rgb), (h_int, out_int)):
                torch.from_numpy(h.view(np.uint8).reshape(-1)).copy_(d.view(torch.uint8).reshape(-1), non_blocking=True)
        out["copy_ms"] = timed(copy, repeat=2)
        out["copied_bytes"] = n * 29

        def convert():
            f32 = h_xyz.astype(np.float32).reshape(-1).view(np.uint8)
            b_rgb, b_int = h_rgb.reshape(-1), h_int.view(np.uint8)
            for k in np.flatnonzero(nodes["count"]):
                o, c, at = int(nodes["offset"][k]), int(nodes["count"][k]), int(lay["offset"][k])
                body = h_image[at:at + int(lay["size"][k])]
                body[:12 * c] = f32[12 * o:12 * (o + c)]
                r, i = int(lay["rgb_offset"][k]), int(lay["intensity_offset"][k])
                body[r:r + 3 * c] = b_rgb[3 * o:3 * (o + c)]
                body[r + 3 * c:i] = 0
                body[i:i + 2 * c] = b_int[2 * o:2 * (o + c)]
                body[i + 2 * c:] = 0
        out["host_convert_ms"] = timed(convert)
        out["total_ms"] = out["gather_ms"] + out["copy_ms"] + out["host_convert_ms"]
    else:
        image = torch.empty(total, dtype=torch.uint8, device=dev)
        out["pack_ms"] = timed(lambda: ctx.pnts_pack_device(perm.data_ptr(), order.data_ptr(), n, xyz.data_ptr(), attrs, nodes,
                                                            image.data_ptr(), total, attrs=NAMES), repeat=3)
        # what the kernel has to move: order + perm, the 29-byte source row, the image
        out["pack_bytes"] = n * (8 + 29) + total
        out["pack_GBps"] = out["pack_bytes"] / out["pack_ms"] / 1e6
        out["pack_payload_GBps"] = (n * 29 + total) / out["pack_ms"] / 1e6
        out["copy_ms"] = timed(lambda: torch.from_numpy(h_image).copy_(image, non_blocking=True), repeat=2)
        out["copied_bytes"] = total
        out["total_ms"] = out["pack_ms"] + out["copy_ms"]
    out["image_crc32"] = zlib.crc32(h_image[:min(total, 1 << 28)])
    ctx.close()
    print("PNTS_PROBE " + json.dumps(out), flush=True)


def main():
    args = sys.argv[1:]
    if args and args[0] == "--step":
        return step(args[1], int(args[2]))
    n = int(args[0]) if args and not args[0].startswith("--") else 100_000_000
    limit = str(max(120, n // 250_000))
    results = {}
    for which in ("a", "b"):
        # one child per path, each under its own time limit; check=True: a failure ends the script here
        r = subprocess.run(["timeout", "-k", "10", limit, sys.executable, os.path.abspath(__file__), "--step", which, str(n)],
                           check=True, stdout=subprocess.PIPE, text=True)
        line = [l for l in r.stdout.splitlines() if l.startswith("PNTS_PROBE ")][-1]
        results[which] = json.loads(line[len("PNTS_PROBE "):])
    a, b = results["a"], results["b"]
    print("%d points, %d nodes, image %.3f GB (%.2f B/point)" % (n, a["nodes"], a["image_bytes"] / 1e9, a["image_bytes"] / n))
    print("(a) gather %.1f ms + copy of %.3f GB %.1f ms + host narrow and lay out %.1f ms = %.1f ms"
          % (a["gather_ms"], a["copied_bytes"] / 1e9, a["copy_ms"], a["host_convert_ms"], a["total_ms"]))
    print("(b) pack %.1f ms (%.0f GB/s of order + perm + 29 B read + image written; %.0f GB/s of the 29 B + image alone)"
          " + copy of %.3f GB %.1f ms = %.1f ms" % (b["pack_ms"], b["pack_GBps"], b["pack_payload_GBps"], b["copied_bytes"] / 1e9,
                                                    b["copy_ms"], b["total_ms"]))
    print("images agree: %s" % (a["image_crc32"] == b["image_crc32"]))
    if "--json" in args:
        with open(args[args.index("--json") + 1], "w") as f:
            json.dump(results, f, indent=1)
    if a["image_crc32"] != b["image_crc32"]:
        sys.exit("the two paths produced different images")


if __name__ == "__main__":
    main()
