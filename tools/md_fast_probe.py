#!/usr/bin/env python3
"""MIN_DISTANCE and MIN_DISTANCE_FAST side by side on one GPU: uniform points in the unit cube, spacing = diagonal / 250,
20 000 points per node, one batch, ACCURATE.  Reports per sampler the wall time of swz_tile_device (best of the repeats), the
tile statistics (points_visited, nodes, levels) and the swz_profile_* classes of one profiled run -- among them
md_fast_candidates and md_fast_scatter, the two passes MIN_DISTANCE_FAST adds, next to level_compact, a pass of the same kind.
Each sampler runs in a child process of its own under `timeout`; the first one that fails ends the script.
usage: md_fast_probe.py [points] [--repeat K] [--json FILE]"""
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
SAMPLERS = ("MIN_DISTANCE", "MIN_DISTANCE_FAST")


def step(name, n, repeat):
    import torch
    import schwarzwald_amd as swz
    dev = torch.device("cuda", 0)
    ctx = swz.Context(0)
    bmin, bmax = [0.0] * 3, [1.0] * 3
    xyz = torch.empty((n, 3), dtype=torch.float64, device=dev)
    keys = torch.empty(n, dtype=torch.int64, device=dev)
    perm = torch.empty(n, dtype=torch.int32, device=dev)
    level = torch.empty(n, dtype=torch.int8, device=dev)
    torch.cuda.synchronize()
    params = swz.TileParams(sampler=swz.ALL_SAMPLERS[name], max_points_per_node=20000,
                            spacing_at_root=swz.spacing_from_diagonal(bmin, bmax, 250))

    def run():
        ctx.generate_uniform_device(2025, 0, n, xyz.data_ptr())  # (the tile clamps in place: the same input every time)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        stats = ctx.tile_device(xyz.data_ptr(), n, bmin, bmax, params, keys.data_ptr(), perm.data_ptr(), level.data_ptr())
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, stats

    run()  # warm-up: the workspace grows to its size
    walls = []
    for _ in range(repeat):
        ms, stats = run()
        walls.append(ms)
    ctx.profile_enable(True)
    ctx.profile_reset()
    profiled_ms, _ = run()
    classes = ctx.profile_get()
    ctx.profile_enable(False)
    per_level = torch.bincount(level.to(torch.int64) + 1, minlength=22).cpu().tolist()
    out = dict(sampler=name, points=n, wall_ms=min(walls), wall_ms_all=walls, profiled_wall_ms=profiled_ms, stats=stats,
               points_per_level={str(l - 1): c for l, c in enumerate(per_level) if c},
               classes={k: dict(ms=v["total_ms"], launches=v["launches"]) for k, v in sorted(classes.items())})
    ctx.close()
    print("MD_FAST_PROBE " + json.dumps(out), flush=True)


def main():
    args = sys.argv[1:]
    if args and args[0] == "--step":
        return step(args[1], int(args[2]), int(args[3]))
    n = int(args[0]) if args and not args[0].startswith("--") else 1_000_000_000
    repeat = int(args[args.index("--repeat") + 1]) if "--repeat" in args else 3
    limit = str(max(120, n // 2_000_000))
    results = {}
    for name in SAMPLERS:
        # one child per sampler, each under its own time limit; check=True: a failure ends the script here
        r = subprocess.run(["timeout", "-k", "10", limit, sys.executable, os.path.abspath(__file__), "--step", name, str(n), str(repeat)],
                           check=True, stdout=subprocess.PIPE, text=True)
        line = [l for l in r.stdout.splitlines() if l.startswith("MD_FAST_PROBE ")][-1]
        results[name] = json.loads(line[len("MD_FAST_PROBE "):])
    for name in SAMPLERS:
        r = results[name]
        s = r["stats"]
        print("%-17s %d points: wall %.1f ms (runs: %s), points_visited %d, nodes %d, levels %d, deepest %d"
              % (name, n, r["wall_ms"], " ".join("%.1f" % w for w in r["wall_ms_all"]), s["points_visited"], s["num_nodes"],
                 s["num_levels"], s["max_level"]))
        print("  points persisted per level: " + ", ".join("%s: %d" % kv for kv in r["points_per_level"].items()))
        print("  profile classes (ms, one profiled run of %.1f ms): " % r["profiled_wall_ms"]
              + ", ".join("%s %.2f" % (k, v["ms"]) for k, v in r["classes"].items()))
    a, b = results["MIN_DISTANCE"], results["MIN_DISTANCE_FAST"]
    print("MIN_DISTANCE_FAST / MIN_DISTANCE: wall %.3f, points_visited %.3f"
          % (b["wall_ms"] / a["wall_ms"], b["stats"]["points_visited"] / max(1, a["stats"]["points_visited"])))
    if "--json" in args:
        with open(args[args.index("--json") + 1], "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
