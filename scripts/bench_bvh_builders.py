#!/usr/bin/env python3
"""The three BVH builders side by side on one GPU, one process (bench.py stays the flagship's yardstick): commit ms, render ms, k_trace
ms and node visits per closest-hit ray for BVH_HOST_SAH (0), BVH_GPU_LBVH (1) and BVH_GPU_LBVH_WIDE (2) on the geometry of C2 (the
Cornell box with the two meshes, GGX) or C4 (the hair scene), 1920 x 1080 x 64 spp.  The builders alternate (0 1 2 0 1 2 ...), best of
--rounds each; the median and the spread (max - min over the rounds) are printed beside every best so that a difference can be held
against them.  Every round's figures are printed as they come: on a shared machine a render can hit a host stall of seconds, which the
spread then shows and the median and k_trace (device events) do not.

    python scripts/bench_bvh_builders.py [--scene c2|c4] [--rounds 5] [--spp 64] [--width 1920 --height 1080]

Prints one table and one JSON line.  Commit is CommitScene alone (scene ingestion is not timed); with PBRHIP_DEBUG=1 in the environment
the library prints how builder 2's commit splits into the collapse, the download and the walk entries."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="c2", choices=["c2", "c4"])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    a = ap.parse_args()
    import torch
    import pbrlab_amd as pa
    from pbrlab_amd import scenes
    if pa.device_count() < 1:
        raise SystemExit("no HIP device")
    pa.set_device(0)
    desc = scenes.cornell_scene("ggx", seed=1) if a.scene == "c2" else scenes.hair_scene(seed=1)
    rgba = torch.empty((a.height, a.width, 4), dtype=torch.float32, device="cuda:0")
    count = torch.empty((a.height, a.width), dtype=torch.int32, device="cuda:0")
    out = (rgba.data_ptr(), count.data_ptr())
    names = {0: "host SAH", 1: "GPU LBVH", 2: "GPU LBVH + Q tree"}
    res = {b: dict(commit=[], render=[], trace=[]) for b in names}
    info = {}

    def commit(builder):
        s = pa.Scene()
        s.SetBvhBuilder(builder)
        took = {}
        inner = s.CommitScene

        def timed():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            inner()
            took["ms"] = (time.perf_counter() - t0) * 1e3
        s.CommitScene = timed
        scenes.build_scene(s, desc, pa.make_principled, pa.make_hair)
        return s, took["ms"]

    for b in names:                                                       # warm-up: code objects, allocator, clocks
        s, _ = commit(b)
        pa.Render(s, a.width, a.height, min(a.spp, 4), device_out=out)
    for r in range(a.rounds):
        for b in names:
            s, ms = commit(b)
            res[b]["commit"].append(ms)
            t0 = time.perf_counter()
            pa.Render(s, a.width, a.height, a.spp, device_out=out)
            res[b]["render"].append((time.perf_counter() - t0) * 1e3)
            _, st = pa.Render(s, a.width, a.height, a.spp, device_out=out, flags=pa.api.RENDER_TIMING_TRACE)
            res[b]["trace"].append(st["ms_trace_closest"])
            if r == 0:                                                    # an untimed extra render for the counters
                _, st = pa.Render(s, a.width, a.height, min(a.spp, 8), device_out=out, flags=pa.api.RENDER_STATS)
                info[b] = dict(s.wide_info(), **s.info(), visits=st["closest_nodes"] / max(st["closest_rays"], 1))
            print(f"round {r} builder {b}: commit {ms:.1f} ms, render {res[b]['render'][-1]:.1f} ms, k_trace {res[b]['trace'][-1]:.1f} ms", flush=True)
            del s
    line = {"scene": a.scene, "width": a.width, "height": a.height, "spp": a.spp, "rounds": a.rounds, "gpu": torch.cuda.get_device_name(0)}
    print(f"\n{a.scene} {a.width}x{a.height}x{a.spp}, best of {a.rounds} / median (spread = max - min):")
    print(f"{'builder':<20}{'commit ms':>26}{'render ms':>28}{'k_trace ms':>26}{'visits/ray':>12}{'Q nodes':>10}{'need':>6}")
    for b, nm in names.items():
        cell = lambda v: f"{min(v):.1f} / {sorted(v)[len(v) // 2]:.1f} (+{max(v) - min(v):.1f})"         # noqa: E731
        print(f"{nm:<20}{cell(res[b]['commit']):>26}{cell(res[b]['render']):>28}{cell(res[b]['trace']):>26}{info[b]['visits']:>12.2f}"
              f"{info[b]['wide_nodes']:>10}{info[b]['stack_need']:>6}")
        line[f"builder{b}"] = dict(commit_ms=min(res[b]["commit"]), commit_spread=max(res[b]["commit"]) - min(res[b]["commit"]),
                                   render_ms=min(res[b]["render"]), render_median=sorted(res[b]["render"])[len(res[b]["render"]) // 2], render_spread=max(res[b]["render"]) - min(res[b]["render"]),
                                   trace_ms=min(res[b]["trace"]), trace_spread=max(res[b]["trace"]) - min(res[b]["trace"]),
                                   visits_per_ray=info[b]["visits"], wide_nodes=info[b]["wide_nodes"], stack_need=info[b]["stack_need"],
                                   built_on_gpu=info[b]["built_on_gpu"], depth=info[b]["depth"])
    r0, r1, r2 = (min(res[b]["render"]) for b in (0, 1, 2))
    print(f"render: builder 2 vs builder 1 {100 * (r2 / r1 - 1):+.1f} % (builder 1's own spread {100 * (max(res[1]['render']) / r1 - 1):.1f} %), "
          f"builder 2 vs builder 0 {100 * (r2 / r0 - 1):+.1f} %; commit: builder 2 adds {min(res[2]['commit']) - min(res[1]['commit']):.1f} ms to builder 1")
    print(json.dumps(line))


if __name__ == "__main__":
    main()
