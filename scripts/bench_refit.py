#!/usr/bin/env python3
"""pbrhip_scene_refit against the same builder's commit, one GPU, one process (bench.py stays the flagship's yardstick).

    python scripts/bench_refit.py [--scene c2|c4] [--rounds 3] [--spp 64] [--width 1920 --height 1080]

c2 (the Cornell box with the two meshes, GGX): builders 0 (host SAH) and 2 (GPU LBVH + collapse) alternate; per round the commit of
that builder, then three refits of the committed scene -- only the monkey's mesh dirty, only Lucy's transform changed, every instance
dirty -- each split by the library's PBRHIP_DEBUG=1 line into host staging, upload + scatter, plan (first refit of a commit only), leaf
records + both trees, and the Q-node download + walk entries.  Then tree quality: the monkey displaced by 0.1, 0.5 and 2 of its box
sizes, node visits per closest-hit ray and k_trace ms after a refit against a fresh commit at the same pose.
c4 (the hair scene): one round on builder 2 with every strand swayed.

Prints every figure as it comes, a summary and one JSON line."""
import argparse
import json
import os
import re
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SPLIT = re.compile(r"refit: (\d+) of (\d+) slots dirty: host staging ([\d.]+) ms, upload \+ scatter ([\d.]+) ms, plan ([\d.]+) ms, "
                   r"pack \+ trees ([\d.]+) ms \((\d+) \+ (\d+) levels\), Q-node download \+ walk entries ([\d.]+) ms")


class Stderr:
    """what the library writes to file descriptor 2 while the block runs"""

    def __enter__(self):
        sys.stderr.flush()
        self.tmp = tempfile.TemporaryFile()
        self.keep = os.dup(2)
        os.dup2(self.tmp.fileno(), 2)
        return self

    def __exit__(self, *a):
        os.dup2(self.keep, 2)
        os.close(self.keep)
        self.tmp.seek(0)
        self.text = self.tmp.read().decode(errors="replace")
        self.tmp.close()


def timed_refit(s):
    import torch
    torch.cuda.synchronize()
    os.environ["PBRHIP_DEBUG"] = "1"
    try:
        with Stderr() as err:
            t0 = time.perf_counter()
            s.RefitScene()
            ms = (time.perf_counter() - t0) * 1e3
    finally:
        os.environ.pop("PBRHIP_DEBUG", None)
    m = SPLIT.search(err.text)
    keys = ("dirty", "slots", "host_ms", "upload_ms", "plan_ms", "trees_ms", "bin_levels", "q_levels", "entries_ms")
    split = {k: (float(v) if "ms" in k else int(v)) for k, v in zip(keys, m.groups())} if m else {}
    return dict(ms=ms, **split)


def build(pa, scenes, desc, builder):
    import torch
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


def cell(v):
    return f"{min(v):.2f} / {sorted(v)[len(v) // 2]:.2f} (+{max(v) - min(v):.2f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="c2", choices=["c2", "c4"])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    a = ap.parse_args()
    import copy
    import torch
    import pbrlab_amd as pa
    from pbrlab_amd import scenes
    if pa.device_count() < 1:
        raise SystemExit("no HIP device")
    pa.set_device(0)
    rgba = torch.empty((a.height, a.width, 4), dtype=torch.float32, device="cuda:0")
    count = torch.empty((a.height, a.width), dtype=torch.int32, device="cuda:0")
    out = (rgba.data_ptr(), count.data_ptr())
    line = {"scene": a.scene, "width": a.width, "height": a.height, "spp": a.spp, "rounds": a.rounds, "gpu": torch.cuda.get_device_name(0)}

    def quality(s):
        _, st = pa.Render(s, a.width, a.height, min(a.spp, 8), device_out=out, flags=pa.api.RENDER_STATS)
        _, tt = pa.Render(s, a.width, a.height, a.spp, device_out=out, flags=pa.api.RENDER_TIMING_TRACE)
        return st["closest_nodes"] / max(st["closest_rays"], 1), tt["ms_trace_closest"]

    if a.scene == "c4":
        desc = scenes.hair_scene(seed=1)
        hair = len(desc.shapes)
        s, _ = build(pa, scenes, desc, 2)                                 # warm-up: code objects, allocator
        s.UpdateInstanceTransform(0, None)
        s.RefitScene()
        del s
        s, commit_ms = build(pa, scenes, desc, 2)
        cv = desc.curves[0].vertices.copy()
        cv[:, 0] += (0.05 * np.sin(5.0 * cv[:, 1])).astype(np.float32)
        s.UpdateCurveMesh(hair, cv)
        r = timed_refit(s)
        v, t = quality(s)
        d1 = copy.deepcopy(desc)
        d1.curves[0].vertices = cv
        f, _ = build(pa, scenes, d1, 2)
        fv, ft = quality(f)
        print(f"c4 builder 2: commit {commit_ms:.1f} ms; refit with every strand swayed {r['ms']:.1f} ms = {r['ms'] / commit_ms:.2f} of it: {r}")
        print(f"c4 after the refit: {v:.2f} visits per ray, k_trace {t:.1f} ms; fresh commit at that pose: {fv:.2f}, {ft:.1f} ms; {s.wide_info()}")
        line.update(commit_ms=commit_ms, refit=r, visits=v, trace_ms=t, fresh_visits=fv, fresh_trace_ms=ft)
        print(json.dumps(line))
        return

    desc = scenes.cornell_scene("ggx", seed=1)
    names = [sh.name for sh in desc.shapes]
    monkey, lucy = names.index("monkey"), names.index("lucy")
    ids = np.unique(desc.shapes[monkey].vertex_ids)
    box = desc.vertices[ids, :3].max(axis=0) - desc.vertices[ids, :3].min(axis=0)

    def displaced(k):
        v = desc.vertices.copy()
        v[ids, 0] += np.float32(k * box[0])
        return v
    kinds = ("monkey mesh", "lucy transform", "every instance")
    res = {b: dict(commit=[], **{k: [] for k in kinds}) for b in (0, 2)}
    split = {b: {} for b in (0, 2)}
    for b in (0, 2):                                                      # warm-up
        s, _ = build(pa, scenes, desc, b)
        s.UpdateInstanceTransform(0, None)
        s.RefitScene()
        pa.Render(s, a.width, a.height, min(a.spp, 4), device_out=out)
        del s
    for r in range(a.rounds):
        for b in (0, 2):
            s, ms = build(pa, scenes, desc, b)
            res[b]["commit"].append(ms)
            v = desc.vertices.copy()
            v[ids, :3] *= np.float32(1.0 + 0.01 * (r + 1))
            s.UpdateTriangleMesh(monkey, v)
            one = timed_refit(s)
            s.UpdateInstanceTransform(lucy, scenes.instance_matrix((0.0, 10.0 * (r + 1), 0.0), (1.0, 1.0, 1.0), (0.02, 0.0, 0.0)))
            two = timed_refit(s)
            for i in range(len(names)):
                s.UpdateInstanceTransform(i, desc.shapes[i].transform if i != lucy else None)
            three = timed_refit(s)
            for k, x in zip(kinds, (one, two, three)):
                res[b][k].append(x["ms"])
                split[b].setdefault(k, []).append(x)
                print(f"round {r} builder {b}: commit {ms:.1f} ms; refit, {k}: {x}", flush=True)
            del s
    print(f"\nc2, best / median (spread) over {a.rounds} rounds, ms:")
    for b in (0, 2):
        c = min(res[b]["commit"])
        print(f"builder {b}: commit {cell(res[b]['commit'])}")
        line[f"builder{b}"] = dict(commit_ms=c, commit_spread=max(res[b]["commit"]) - c)
        for k in kinds:
            best = min(split[b][k][1:] or split[b][k], key=lambda x: x["ms"])   # (the first refit of a commit also builds the plan)
            part = max((p for p in ("host_ms", "upload_ms", "plan_ms", "trees_ms", "entries_ms") if p in best), key=lambda p: best[p], default=None)
            print(f"  refit, {k:<15} {cell(res[b][k])} = {min(res[b][k]) / c:.3f} of the commit; largest part: {part}; split of the best: {best}")
            line[f"builder{b}"][k] = dict(ms=min(res[b][k]), spread=max(res[b][k]) - min(res[b][k]), ratio=min(res[b][k]) / c, split=best, largest=part)
    # tree quality after growing displacements of the monkey
    line["quality"] = []
    for b in (0, 2):
        for k in (0.1, 0.5, 2.0):
            s, _ = build(pa, scenes, desc, b)
            s.UpdateTriangleMesh(monkey, displaced(k))
            s.RefitScene()
            v, t = quality(s)
            d1 = copy.deepcopy(desc)
            d1.vertices = displaced(k)
            f, _ = build(pa, scenes, d1, b)
            fv, ft = quality(f)
            print(f"builder {b}, monkey displaced by {k} box sizes: refit {v:.2f} visits per ray, k_trace {t:.2f} ms; fresh commit {fv:.2f}, {ft:.2f} ms", flush=True)
            line["quality"].append(dict(builder=b, displacement=k, visits=v, trace_ms=t, fresh_visits=fv, fresh_trace_ms=ft))
            del s, f
    print(json.dumps(line))


if __name__ == "__main__":
    main()
