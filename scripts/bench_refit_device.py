#!/usr/bin/env python3
"""The device-path refit (mesh updates from device memory, staging on the GPU: DESIGN.md section 8, "Staging on the device") against the
host-path refit of the same process, one GPU (bench.py stays the flagship's yardstick; scripts/bench_refit.py measures the host path alone).

    python scripts/bench_refit_device.py [--scene c2|c4] [--builders 0,2] [--rounds 3]

Per builder two scenes are committed from the same description: H is edited through the host calls, D through the *_device calls with
torch tensors that are already on the GPU.  Per round the same edits go to both, H first, then D (so the two paths alternate):
c2 -- only the monkey's vertices, Lucy's vertices replaced (524 288 slots), every instance dirty through its transform; c4 -- every strand
swayed.  Every figure is the caller's wall clock in ms: the update calls (host: a copy into the model; device: check, download to the
model and, on the first call after a commit, the switch-on, which the library's PBRHIP_DEBUG=1 line reports on its own) and the refit,
with the library's split of it.  Prints every figure as it comes, a summary and one JSON line."""
import argparse
import json
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bench_refit as BR  # noqa: E402

DSPLIT = re.compile(r"refit \(device geometry\): (\d+) of (\d+) slots dirty: switch-on ([\d.]+) ms, updates' check \+ download to the model ([\d.]+) ms, "
                    r"staging \+ bounds kernels ([\d.]+) ms, light tables ([\d.]+) ms, plan ([\d.]+) ms, pack \+ trees ([\d.]+) ms \((\d+) \+ (\d+) levels\), "
                    r"Q-node download \+ walk entries ([\d.]+) ms")
DKEYS = ("dirty", "slots", "switch_on_ms", "download_ms", "stage_ms", "lights_ms", "plan_ms", "trees_ms", "bin_levels", "q_levels", "entries_ms")


def timed(f):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    f()
    return (time.perf_counter() - t0) * 1e3


def refit(s):
    """-> the refit's wall clock and the library's split of it, whichever path it took"""
    os.environ["PBRHIP_DEBUG"] = "1"
    try:
        with BR.Stderr() as err:
            ms = timed(s.RefitScene)
    finally:
        os.environ.pop("PBRHIP_DEBUG", None)
    m, h = DSPLIT.search(err.text), BR.SPLIT.search(err.text)
    if m:
        return dict(refit_ms=ms, **{k: (float(v) if "ms" in k else int(v)) for k, v in zip(DKEYS, m.groups())})
    keys = ("dirty", "slots", "host_ms", "upload_ms", "plan_ms", "trees_ms", "bin_levels", "q_levels", "entries_ms")
    return dict(refit_ms=ms, **({k: (float(v) if "ms" in k else int(v)) for k, v in zip(keys, h.groups())} if h else {}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="c2", choices=["c2", "c4"])
    ap.add_argument("--builders", default="0,2")
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    import torch
    import pbrlab_amd as pa
    from pbrlab_amd import scenes
    if pa.device_count() < 1:
        raise SystemExit("no HIP device")
    pa.set_device(0)
    builders = [int(b) for b in a.builders.split(",")]
    line = {"scene": a.scene, "rounds": a.rounds, "gpu": torch.cuda.get_device_name(0)}

    def dev(x):
        t = torch.from_numpy(np.ascontiguousarray(x, np.float32)).to("cuda:0")
        torch.cuda.synchronize()
        return t

    if a.scene == "c2":
        desc = scenes.cornell_scene("ggx", seed=1)
        names = [sh.name for sh in desc.shapes]
        monkey, lucy = names.index("monkey"), names.index("lucy")
        ids = {k: np.unique(desc.shapes[i].vertex_ids) for k, i in (("monkey", monkey), ("lucy", lucy))}

        def edits(r):
            vm, vl = desc.vertices.copy(), desc.vertices.copy()
            vm[ids["monkey"], :3] *= np.float32(1.0 + 0.01 * (r + 1))
            vl[ids["lucy"], :3] *= np.float32(1.0 + 0.001 * (r + 1))
            xf = [scenes.instance_matrix((0.0, 1.0 * (r + 1), 0.0), (1.0, 1.0, 1.0), (0.0, 0.001 * (r + 1), 0.0)) for _ in names]
            return [("monkey's vertices", [("tri", monkey, vm)]), ("Lucy's vertices", [("tri", lucy, vl)]),
                    ("every instance", [("xf", i, xf[i]) for i in range(len(names))])]
    else:
        desc = scenes.hair_scene(seed=1)
        hair = len(desc.shapes)

        def edits(r):
            cv = desc.curves[0].vertices.copy()
            cv[:, 0] += (0.05 * (r + 1) * np.sin(5.0 * cv[:, 1])).astype(np.float32)
            return [("every strand swayed", [("curve", hair, cv)])]

    def apply(s, ops, device):
        for kind, i, x in ops:
            if kind == "xf":
                s.UpdateInstanceTransform(i, x)
            elif kind == "tri":
                s.UpdateTriangleMeshDevice(i, x) if device else s.UpdateTriangleMesh(i, x)
            else:
                s.UpdateCurveMeshDevice(i, x) if device else s.UpdateCurveMesh(i, x)

    w, _ = BR.build(pa, scenes, desc, builders[-1])                       # warm-up: code objects, allocator, both paths
    for device in (False, True):
        ops = edits(0)[0][1]
        apply(w, [(k, i, dev(x) if device and k != "xf" else x) for k, i, x in ops], device)
        w.RefitScene()
    del w
    res = {}
    for b in builders:
        H, commit_h = BR.build(pa, scenes, desc, b)
        D, commit_d = BR.build(pa, scenes, desc, b)
        res[b] = dict(commit_ms=[commit_h, commit_d], cases={})
        print(f"builder {b}: commit {commit_h:.1f} / {commit_d:.1f} ms", flush=True)
        for r in range(a.rounds):
            for case, ops in edits(r):
                dops = [(k, i, dev(x) if k != "xf" else x) for k, i, x in ops]     # (the simulation's arrays: on the GPU already)
                up_h = timed(lambda: apply(H, ops, False))
                rh = refit(H)
                up_d = timed(lambda: apply(D, dops, True))
                rd = refit(D)
                res[b]["cases"].setdefault(case, []).append(dict(host=dict(update_ms=up_h, **rh), device=dict(update_ms=up_d, **rd)))
                print(f"round {r} builder {b}, {case}: host path update {up_h:.2f} + refit {rh['refit_ms']:.2f} ms {rh}; "
                      f"device path update {up_d:.2f} + refit {rd['refit_ms']:.2f} ms {rd}", flush=True)
        lo_h, hi_h = H.FetchSceneAABB()
        lo_d, hi_d = D.FetchSceneAABB()
        same = H.read_slots()[0].tobytes() == D.read_slots()[0].tobytes() and H.read_slots()[1].tobytes() == D.read_slots()[1].tobytes()
        print(f"builder {b}: after the last round both scenes hold the same slots and ShadeRecs: {same}; boxes equal: {bool((lo_h == lo_d).all() and (hi_h == hi_d).all())}")
        res[b]["same_bytes"] = bool(same)
        del H, D
    print(f"\n{a.scene}: update + refit, ms, rounds in order (host path | device path); the first device update of a commit includes the switch-on")
    for b in builders:
        print(f"builder {b}: commit {min(res[b]['commit_ms']):.1f} ms")
        for case, rows in res[b]["cases"].items():
            h = [x["host"]["update_ms"] + x["host"]["refit_ms"] for x in rows]
            d = [x["device"]["update_ms"] + x["device"]["refit_ms"] for x in rows]
            rh, rd = [x["host"]["refit_ms"] for x in rows], [x["device"]["refit_ms"] for x in rows]
            fmt = lambda v: " / ".join(f"{q:.2f}" for q in v)  # noqa: E731
            print(f"  {case:<20} host {fmt(h)} (spread {max(h) - min(h):.2f}) | device {fmt(d)} | refit alone: host {fmt(rh)} | device {fmt(rd)}")
    line["builders"] = {str(b): res[b] for b in builders}
    print(json.dumps(line))


if __name__ == "__main__":
    main()
