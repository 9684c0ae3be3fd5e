"""bench_queries.py -- rates of the ray and nearest-point queries on bench.py's C2 scene (the Lambert + GGX Cornell box).

Rays: the camera rays of one pass of a --width x --height frame (coherent) and as many random rays through the scene's box (incoherent),
held in device memory; M rays/s of pbrhip_trace_closest_device (both outputs) and pbrhip_trace_any_device, beside the render's own rate on
the same scene: the rays k_trace traced in a --spp frame (closest_rays + shadow_rays of a PBRHIP_RENDER_STATS render) over the time of its
launches (ms_trace_closest of a PBRHIP_RENDER_TIMING_TRACE render of the same frame; the statistics build is slower, so the two come from
two renders), and closest_rays alone over the same time for the record.  Nearest point: --grid cubed points on a regular grid through the
scene's box, no bound; M queries/s of the device variant and of the host variant (upload, download and allocation included) beside it.
Method: the median ms per call after --warmup untimed calls over --reps timed ones, a device synchronisation on both sides.  One JSON line.

    python scripts/bench_queries.py [--grid 128] [--spp 8]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=8)
    ap.add_argument("--grid", type=int, default=128)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    import torch
    import pbrlab_amd as pa
    from pbrlab_amd import api, scenes
    pa.set_device(0)
    W, H = a.width, a.height

    def median_ms(f, reps=a.reps):
        for _ in range(a.warmup):
            f()
        ts = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(ts))

    t0 = time.perf_counter()
    s = pa.scene_from_desc(scenes.cornell_scene("ggx", seed=1))
    res = {"scene": "c2", "commit_s": round(time.perf_counter() - t0, 2), "slots": int(s.info()["num_slots"])}
    lo, hi = s.FetchSceneAABB()

    # ---- the render's own rate
    layer = pa.RenderLayer()
    _, st = pa.Render(s, W, H, a.spp, layer=layer, flags=api.RENDER_STATS)
    pa.Render(s, W, H, a.spp, layer=layer, flags=api.RENDER_TIMING_TRACE)
    _, tm = pa.Render(s, W, H, a.spp, layer=layer, flags=api.RENDER_TIMING_TRACE)
    traced = st["closest_rays"] + st["shadow_rays"]
    res["render"] = {"spp": a.spp, "closest_rays": int(st["closest_rays"]), "shadow_rays": int(st["shadow_rays"]), "ms_trace": round(tm["ms_trace_closest"], 3),
                     "mrays_per_s_closest_plus_shadow": round(traced / tm["ms_trace_closest"] / 1e3, 1),
                     "mrays_per_s_closest_only": round(st["closest_rays"] / tm["ms_trace_closest"] / 1e3, 1)}

    # ---- ray queries
    n = W * H
    xy = np.stack(np.meshgrid(np.arange(W, dtype=np.uint32), np.arange(H, dtype=np.uint32)), axis=-1).reshape(-1, 2)
    cam = s.CameraRays(W, H, np.concatenate([xy, np.zeros((n, 1), np.uint32)], axis=1))
    rnd = scenes.random_rays((lo, hi), n, seed=1)
    for name, rays in (("camera", cam), ("random", rnd)):
        d = torch.from_numpy(np.ascontiguousarray(rays).view(np.float32).reshape(-1, 8).copy()).to("cuda:0")
        ident = torch.zeros((n, 4), dtype=torch.int32, device="cuda:0")
        hits = torch.zeros((n, 9), dtype=torch.int32, device="cuda:0")
        occ = torch.zeros((n,), dtype=torch.uint8, device="cuda:0")
        ms_c = median_ms(lambda: s.TraceClosestDevice(d, ident, hits))
        ms_i = median_ms(lambda: s.TraceClosestDevice(d, ident=ident))
        ms_a = median_ms(lambda: s.TraceAnyDevice(d, occ))
        t0 = time.perf_counter()
        s.trace_closest(rays)
        ms_h = (time.perf_counter() - t0) * 1e3
        res["rays_" + name] = {"n": n, "hit_fraction": round(float((ident[:, 0] != -1).float().mean()), 3), "closest_ms": round(ms_c, 3), "closest_mrays_per_s": round(n / ms_c / 1e3, 1),
                               "closest_ident_only_mrays_per_s": round(n / ms_i / 1e3, 1), "any_ms": round(ms_a, 3), "any_mrays_per_s": round(n / ms_a / 1e3, 1),
                               "host_hook_closest_mrays_per_s": round(n / ms_h / 1e3, 1)}

    # ---- nearest point
    g = a.grid
    ax = [np.linspace(lo[k], hi[k], g, dtype=np.float32) for k in range(3)]
    pts = np.stack(np.meshgrid(*ax, indexing="ij"), axis=-1).reshape(-1, 3)
    pts = np.ascontiguousarray(np.concatenate([pts, np.full((len(pts), 1), np.inf, np.float32)], axis=1), np.float32)
    d = torch.from_numpy(pts).to("cuda:0")
    ident = torch.zeros((len(pts), 4), dtype=torch.int32, device="cuda:0")
    closest = torch.zeros((len(pts), 4), dtype=torch.float32, device="cuda:0")
    ms_d = median_ms(lambda: s.NearestPointDevice(d, ident, closest))
    ms_h = median_ms(lambda: s.NearestPoint(pts), reps=3)
    res["nearest"] = {"n": len(pts), "grid": g, "device_ms": round(ms_d, 3), "device_mqueries_per_s": round(len(pts) / ms_d / 1e3, 1), "host_ms": round(ms_h, 3),
                      "host_mqueries_per_s": round(len(pts) / ms_h / 1e3, 1), "mean_distance": round(float(closest[:, 3].sqrt().mean()), 4)}
    before = os.environ.get("PBRHIP_WIDE")
    os.environ["PBRHIP_WIDE"] = "0"  # the binary tree
    ms_b = median_ms(lambda: s.NearestPointDevice(d, ident, closest), reps=3)
    if before is None:
        del os.environ["PBRHIP_WIDE"]
    else:
        os.environ["PBRHIP_WIDE"] = before
    res["nearest"]["binary_tree_mqueries_per_s"] = round(len(pts) / ms_b / 1e3, 1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
