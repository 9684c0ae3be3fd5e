"""bench_sdf.py -- rates of the signed-distance queries on bench.py's C2 scene (the Lambert + GGX Cornell box).

Signed queries: --grid cubed points on a regular grid through the scene's box, no bound (bench_queries.py's nearest-point set); M queries/s
of pbrhip_signed_distance_device with all three outputs and with sd alone, beside pbrhip_nearest_point_device on the same points in the
same process.  The table: the time pbrhip_scene_signed_distance_info reports for the topology lists (host, once per commit) and for the
table's two launches, the latter again after a refit, beside the time of that pbrhip_scene_refit (one mesh's vertices edited on the host).
The grid: pbrhip_signed_distance_grid_device over the same box at --grid cubed.
Method: the median ms per call after --warmup untimed calls over --reps timed ones, a device synchronisation on both sides.  One JSON line.

    python scripts/bench_sdf.py [--grid 128]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=128)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    import torch
    import pbrlab_amd as pa
    from pbrlab_amd import scenes
    pa.set_device(0)

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

    desc = scenes.cornell_scene("ggx", seed=1)
    t0 = time.perf_counter()
    s = pa.scene_from_desc(desc)
    res = {"scene": "c2", "commit_s": round(time.perf_counter() - t0, 2), "slots": int(s.info()["num_slots"])}
    lo, hi = s.FetchSceneAABB()
    lo, hi = np.asarray(lo, np.float32), np.asarray(hi, np.float32)

    # ---- the table
    info = s.SignedDistanceInfo()
    res["table"] = {k: (round(v, 3) if isinstance(v, float) else int(v)) for k, v in info.items()}
    moved = desc.vertices.copy()
    moved[:, 1] += np.float32(0.001)
    mesh = len(desc.shapes) - 1  # the small box
    s.UpdateTriangleMesh(mesh, moved)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    s.RefitScene()
    res["refit_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
    res["table_ms_after_refit"] = round(s.SignedDistanceInfo()["table_ms"], 3)

    # ---- signed queries beside the unsigned ones
    g = a.grid
    ax = [np.linspace(lo[k], hi[k], g, dtype=np.float32) for k in range(3)]
    pts = np.stack(np.meshgrid(*ax, indexing="ij"), axis=-1).reshape(-1, 3)
    pts = np.ascontiguousarray(np.concatenate([pts, np.full((len(pts), 1), np.inf, np.float32)], axis=1), np.float32)
    n = len(pts)
    d = torch.from_numpy(pts).to("cuda:0")
    ident = torch.zeros((n, 4), dtype=torch.int32, device="cuda:0")
    closest, sd = (torch.zeros((n, 4), dtype=torch.float32, device="cuda:0") for _ in range(2))
    ms_u = median_ms(lambda: s.NearestPointDevice(d, ident, closest))
    ms_s = median_ms(lambda: s.SignedDistanceDevice(d, ident, closest, sd))
    ms_o = median_ms(lambda: s.SignedDistanceDevice(d, sd=sd))
    ms_u2 = median_ms(lambda: s.NearestPointDevice(d, ident, closest))
    res["queries"] = {"n": n, "grid": g, "nearest_ms": round(ms_u, 3), "nearest_mqueries_per_s": round(n / ms_u / 1e3, 1), "nearest_again_ms": round(ms_u2, 3),
                      "signed_ms": round(ms_s, 3), "signed_mqueries_per_s": round(n / ms_s / 1e3, 1), "signed_sd_only_ms": round(ms_o, 3),
                      "signed_sd_only_mqueries_per_s": round(n / ms_o / 1e3, 1), "signed_over_nearest": round(ms_u / ms_s, 3),
                      "inside_fraction": round(float((sd[:, 3] < 0).float().mean()), 4)}

    # ---- the grid
    spacing = (hi - lo) / np.float32(g - 1)
    out = torch.zeros((g, g, g), dtype=torch.float32, device="cuda:0")
    ms_g = median_ms(lambda: s.SignedDistanceGridDevice(lo, spacing, (g, g, g), out=out))
    res["grid"] = {"dims": [g, g, g], "ms": round(ms_g, 3), "mpoints_per_s": round(n / ms_g / 1e3, 1)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
