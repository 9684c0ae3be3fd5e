"""bench_allhits.py -- rates of the all-hits ray queries on bench.py's C2 scene (the Lambert + GGX Cornell box).

Rays as scripts/bench_queries.py's: the camera rays of one pass of a --width x --height frame (coherent) and as many random rays through
the scene's box (incoherent), held in device memory.  M rays/s of pbrhip_trace_all_device for
  K = 1 without count, beside pbrhip_trace_closest_device (ident only) on the same rays;
  K = 4 and K = 8 without count, beside peeling: K calls of pbrhip_trace_closest_device with tmin advanced to the last t on the device
    (a torch.where between the calls; a ray that has missed keeps its interval and is traced again, as a caller without a compaction
    step would);
  the count alone (max_hits = 0), and K = 8 with count.
Method: the median ms per call after --warmup untimed calls over --reps timed ones, a device synchronisation on both sides.  One JSON line.

    python scripts/bench_allhits.py [--width 1920] [--height 1080]"""
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
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    import torch
    import pbrlab_amd as pa
    from pbrlab_amd import scenes
    pa.set_device(0)
    W, H = a.width, a.height

    def median_ms(f):
        for _ in range(a.warmup):
            f()
        ts = []
        for _ in range(a.reps):
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
    n = W * H
    xy = np.stack(np.meshgrid(np.arange(W, dtype=np.uint32), np.arange(H, dtype=np.uint32)), axis=-1).reshape(-1, 2)
    cam = s.CameraRays(W, H, np.concatenate([xy, np.zeros((n, 1), np.uint32)], axis=1))
    rnd = scenes.random_rays((lo, hi), n, seed=1)
    rate = lambda ms: round(n / ms / 1e3, 1)
    for name, rays in (("camera", cam), ("random", rnd)):
        d = torch.from_numpy(np.ascontiguousarray(rays).view(np.float32).reshape(-1, 8).copy()).to("cuda:0")
        one = torch.zeros((n, 4), dtype=torch.int32, device="cuda:0")
        count = torch.zeros((n,), dtype=torch.int32, device="cuda:0")
        work = d.clone()

        def peel(k):
            work.copy_(d)
            for j in range(k):
                s.TraceClosestDevice(work, ident=one)
                if j + 1 < k:
                    work[:, 3] = torch.where(one[:, 0] != -1, one[:, 3].contiguous().view(torch.float32), work[:, 3])

        out = {"n": n}
        ms = median_ms(lambda: s.TraceClosestDevice(d, ident=one))
        out["closest_ident_only"] = {"ms": round(ms, 3), "mrays_per_s": rate(ms)}
        for k in (1, 4, 8):
            rows = torch.zeros((n, k, 4), dtype=torch.int32, device="cuda:0")
            ms = median_ms(lambda: s.TraceAllDevice(d, k, count=False, ident=rows))
            out[f"all_k{k}"] = {"ms": round(ms, 3), "mrays_per_s": rate(ms)}
            if k > 1:
                ms_p = median_ms(lambda: peel(k))
                out[f"peel_k{k}"] = {"ms": round(ms_p, 3), "mrays_per_s": rate(ms_p), "all_hits_speedup": round(ms_p / ms, 2)}
        ms = median_ms(lambda: s.TraceAllDevice(d, 8, count=count, ident=rows))
        out["all_k8_with_count"] = {"ms": round(ms, 3), "mrays_per_s": rate(ms)}
        ms = median_ms(lambda: s.TraceAllDevice(d, 0, count=count))
        out["count_only"] = {"ms": round(ms, 3), "mrays_per_s": rate(ms)}
        c = count.to(torch.int64)
        out["hits_per_ray"] = {"mean": round(float(c.float().mean()), 3), "max": int(c.max()), "none": round(float((c == 0).float().mean()), 3),
                               "more_than_8": round(float((c > 8).float().mean()), 4)}
        out["k1_over_closest"] = round(out["all_k1"]["mrays_per_s"] / out["closest_ident_only"]["mrays_per_s"], 3)
        res["rays_" + name] = out
    print(json.dumps(res))


if __name__ == "__main__":
    main()
