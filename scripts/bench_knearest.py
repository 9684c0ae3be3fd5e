"""bench_knearest.py -- rates of the k-nearest queries on bench.py's C2 scene (the Lambert + GGX Cornell box).

Points as scripts/bench_queries.py's nearest-point sets: --n points near the surface (a uniform point of a uniform slot, moved by up to
1 % of the box's diagonal) and as many uniform in the scene's box, held in device memory.  M queries/s of pbrhip_k_nearest_device for
  the list only, K = 1, 8 and 32, without a bound, beside pbrhip_nearest_point_device (ident only) on the same points;
  the count alone and the count with K = 8 at the radius at which a point of the set has about 8 primitives in reach (found by
    bisection on the mean count of the first 65 536 points);
  K = 8 without a bound with the closest rows beside the ident rows: what they cost.
Method: the median ms per call after --warmup untimed calls over --reps timed ones, a device synchronisation on both sides.  One JSON line.

    python scripts/bench_knearest.py [--n 1048576]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    import torch
    import pbrlab_amd as pa
    from pbrlab_amd import scenes
    pa.set_device(0)
    n = a.n
    F = np.float32

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
    diag = float(np.linalg.norm(hi - lo))
    slots, shade = s.read_slots()
    rng = np.random.RandomState(1)
    k = rng.randint(len(slots), size=n)
    b = rng.rand(n, 2).astype(F)
    flip = b.sum(axis=1) > 1
    b[flip] = 1 - b[flip]
    v0, v1, v2 = slots[k, 0, :3], slots[k, 1, :3], slots[k, 2, :3]
    near = v0 + b[:, :1] * (v1 - v0) + b[:, 1:] * (v2 - v0) + ((rng.rand(n, 3) * 2 - 1) * 0.01 * diag).astype(F)
    box = lo + rng.rand(n, 3).astype(F) * (hi - lo)
    rate = lambda ms: round(n / ms / 1e3, 1)
    for name, p in (("surface", near), ("box", box)):
        pts = np.concatenate([p.astype(F), np.full((n, 1), np.inf, F)], axis=1)
        d = torch.from_numpy(np.ascontiguousarray(pts)).to("cuda:0")
        one = torch.zeros((n, 4), dtype=torch.int32, device="cuda:0")
        count = torch.zeros((n,), dtype=torch.int32, device="cuda:0")
        out = {"n": n}
        ms = median_ms(lambda: s.NearestPointDevice(d, ident=one))
        out["nearest_ident_only"] = {"ms": round(ms, 3), "mqueries_per_s": rate(ms)}
        for K in (1, 8, 32):
            rows = torch.zeros((n, K, 4), dtype=torch.int32, device="cuda:0")
            ms = median_ms(lambda: s.KNearestDevice(d, K, count=False, ident=rows))
            out[f"list_k{K}"] = {"ms": round(ms, 3), "mqueries_per_s": rate(ms)}
        out["k1_over_nearest"] = round(out["list_k1"]["mqueries_per_s"] / out["nearest_ident_only"]["mqueries_per_s"], 3)
        rows = torch.zeros((n, 8, 4), dtype=torch.int32, device="cuda:0")
        cl = torch.zeros((n, 8, 4), dtype=torch.float32, device="cuda:0")
        ms = median_ms(lambda: s.KNearestDevice(d, 8, count=False, ident=rows, closest=cl))
        out["list_k8_with_closest"] = {"ms": round(ms, 3), "mqueries_per_s": rate(ms), "over_list_k8": round(ms / out["list_k8"]["ms"], 3)}
        # the radius that holds about 8 primitives: bisection on the mean count of a sample
        m = min(n, 1 << 16)
        sample = d[:m].clone()
        r_lo, r_hi = 0.0, diag
        for _ in range(20):
            r = 0.5 * (r_lo + r_hi)
            sample[:, 3] = r
            c = s.KNearestDevice(sample, 0)[0]
            if float(c.float().mean()) > 8.0:
                r_hi = r
            else:
                r_lo = r
        r = 0.5 * (r_lo + r_hi)
        dr = d.clone()
        dr[:, 3] = r
        ms = median_ms(lambda: s.KNearestDevice(dr, 0, count=count))
        out["count_only_at_radius"] = {"ms": round(ms, 3), "mqueries_per_s": rate(ms)}
        ms = median_ms(lambda: s.KNearestDevice(dr, 8, count=count, ident=rows))
        out["count_and_k8_at_radius"] = {"ms": round(ms, 3), "mqueries_per_s": rate(ms)}
        ms = median_ms(lambda: s.KNearestDevice(dr, 8, count=False, ident=rows))
        out["list_k8_at_radius"] = {"ms": round(ms, 3), "mqueries_per_s": rate(ms)}
        c = count.to(torch.int64)
        out["radius"] = {"r": round(r, 5), "over_diagonal": round(r / diag, 5), "mean_count": round(float(c.float().mean()), 3), "max_count": int(c.max()),
                         "none": round(float((c == 0).float().mean()), 3), "more_than_8": round(float((c > 8).float().mean()), 4)}
        res["points_" + name] = out
    print(json.dumps(res))


if __name__ == "__main__":
    main()
