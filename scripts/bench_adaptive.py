"""bench_adaptive.py -- what adaptive sampling buys and costs: C2's geometry (the Lambert + GGX Cornell box) at 1920x1080
on device buffers (torch tensors), best of --reps each, every call ending in the library's stream synchronise.  Beside each other:

  uniform     Render at --spp (64): time, and relative MSE against a reference of --ref-spp (1024) passes of its own
  adaptive    RenderAdaptive over a threshold sweep at maximum --spp and at maximum 4 x --spp: samples, rounds, time, relative MSE
  threshold 0 the whole schedule with no tile ever stopping: its time over the uniform frame's is what the rounds and decisions cost

relative MSE = mean over pixels and channels of (x - ref)^2 / (ref^2 + 0.01), x = rgb / count.  One JSON line.
`--profile-run` renders one adaptive frame and exits: run it under `rocprofv3 --kernel-trace --stats` for the time of the decision
kernels (k_as_*) alone.

    python scripts/bench_adaptive.py [--reps 5] [--spp 64] [--thresholds 0.01,0.02,...]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--ref-spp", type=int, default=1024)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--first-level", type=int, default=0)
    ap.add_argument("--thresholds", default="0.005,0.01,0.02,0.03,0.05,0.08,0.12,0.2")
    ap.add_argument("--profile-run", action="store_true")
    a = ap.parse_args()
    import torch
    import pbrlab_amd as pa
    from pbrlab_amd import api, scenes
    if pa.device_count() < 1:
        raise SystemExit("bench_adaptive.py needs an MI355X: no HIP device visible")
    pa.set_device(0)
    s = pa.scene_from_desc(scenes.cornell_scene("ggx", seed=1))
    W, H = a.width, a.height
    dev = "cuda:0"
    rgba = torch.zeros((H, W, 4), dtype=torch.float32, device=dev)
    count = torch.zeros((H, W), dtype=torch.int32, device=dev)
    terr = torch.zeros((-(-H // 8), -(-W // 8)), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    out = (rgba.data_ptr(), count.data_ptr(), terr.data_ptr())

    def adaptive(max_spp, thr):
        return api.RenderAdaptive(s, W, H, max_spp, threshold=thr, first_level=a.first_level, device_out=out)

    if a.profile_run:
        print(json.dumps(dict(zip(("samples", "rounds"), adaptive(a.spp, api.ADAPTIVE_THRESHOLD)))))
        return

    def mean_image():
        return (rgba[..., :3].double() / count.clamp(min=1)[..., None].double()).clone()

    pa.Render(s, W, H, a.ref_spp, device_out=out[:2], first_pass=1 << 20)  # passes no frame below draws from
    ref = mean_image()

    def rel_mse():
        return float((((mean_image() - ref) ** 2) / (ref ** 2 + 1e-2)).mean())

    def best_of(f):
        best, ret = float("inf"), None
        for rep in range(a.reps + 1):  # the first call warms up
            t0 = time.perf_counter()
            ret = f()  # (every entry point returns after its stream is idle)
            dt = time.perf_counter() - t0
            if rep:
                best = min(best, dt)
        return best * 1e3, ret

    npix = W * H
    res = {"scene": "C2 geometry", "width": W, "height": H, "reps": a.reps, "ref_spp": a.ref_spp, "first_level": a.first_level or api.ADAPTIVE_FIRST_LEVEL,
           "default_threshold": api.ADAPTIVE_THRESHOLD}
    for spp in (a.spp, 4 * a.spp):
        ms, _ = best_of(lambda: pa.Render(s, W, H, spp, device_out=out[:2]))
        res[f"uniform_{spp}"] = {"ms": round(ms, 2), "rel_mse": rel_mse(), "samples_per_pixel": spp}
    for max_spp in (a.spp, 4 * a.spp):
        rows = []
        for thr in [0.0] + [float(t) for t in a.thresholds.split(",")]:
            ms, (samples, rounds) = best_of(lambda: adaptive(max_spp, thr))
            rows.append({"threshold": thr, "samples_per_pixel": round(samples / npix, 3), "rounds": rounds, "ms": round(ms, 2), "rel_mse": rel_mse(),
                         "ms_over_uniform_max": round(ms / res[f"uniform_{max_spp}"]["ms"], 4)})
        res[f"adaptive_max_{max_spp}"] = rows
    print(json.dumps(res))


if __name__ == "__main__":
    main()
