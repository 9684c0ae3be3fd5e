"""bench_features.py -- what the first-hit features and the denoiser cost: C2's geometry (the Lambert + GGX Cornell box) at
1920x1080, in one process and alternating, best of --reps each: Render at --spp alone (the yardstick), RenderFeatures for --spp and for
16 passes, Denoise with 5 iterations.  Features and filter are timed on device buffers (torch tensors), as a renderer that keeps its
layer on the GPU would call them; one JSON line with ms and the share of the frame.

    python scripts/bench_features.py [--reps 5] [--spp 64]"""
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
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    a = ap.parse_args()
    import torch
    import pbrlab_amd as pa
    from pbrlab_amd import scenes
    pa.set_device(0)
    s = pa.scene_from_desc(scenes.cornell_scene("ggx", seed=1))
    W, H = a.width, a.height
    dev = "cuda:0"
    rgba = torch.zeros((H, W, 4), dtype=torch.float32, device=dev)
    count = torch.zeros((H, W), dtype=torch.int32, device=dev)
    alb, nd, out = torch.zeros_like(rgba), torch.zeros_like(rgba), torch.zeros_like(rgba)
    fcount = torch.zeros_like(count)
    torch.cuda.synchronize()

    def render():
        pa.Render(s, W, H, a.spp, device_out=(rgba.data_ptr(), count.data_ptr()))

    def features(n):
        return lambda: pa.RenderFeatures(s, W, H, n, device_out=(alb.data_ptr(), nd.data_ptr(), fcount.data_ptr()))

    def denoise():
        pa.DenoiseDevice(0, W, H, rgba.data_ptr(), count.data_ptr(), out.data_ptr(), (alb.data_ptr(), nd.data_ptr(), fcount.data_ptr()), iterations=5)

    jobs = {"render": render, f"features_{a.spp}": features(a.spp), "features_16": features(16), "denoise_5": denoise}
    best = {k: float("inf") for k in jobs}
    for rep in range(a.reps + 1):  # the first round warms up
        for k, f in jobs.items():
            t0 = time.perf_counter()
            f()  # (every entry point returns after its stream is idle)
            dt = time.perf_counter() - t0
            if rep:
                best[k] = min(best[k], dt)
    res = {"scene": "C2 geometry", "width": W, "height": H, "spp": a.spp, "reps": a.reps}
    for k, t in best.items():
        res[k] = {"ms": round(t * 1e3, 2), "share_of_frame": round(t / best["render"], 4)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
