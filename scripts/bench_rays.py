"""bench_rays.py -- what rendering along a ray list costs: C2's geometry at 1920x1080 x 64 spp through an oblique pinhole,
on device buffers (torch tensors), best of --reps each after a warm-up call, every call ending in the library's stream synchronise.

  --mode render   Render with the pinhole set on the scene (k_generate_camera): the frame a build without ray lists makes too
  --mode rays     the same frame through RenderRays with the pinhole's own per-pass rays (Scene.CameraRays, filled into device memory
                  before anything is timed): in one call, and in chunks of --chunk passes (first_pass + RENDER_NO_CLEAR, what
                  RenderProjection does, here without the projection kernel); checks that both equal Render's frame bit for bit
  --mode project  RenderProjection("latlong"): the chunked loop with k_project_rays in it

--root DIR imports pbrlab_amd from DIR instead of this checkout (an A/B against another build's --mode render).  One JSON line.

    python scripts/bench_rays.py --mode rays [--reps 5] [--chunk 4]"""
import argparse
import json
import os
import sys
import time


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("render", "rays", "project"), default="rays")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--chunk", type=int, default=4)  # 4 passes of 1080p rays = 253 MiB: RenderProjection's chunk under its 256 MiB cap
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    a = ap.parse_args()
    sys.path.insert(0, a.root)
    import numpy as np
    import torch
    import pbrlab_amd as pa
    from pbrlab_amd import api, scenes
    if pa.device_count() < 1:
        raise SystemExit("bench_rays.py needs an MI355X: no HIP device visible")
    pa.set_device(0)
    s = pa.scene_from_desc(scenes.cornell_scene("ggx", seed=1))
    W, H, spp = a.width, a.height, a.spp
    lo, hi = (np.array(v, np.float64) for v in s.FetchSceneAABB())
    c, e = 0.5 * (lo + hi), hi - lo
    s.SetCamera(c + np.array([0.1, 0.05, 1.6]) * e, c, (0.0, 1.0, 0.0), 40.0)  # in front of the box, slightly off its axis
    dev = "cuda:0"
    rgba = torch.zeros((H, W, 4), dtype=torch.float32, device=dev)
    count = torch.zeros((H, W), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    out = (rgba.data_ptr(), count.data_ptr())

    def best_of(f):
        best = float("inf")
        for rep in range(a.reps + 1):  # the first call warms up
            t0 = time.perf_counter()
            f()  # (every entry point returns after its stream is idle)
            dt = time.perf_counter() - t0
            if rep:
                best = min(best, dt)
        return round(best * 1e3, 2)

    res = {"mode": a.mode, "root": a.root, "scene": "C2 geometry, oblique pinhole", "width": W, "height": H, "spp": spp, "reps": a.reps}
    if a.mode == "render":
        res["render_ms"] = best_of(lambda: pa.Render(s, W, H, spp, device_out=out))
    elif a.mode == "project":
        layer = pa.RenderLayer()
        res["project_latlong_ms_host_layer"] = best_of(lambda: pa.RenderProjection(s, "latlong", W, H, spp, layer))
        res["ray_buffer_bytes"] = api.RAY_BUFFER_BYTES
    else:
        pa.Render(s, W, H, spp, device_out=out)
        want = (rgba.clone(), count.clone())
        rays = torch.zeros((spp, H, W, 8), dtype=torch.float32, device=dev)
        yy, xx = np.mgrid[0:H, 0:W]
        for p in range(spp):  # the pinhole's own ray of every (pixel, pass), one pass at a time through the host hook
            xyp = np.stack([xx, yy, np.full_like(xx, p)], -1).reshape(-1, 3)
            rays[p] = torch.from_numpy(s.CameraRays(W, H, xyp).view(np.float32).reshape(H, W, 8)).to(dev)
        torch.cuda.synchronize()
        res["render_ms"] = best_of(lambda: pa.Render(s, W, H, spp, device_out=out))
        res["rays_one_call_ms"] = best_of(lambda: pa.RenderRays(s, rays, spp, device_out=out))
        res["rays_one_call_equal"] = bool(torch.equal(rgba, want[0]) and torch.equal(count, want[1]))

        def chunked():
            for p in range(0, spp, a.chunk):
                n = min(a.chunk, spp - p)
                pa.RenderRays(s, rays[p:p + n], n, device_out=out, first_pass=p, flags=api.RENDER_NO_CLEAR if p else 0)

        res["rays_chunked_ms"] = best_of(chunked)
        res["rays_chunked_equal"] = bool(torch.equal(rgba, want[0]) and torch.equal(count, want[1]))
        res["chunk_passes"] = a.chunk

        def render_chunked():  # the same pass ranges through the camera: what the chunking alone costs
            for p in range(0, spp, a.chunk):
                n = min(a.chunk, spp - p)
                pa.Render(s, W, H, n, device_out=out, first_pass=p, flags=api.RENDER_NO_CLEAR if p else 0)

        res["render_chunked_ms"] = best_of(render_chunked)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
