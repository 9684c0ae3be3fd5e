"""bench_camera.py -- what a user camera costs: C2's geometry (the Lambert + GGX Cornell box) at 1920x1080, 64 spp,
rendered four ways in one process -- the reference's camera, a pinhole user camera at the reference camera's pose, an oblique pinhole
and a thin lens -- and reported as Msamples/s each (median of --reps timed renders after one warm-up), one JSON line.

    python scripts/bench_camera.py [--reps 3] [--spp 64]

PBRHIP_LIB picks another build of the library for same-box A/Bs."""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def reference_pose(bmin, bmax, width, height):
    """eye, lookat, up, vfov of the reference's camera (make_camera, render.cc:132-158) for this box and image"""
    bmin, bmax = np.asarray(bmin, np.float64), np.asarray(bmax, np.float64)
    if bmax[0] - bmin[0] > bmax[1] - bmin[1]:
        hs = bmax[0] - bmin[0]
        vs = hs * height / width
    else:
        vs = bmax[1] - bmin[1]
        hs = vs * width / height
    eye = np.array([(bmax[0] + bmin[0]) * 0.5, (bmax[1] + bmin[1]) * 0.5, bmax[2] + hs * 0.5 * math.sqrt(3.0)])
    return eye, eye - np.array([0.0, 0.0, 1.0]), (0.0, 1.0, 0.0), math.degrees(2.0 * math.atan(vs / (hs * math.sqrt(3.0))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    a = ap.parse_args()
    import pbrlab_amd as pa
    from pbrlab_amd import scenes
    pa.set_device(0)
    s = pa.scene_from_desc(scenes.cornell_scene("ggx", seed=1))
    W, H = a.width, a.height
    bmin, bmax = (np.array(v, np.float64) for v in s.FetchSceneAABB())
    eye, at, up, fov = reference_pose(bmin, bmax, W, H)
    c, e = 0.5 * (bmin + bmax), bmax - bmin
    oblique = (c + np.array([0.35, 0.3, 0.45]) * e, c - np.array([0.05, 0.1, 0.1]) * e, (0.0, 1.0, 0.0), 60.0)
    cams = {"default": None, "pinhole_reference_pose": (eye, at, up, fov, 0.0, 0.0), "pinhole_oblique": oblique + (0.0, 0.0),
            "thin_lens": oblique + (0.01 * float(e.max()), 0.0)}
    out = {"scene": "C2 geometry", "lib": os.environ.get("PBRHIP_LIB", "default"), "width": W, "height": H, "spp": a.spp, "reps": a.reps}
    for name, cam in cams.items():
        if cam is None:
            s.SetCamera(None)
        else:
            s.SetCamera(*cam)
        layer = pa.RenderLayer()
        pa.Render(s, W, H, a.spp, layer=layer)  # warm-up
        ts = []
        for _ in range(a.reps):
            layer = pa.RenderLayer()
            t0 = time.perf_counter()
            pa.Render(s, W, H, a.spp, layer=layer)
            ts.append(time.perf_counter() - t0)
        out[name] = {"Msamples/s": round(W * H * a.spp / float(np.median(ts)) / 1e6, 1), "ms": round(float(np.median(ts)) * 1e3, 1)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
