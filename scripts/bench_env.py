"""bench_env.py -- what the environment light costs: C2's geometry (the Lambert + GGX Cornell box) at 1920x1080,
64 spp, rendered three ways in one process -- no environment, a constant environment, and a procedural 2048 x 1024 sky with a
small bright sun -- and reported as Msamples/s each (median of --reps timed renders after one warm-up), one JSON line.

    python scripts/bench_env.py [--reps 3] [--spp 64] [--variant ggx|sss]

--variant sss renders C3's geometry instead (random-walk subsurface: the media kernels); PBRHIP_LIB picks another build of the library
for same-box A/Bs."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def procedural_sky(w=2048, h=1024):
    """a blue-to-pale sky gradient over a dark ground, and a sun of ~0.5 degrees 35 degrees above the horizon (no assets)"""
    theta = (np.arange(h) + 0.5) / h * np.pi
    phi = (np.arange(w) + 0.5) / w * 2 * np.pi
    up = np.cos(theta)[:, None] * np.ones((1, w))
    sky = np.where(up[..., None] > 0, np.stack([0.25 + 0.5 * (1 - up), 0.4 + 0.4 * (1 - up), 0.9 - 0.2 * (1 - up)], -1),
                   np.array([0.08, 0.07, 0.06]))
    st, sp = np.radians(90 - 35), np.radians(120)
    d = np.stack([np.sin(theta)[:, None] * np.sin(phi - np.pi)[None], np.cos(theta)[:, None] * np.ones((1, w)),
                  -np.sin(theta)[:, None] * np.cos(phi - np.pi)[None]], -1)
    s = np.array([np.sin(st) * np.sin(sp - np.pi), np.cos(st), -np.sin(st) * np.cos(sp - np.pi)])
    sun = (d @ s) > np.cos(np.radians(0.5))
    sky[sun] = [2.0e4, 1.9e4, 1.6e4]
    return sky.astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--variant", default="ggx", choices=["ggx", "sss"])
    a = ap.parse_args()
    import pbrlab_amd as pa
    from pbrlab_amd import scenes
    pa.set_device(0)
    s = pa.scene_from_desc(scenes.cornell_scene(a.variant, seed=1))
    W, H = a.width, a.height
    maps = {"none": None, "constant": np.full((4, 8, 3), 0.5, np.float32), "sky_sun_2048x1024": procedural_sky()}
    out = {"scene": {"ggx": "C2", "sss": "C3"}[a.variant] + " geometry", "lib": os.environ.get("PBRHIP_LIB", "default"), "width": W, "height": H, "spp": a.spp, "reps": a.reps}
    for name, env in maps.items():
        s.SetEnvironment(env)
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
