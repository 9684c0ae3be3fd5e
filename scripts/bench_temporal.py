"""bench_temporal.py -- what motion vectors and temporal accumulation cost and buy: a short sequence on the Lambert + GGX
Cornell box -- the camera orbits, the monkey and the small box move as instances -- rendered at --spp samples per pixel per frame.

Cost, at --width x --height (1920 x 1080), from one process: per frame the ms of SnapshotPose, of the edits + RefitScene, of the --spp
Render they accompany, of RenderMotion and of TemporalAccumulate, the last three on device buffers (torch tensors); the median over the
frames after the first.  Quality, at --qsize squared: the relative MSE against 1024-spp frames of the same poses of the raw, the
accumulated, the denoised and the accumulated + denoised frames, averaged over the last --qframes frames -- over the whole frame, and over the frame without the pixels
that show the ceiling or the emitter, which lies a hundredth of a unit below it with the ceiling's normal: no test of the accumulation
can tell the two apart, and under a moving camera the emitter's radiance bleeds into the ceiling's history.  --sweep adds one-at-a-time
sweeps of the four parameters around the defaults (the frames are rendered once; only the accumulation is repeated).  One JSON line.

    python scripts/bench_temporal.py [--frames 12] [--spp 8] [--sweep]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CEILING, LIGHT, MONKEY, BOX = 1, 5, 6, 8  # instances of scenes.cornell_scene, in build order


def pose(pa, s, k, n):
    """frame k of n: the camera a few degrees further round the box, the monkey hopping sideways, the small box turning"""
    from pbrlab_amd import scenes
    a = np.deg2rad(-12.0 + 24.0 * k / max(n - 1, 1))
    s.SetCamera((3.6 * np.sin(a), 0.1, 3.6 * np.cos(a)), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 35.0)
    s.UpdateInstanceTransform(MONKEY, scenes.instance_matrix(translate=(0.04 * k, 0.02 * (k % 3), 0.0)))
    s.UpdateInstanceTransform(BOX, scenes.instance_matrix(rotate_deg=(0.0, 3.0 * k, 0.0), translate=(-0.02 * k, 0.0, 0.0)))


def rel_mse(img, truth, keep=None):
    e = (((img - truth) ** 2) / (truth ** 2 + 1e-2)).mean(-1)
    return float(e.mean() if keep is None else e[keep].mean())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=12)
    ap.add_argument("--spp", type=int, default=8)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--qsize", type=int, default=256)
    ap.add_argument("--qframes", type=int, default=4)
    ap.add_argument("--ref-spp", type=int, default=1024)
    ap.add_argument("--sweep", action="store_true")
    a = ap.parse_args()
    import torch
    import pbrlab_amd as pa
    from pbrlab_amd import api, scenes
    pa.set_device(0)
    s = pa.scene_from_desc(scenes.cornell_scene("ggx", seed=1))
    n, W, H = a.frames, a.width, a.height
    res = {"scene": "C2 geometry, orbiting camera, two moving instances", "frames": n, "spp": a.spp}

    # ---- cost
    dev = "cuda:0"
    rgba = torch.zeros((H, W, 4), dtype=torch.float32, device=dev)
    count = torch.zeros((H, W), dtype=torch.int32, device=dev)
    bufs = [(torch.zeros_like(rgba), torch.zeros_like(rgba), torch.zeros((H, W, 4), dtype=torch.int32, device=dev)) for _ in range(2)]
    layer = type("DeviceLayer", (), dict(rgba=rgba, count=count))()
    torch.cuda.synchronize()
    ms = {k: [] for k in ("snapshot", "edit_refit", "render", "motion", "accumulate")}
    hist = None
    pose(pa, s, 0, n)
    s.RefitScene()
    for k in range(n):
        def timed(name, f):
            t0 = time.perf_counter()
            out = f()
            torch.cuda.synchronize()  # (the snapshot's copy is asynchronous; every other call returns after its stream is idle)
            if k:
                ms[name].append((time.perf_counter() - t0) * 1e3)
            return out
        timed("snapshot", s.SnapshotPose)
        timed("edit_refit", lambda: (pose(pa, s, k, n), s.RefitScene()))
        timed("render", lambda: pa.Render(s, W, H, a.spp, first_pass=a.spp * k, device_out=(rgba.data_ptr(), count.data_ptr())))
        ml = timed("motion", lambda: pa.RenderMotion(s, W, H, device_out=bufs[k & 1]))
        hist = timed("accumulate", lambda: pa.TemporalAccumulate(layer, ml, hist))
    cost = {k: round(float(np.median(v)), 3) for k, v in ms.items()}
    cost["motion_plus_accumulate_share_of_render"] = round((cost["motion"] + cost["accumulate"]) / cost["render"], 4)
    res["cost_ms"] = dict(cost, width=W, height=H)
    del rgba, count, bufs, hist, ml, layer
    torch.cuda.empty_cache()

    # ---- quality
    Q = a.qsize
    frames = []
    shade = s.read_slots()[1]  # (a refit keeps the slot order: read once)
    for k in range(n):
        s.SnapshotPose()
        pose(pa, s, k, n)
        s.RefitScene()
        lay = pa.RenderLayer()
        pa.Render(s, Q, Q, a.spp, layer=lay, first_pass=a.spp * k)
        ml = pa.RenderMotion(s, Q, Q)
        feat = truth = keep = None
        if k >= n - a.qframes:
            hit = ml.ident[..., 0] != api.NONE
            inst = shade[np.where(hit, ml.ident[..., 0], 0), 25]
            keep = ~(hit & ((inst == CEILING) | (inst == LIGHT)))
            feat = pa.RenderFeatures(s, Q, Q, a.spp, first_pass=a.spp * k)
            ref = pa.RenderLayer()
            pa.Render(s, Q, Q, a.ref_spp, layer=ref, first_pass=1 << 20)
            truth = ref.rgba[..., :3].astype(np.float64) / a.ref_spp
        frames.append((lay, ml, feat, truth, keep))

    def run(**params):
        """the sequence accumulated with `params` -> the mean relative MSE over the judged frames of the accumulated and the accumulated +
        denoised frames, whole frame; then the same two without the ceiling and the emitter"""
        hist, out = None, [[], [], [], []]
        for lay, ml, feat, truth, keep in frames:
            hist = pa.TemporalAccumulate(lay, ml, hist, **params)
            if truth is not None:
                acc, den = hist.rgba[..., :3].astype(np.float64), pa.Denoise(hist.layer(), feat)[..., :3].astype(np.float64)
                for o, v in zip(out, (rel_mse(acc, truth), rel_mse(den, truth), rel_mse(acc, truth, keep), rel_mse(den, truth, keep))):
                    o.append(v)
        return [round(float(np.mean(o)), 5) for o in out]

    judged = [f for f in frames if f[3] is not None]
    raws = [(l.rgba[..., :3].astype(np.float64) / a.spp, pa.Denoise(l, f)[..., :3].astype(np.float64), t, k) for l, _, f, t, k in judged]
    acc = run()
    res["relative_mse"] = dict(size=Q, ref_spp=a.ref_spp, judged_frames=len(judged),
                               raw=round(float(np.mean([rel_mse(r, t) for r, _, t, _ in raws])), 5),
                               denoised=round(float(np.mean([rel_mse(d, t) for _, d, t, _ in raws])), 5),
                               accumulated=acc[0], accumulated_denoised=acc[1])
    res["relative_mse_without_ceiling_and_emitter"] = dict(share_of_pixels=round(float(np.mean([k.mean() for _, _, _, k in raws])), 4),
                                                           raw=round(float(np.mean([rel_mse(r, t, k) for r, _, t, k in raws])), 5),
                                                           denoised=round(float(np.mean([rel_mse(d, t, k) for _, d, t, k in raws])), 5),
                                                           accumulated=acc[2], accumulated_denoised=acc[3])
    if a.sweep:
        grid = dict(alpha_min=(0.0, 0.02, 0.05, 0.1, 0.2, 0.4), sigma_depth=(0.01, 0.02, 0.05, 0.1, 0.2, 0.5),
                    normal_cos_min=(-1.0, 0.5, 0.8, 0.9, 0.95, 0.99), max_history=(4, 8, 16, 32, 64))
        res["sweep_columns"] = ["accumulated", "accumulated_denoised", "accumulated, no ceiling / emitter", "accumulated_denoised, no ceiling / emitter"]
        res["sweep"] = {name: {str(v): run(**{name: v}) for v in values} for name, values in grid.items()}
        res["sweep_defaults"] = dict(alpha_min=api.TEMPORAL_ALPHA_MIN, sigma_depth=api.TEMPORAL_SIGMA_DEPTH,
                                     normal_cos_min=api.TEMPORAL_NORMAL_COS_MIN, max_history=api.TEMPORAL_MAX_HISTORY)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
