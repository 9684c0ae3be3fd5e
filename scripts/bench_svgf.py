"""bench_svgf.py -- what variance-guided filtering and the identity test cost and buy, on bench_temporal.py's sequence: the
Lambert + GGX Cornell box under an orbiting camera with two moving instances, --spp samples per pixel per frame.

Cost, at --width x --height (1920 x 1080) on device buffers, from one process: the median ms per call of Scene.ObjectIds, SvgfAccumulate and
SvgfFilter, and of the parent pipeline's TemporalAccumulate and DenoiseDevice at the same size and iteration count -- each after
--warmup untimed calls, over --reps timed ones, a device synchronisation on both sides of every call -- and the ratios of the new stages
to their counterparts (expected from byte counts alone: within 1.5).  Quality, at --qsize squared: the relative MSE (bench_temporal.rel_mse)
against --ref-spp frames of the same poses, averaged over the last --qframes frames, over the whole frame and over the frame without the
ceiling and the emitter, of: the raw frames; the parent pipeline (TemporalAccumulate + Denoise); SVGF without ids; SVGF with ids, with
and without the feedback of the first iteration; and the last three without a FeatureLayer (albedo 1: the colour itself is accumulated and
filtered -- what a black-albedo emitter in view calls for).  --sweep adds sigma_lum in (1, 2, 4, 8, 16) and alpha_min in (0.05, 0.1, 0.2, 0.4) for
SVGF with ids and feedback (the frames are rendered once).  One JSON line.

    python scripts/bench_svgf.py [--frames 12] [--spp 8] [--sweep]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bench_temporal import CEILING, LIGHT, pose, rel_mse  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=12)
    ap.add_argument("--spp", type=int, default=8)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--qsize", type=int, default=256)
    ap.add_argument("--qframes", type=int, default=4)
    ap.add_argument("--ref-spp", type=int, default=1024)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--sweep", action="store_true")
    a = ap.parse_args()
    import torch
    import pbrlab_amd as pa
    from pbrlab_amd import api, scenes
    pa.set_device(0)
    s = pa.scene_from_desc(scenes.cornell_scene("ggx", seed=1))
    n, W, H = a.frames, a.width, a.height
    res = {"scene": "C2 geometry, orbiting camera, two moving instances", "frames": n, "spp": a.spp}

    # ---- cost: two frames of the sequence give every stage real inputs (a history with lengths 1 and 2, real ids and features)
    dev = "cuda:0"
    f32 = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=dev)  # noqa: E731
    i32 = lambda *shape: torch.zeros(shape, dtype=torch.int32, device=dev)  # noqa: E731
    layer = type("DeviceLayer", (), dict(rgba=f32(H, W, 4), count=i32(H, W)))()
    feat = type("DeviceFeatures", (), dict(albedo=f32(H, W, 4), normal_depth=f32(H, W, 4), count=i32(H, W)))()
    hist = thist = ids = ml = None
    pose(pa, s, 0, n)
    s.RefitScene()
    for k in range(2):
        s.SnapshotPose()
        pose(pa, s, k, n)
        s.RefitScene()
        pa.Render(s, W, H, a.spp, first_pass=a.spp * k, device_out=(layer.rgba.data_ptr(), layer.count.data_ptr()))
        fh = pa.RenderFeatures(s, W, H, a.spp, first_pass=a.spp * k)
        feat.albedo.copy_(torch.from_numpy(fh.albedo)), feat.normal_depth.copy_(torch.from_numpy(fh.normal_depth))
        feat.count.copy_(torch.from_numpy(fh.count.view(np.int32)))
        ml = pa.RenderMotion(s, W, H, device_out=(f32(H, W, 4), f32(H, W, 4), i32(H, W, 4)))
        ids = s.ObjectIds(ml, api.ID_INSTANCE)
        if k == 0:
            hist, thist = pa.SvgfAccumulate(layer, ml, None, feat, ids), pa.TemporalAccumulate(layer, ml, None)
    out = f32(H, W, 4)

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
        return round(float(np.median(ts)), 3), round(float(np.min(ts)), 3)

    stages = dict(
        object_ids=lambda: s.ObjectIds(ml, api.ID_INSTANCE, device_out=ids),
        svgf_accumulate=lambda: pa.SvgfAccumulate(layer, ml, hist, feat, ids),
        svgf_filter=lambda: pa.SvgfFilter(pa.SvgfHistory(hist.illum, hist.var, hist.guide, hist.ids), feat, feedback=True),
        temporal_accumulate=lambda: pa.TemporalAccumulate(layer, ml, thist),
        denoise=lambda: pa.DenoiseDevice(0, W, H, layer.rgba.data_ptr(), layer.count.data_ptr(), out.data_ptr(),
                                         (feat.albedo.data_ptr(), feat.normal_depth.data_ptr(), feat.count.data_ptr()),
                                         iterations=api.SVGF_ITERATIONS))
    cost = {}
    for name, f in stages.items():
        cost[name], cost[name + "_min"] = median_ms(f)
    cost["accumulate_ratio"] = round(cost["svgf_accumulate"] / cost["temporal_accumulate"], 3)
    cost["filter_ratio"] = round(cost["svgf_filter"] / cost["denoise"], 3)
    res["cost_ms"] = dict(cost, width=W, height=H, iterations=api.SVGF_ITERATIONS, warmup=a.warmup, reps=a.reps)
    del layer, feat, hist, thist, ids, ml, out
    torch.cuda.empty_cache()

    # ---- quality
    Q = a.qsize
    frames = []
    for k in range(n):
        s.SnapshotPose()
        pose(pa, s, k, n)
        s.RefitScene()
        lay = pa.RenderLayer()
        pa.Render(s, Q, Q, a.spp, layer=lay, first_pass=a.spp * k)
        ml = pa.RenderMotion(s, Q, Q)
        ft = pa.RenderFeatures(s, Q, Q, a.spp, first_pass=a.spp * k)
        ids = s.ObjectIds(ml, api.ID_INSTANCE)
        truth = keep = None
        if k >= n - a.qframes:
            keep = ~((ids == CEILING) | (ids == LIGHT))
            ref = pa.RenderLayer()
            pa.Render(s, Q, Q, a.ref_spp, layer=ref, first_pass=1 << 20)
            truth = ref.rgba[..., :3].astype(np.float64) / a.ref_spp
        frames.append((lay, ml, ft, ids, truth, keep))

    def both(img, truth, keep):
        return rel_mse(img, truth), rel_mse(img, truth, keep)

    def mean(rows):
        return [round(float(v), 5) for v in np.mean(rows, 0)]

    def svgf(with_ids, feedback, sigma_lum=None, albedo=True, **params):
        """-> [whole frame, without ceiling and emitter] of the accumulated and of the filtered frames; albedo=False: no FeatureLayer, the
        colour itself is accumulated and filtered"""
        hist, acc, fil = None, [], []
        for lay, ml, ft, ids, truth, keep in frames:
            hist = pa.SvgfAccumulate(lay, ml, hist, ft if albedo else None, ids if with_ids else None, **params)
            img, fed = pa.SvgfFilter(hist, ft if albedo else None, sigma_lum=sigma_lum, feedback=True)
            if truth is not None:
                alb = np.maximum(np.where((ft.count > 0)[..., None], (ft.albedo[..., :3] + (ft.count - ft.albedo[..., 3])[..., None])
                                          / np.maximum(ft.count, 1)[..., None], 1.0), 1e-3) if albedo else 1.0
                acc.append(both(hist.illum[..., :3].astype(np.float64) * alb, truth, keep))
                fil.append(both(img[..., :3].astype(np.float64), truth, keep))
            if feedback:
                hist = fed
        return dict(accumulated=mean(acc), filtered=mean(fil))

    raw, parent_acc, parent = [], [], []
    th = None
    for lay, ml, ft, ids, truth, keep in frames:
        th = pa.TemporalAccumulate(lay, ml, th)
        if truth is not None:
            raw.append(both(lay.rgba[..., :3].astype(np.float64) / a.spp, truth, keep))
            parent_acc.append(both(th.rgba[..., :3].astype(np.float64), truth, keep))
            parent.append(both(pa.Denoise(th.layer(), ft)[..., :3].astype(np.float64), truth, keep))
    res["relative_mse_columns"] = ["whole frame", "without ceiling and emitter"]
    res["relative_mse"] = dict(size=Q, ref_spp=a.ref_spp, judged_frames=a.qframes,
                               share_of_pixels_without_ceiling_and_emitter=round(float(np.mean([f[5].mean() for f in frames if f[5] is not None])), 4),
                               raw=mean(raw), temporal_accumulate=mean(parent_acc), temporal_accumulate_denoise=mean(parent),
                               svgf_without_ids=svgf(False, False), svgf_with_ids=svgf(True, False), svgf_with_ids_feedback=svgf(True, True),
                               svgf_without_ids_no_albedo=svgf(False, False, albedo=False), svgf_with_ids_no_albedo=svgf(True, False, albedo=False),
                               svgf_with_ids_feedback_no_albedo=svgf(True, True, albedo=False))
    if a.sweep:
        res["sweep"] = dict(sigma_lum={str(v): svgf(True, True, sigma_lum=v) for v in (1.0, 2.0, 4.0, 8.0, 16.0)},
                            alpha_min={str(v): svgf(True, True, alpha_min=v) for v in (0.05, 0.1, 0.2, 0.4)})
        res["sweep_no_albedo"] = dict(sigma_lum={str(v): svgf(True, True, sigma_lum=v, albedo=False) for v in (1.0, 2.0, 4.0, 8.0, 16.0)},
                                      alpha_min={str(v): svgf(True, True, alpha_min=v, albedo=False) for v in (0.05, 0.1, 0.2, 0.4)})
        res["sweep_defaults"] = dict(sigma_lum=api.SVGF_SIGMA_LUM, alpha_min=api.SVGF_ALPHA_MIN)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
