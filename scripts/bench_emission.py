"""bench_emission.py -- what the first-hit emission layer costs and buys.

Cost, at --width x --height (1920 x 1080) on device buffers, from one process, bench_svgf.py's method (the median ms per call after
--warmup untimed calls over --reps timed ones, a device synchronisation on both sides of every call): RenderFeaturesEmission against
RenderFeatures at --spp samples on the Lambert + GGX Cornell box (expected from the code: close to 1, one more 16-byte load and store per
pixel and one light-record gather per emitting hit beside a full traversal per sample), and pbrhip_emission_split_device /
pbrhip_emission_merge_device against their byte counts (split: rgba, count, emission, albedo_hits, feature_count in, two images out = 92
bytes per pixel; merge: filtered, emission, count in, one image out = 52).

Error, at --qsize squared on bench_temporal.py's orbit, on the Cornell box AND on scenes.textured_cornell_scene (where demodulation is
supposed to pay: the filter without albedo blurs the floor's checker): the relative MSE (bench_temporal.rel_mse) against --ref-spp frames,
averaged over the last --qframes frames, of the raw frame, the SVGF pipeline without a FeatureLayer, with a plain FeatureLayer, and with
the split (SplitEmission -> SvgfAccumulate -> SvgfFilter -> MergeEmission), each accumulated and accumulated + filtered.  One JSON line.

    python scripts/bench_emission.py [--frames 8] [--spp 8] [--qspp 4]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bench_temporal import pose, rel_mse  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--spp", type=int, default=8)
    ap.add_argument("--qspp", type=int, default=4)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--qsize", type=int, default=256)
    ap.add_argument("--qframes", type=int, default=4)
    ap.add_argument("--ref-spp", type=int, default=1024)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=15)
    a = ap.parse_args()
    import torch
    import pbrlab_amd as pa
    from pbrlab_amd import _lib, api, scenes
    pa.set_device(0)
    L = _lib.lib()
    n, W, H = a.frames, a.width, a.height
    res = {"frames": n, "spp": a.spp}

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

    # ---- cost
    s = pa.scene_from_desc(scenes.cornell_scene("ggx", seed=1))
    pose(pa, s, 0, n)
    s.RefitScene()
    dev = "cuda:0"
    f32 = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=dev)  # noqa: E731
    i32 = lambda *shape: torch.zeros(shape, dtype=torch.int32, device=dev)  # noqa: E731
    rgba, count, alb, nd, fc, em, out, oalb = f32(H, W, 4), i32(H, W), f32(H, W, 4), f32(H, W, 4), i32(H, W), f32(H, W, 4), f32(H, W, 4), f32(H, W, 4)
    pa.Render(s, W, H, a.spp, device_out=(rgba.data_ptr(), count.data_ptr()))
    p = lambda t: t.data_ptr()  # noqa: E731
    stages = dict(
        render_features=lambda: pa.RenderFeatures(s, W, H, a.spp, device_out=(p(alb), p(nd), p(fc))),
        render_features_emission=lambda: pa.RenderFeaturesEmission(s, W, H, a.spp, device_out=(p(alb), p(nd), p(fc), p(em))),
        emission_split=lambda: api._chk(L.pbrhip_emission_split_device(0, W, H, p(rgba), p(count), p(em), p(alb), p(fc), p(out), p(oalb))),
        emission_merge=lambda: api._chk(L.pbrhip_emission_merge_device(0, W, H, p(out), p(em), p(count), p(out))))
    cost = {}
    for name, f in stages.items():
        cost[name], cost[name + "_min"] = median_ms(f)
    cost["features_ratio"] = round(cost["render_features_emission"] / cost["render_features"], 3)
    for name, nbytes in (("emission_split", 92), ("emission_merge", 52)):
        cost[name + "_bytes_per_pixel"] = nbytes
        cost[name + "_GBps"] = round(nbytes * W * H / (cost[name] * 1e-3) / 1e9, 1)
    res["cost_ms"] = dict(cost, width=W, height=H, warmup=a.warmup, reps=a.reps)
    s.close()
    del rgba, count, alb, nd, fc, em, out, oalb
    torch.cuda.empty_cache()

    # ---- error
    Q, spp = a.qsize, a.qspp

    def mean(rows):
        return round(float(np.mean(rows)), 5)

    def sequence(desc):
        s = pa.scene_from_desc(desc)
        pose(pa, s, 0, n)
        s.RefitScene()
        h_split = h_plain = h_none = None
        rows = {k: [] for k in ("raw", "none_accumulated", "none_filtered", "plain_accumulated", "plain_filtered", "split_accumulated", "split_filtered")}
        for k in range(n):
            s.SnapshotPose()
            pose(pa, s, k, n)
            s.RefitScene()
            lay = pa.RenderLayer()
            pa.Render(s, Q, Q, spp, layer=lay, first_pass=spp * k)
            ml = pa.RenderMotion(s, Q, Q)
            ft, em = pa.RenderFeaturesEmission(s, Q, Q, spp, first_pass=spp * k)
            ids = s.ObjectIds(ml, api.ID_INSTANCE)
            sl, sf = pa.SplitEmission(lay, em, ft)
            h_split = pa.SvgfAccumulate(sl, ml, h_split, sf, ids)
            h_plain = pa.SvgfAccumulate(lay, ml, h_plain, ft, ids)
            h_none = pa.SvgfAccumulate(lay, ml, h_none, None, ids)
            if k < n - a.qframes:
                continue
            ref = pa.RenderLayer()
            pa.Render(s, Q, Q, a.ref_spp, layer=ref, first_pass=1 << 20)
            truth = ref.rgba[..., :3].astype(np.float64) / a.ref_spp
            m = ft.count.astype(np.float64)[..., None]
            hit = np.maximum(m, 1)
            a_plain = np.maximum(np.where(m > 0, (ft.albedo[..., :3] + (m - ft.albedo[..., 3:4])) / hit, 1.0), 1e-3)
            a_split = np.maximum(np.where(m > 0, ft.albedo[..., :3] / hit, 1.0), 1e-3)
            e_mean = em.emission[..., :3].astype(np.float64) / spp
            rows["raw"].append(rel_mse(lay.rgba[..., :3].astype(np.float64) / spp, truth))
            rows["none_accumulated"].append(rel_mse(h_none.illum[..., :3].astype(np.float64), truth))
            rows["none_filtered"].append(rel_mse(pa.SvgfFilter(h_none)[..., :3].astype(np.float64), truth))
            rows["plain_accumulated"].append(rel_mse(h_plain.illum[..., :3].astype(np.float64) * a_plain, truth))
            rows["plain_filtered"].append(rel_mse(pa.SvgfFilter(h_plain, ft)[..., :3].astype(np.float64), truth))
            rows["split_accumulated"].append(rel_mse(h_split.illum[..., :3].astype(np.float64) * a_split + e_mean, truth))
            rows["split_filtered"].append(rel_mse(pa.MergeEmission(pa.SvgfFilter(h_split, sf), em, lay.count)[..., :3].astype(np.float64), truth))
        s.close()
        return {k: mean(v) for k, v in rows.items()}

    res["relative_mse"] = dict(size=Q, spp=spp, ref_spp=a.ref_spp, judged_frames=a.qframes,
                               cornell=sequence(scenes.cornell_scene("ggx", seed=1)),
                               textured_cornell=sequence(scenes.textured_cornell_scene(seed=1)))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
