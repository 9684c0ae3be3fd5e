"""The numpy float32 model of pbrhip_emission_split and pbrhip_emission_merge (include/pbrhip.h): every operation is one
float32 operation, in the header's order, so the device results are compared with it bit for bit."""
import numpy as np

F = np.float32


def split(rgba, count, emission, albedo_hits=None, feature_count=None):
    """-> (out_rgba, out_albedo_hits or None).  out_rgba = (max(rgba.rgb - emission.rgb, 0), rgba.a), zeros where count == 0 (a
    difference that is not > 0 -- a NaN among them -- gives +0); out_albedo_hits = (albedo_hits.rgb, (float)feature_count)."""
    rgba, emission = np.asarray(rgba, F), np.asarray(emission, F)
    out = np.zeros_like(rgba)
    with np.errstate(invalid="ignore"):
        d = rgba[..., :3] - emission[..., :3]
        out[..., :3] = np.where(d > 0, d, F(0))
    out[..., 3] = rgba[..., 3]
    out[np.asarray(count) == 0] = 0
    if albedo_hits is None:
        return out, None
    alb = np.array(albedo_hits, F)
    alb[..., 3] = np.asarray(feature_count).astype(F)
    return out, alb


def merge(filtered, emission, count):
    """out.rgb = filtered.rgb + emission.rgb / (float)count, out.a = filtered.a; count == 0 copies filtered"""
    out = np.array(filtered, F)
    count = np.asarray(count)
    live = count != 0
    fc = np.where(live, count, 1).astype(F)[..., None]
    mean = np.asarray(emission, F)[..., :3] / fc
    out[..., :3] = np.where(live[..., None], out[..., :3] + mean, out[..., :3])
    return out


def clamped_albedo(albedo_hits, feature_count):
    """What pbrhip_svgf_accumulate / pbrhip_svgf_filter / pbrhip_denoise divide by, in float32: max((albedo.rgb + misses) / samples,
    1e-3) with misses = samples - hits; 1 without samples"""
    m = np.asarray(feature_count).astype(F)[..., None]
    ah = np.asarray(albedo_hits, F)
    miss = m - ah[..., 3:4]
    with np.errstate(invalid="ignore", divide="ignore"):
        a = np.maximum((ah[..., :3] + miss) / m, F(1e-3))
    return np.where(m > 0, a, F(1)).astype(F)
