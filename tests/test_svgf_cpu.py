"""Variance-guided filtering without a GPU: the symbols and Python names exist, the ABI version stands, bad arguments are
refused before any device work, and the float64 model of tests/_svgf_model.py agrees with closed forms and with _temporal_model."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _svgf_model as SM
import _temporal_model as TM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("pbrhip_scene_object_ids", "pbrhip_scene_object_ids_device", "pbrhip_svgf_accumulate", "pbrhip_svgf_accumulate_device",
           "pbrhip_svgf_filter", "pbrhip_svgf_filter_device")
EINVAL, ENODEVICE = -1, -3
F = np.float32


def test_symbols_and_names_exist():
    import pbrlab_amd as pa
    from pbrlab_amd import _lib, api
    L = _lib.lib()
    hdr = open(os.path.join(ROOT, "include", "pbrhip.h")).read()
    for name in SYMBOLS:
        assert name in _lib.EXPORTS and hasattr(L, name) and re.search(r"\b" + name + r"\s*\(", hdr), name
    for name in ("SvgfHistory", "SvgfAccumulate", "SvgfFilter"):
        assert hasattr(api, name) and hasattr(pa, name), name
    assert hasattr(pa.Scene, "ObjectIds")
    assert L.pbrhip_abi_version() == 6 and re.search(r"#define PBRHIP_ABI_VERSION 6u\b", hdr)
    assert "Not provided: variance-guided filtering" not in hdr
    # the header's defaults are the binding's and the model's
    for macro, value in (("ALPHA_MIN", api.SVGF_ALPHA_MIN), ("ITERATIONS", api.SVGF_ITERATIONS), ("SIGMA_LUM", api.SVGF_SIGMA_LUM),
                         ("LUM_EPS", api.SVGF_LUM_EPS)):
        m = re.search(r"#define PBRHIP_SVGF_" + macro + r" ([0-9.e-]+)f?\b", hdr)
        assert m and float(m.group(1)) == float(value), macro
    for k, name in enumerate(("PRIMITIVE", "INSTANCE", "GEOM")):
        assert re.search(r"#define PBRHIP_ID_" + name + rf" {k}u\b", hdr) and getattr(api, "ID_" + name) == k == getattr(SM, "ID_" + name)
    assert SM.ITERATIONS == api.SVGF_ITERATIONS and SM.SIGMA_LUM == api.SVGF_SIGMA_LUM and SM.SIGMA_DEPTH == api.DENOISE_SIGMA_DEPTH and float(SM.LUM_EPS) == float(F(api.SVGF_LUM_EPS))


def _refused(fs, args, word=b""):
    from pbrlab_amd import _lib
    L = _lib.lib()
    for f in fs:
        rc = f(*args)
        assert rc == EINVAL and word in L.pbrhip_last_error(), (rc, L.pbrhip_last_error())


def test_accumulate_refuses_bad_arguments_before_any_device_work():
    from pbrlab_amd import _lib
    L = _lib.lib()
    W, H = 8, 4
    img = [np.zeros((H, W, 4), F) for _ in range(7)]
    rgba, alb, motion, guide, hi, hg, out = (a.ctypes.data for a in img)
    one = [np.zeros((H, W), np.uint32) for _ in range(6)]
    count, fc, ids, hids, hv, ov = (a.ctypes.data for a in one)
    par = [C.c_float(0.1), C.c_float(0.05), C.c_float(0.9), 32]
    nan = C.c_float(float("nan"))
    fs = (L.pbrhip_svgf_accumulate, L.pbrhip_svgf_accumulate_device)
    #       0  1  2  3     4      5    6   7       8      9    10  11  12  13    14..17 18   19
    good = [0, W, H, rgba, count, alb, fc, motion, guide, ids, hi, hv, hg, hids, *par, out, ov]

    def swap(**kw):
        a = list(good)
        for k, v in kw.items():
            a[int(k[1:])] = v
        return a
    for k in (3, 4, 7, 8, 18, 19):  # NULL rgba, count, motion, guide, out_illum, out_var
        _refused(fs, swap(**{f"_{k}": None}), b"NULL")
    _refused(fs, swap(_5=None), b"albedo_hits and feature_count")  # half an albedo pair
    _refused(fs, swap(_6=None), b"albedo_hits and feature_count")
    for k in (10, 11, 12):  # one of the three history buffers missing
        _refused(fs, swap(**{f"_{k}": None}), b"together")
    _refused(fs, swap(_10=None, _11=None), b"together")
    _refused(fs, swap(_13=None), b"hist_ids")                           # ids and a history, no hist_ids
    _refused(fs, swap(_9=None), b"hist_ids")                            # hist_ids without ids
    _refused(fs, swap(_10=None, _11=None, _12=None), b"hist_ids")       # hist_ids without a history
    for k in (14, 15, 16):
        _refused(fs, swap(**{f"_{k}": nan}), b"NaN")
    _refused(fs, swap(_14=C.c_float(-0.01)), b"alpha_min")
    _refused(fs, swap(_14=C.c_float(1.5)), b"alpha_min")
    _refused(fs, swap(_17=0), b"max_history")
    _refused(fs, swap(_17=(1 << 24) + 1), b"max_history")
    _refused(fs, swap(_1=0), b"empty")
    _refused(fs, swap(_2=0), b"empty")
    _refused(fs, swap(_18=hi), b"history buffer")   # in place
    _refused(fs, swap(_18=hg), b"history buffer")
    _refused(fs, swap(_19=hv), b"history buffer")
    _refused(fs, swap(_19=out), b"out_var")
    # what is allowed gets as far as the device (none here: ENODEVICE; one there: 0)
    import pbrlab_amd as pa
    want = 0 if pa.device_count() > 0 else ENODEVICE
    assert L.pbrhip_svgf_accumulate(*swap(_5=None, _6=None, _9=None, _13=None)) == want
    assert L.pbrhip_svgf_accumulate(*swap(_10=None, _11=None, _12=None, _13=None)) == want


def test_filter_and_object_ids_refuse_bad_arguments_before_any_device_work():
    from pbrlab_amd import _lib
    L = _lib.lib()
    W, H = 8, 4
    img = [np.ones((H, W, 4), F) for _ in range(5)]
    illum, guide, alb, out, fb = (a.ctypes.data for a in img)
    one = [np.zeros((H, W), np.uint32) for _ in range(3)]
    var, ids, fc = (a.ctypes.data for a in one)
    nan = C.c_float(float("nan"))
    fs = (L.pbrhip_svgf_filter, L.pbrhip_svgf_filter_device)
    #       0  1  2  3      4    5      6    7    8   9  10               11               12 13   14
    good = [0, W, H, illum, var, guide, ids, alb, fc, 5, C.c_float(4.0), C.c_float(0.2), 7, out, fb]

    def swap(k, v):
        return good[:k] + [v] + good[k + 1:]
    for k in (3, 4, 5, 13):
        _refused(fs, swap(k, None), b"NULL")
    _refused(fs, swap(7, None), b"albedo_hits and feature_count")
    _refused(fs, swap(8, None), b"albedo_hits and feature_count")
    _refused(fs, swap(10, nan), b"NaN")
    _refused(fs, swap(11, nan), b"NaN")
    _refused(fs, swap(9, 9), b"iterations")
    _refused(fs, swap(12, 17), b"squarings")
    _refused(fs, swap(1, 0), b"empty")
    _refused(fs, swap(2, 0), b"empty")
    _refused(fs, swap(13, illum), b"output")
    _refused(fs, swap(14, out), b"output")
    # object ids: NULL scene, an unknown id, NULL buffers with pixels to write -- the scene is never dereferenced
    fake = C.c_void_p(16)
    for f, tail in ((L.pbrhip_scene_object_ids, ()), (L.pbrhip_scene_object_ids_device, (None,))):
        assert f(None, illum, 4, 1, var, *tail) == EINVAL and b"NULL" in L.pbrhip_last_error()
        assert f(fake, illum, 4, 3, var, *tail) == EINVAL and b"unknown" in L.pbrhip_last_error()
        assert f(fake, None, 4, 1, var, *tail) == EINVAL and b"NULL" in L.pbrhip_last_error()
        assert f(fake, illum, 4, 1, None, *tail) == EINVAL and b"NULL" in L.pbrhip_last_error()


def test_python_refuses_mixed_and_misshapen_buffers():
    import pbrlab_amd as pa
    layer = pa.RenderLayer(8, 4)
    m = pa.MotionLayer(np.zeros((4, 8, 4), F), np.zeros((4, 9, 4), F), None)
    with pytest.raises(ValueError):
        pa.SvgfAccumulate(layer, m)
    m = pa.MotionLayer(np.zeros((4, 8, 4), F), np.zeros((4, 8, 4), F), None)
    with pytest.raises(ValueError):
        pa.SvgfAccumulate(layer, m, ids=np.zeros((4, 7), np.uint32))
    with pytest.raises(ValueError):
        pa.SvgfFilter(pa.SvgfHistory(np.zeros((4, 8, 4), F), np.zeros((4, 8, 1), F), m.guide))
    if pa.device_count() == 0:
        with pytest.raises(pa.PbrHipError) as e:
            pa.SvgfAccumulate(layer, m)
        assert e.value.code == ENODEVICE
        with pytest.raises(pa.PbrHipError) as e:
            pa.SvgfFilter(pa.SvgfHistory(np.zeros((4, 8, 4), F), np.zeros((4, 8), F), m.guide))
        assert e.value.code == ENODEVICE


# ---------------------------------------------------------------------------------------------------- the float64 model
def _static(W, H):
    guide = np.zeros((H, W, 4), F)
    guide[..., 2], guide[..., 3] = 1.0, 3.0
    motion = np.zeros((H, W, 4), F)
    motion[..., 2], motion[..., 3] = 3.0, 1.0
    return guide, motion


def test_model_static_pixel_holds_mean_and_population_variance():
    """alpha_min = 0, zero motion: after k frames the pixel holds np.mean and np.var of its k luminances (Welford's recurrence); the
    history is rounded to float32 between the frames, as the library hands it on: agreement to 1e-5 and 1e-4"""
    W, H, K = 5, 4, 12
    rng = np.random.RandomState(6)
    guide, motion = _static(W, H)
    count = np.full((H, W), 1, np.uint32)
    ls = rng.uniform(0.2, 3.0, (K, H, W)).astype(F)
    hi = hv = None
    for k in range(K):
        rgba = np.repeat(ls[k][..., None], 4, -1)
        hi, hv = SM.accumulate(rgba, count, motion, guide, hi, hv, None if hi is None else guide, 0.0, 0.05, 0.9, 1 << 20)
        hi, hv = hi.astype(F), hv.astype(F)
    grey = ls.astype(np.float64) * SM.LUM.sum()
    assert np.allclose(SM.lum(hi[..., :3].astype(np.float64)), grey.mean(0), rtol=1e-5) and np.allclose(hv, grey.var(0), rtol=1e-4)
    assert (hv >= 0).all()


def test_model_without_ids_and_albedo_is_the_temporal_model():
    W, H = 23, 17
    rng = np.random.RandomState(7)
    count = rng.randint(0, 5, (H, W)).astype(np.uint32)
    rgba = (rng.uniform(0, 2, (H, W, 4)) * count[..., None]).astype(F)
    guide = np.zeros((H, W, 4), F)
    guide[..., :3], guide[..., 3] = (0.0, 0.6, 0.8), 2.0 + rng.uniform(0, 0.3, (H, W))
    motion = np.zeros((H, W, 4), F)
    motion[..., :2] = rng.uniform(-2, 2, (H, W, 2))
    motion[..., 2], motion[..., 3] = guide[..., 3] * rng.choice([1.0, 1.2], (H, W)), rng.choice([0.0, 1.0, 2.0], (H, W))
    hist = rng.uniform(0, 2, (H, W, 4)).astype(F)
    hist[..., 3] = rng.randint(0, 6, (H, W))
    hv = rng.uniform(0, 1, (H, W)).astype(F)
    par = (0.1, 0.1, 0.9, 4)
    m0, m1, b0, b1 = [], [], [], []
    want = TM.accumulate(rgba, count, motion, guide, hist, guide, *par, margins=m0, bound=b0)
    got, var = SM.accumulate(rgba, count, motion, guide, hist, hv, guide, *par, margins=m1, bound=b1)
    assert np.array_equal(got, want) and (got[..., 3] > 1).sum() > 20 and (var >= 0).all() and (var[got[..., 3] <= 1] == 0).all()
    assert m0 == m1 and (b1[0][0] >= b0[0]).all() and b1[0][1].shape == (H, W)
    # no history at all
    got, var = SM.accumulate(rgba, count, motion, guide, None, None, None, *par)
    assert np.array_equal(got, TM.accumulate(rgba, count, motion, guide, None, None, *par)) and (var == 0).all()
    # the id test rejects what the other tests accept; an albedo divides the illumination
    ids = np.ones((H, W), np.uint32)
    same = SM.accumulate(rgba, count, motion, guide, hist, hv, guide, *par, ids=ids, hist_ids=ids)[0]
    other = SM.accumulate(rgba, count, motion, guide, hist, hv, guide, *par, ids=ids, hist_ids=ids + 1)[0]
    assert np.array_equal(same, want) and (other[..., 3] <= 1).all()
    ah = np.zeros((H, W, 4), F)
    ah[..., :3], ah[..., 3] = 1.0, 2.0  # two hits of albedo 0.5 out of four samples: a = (1 + 2) / 4
    half = SM.accumulate(rgba, count, motion, guide, None, None, None, *par, albedo_hits=ah, feature_count=np.full((H, W), 4, np.uint32))[0]
    assert np.allclose(half[..., :3] * 0.75, TM.accumulate(rgba, count, motion, guide, None, None, *par)[..., :3], rtol=1e-14)


def _planes(W, H, seed):
    rng = np.random.RandomState(seed)
    illum = rng.uniform(0.1, 2.0, (H, W, 4)).astype(F)
    illum[..., 3] = rng.randint(0, 9, (H, W))
    var = rng.uniform(0.0, 0.2, (H, W)).astype(F)
    guide = np.zeros((H, W, 4), F)
    guide[..., :3], guide[..., 3] = (0.0, 0.0, 1.0), 3.0  # (a normal whose float32 square is 1: w_n = 1)
    return rng, illum, var, guide


def test_model_constant_image_passes_unchanged_with_variance_zero():
    rng, illum, var, guide = _planes(19, 13, 8)
    illum[..., :3] = (0.3, 0.6, 0.9)
    illum[..., 3] = rng.randint(1, 4, illum.shape[:2])  # every pixel young: the variance is the spatial estimate
    e = illum[..., :3].astype(np.float64)
    v0, dv0 = SM.variance_in(illum.astype(np.float64), var.astype(np.float64), guide.astype(np.float64), None, 0.2, 7)
    assert (v0 == 0).all() and (dv0 < 1e-12).all()
    bound = []
    out, fb = SM.filter(illum, var, guide, iterations=5, bound=bound)
    assert np.array_equal(out[..., :3], e) and (out[..., 3] == 1).all() and np.array_equal(fb[..., :3], e) and np.array_equal(fb[..., 3], illum[..., 3])
    assert bound[0][0].max() < 64 * SM.EPS and bound[0][1].max() < 64 * SM.EPS
    live = np.ones(illum.shape[:2], bool)
    v = SM.iterate(e, v0, np.zeros_like(v0), dv0, live, guide.astype(np.float64), None, 0, 4.0, 0.2, 7)[1]
    assert (v == 0).all()


def test_model_one_iteration_without_weights_is_the_b3_convolution():
    """sigma_lum <= 0, no ids, constant guides, every pixel live: e(1) is the separable B3 convolution renormalised at the border, and
    v(1) the convolution of v with the squared kernel"""
    rng, illum, var, guide = _planes(21, 15, 9)
    illum[..., 3] = 8
    out, fb = SM.filter(illum, var, guide, iterations=1, sigma_lum=0.0, sigma_depth=0.2)
    e = illum[..., :3].astype(np.float64)
    H, W = var.shape
    num, den = np.zeros_like(e), np.zeros((H, W))
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            k = SM.B3[dx + 2] * SM.B3[dy + 2]
            ys, xs = np.mgrid[0:H, 0:W]
            ok = (ys + dy >= 0) & (ys + dy < H) & (xs + dx >= 0) & (xs + dx < W)
            q = e[np.clip(ys + dy, 0, H - 1), np.clip(xs + dx, 0, W - 1)]
            num += np.where(ok[..., None], k * q, 0.0)
            den += np.where(ok, k, 0.0)
    assert np.allclose(out[..., :3], num / den[..., None], rtol=1e-13) and np.array_equal(out[..., :3], fb[..., :3])
    assert np.isclose(den[H // 2, W // 2], 1.0)
    # pixels that are not live come out zero and take no part
    illum[3, 4, 3] = 0
    out2 = SM.filter(illum, var, guide, iterations=1, sigma_lum=0.0)[0]
    assert (out2[3, 4] == 0).all() and not np.allclose(out2[3, 5, :3], out[3, 5, :3]) and np.array_equal(out2[10, 15], out[10, 15])


def test_model_weights_ids_background_and_young_pixels():
    rng, illum, var, guide = _planes(21, 15, 10)
    illum[..., 3] = 8
    H, W = var.shape
    ids = np.where(np.arange(W)[None, :] < W // 2, 7, 9).astype(np.uint32) * np.ones((H, 1), np.uint32)
    illum[..., :3] = np.where((ids == 7)[..., None], 1.0, 0.25)
    margins = []
    with_ids = SM.filter(illum, var, guide, ids=ids, iterations=3, sigma_lum=0.0, margins=margins)[0]
    without = SM.filter(illum, var, guide, iterations=3, sigma_lum=0.0)[0]
    assert np.array_equal(with_ids[..., :3], illum[..., :3].astype(np.float64)) and not np.array_equal(without, with_ids)
    assert SM.conditioned(margins) and margins[0] == ("len", np.inf)
    # a background pixel (guide.w == 0) mixes with background only
    guide[:, :5] = 0
    bg = SM.filter(illum, var, guide, iterations=2, sigma_lum=0.0)[0]
    illum2 = illum.copy()
    illum2[:, 5:, :3] += 1.0
    assert np.array_equal(SM.filter(illum2, var, guide, iterations=2, sigma_lum=0.0)[0][:, :5], bg[:, :5])
    # a young pixel's variance is 4 / len of its neighbourhood's; an old one keeps its own; a blended length near 4 is flagged
    illum[..., :3] = rng.uniform(0.5, 1.5, (H, W, 1))
    illum[..., 3] = np.where(np.arange(W)[None, :] % 2 == 0, 2.0, 6.0)
    v0 = SM.variance_in(illum.astype(np.float64), var.astype(np.float64), guide.astype(np.float64), None, 0.0, 0)[0]
    assert np.array_equal(v0[:, 1::2], var[:, 1::2].astype(np.float64)) and (v0[:, 6::2] > 0).all()
    illum[2, 2, 3] = F(3.9999998)
    margins = []
    SM.filter(illum, var, guide, iterations=1, margins=margins)
    assert not SM.conditioned(margins)


def test_model_object_ids():
    shade = np.arange(5 * 32, dtype=np.uint32).reshape(5, 32)
    ident = np.zeros((2, 3, 4), np.uint32)
    ident[..., 0] = [[0, 4, SM.NONE], [5, 2, 1 << 27]]
    for what in range(3):
        got = SM.object_ids(shade, ident, what)
        assert got.tolist() == [[24 + what, 4 * 32 + 24 + what, SM.NONE], [SM.NONE, 2 * 32 + 24 + what, SM.NONE]]
