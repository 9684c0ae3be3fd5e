"""Motion vectors and temporal accumulation without a GPU: the symbols and Python names exist, the ABI version stands, bad
arguments are refused before any device work, and the float64 model of tests/_temporal_model.py agrees with itself and closed forms."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _temporal_model as TM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("pbrhip_scene_snapshot_pose", "pbrhip_render_motion", "pbrhip_render_motion_device", "pbrhip_temporal_accumulate",
           "pbrhip_temporal_accumulate_device")
EINVAL, ENODEVICE = -1, -3


def test_symbols_and_names_exist():
    import pbrlab_amd as pa
    from pbrlab_amd import _lib, api
    L = _lib.lib()
    hdr = open(os.path.join(ROOT, "include", "pbrhip.h")).read()
    for name in SYMBOLS:
        assert name in _lib.EXPORTS and hasattr(L, name) and re.search(r"\b" + name + r"\s*\(", hdr), name
    for name in ("MotionLayer", "TemporalHistory", "RenderMotion", "TemporalAccumulate"):
        assert hasattr(api, name) and hasattr(pa, name), name
    assert hasattr(pa.Scene, "SnapshotPose")
    assert L.pbrhip_abi_version() == 6 and re.search(r"#define PBRHIP_ABI_VERSION 6u\b", hdr)
    # the header's defaults are the binding's
    for macro, value in (("ALPHA_MIN", api.TEMPORAL_ALPHA_MIN), ("SIGMA_DEPTH", api.TEMPORAL_SIGMA_DEPTH),
                         ("NORMAL_COS_MIN", api.TEMPORAL_NORMAL_COS_MIN), ("MAX_HISTORY", api.TEMPORAL_MAX_HISTORY)):
        m = re.search(r"#define PBRHIP_TEMPORAL_" + macro + r" ([0-9.]+)[fu]", hdr)
        assert m and float(m.group(1)) == float(value), macro


def test_bad_arguments_are_refused_before_any_device_work():
    from pbrlab_amd import _lib, api
    L = _lib.lib()
    W, H = 8, 4
    img = [np.zeros((H, W, 4), np.float32) for _ in range(6)]
    rgba, motion, guide, hr, hg, out = (a.ctypes.data for a in img)
    count = np.ones((H, W), np.uint32)
    par = (C.c_float(0.1), C.c_float(0.05), C.c_float(0.9), 32)
    nan = C.c_float(float("nan"))

    def refused(args, word=b""):
        for f in (L.pbrhip_temporal_accumulate, L.pbrhip_temporal_accumulate_device):
            rc = f(*args)
            assert rc == EINVAL and word in L.pbrhip_last_error(), (rc, L.pbrhip_last_error())

    good = [0, W, H, rgba, count.ctypes.data, motion, guide, hr, hg, *par, out]
    for k in (3, 4, 5, 6, 13):  # NULL rgba, count, motion, guide, out_rgba
        refused(good[:k] + [None] + good[k + 1:], b"NULL")
    refused(good[:7] + [None, hg] + good[9:], b"together")  # half a history pair
    refused(good[:7] + [hr, None] + good[9:], b"together")
    for k in (9, 10, 11):
        refused(good[:k] + [nan] + good[k + 1:], b"NaN")
    refused(good[:12] + [0] + good[13:], b"max_history")
    refused([0, 0, H] + good[3:], b"empty")
    refused([0, W, 0] + good[3:], b"empty")
    refused(good[:13] + [hr], b"hist_rgba")  # in place
    # the scene calls: NULL scene, NULL descriptor
    desc = api._desc(W, H, 1)
    fake = C.c_void_p(16)  # never dereferenced
    assert L.pbrhip_scene_snapshot_pose(None) == EINVAL
    for f in (L.pbrhip_render_motion, L.pbrhip_render_motion_device):
        assert f(None, C.byref(desc), motion, guide, None) == EINVAL and b"NULL" in L.pbrhip_last_error()
        assert f(fake, None, motion, guide, None) == EINVAL and b"NULL" in L.pbrhip_last_error()


def test_python_refuses_mixed_and_misshapen_buffers():
    import pbrlab_amd as pa
    layer = pa.RenderLayer(8, 4)
    m = pa.MotionLayer(np.zeros((4, 8, 4), np.float32), np.zeros((4, 9, 4), np.float32), None)
    with pytest.raises(ValueError):
        pa.TemporalAccumulate(layer, m)


def test_fails_loudly_without_device():
    import pbrlab_amd as pa
    if pa.device_count() > 0:
        pytest.skip("a GPU is present")
    layer = pa.RenderLayer(8, 4)
    layer.count[...] = 1
    m = pa.MotionLayer(np.zeros((4, 8, 4), np.float32), np.zeros((4, 8, 4), np.float32), None)
    with pytest.raises(pa.PbrHipError) as e:
        pa.TemporalAccumulate(layer, m)
    assert e.value.code == ENODEVICE
    h = pa.TemporalHistory(np.ones((4, 8, 4), np.float32), m.guide).layer()
    assert h.count.all() and (h.rgba[..., 3] == 1).all()


# ---------------------------------------------------------------------------------------------------- the float64 model
def _random_cameras(rng, W, H):
    eye = rng.uniform(-3, 3, 3)
    cams = [TM.user_camera(eye, eye + rng.normal(size=3), (0.1, 1.0, 0.2), rng.uniform(20, 100), W, H)]
    lo = rng.uniform(-2, 0, 3)
    cams.append(TM.reference_camera(lo, lo + rng.uniform(0.5, 3, 3), W, H))
    return cams


@pytest.mark.parametrize("size", [(67, 45), (40, 96)])
def test_model_projection_inverts_the_centre_rays(size):
    """project(a point on the centre ray of pixel (x, y)) = (x + 0.5, y + 0.5): the rays are float32 (u = 2^-24 per operation, a dozen
    operations, amplified by the image size), the inverse float64"""
    W, H = size
    rng = np.random.RandomState(W)
    for _ in range(4):
        for cam in _random_cameras(rng, W, H):
            o, d = TM.centre_rays(cam, W, H)
            assert o.dtype == np.float32 and d.dtype == np.float32
            assert np.abs(np.sqrt((d.astype(np.float64) ** 2).sum(-1)) - 1).max() < 4 * TM.EPS
            t = rng.uniform(0.5, 20.0, (H, W))
            X = o.astype(np.float64) + t[..., None] * d.astype(np.float64)
            px, py, dist, front = TM.project(cam, X, W, H)
            y, x = np.mgrid[0:H, 0:W]
            assert front.all()
            assert np.abs(px - (x + 0.5)).max() < 64 * TM.EPS * max(W, H) and np.abs(py - (y + 0.5)).max() < 64 * TM.EPS * max(W, H)
            assert np.abs(dist / t - 1).max() < 16 * TM.EPS
            # behind the camera: not in front
            back = TM.project(cam, o.astype(np.float64) - t[..., None] * d.astype(np.float64), W, H)[3]
            assert not back.any()


def test_model_x_prev_and_motion_of_a_translation():
    """a triangle and a curve piece moved by one vector: X_prev is the hit's point minus that vector, the motion its projection"""
    W, H = 32, 16
    cam = TM.user_camera((0, 0, 5), (0, 0, 0), (0, 1, 0), 90.0, W, H)
    slots = np.zeros((2, 4, 4), np.float32)
    slots[0, :3, :3] = [(-4, -4, 0), (4, -4, 0), (-4, 4, 0)]
    slots[1, 0], slots[1, 1] = (1, 1, 1, 0.1), (2, 1, 1, 0.1)
    slots[1, 2, 0] = np.array([2], np.uint32).view(np.float32)[0]  # piece 2 of its cubic: u in [0.5, 0.75]
    shade = np.zeros((2, 32), np.uint32)
    shade[1, 3] = 2 << 24  # kSlotIsCurve
    ident = np.zeros((H, W, 4), np.uint32)
    ident[..., 0] = TM.NONE
    f = lambda v: np.array([v], np.float32).view(np.uint32)[0]  # noqa: E731
    ident[3, 5] = (0, f(0.25), f(0.5), f(5.0))
    ident[4, 6] = (1, f(0.625), f(0.0), f(4.0))
    X, hit, curve = TM.x_prev(slots, shade, ident)
    assert hit.sum() == 2 and curve[4, 6] and not curve[3, 5]
    assert np.allclose(X[3, 5], (-4 + 0.25 * 8, -4 + 0.5 * 8, 0)) and np.allclose(X[4, 6], (1.5, 1, 1))
    m = TM.motion(slots, shade, ident, cam, W, H)
    assert (m[~hit] == 0).all() and m[3, 5, 3] == 1 and m[4, 6, 3] == 2
    # (-2, 0, 0) seen from (0, 0, 5) at 90 degrees: sx = -2 / 5, ha = 2 -> px = (1 - 0.2) 16
    assert np.isclose(m[3, 5, 0] + 5.5, 0.8 * 16) and np.isclose(m[3, 5, 1] + 3.5, 8.0) and np.isclose(m[3, 5, 2], np.sqrt(29.0))


def test_model_accumulation_is_the_running_mean():
    """zero motion, identical guides, full history: frame k of a constant-guide sequence holds the mean of the k frames, length k, until
    max_history or alpha_min caps the window"""
    W, H, K = 9, 7, 6
    rng = np.random.RandomState(3)
    guide = np.zeros((H, W, 4), np.float32)
    guide[..., 2], guide[..., 3] = 1.0, 3.0
    motion = np.zeros((H, W, 4), np.float32)
    motion[..., 2], motion[..., 3] = 3.0, 1.0
    count = np.full((H, W), 2, np.uint32)
    frames = rng.uniform(0, 2, (K, H, W, 3))
    hist = None
    for k in range(K):
        rgba = np.concatenate([frames[k] * 2, np.full((H, W, 1), 2.0)], -1).astype(np.float32)
        out = TM.accumulate(rgba, count, motion, guide, hist, None if hist is None else guide, 0.0, 0.05, 0.9, 4)
        mean = (rgba[..., :3].astype(np.float64) / 2)
        if k == 0:
            run = mean
        else:
            a = 1.0 / min(k + 1, 4)
            run = run + a * (mean - run)
        assert np.allclose(out[..., :3], run, rtol=1e-12, atol=0) and (out[..., 3] == min(k + 1, 4)).all()
        hist = out.astype(np.float32)
        run = hist[..., :3].astype(np.float64)  # (the history travels as float32)
    # a hole, an invalid pixel and a pixel without count
    motion[0, 0, 3] = 0.0
    count[1, 1] = 0
    hist[2, 2, 3] = 0.0
    out = TM.accumulate(rgba, count, motion, guide, hist, guide, 0.0, 0.05, 0.9, 4)
    assert out[0, 0, 3] == 1 and np.array_equal(out[0, 0, :3], rgba[0, 0, :3].astype(np.float64) / 2)
    assert (out[1, 1] == 0).all() and out[2, 2, 3] == 1


def test_model_rejections_and_conditioning():
    W, H = 6, 5
    guide = np.zeros((H, W, 4), np.float32)
    guide[..., 2], guide[..., 3] = 1.0, 2.0
    motion = np.zeros((H, W, 4), np.float32)
    motion[..., :2], motion[..., 2], motion[..., 3] = (0.25, 0.5), 2.0, 1.0
    rgba = np.ones((H, W, 4), np.float32)
    count = np.ones((H, W), np.uint32)
    hist = np.zeros((H, W, 4), np.float32)
    hist[..., :3], hist[..., 3] = 3.0, 5.0
    hg = guide.copy()
    hg[:, 3:, 3] = 4.0          # a depth edge: columns 3.. are another surface
    hg[3:, :3, :3] = (1, 0, 0)  # a normal edge
    margins, bound = [], []
    out = TM.accumulate(rgba, count, motion, guide, hist, hg, 0.2, 0.05, 0.9, 16, margins, bound)
    assert TM.conditioned(margins)
    assert out[0, 0, 3] == 6 and np.allclose(out[0, 0, :3], 3 + 0.2 * (1 - 3))  # a = max(1 / 6, 0.2)
    assert out[0, 3, 3] == 1 and out[4, 0, 3] == 1 and out[0, 5, 3] == 1         # depth, normal, and depth at the border
    assert out[2, 2, 3] == 6  # taps (2, 2) accepted, (3, *) and (*, 3) rejected: the accepted ones renormalised
    assert bound[0].shape == (H, W, 4) and (bound[0] >= 0).all() and bound[0].max() < 1e-4
    # a curve accepts the opposite tangent, a surface does not
    hg2 = guide.copy()
    hg2[..., :3] = (0, 0, -1)
    assert (TM.accumulate(rgba, count, motion, guide, hist, hg2, 0.2, 0.05, 0.9, 16)[..., 3] == 1).all()
    motion[..., 3] = 2.0
    assert (TM.accumulate(rgba, count, motion, guide, hist, hg2, 0.2, 0.05, 0.9, 16)[:4, :5, 3] == 6).all()
    # a fractional part on a pixel centre is flagged
    motion[..., 0] = 1.0
    margins = []
    TM.accumulate(rgba, count, motion, guide, hist, hg, 0.2, 0.05, 0.9, 16, margins)
    assert not TM.conditioned(margins)
