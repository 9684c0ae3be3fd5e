"""GPU (-m gpu): pbrhip_scene_object_ids, pbrhip_svgf_accumulate and pbrhip_svgf_filter against the float64 model of
tests/_svgf_model.py within its derived rounding bounds, their exact properties, the bit-for-bit tie to pbrhip_temporal_accumulate, the
identity test on the emitter-under-the-ceiling case made deterministic, and the orbiting Cornell sequence the feature exists for.

The two stages are compared stage by stage: the accumulation on synthetic frames and histories, the filter on synthetic accumulation
outputs whose lengths are whole numbers -- both sides then take every decision on the same float32 inputs (the model's docstring says
which decisions those are).  Synthetic inputs are made once per (size, seed) and shared.  The figures the tests print were measured on an
MI355X; DESIGN.md §17 quotes them."""
import os
import sys

import numpy as np
import pytest

import _svgf_model as SM

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
U = 2.0 ** -24
SIZES = [(67, 45, 1), (131, 23, 2)]  # width, height, seed
NORMALS = np.array([[0, 0, 1], [0.6, 0, 0.8], [0, 1, 0], [0.48, 0.6, 0.64], [-0.6, 0.64, 0.48]], np.float64)


@pytest.fixture(scope="module")
def pa():
    import pbrlab_amd as pa
    if pa.device_count() < 1:
        pytest.fail("no HIP device: the GPU tests must run on an MI355X (there is no CPU fallback)")
    pa.set_device(0)
    return pa


def _dev(a, dt=None):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a if dt is None else a.view(dt))).to("cuda:0")


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ------------------------------------------------------------------------------------------------ object ids
_SCENES = {}


def _scene(pa, name, builder):
    """a small Cornell box / a small head of hair, committed with `builder`, with the identity buffer of its centre rays"""
    if (name, builder) not in _SCENES:
        from pbrlab_amd import scenes
        d = (scenes.cornell_scene("ggx", seed=1, monkey_subdiv=2, lucy_nu=64, lucy_nv=8) if name == "cornell"
             else scenes.hair_scene(seed=1, n_strands=300, n_segments=8, head_subdiv=2))
        s = pa.scene_from_desc(d, bvh_builder=builder)
        s.SetCamera((0.3, 0.2, 3.4), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 70.0)
        s.SnapshotPose()
        _SCENES[name, builder] = (s, pa.RenderMotion(s, 67, 45), s.read_slots()[1])
    return _SCENES[name, builder]


@pytest.mark.parametrize("name", ["cornell", "hair"])
def test_object_ids(pa, name):
    """against pbrhip_scene_read_slots' words 24 / 25 / 26; the three builders agree on all three; a forged slot reads nothing; the device
    variant gives the host variant's bits"""
    import torch
    s, ml, shade = _scene(pa, name, 0)
    hit = ml.ident[..., 0] != SM.NONE
    assert hit.sum() > 300 and (~hit).any()
    per_mode = []
    for what in (SM.ID_PRIMITIVE, SM.ID_INSTANCE, SM.ID_GEOM):
        ids = s.ObjectIds(ml, what)
        assert ids.dtype == np.uint32 and ids.shape == (45, 67)
        assert np.array_equal(ids, SM.object_ids(shade, ml.ident, what)) and np.array_equal(ids[hit], shade[ml.ident[..., 0][hit], 24 + what])
        assert (ids[~hit] == SM.NONE).all()
        per_mode.append(ids)
        on = s.ObjectIds(_dev(ml.ident, np.int32), what)
        assert on.dtype == torch.int32 and np.array_equal(on.cpu().numpy().view(np.uint32), ids)
        given = torch.full((45, 67), 7, dtype=torch.int32, device="cuda:0")
        assert s.ObjectIds(_dev(ml.ident, np.int32), what, device_out=given) is given and np.array_equal(given.cpu().numpy().view(np.uint32), ids)
    assert len(np.unique(per_mode[1][hit])) >= 3  # several instances in view: the buffer is an object matte
    for builder in (1, 2):
        so, mlo, _ = _scene(pa, name, builder)
        for what in range(3):
            assert np.array_equal(so.ObjectIds(mlo, what), per_mode[what]), (builder, what)
    # a forged slot index >= the slot count: NONE, and nothing is read
    n = len(shade)
    forged = ml.ident.copy()
    forged[0, :4, 0] = (n, n + 12345, 0x7FFFFFFF, 0xFFFFFFFE)
    forged[1, 0, 0] = n - 1
    for f in (forged, _dev(forged, np.int32)):
        got = s.ObjectIds(f, SM.ID_INSTANCE)
        got = got if isinstance(got, np.ndarray) else got.cpu().numpy().view(np.uint32)
        assert (got[0, :4] == SM.NONE).all() and got[1, 0] == shade[n - 1, 25] and np.array_equal(got[2:], per_mode[1][2:])
    with pytest.raises(ValueError):
        s.ObjectIds(ml, 3)


# ------------------------------------------------------------------------------------------------ synthetic accumulation inputs
_MADE = {}


def _features(pa, rng, region, w, h):
    """a FeatureLayer: random albedo, partly covered pixels, a region of black albedo, the background without hits"""
    feat = pa.FeatureLayer(w, h)
    spp = rng.randint(1, 9, (h, w)).astype(np.uint32)
    hits = np.where(region == 0, 0, spp)
    hits = np.where((region == 3) & (rng.rand(h, w) < 0.3), np.maximum(hits // 2, 1), hits)
    alb = rng.uniform(0.05, 0.95, (h, w, 3))
    alb[region == 4] = 0.0
    feat.albedo[..., :3] = alb * hits[..., None]
    feat.albedo[..., 3] = hits
    feat.count[...] = spp
    return feat


def _synthetic(pa, w, h, seed, max_history=8):
    """test_temporal_gpu._synthetic's construction, made here: planes of distinct normals and depths in the frame and -- shifted -- in the
    history, background, count == 0 holes, history holes, motions that leave the frame, a curve region; on top of it object ids (two per
    plane, so that the id test rejects taps the other tests accept), a history variance and a FeatureLayer.  Re-drawn from the next seed
    until no input lies near a decision threshold."""
    if (w, h, seed, max_history) in _MADE:
        return _MADE[w, h, seed, max_history]
    rng = np.random.RandomState(seed)
    params = dict(alpha_min=0.05, sigma_depth=0.1, normal_cos_min=0.9, max_history=max_history)
    yy, xx = np.mgrid[0:h, 0:w]
    for tries in range(50):
        region = ((xx * 5) // w + 2 * ((yy * 3) // h)) % 5   # 0 = background
        region_h = (((xx + 3) * 5) // w + 2 * (((yy + 1) * 3) // h)) % 5
        layer = pa.RenderLayer(w, h)
        spp = np.where(rng.rand(h, w) < 0.03, 0, rng.randint(1, 9, (h, w))).astype(np.uint32)
        layer.rgba[..., :3] = rng.uniform(0.0, 2.0, (h, w, 3)) * spp[..., None]
        layer.rgba[..., 3] = spp
        layer.count[...] = spp

        def guide_of(reg):
            n = NORMALS[reg] + 0.02 * rng.normal(size=(h, w, 3))
            n /= np.linalg.norm(n, axis=-1, keepdims=True)
            g = np.concatenate([n, (2.0 + reg + 0.01 * xx + rng.uniform(0, 0.05, (h, w)))[..., None]], -1)
            return np.where((reg == 0)[..., None], 0.0, g).astype(F)
        guide, hist_guide = guide_of(region), guide_of(region_h)
        motion = np.zeros((h, w, 4), F)
        motion[..., 0] = rng.uniform(-4.0, 2.0, (h, w)) + np.where(xx > w - 6, 9.0, 0.0)
        motion[..., 1] = rng.uniform(-1.5, 1.5, (h, w)) - np.where(yy < 2, 3.0, 0.0)
        motion[..., 2] = guide[..., 3] * rng.choice([1.0, 1.0, 1.0, 1.3], (h, w)) + rng.uniform(-0.03, 0.03, (h, w))
        motion[..., 3] = np.where(region == 0, 0.0, np.where(region == 4, 2.0, 1.0))
        for _ in range(100):
            fx, fy = SM.TM._taps(motion, w, h)[:2]
            bad = (np.minimum(fx, 1 - fx) < 2e-3) | (np.minimum(fy, 1 - fy) < 2e-3)
            if not bad.any():
                break
            motion[..., 0][bad] += rng.uniform(0.1, 0.4, bad.sum()).astype(F)
            motion[..., 1][bad] += rng.uniform(0.1, 0.4, bad.sum()).astype(F)
        hist = np.zeros((h, w, 4), F)
        hist[..., :3] = rng.uniform(0.0, 2.0, (h, w, 3))
        hist[..., 3] = np.where(rng.rand(h, w) < 0.05, 0.0, np.where(rng.rand(h, w) < 0.5, max_history, rng.randint(1, max_history + 1, (h, w))))
        hist_var = rng.uniform(0.0, 0.5, (h, w)).astype(F)
        ids = np.where(region == 0, SM.NONE, region * 2 + (yy // 6) % 2).astype(np.uint32)
        hist_ids = np.where(region_h == 0, SM.NONE, region_h * 2 + ((yy + 2) // 6) % 2).astype(np.uint32)
        feat = _features(pa, rng, region, w, h)
        margins = []
        SM.accumulate(layer.rgba, layer.count, motion, guide, hist, hist_var, hist_guide, margins=margins, **params)
        if SM.conditioned(margins):
            out = dict(layer=layer, ml=pa.MotionLayer(motion, guide, None), hist=pa.SvgfHistory(hist, hist_var, hist_guide, hist_ids), ids=ids,
                       feat=feat, params=params, tries=tries + 1)
            _MADE[w, h, seed, max_history] = out
            return out
        rng = np.random.RandomState(rng.randint(1 << 30))
    raise AssertionError("no conditioned input in 50 draws")


def _e32(layer, feat):
    """e = (rgb / count) / max(a, 1e-3) in float32, operation for operation"""
    with np.errstate(invalid="ignore", divide="ignore"):
        c = (layer.rgba[..., :3] / layer.count[..., None].astype(F)).astype(F)
        if feat is None:
            return c
        fm = feat.count.astype(F)
        a = ((feat.albedo[..., :3] + (fm - feat.albedo[..., 3])[..., None]) / fm[..., None]).astype(F)
        a = np.where((feat.count > 0)[..., None], a, F(1.0))
        return (c / np.maximum(a, F(1e-3))).astype(F)


# ------------------------------------------------------------------------------------------------ accumulate, exact
@pytest.mark.parametrize("case", SIZES)
def test_accumulate_without_ids_and_albedo_is_temporal_accumulate_bit_for_bit(pa, case):
    w, h, seed = case
    s = _synthetic(pa, w, h, seed)
    hist = s["hist"]
    got = pa.SvgfAccumulate(s["layer"], s["ml"], pa.SvgfHistory(hist.illum, hist.var, hist.guide), **s["params"])
    want = pa.TemporalAccumulate(s["layer"], s["ml"], pa.TemporalHistory(hist.illum, hist.guide), **s["params"])
    assert np.array_equal(_bits(got.illum), _bits(want.rgba)) and (want.rgba[..., 3] > 1).sum() > 100
    assert got.guide is s["ml"].guide and got.ids is None and got.var.shape == (h, w)
    none = pa.SvgfAccumulate(s["layer"], s["ml"], None, **s["params"])
    assert np.array_equal(_bits(none.illum), _bits(pa.TemporalAccumulate(s["layer"], s["ml"], None, **s["params"]).rgba)) and (none.var == 0).all()


@pytest.mark.parametrize("case", SIZES)
def test_accumulate_exact_properties(pa, case):
    """rejected and history-less pixels are (e, 1) with variance 0 to the bit, holes zero, the variance never negative; a constant colour
    keeps its variance within the bound's value for it; the device variant gives the host variant's bits"""
    w, h, seed = case
    s = _synthetic(pa, w, h, seed)
    layer, ml, hist, ids, feat, params = (s[k] for k in ("layer", "ml", "hist", "ids", "feat", "params"))
    for f, i in ((None, None), (feat, ids)):
        got = pa.SvgfAccumulate(layer, ml, hist, f, i, **params)
        e = _e32(layer, f)
        live, fresh = layer.count > 0, (got.illum[..., 3] == 1) & (layer.count > 0)
        assert fresh.sum() > 10 and (got.illum[..., 3] > 1).sum() > 10
        assert np.array_equal(_bits(got.illum[fresh][:, :3]), _bits(e[fresh])) and (got.var[fresh] == 0).all()
        assert (got.illum[~live] == 0).all() and (got.var[~live] == 0).all() and (~live).any()
        assert (got.var >= 0).all() and (got.var > 0).any()
        none = pa.SvgfAccumulate(layer, ml, None, f, i, **params)
        assert np.array_equal(_bits(none.illum[live][:, :3]), _bits(e[live])) and (none.illum[live][:, 3] == 1).all() and (none.var == 0).all()
        assert none.ids is i
        # on tensors: the same bits
        tl = type("L", (), dict(rgba=_dev(layer.rgba), count=_dev(layer.count, np.int32)))()
        tf = None if f is None else type("Ft", (), dict(albedo=_dev(f.albedo), count=_dev(f.count, np.int32)))()
        th = pa.SvgfHistory(_dev(hist.illum), _dev(hist.var), _dev(hist.guide), None if i is None else _dev(hist.ids, np.int32))
        on = pa.SvgfAccumulate(tl, pa.MotionLayer(_dev(ml.motion), _dev(ml.guide), None), th, tf, None if i is None else _dev(i, np.int32), **params)
        assert np.array_equal(_bits(on.illum.cpu().numpy()), _bits(got.illum)) and np.array_equal(_bits(on.var.cpu().numpy()), _bits(got.var))
    # a constant colour in the frame and in the history, history variance 0: the exact variance is 0
    const = pa.RenderLayer(w, h)
    const.count[...] = layer.count
    const.rgba[..., :3] = np.array([0.25, 0.5, 1.0], F) * layer.count[..., None].astype(F)  # (sums whose mean is the colour exactly)
    ch = hist.illum.copy()
    ch[..., :3] = (0.25, 0.5, 1.0)
    zero = np.zeros((h, w), F)
    got = pa.SvgfAccumulate(const, ml, pa.SvgfHistory(ch, zero, hist.guide), **params)
    bound = []
    SM.accumulate(const.rgba, const.count, ml.motion, ml.guide, ch, zero, hist.guide, bound=bound, **params)
    print(f"{w}x{h}: a constant colour: max variance {got.var.max():.3e}, its bound {bound[0][1].max():.3e}")
    assert (got.var <= bound[0][1]).all() and bound[0][1].max() < 1e-6  # (second order: the square of the blend's own bound)


def test_accumulate_identity_test_keeps_the_neighbour_out(pa):
    """Two regions of equal depth and normal, different id and colour -- the emitter flush under the ceiling -- and a motion that lays
    every footprint across their border.  With ids every output pixel of a region lies within [min, max] of that region's inputs and
    history (4 u of the range's largest value for the roundings of a convex combination); without, the same pixels leave the interval."""
    for w, h in ((67, 45), (131, 23)):
        rng = np.random.RandomState(w)
        yy, xx = np.mgrid[0:h, 0:w]
        A = xx < w // 2
        guide = np.zeros((h, w, 4), F)
        guide[..., :3], guide[..., 3] = (0.0, -1.0, 0.0), 3.0
        motion = np.zeros((h, w, 4), F)
        motion[..., 0] = (w // 2 - 1 - xx) + rng.uniform(0.3, 0.7, (h, w))   # x0 = w/2 - 1, the last column of A; x0 + 1 the first of B
        motion[..., 1] = rng.uniform(-0.4, 0.4, (h, w))
        motion[..., 2], motion[..., 3] = 3.0, 1.0
        ids = np.where(A, 11, 22).astype(np.uint32)
        layer = pa.RenderLayer(w, h)
        layer.count[...] = 2
        layer.rgba[..., :3] = np.where(A[..., None], rng.uniform(0.2, 0.4, (h, w, 3)), rng.uniform(5.0, 6.0, (h, w, 3))) * 2
        hist = np.zeros((h, w, 4), F)
        hist[..., :3] = np.where(A[..., None], rng.uniform(0.2, 0.4, (h, w, 3)), rng.uniform(5.0, 6.0, (h, w, 3)))
        hist[..., 3] = rng.randint(3, 9, (h, w))
        var = rng.uniform(0, 0.1, (h, w)).astype(F)
        ml = pa.MotionLayer(motion, guide, None)
        par = dict(alpha_min=0.1, max_history=16)
        with_ids = pa.SvgfAccumulate(layer, ml, pa.SvgfHistory(hist, var, guide, ids), ids=ids, **par)
        without = pa.SvgfAccumulate(layer, ml, pa.SvgfHistory(hist, var, guide), **par)
        e = (layer.rgba[..., :3] / F(2)).astype(F)
        for reg in (A, ~A):
            lo = min(e[reg].min(), hist[reg][:, :3].min())
            hi = max(e[reg].max(), hist[reg][:, :3].max())
            tol = 4 * U * hi
            inside = (with_ids.illum[reg][:, :3] >= lo - tol) & (with_ids.illum[reg][:, :3] <= hi + tol)
            assert inside.all() and (with_ids.illum[reg][:, 3] > 1).all()
            out = without.illum[reg][:, :3]
            assert ((out < lo - tol) | (out > hi + tol)).all()


@pytest.mark.parametrize("case", SIZES)
def test_accumulate_against_the_float64_model(pa, case):
    """|gpu - model| <= the bound _svgf_model.accumulate derives, for out_illum and out_var, with and without ids and albedo"""
    w, h, seed = case
    s = _synthetic(pa, w, h, seed)
    layer, ml, hist, ids, feat, params = (s[k] for k in ("layer", "ml", "hist", "ids", "feat", "params"))
    assert s["tries"] <= 8
    for f, i in ((None, None), (feat, None), (None, ids), (feat, ids)):
        bound = []
        want, wvar = SM.accumulate(layer.rgba, layer.count, ml.motion, ml.guide, hist.illum, hist.var, hist.guide, bound=bound,
                                   albedo_hits=None if f is None else f.albedo, feature_count=None if f is None else f.count,
                                   ids=i, hist_ids=None if i is None else hist.ids, **params)
        got = pa.SvgfAccumulate(layer, ml, hist, f, i, **params)
        err, ev, (B, Bv) = np.abs(got.illum - want), np.abs(got.var - wvar), bound[0]
        blended = want[..., 3] > 1
        print(f"{w}x{h} albedo={f is not None} ids={i is not None} (draw {s['tries']}): {blended.sum()} blended pixels; max error illum {err[..., :3].max():.3e} "
              f"(worst error / bound {(err / np.maximum(B, 1e-300))[B > 0].max():.3f}), var {ev.max():.3e} ({(ev / np.maximum(Bv, 1e-300))[Bv > 0].max():.3f})")
        assert blended.sum() > 50 and (err <= B).all() and (ev <= Bv).all()
        if i is not None:
            assert blended.sum() < (SM.accumulate(layer.rgba, layer.count, ml.motion, ml.guide, hist.illum, hist.var, hist.guide, **params)[0][..., 3] > 1).sum()


# ------------------------------------------------------------------------------------------------ the filter
def _filter_input(pa, w, h, seed, max_history=8):
    """what an accumulation hands the filter: planes of distinct normals, depths and ids (two ids per plane), a background region, pixels
    that are not live, whole-number lengths 1 .. max_history, a piecewise smooth illumination under noise of relative standard deviation
    0.05 .. 0.3, and a variance that says so where len >= 4"""
    key = ("filter", w, h, seed)
    if key not in _MADE:
        rng = np.random.RandomState(seed + 100)
        yy, xx = np.mgrid[0:h, 0:w]
        region = ((xx * 5) // w + 2 * ((yy * 3) // h)) % 5
        n = NORMALS[region] + 0.02 * rng.normal(size=(h, w, 3))
        n /= np.linalg.norm(n, axis=-1, keepdims=True)
        guide = np.concatenate([n, (2.0 + region + 0.01 * xx + 0.02 * yy * (region % 2))[..., None]], -1)
        guide = np.where((region == 0)[..., None], 0.0, guide).astype(F)
        ids = np.where(region == 0, SM.NONE, region * 2 + (yy // 6) % 2).astype(np.uint32)
        ln = np.where(rng.rand(h, w) < 0.04, 0, rng.randint(1, max_history + 1, (h, w)))
        rel = rng.uniform(0.05, 0.3, (h, w))
        base = np.array([[0.8, 0.8, 0.8], [1.5, 0.4, 0.3], [0.2, 0.9, 0.4], [0.3, 0.3, 1.8], [1.0, 0.7, 0.1]])[region] * (1 + 0.3 * np.sin(0.2 * xx))[..., None]
        illum = np.concatenate([base * (1 + rel[..., None] * rng.normal(size=(h, w, 3))).clip(0.1, 3.0), ln[..., None]], -1).astype(F)
        var = ((rel * SM.lum(base)) ** 2).astype(F)
        _MADE[key] = dict(hist=pa.SvgfHistory(illum, var, guide, ids), feat=_features(pa, rng, region, w, h), region=region)
    return _MADE[key]


@pytest.mark.parametrize("iterations", [1, 3, 5])
@pytest.mark.parametrize("case", SIZES)
def test_filter_against_the_float64_model(pa, case, iterations):
    """|gpu - model| <= the bound _svgf_model.filter propagates through the iterations, for out_rgba and out_feedback, with and without
    ids and albedo"""
    w, h, seed = case
    s = _filter_input(pa, w, h, seed)
    hist, feat = s["hist"], s["feat"]
    live = hist.illum[..., 3] > 0
    assert (hist.illum[..., 3][live] < 4).sum() > 100 and (hist.illum[..., 3] >= 4).sum() > 100 and (~live).sum() > 10
    for f, use_ids in ((None, False), (feat, False), (None, True), (feat, True)):
        margins, bound = [], []
        want, wfb = SM.filter(hist.illum, hist.var, hist.guide, hist.ids if use_ids else None, None if f is None else f.albedo,
                              None if f is None else f.count, iterations, margins=margins, bound=bound)
        assert SM.conditioned(margins)
        got, fb = pa.SvgfFilter(hist, f, iterations=iterations, use_ids=use_ids, feedback=True)
        (B, Bf), err, ef = bound[0], np.abs(got - want), np.abs(fb.illum - wfb)
        print(f"{w}x{h} it={iterations} albedo={f is not None} ids={use_ids}: max error rgba {err.max():.3e}, bound there "
              f"{B.reshape(-1)[err.argmax()]:.3e}, worst error / bound {(err / np.maximum(B, 1e-300))[B > 0].max():.3f}; feedback {ef.max():.3e} "
              f"({(ef / np.maximum(Bf, 1e-300))[Bf > 0].max():.3f}); largest bound {B.max():.3e}")
        assert (err <= B).all() and (ef <= Bf).all()
        assert B.max() < 0.05 * np.abs(want).max()  # (the bound says something: it stays below the 5 % noise the inputs carry at the least)
        assert fb.var is hist.var and fb.guide is hist.guide and fb.ids is hist.ids


def _ulp_close(a, b, ulps=2):
    a, b = np.asarray(a, F), np.asarray(b, F)
    return (np.abs(a.astype(np.float64) - b) <= ulps * np.spacing(np.abs(b).astype(F))).all()


@pytest.mark.parametrize("case", SIZES)
def test_filter_exact_properties(pa, case):
    w, h, seed = case
    s = _filter_input(pa, w, h, seed)
    hist, feat = s["hist"], s["feat"]
    live = hist.illum[..., 3] > 0
    fm = feat.count.astype(F)
    a = np.maximum(((feat.albedo[..., :3] + (fm - feat.albedo[..., 3])[..., None]) / fm[..., None]).astype(F), F(1e-3))
    # pixels that are not live come out zero, in both outputs, and influence nobody
    out, fb = pa.SvgfFilter(hist, feat, feedback=True)
    assert (out[~live] == 0).all() and (fb.illum[~live] == 0).all() and (out[live][:, 3] == 1).all()
    assert np.array_equal(fb.illum[..., 3], hist.illum[..., 3])
    loud = hist.illum.copy()
    loud[~live, :3] = 1e6
    assert np.array_equal(_bits(pa.SvgfFilter(pa.SvgfHistory(loud, hist.var, hist.guide, hist.ids), feat)), _bits(out))
    # a constant illumination returns to 2 ulp times the albedo
    const = hist.illum.copy()
    const[..., :3] = (0.3, 0.6, 0.9)
    got = pa.SvgfFilter(pa.SvgfHistory(const, hist.var, hist.guide, hist.ids), feat)
    assert _ulp_close(got[live][:, :3], (const[..., :3] * a)[live])
    assert _ulp_close(pa.SvgfFilter(pa.SvgfHistory(const, hist.var, hist.guide), None, sigma_lum=0.0)[live][:, :3], const[live][:, :3], 0)
    # one iteration: the feedback is the output with the albedo taken out again
    out1, fb1 = pa.SvgfFilter(hist, feat, iterations=1, feedback=True)
    assert _ulp_close((out1[..., :3] / a)[live], fb1.illum[live][:, :3])
    # the two sides of an id border never mix when the colours are painted by id
    painted = hist.illum.copy()
    painted[..., :3] = (hist.ids % 7 + 1)[..., None].astype(F)
    got = pa.SvgfFilter(pa.SvgfHistory(painted, hist.var, hist.guide, hist.ids), None)
    assert np.array_equal(got[live][:, :3], painted[live][:, :3])
    # the device variant gives the host variant's bits
    th = pa.SvgfHistory(_dev(hist.illum), _dev(hist.var), _dev(hist.guide), _dev(hist.ids, np.int32))
    tf = type("Ft", (), dict(albedo=_dev(feat.albedo), count=_dev(feat.count, np.int32)))()
    on, onfb = pa.SvgfFilter(th, tf, feedback=True)
    assert np.array_equal(_bits(on.cpu().numpy()), _bits(out)) and np.array_equal(_bits(onfb.illum.cpu().numpy()), _bits(fb.illum))
    # refusals reach Python as errors
    with pytest.raises(pa.PbrHipError) as e:
        pa.SvgfFilter(hist, feat, iterations=9)
    assert e.value.code == -1


# ------------------------------------------------------------------------------------------------ end to end
def test_orbiting_cornell_sequence(pa):
    """scripts/bench_temporal.py's orbiting sequence (pose()) on the Lambert + GGX Cornell box, 128 x 128, 8 frames at 4 spp, judged on
    the last frame by that script's rel_mse against 1024 spp:
      (a) on the ceiling's pixels the accumulation with ids is closer to the truth than the same call without;
      (b) over the whole frame accumulate-with-ids + filter is closer than the raw frame;
      (c) over the whole frame accumulate-with-ids + filter is closer than accumulate-with-ids alone.
    The three are asserted on the calls as the header says to make them for this scene: SvgfAccumulate(layer, motion, history, ids=ids)
    and SvgfFilter(history), features left at their default None.  The box's light has BLACK albedo, and pbrhip.h's filter block says
    to pass no albedo_hits / feature_count while such an emitter is in view (DESIGN.md section 17 says why: a pixel it covers partly has
    an albedo estimate anywhere between the clamp 1e-3 and the ceiling's 0.8 from one frame's four jittered samples to the next, and a
    history e = c / a made with one frame's a is multiplied by another's).

    The same sequence WITH a FeatureLayer is run beside it and its figures are printed, because it is where this pipeline loses.  Of
    the three inequalities only (a) holds there, and it is asserted there too; (b) and (c) do NOT hold with albedo on this scene and
    are not asserted for it.

    Measured on an MI355X.  Without a FeatureLayer: the ceiling's 1726 pixels 0.0468 with ids against 0.4622 without; whole frame raw
    0.0371, accumulated with ids 0.0097, accumulated with ids + filtered 0.0051.  With one: the ceiling 113.1 with ids against 82063
    without; whole frame accumulated with ids 155.4, accumulated with ids + filtered 237.5."""
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        import bench_temporal as BT
    finally:
        sys.path.pop(0)
    from pbrlab_amd import scenes
    s = pa.scene_from_desc(scenes.cornell_scene("ggx", seed=1))
    n, spp, size = 8, 4, 128
    layer = pa.RenderLayer()
    h_ids = h_plain = ha_ids = ha_plain = None
    BT.pose(pa, s, 0, n)
    s.RefitScene()
    for k in range(n):
        s.SnapshotPose()
        BT.pose(pa, s, k, n)
        s.RefitScene()
        pa.Render(s, size, size, spp, layer=layer, first_pass=spp * k)
        ml = pa.RenderMotion(s, size, size)
        feat = pa.RenderFeatures(s, size, size, spp, first_pass=spp * k)
        ids = s.ObjectIds(ml, SM.ID_INSTANCE)
        h_ids = pa.SvgfAccumulate(layer, ml, h_ids, None, ids)
        h_plain = pa.SvgfAccumulate(layer, ml, h_plain, None, None)
        ha_ids = pa.SvgfAccumulate(layer, ml, ha_ids, feat, ids)        # (beside the three: the same calls with albedo)
        ha_plain = pa.SvgfAccumulate(layer, ml, ha_plain, feat, None)
    ref = pa.RenderLayer()
    pa.Render(s, size, size, 1024, layer=ref, first_pass=1 << 20)
    truth = ref.rgba[..., :3].astype(np.float64) / 1024
    raw = layer.rgba[..., :3].astype(np.float64) / spp
    ceiling = ids == BT.CEILING

    def figures(acc_ids, acc_plain, filtered):
        return dict(ceiling_with_ids=BT.rel_mse(acc_ids, truth, ceiling), ceiling_without_ids=BT.rel_mse(acc_plain, truth, ceiling),
                    raw=BT.rel_mse(raw, truth), accumulated=BT.rel_mse(acc_ids, truth), filtered=BT.rel_mse(filtered, truth))

    def show(what, e):
        print(f"{what}: the ceiling's {ceiling.sum()} pixels accumulated with ids {e['ceiling_with_ids']:.5f}, without "
              f"{e['ceiling_without_ids']:.5f}; whole frame raw {e['raw']:.5f}, accumulated with ids {e['accumulated']:.5f}, accumulated with ids + "
              f"filtered {e['filtered']:.5f}")

    print(f"frame {n} of the orbit, {size} x {size}, {spp} spp, relative MSE against 1024 spp")
    e = figures(h_ids.illum[..., :3].astype(np.float64), h_plain.illum[..., :3].astype(np.float64),
                pa.SvgfFilter(h_ids)[..., :3].astype(np.float64))
    show("without a FeatureLayer (albedo 1)", e)
    a = SM.albedo(feat.albedo, feat.count, (size, size))
    ea = figures(ha_ids.illum[..., :3].astype(np.float64) * a, ha_plain.illum[..., :3].astype(np.float64) * a,
                 pa.SvgfFilter(ha_ids, feat)[..., :3].astype(np.float64))
    show("with a FeatureLayer", ea)
    assert ceiling.sum() > 200 and truth.max() > 0
    assert e["ceiling_with_ids"] < e["ceiling_without_ids"]   # (a)
    assert e["filtered"] < e["raw"]                          # (b)
    assert e["filtered"] < e["accumulated"]                  # (c)
    assert ea["ceiling_with_ids"] < ea["ceiling_without_ids"]  # (a) with albedo; (b) and (c) do not hold there, see above
