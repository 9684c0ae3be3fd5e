"""GPU (-m gpu): the host variants of the image-space entry points stage their arrays through one helper (image.cpp's Staging); here every
host / device pair of the family gives the same bits on one small frame, with the cases chosen to walk the helper's branches: every
optional pointer given, each optional group null, an output preloaded from the host (PBRHIP_RENDER_NO_CLEAR), and nothing to stage.

The frame is the Cornell box at 20 x 12: a multiple of the 8 x 8 patch in neither direction.  Two frames of it are made once for the module
(the second behind a camera move, so that the first is its history) and shared by the tests.

Asserted elsewhere already, at frame sizes of their own, and not repeated here: with every pointer given, pbrhip_render_features against
its device variant (test_features_gpu.py::test_device_variant_gives_the_host_variants_bits), pbrhip_render_features_emission against its
(test_emission_gpu.py::test_abi_checks, which also walks every subset of the host variant's four buffers), pbrhip_render_motion against
its (test_temporal_gpu.py::test_device_variant_gives_the_host_variants_bits, with each output null on the device), pbrhip_denoise with
and without features (test_denoise_gpu.py::test_device_variant_gives_the_host_variants_bits)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H = 20, 12
SEED = 1234567890
F = np.float32
# eye, lookat, up, fov: from below, so that the light's front fills the top rows and the emission layer is not empty
CAM0 = ((0.3, -0.6, 3.6), (0.0, 0.6, 0.0), (0.0, 1.0, 0.0), 50.0)
CAM1 = ((0.4, -0.55, 3.5), (0.05, 0.6, 0.0), (0.0, 1.0, 0.0), 50.0)


@pytest.fixture(scope="module")
def pa():
    import pbrlab_amd as pa
    if pa.device_count() < 1:
        pytest.fail("no HIP device: the GPU tests must run on an MI355X (there is no CPU fallback)")
    pa.set_device(0)
    return pa


def _bits(a):
    a = a if isinstance(a, np.ndarray) else a.cpu().numpy()
    return np.ascontiguousarray(a).view(np.uint32)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to("cuda:0")


def _bag(**fields):
    return type("Bag", (), fields)()


def _on_layer(layer):
    return _bag(rgba=_dev(layer.rgba), count=_dev(layer.count))


def _on_features(f):
    return None if f is None else _bag(albedo=_dev(f.albedo), normal_depth=_dev(f.normal_depth), count=_dev(f.count))


def _on_motion(pa, ml):
    return pa.MotionLayer(_dev(ml.motion), _dev(ml.guide), None)


@pytest.fixture(scope="module")
def frames(pa):
    """scene, and per frame: RenderLayer, MotionLayer, FeatureLayer, EmissionLayer, instance ids -- all through the host variants"""
    from pbrlab_amd import scenes
    s = pa.scene_from_desc(scenes.cornell_scene("ggx", seed=1, monkey_subdiv=1, lucy_nu=64, lucy_nv=8))
    out = []
    for i, cam in enumerate((CAM0, CAM1)):
        s.SnapshotPose()
        s.SetCamera(*cam)
        layer = pa.RenderLayer()
        pa.Render(s, W, H, 4, layer=layer, first_pass=4 * i, seed_seq=SEED)
        ml = pa.RenderMotion(s, W, H)
        feat, em = pa.RenderFeaturesEmission(s, W, H, 4, first_pass=4 * i, seed_seq=SEED)
        out.append(_bag(layer=layer, ml=ml, feat=feat, em=em, ids=s.ObjectIds(ml)))
    # the frame is not degenerate: reprojected pixels and pixels without a history, emitting samples, hits (of 240 pixels)
    valid = out[1].ml.motion[..., 3] != 0
    assert valid.sum() > 40 and (~valid).any() and (out[1].em.emission[..., 3] > 0).any() and (out[1].feat.albedo[..., 3] > 0).sum() > 40
    yield s, out
    s.close()


# ------------------------------------------------------------------------------------------------ the scene-bound calls
@pytest.mark.parametrize("emission", [False, True])
def test_no_clear_continues_preloaded_sums(pa, frames, emission):
    """two calls of 2 passes, the second on top of the first's sums, are one call of 4: through the host variant, which uploads the sums,
    and through the device variant, which finds them in place"""
    import torch
    s, _ = frames
    if emission:
        one = pa.RenderFeaturesEmission(s, W, H, 4, seed_seq=SEED)
        want = (one[0].albedo, one[0].normal_depth, one[0].count, one[1].emission)
        f, e = pa.RenderFeaturesEmission(s, W, H, 2, seed_seq=SEED)
        assert f.albedo.any() and f.normal_depth.any() and f.count.any() and e.emission.any() and not _same(f.albedo, want[0])
        pa.RenderFeaturesEmission(s, W, H, 2, f, e, first_pass=2, seed_seq=SEED, no_clear=True)
        got = (f.albedo, f.normal_depth, f.count, e.emission)
    else:
        one = pa.RenderFeatures(s, W, H, 4, seed_seq=SEED)
        want = (one.albedo, one.normal_depth, one.count)
        f = pa.RenderFeatures(s, W, H, 2, seed_seq=SEED)
        assert f.albedo.any() and f.normal_depth.any() and f.count.any() and not _same(f.albedo, want[0])
        pa.RenderFeatures(s, W, H, 2, f, first_pass=2, seed_seq=SEED, no_clear=True)
        got = (f.albedo, f.normal_depth, f.count)
    assert all(_same(g, x) for g, x in zip(got, want))
    t = [torch.full((H, W, 4), 3.0, dtype=torch.float32, device="cuda:0") for _ in range(3)]
    c = torch.full((H, W), 9, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    ptrs = (t[0].data_ptr(), t[1].data_ptr(), c.data_ptr()) + ((t[2].data_ptr(),) if emission else ())
    render = pa.RenderFeaturesEmission if emission else pa.RenderFeatures
    render(s, W, H, 2, seed_seq=SEED, device_out=ptrs)
    render(s, W, H, 2, first_pass=2, seed_seq=SEED, no_clear=True, device_out=ptrs)
    assert all(_same(g, x) for g, x in zip((t[0], t[1], c) + ((t[2],) if emission else ()), want))


def test_features_without_albedo(pa, frames):
    """the albedo pointer null, on the host and on the device: the other buffers are what they are with it"""
    import torch
    from pbrlab_amd import api
    s, fr = frames
    want = fr[1]
    desc = api.RenderDesc(W, H, 4, 4, SEED, 0, 1, 0, 0, 0, 0, 0)
    nd, cnt, em = np.full((H, W, 4), 7.0, F), np.full((H, W), 7, np.uint32), np.full((H, W, 4), 7.0, F)
    api._chk(s.L.pbrhip_render_features_emission(s.h, C.byref(desc), None, nd.ctypes.data, cnt.ctypes.data, em.ctypes.data))
    assert _same(nd, want.feat.normal_depth) and _same(cnt, want.feat.count) and _same(em, want.em.emission)
    t = [torch.full((H, W, 4), 3.0, dtype=torch.float32, device="cuda:0") for _ in range(2)]
    c = torch.full((H, W), 9, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    pa.RenderFeaturesEmission(s, W, H, 4, first_pass=4, seed_seq=SEED, device_out=(0, t[0].data_ptr(), c.data_ptr(), t[1].data_ptr()))
    assert _same(t[0], nd) and _same(c, cnt) and _same(t[1], em)
    nd2, cnt2 = np.full((H, W, 4), 7.0, F), np.full((H, W), 7, np.uint32)
    api._chk(s.L.pbrhip_render_features(s.h, C.byref(desc), None, nd2.ctypes.data, cnt2.ctypes.data))
    pa.RenderFeatures(s, W, H, 4, first_pass=4, seed_seq=SEED, device_out=(0, t[0].data_ptr(), c.data_ptr()))
    assert _same(nd2, nd) and _same(cnt2, cnt) and _same(t[0], nd2) and _same(c, cnt2)


@pytest.mark.parametrize("given", [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1)])
def test_motion_outputs_may_be_null_on_the_host(pa, frames, given):
    import torch
    from pbrlab_amd import api
    s, fr = frames
    ml = fr[1].ml
    desc = api.RenderDesc(W, H, 1, 0, 0, 0, 1, 0, 0, 0, 0, 0)
    bufs = [np.full((H, W, 4), 7.0, F), np.full((H, W, 4), 7.0, F), np.full((H, W, 4), 7, np.uint32)]
    api._chk(s.L.pbrhip_render_motion(s.h, C.byref(desc), *[b.ctypes.data if g else None for b, g in zip(bufs, given)]))
    for b, g, want in zip(bufs, given, (ml.motion, ml.guide, ml.ident)):
        assert _same(b, want) if g else (b == 7).all()
    out = [_dev(np.full((H, W, 4), 7.0, F)) if g else None for g in given[:2]] + [_dev(np.full((H, W, 4), 7, np.int32)) if given[2] else None]
    torch.cuda.synchronize()
    pa.RenderMotion(s, W, H, device_out=out)
    assert all(_same(o, b) for o, b, g in zip(out, bufs, given) if g)


def test_object_ids_and_the_empty_list(pa, frames):
    s, fr = frames
    for what in range(3):
        ids = s.ObjectIds(fr[1].ml, what)
        assert _same(s.ObjectIds(_dev(fr[1].ml.ident), what), ids)
    assert (fr[1].ids != 0xFFFFFFFF).sum() > 40
    # num_pixels == 0: nothing is staged, nothing is read (the pointers may be anything), on either variant
    assert s.L.pbrhip_scene_object_ids(s.h, None, 0, 1, None) == 0
    assert s.L.pbrhip_scene_object_ids_device(s.h, None, 0, 1, None, None) == 0


# ------------------------------------------------------------------------------------------------ the calls on a device index
@pytest.mark.parametrize("history", [True, False])
def test_temporal_accumulate(pa, frames, history):
    _, fr = frames
    hist = pa.TemporalAccumulate(fr[0].layer, fr[0].ml) if history else None
    host = pa.TemporalAccumulate(fr[1].layer, fr[1].ml, hist)
    on = pa.TemporalAccumulate(_on_layer(fr[1].layer), _on_motion(pa, fr[1].ml), None if hist is None else pa.TemporalHistory(_dev(hist.rgba), _dev(hist.guide)))
    assert _same(on.rgba, host.rgba) and (not history or (host.rgba[..., 3] > 1).any())


SVGF_CASES = {  # features, ids, history
    "all": (True, True, True), "no albedo": (False, True, True), "no ids": (True, False, True), "no history": (True, True, False),
    "nothing optional": (False, False, False),
}


@pytest.mark.parametrize("case", list(SVGF_CASES))
def test_svgf_accumulate_and_filter(pa, frames, case):
    with_feat, with_ids, with_hist = SVGF_CASES[case]
    _, fr = frames
    f0, f1 = (fr[i].feat if with_feat else None for i in (0, 1))
    i0, i1 = (fr[i].ids if with_ids else None for i in (0, 1))
    hist = pa.SvgfAccumulate(fr[0].layer, fr[0].ml, None, f0, i0) if with_hist else None
    host = pa.SvgfAccumulate(fr[1].layer, fr[1].ml, hist, f1, i1)
    th = None if hist is None else pa.SvgfHistory(_dev(hist.illum), _dev(hist.var), _dev(hist.guide), None if i0 is None else _dev(i0))
    on = pa.SvgfAccumulate(_on_layer(fr[1].layer), _on_motion(pa, fr[1].ml), th, _on_features(f1), None if i1 is None else _dev(i1))
    assert _same(on.illum, host.illum) and _same(on.var, host.var)
    assert not with_hist or ((host.illum[..., 3] > 1).any() and (host.var > 0).any())
    # the filter of that history: with and without the feedback image
    ton = pa.SvgfHistory(on.illum, on.var, on.guide, on.ids)
    for feedback in (True, False):
        want = pa.SvgfFilter(host, f1, iterations=2, feedback=feedback)
        got = pa.SvgfFilter(ton, _on_features(f1), iterations=2, feedback=feedback)
        if feedback:
            assert _same(got[0], want[0]) and _same(got[1].illum, want[1].illum)
        else:
            assert _same(got, want)
    assert not _same(want, host.illum)


@pytest.mark.parametrize("with_albedo", [True, False])
def test_emission_split_and_merge(pa, frames, with_albedo):
    _, fr = frames
    layer, em, feat = fr[1].layer, fr[1].em, fr[1].feat if with_albedo else None
    sl, sf = pa.SplitEmission(layer, em, feat)
    tl, tf = pa.SplitEmission(_on_layer(layer), _dev(em.emission), _on_features(feat))
    assert _same(tl.rgba, sl.rgba) and not _same(sl.rgba, layer.rgba)
    assert (sf is None and tf is None) if not with_albedo else (_same(tf.albedo, sf.albedo) and not _same(sf.albedo, feat.albedo))
    filtered = pa.Denoise(sl, sf, iterations=1)
    merged = pa.MergeEmission(filtered, em, layer.count)
    assert _same(pa.MergeEmission(_dev(filtered), _dev(em.emission), _dev(layer.count)), merged) and not _same(merged, filtered)
