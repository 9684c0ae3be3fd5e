"""GPU (-m gpu): the first-hit emission layer.  pbrhip_render_features_emission's three old buffers against
pbrhip_render_features bit for bit; its emission layer against the renderer itself -- the frame of the material-less twin of the scene, in
which every path ends at its first hit after path_head has added the emission -- bit for bit with no exclusions; its independence of the
schedule; pbrhip_emission_split / pbrhip_emission_merge against the float32 model of tests/_emission_model.py bit for bit; and the
orbiting Cornell sequence with albedo, which the split exists for.

Scenes are small stand-ins, committed once per (name, builder) for the module together with their twins; frames are 67 x 45 (a multiple
of neither 8 nor 64) at 3 passes unless a test says otherwise."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import _emission_model as EM

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
NONE = 0xFFFFFFFF
EINVAL, ESTATE = -1, -6
W, H, PASSES = 67, 45, 3
SEED = 1234567890
HOST_SAH, GPU_LBVH_WIDE = 0, 2
# eye, lookat, up, fov, lens radius, focus distance: thin lenses (four camera draws per sample)
LENS = {
    "cornell": ((0.3, -0.6, 3.6), (0.0, 0.6, 0.0), (0.0, 1.0, 0.0), 50.0, 0.05, 0.0),  # from below: the light's front fills a few rows
    "hair": ((1.5, 0.8, 4.5), (0.0, 0.6, 0.0), (0.0, 1.0, 0.0), 40.0, 0.04, 0.0),
    "instanced": ((-0.4, -0.5, 3.8), (0.0, 0.6, 0.0), (0.1, 1.0, 0.0), 48.0, 0.06, 4.0),
    "env": ((3.0, 1.5, 4.5), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 55.0, 0.03, 0.0),  # from outside the box: the sky beside it
}
NAMES = ["cornell", "hair", "instanced", "env"]


@pytest.fixture(scope="module")
def pa():
    import pbrlab_amd as pa
    if pa.device_count() < 1:
        pytest.fail("no HIP device: the GPU tests must run on an MI355X (there is no CPU fallback)")
    pa.set_device(0)
    return pa


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _desc(name):
    from pbrlab_amd import scenes
    if name in ("cornell", "env"):
        return scenes.cornell_scene("ggx", monkey_subdiv=1, lucy_nu=64, lucy_nv=8)
    if name == "hair":
        return scenes.hair_scene(n_strands=300, n_segments=6, head_subdiv=2)
    if name == "instanced":  # a smooth-shaded mesh and a flat one under rotations, non-uniform scales and translations
        d = scenes.cornell_scene("ggx", monkey_subdiv=1, lucy_nu=64, lucy_nv=8)
        for sh in d.shapes:
            if sh.name == "monkey":
                sh.transform = scenes.instance_matrix((20.0, 35.0, -10.0), (1.3, 0.8, 1.1), (0.2, 0.25, 0.3))
            elif sh.name == "lucy":
                sh.transform = scenes.instance_matrix((0.0, 50.0, 15.0), (0.9, 1.2, 0.9), (-0.15, 0.1, 0.35))
        return d
    raise KeyError(name)


class _Materialless:
    """A Scene that attaches no material: build_scene's calls pass through, every material id becomes PBRHIP_NONE"""

    def __init__(self, scene):
        self._s = scene

    def __getattr__(self, name):
        return getattr(self._s, name)

    def AddTriangleMesh(self, vertices, normals, texcoords, vertex_ids, normal_ids, texcoord_ids, material_ids):
        return self._s.AddTriangleMesh(vertices, normals, texcoords, vertex_ids, normal_ids, texcoord_ids, np.full(len(material_ids), NONE, np.uint32))

    def AddCubicBezierCurveMesh(self, vertices, indices, material_ids):
        return self._s.AddCubicBezierCurveMesh(vertices, indices, np.full(len(material_ids), NONE, np.uint32))


def _environment():
    rng = np.random.RandomState(5)
    rgb = rng.uniform(0.05, 2.0, (8, 16, 3)).astype(F)  # strictly positive: a miss always shows in the twin's frame
    c, s = np.cos(0.7), np.sin(0.7)
    return rgb, 1.5, np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]], F)


_SCENES = {}


def _scene(pa, name, builder=HOST_SAH):
    """(scene, material-less twin): the same meshes, instances, light attachments and environment, committed with the same builder"""
    if (name, builder) not in _SCENES:
        from pbrlab_amd import scenes
        d = _desc(name)
        s = pa.scene_from_desc(d, bvh_builder=builder)
        t = pa.Scene()
        if builder != HOST_SAH:
            t.SetBvhBuilder(builder)
        scenes.build_scene(_Materialless(t), d, pa.make_principled, pa.make_hair)
        if name == "env":
            rgb, scale, m = _environment()
            s.SetEnvironment(rgb, scale, m)
            t.SetEnvironment(rgb, scale, m)
        _SCENES[name, builder] = (s, t)
    return _SCENES[name, builder]


def _camera(pair, cam):
    for s in pair:
        if cam is None:
            s.SetCamera(None)
        else:
            s.SetCamera(*cam)


def _cameras(name):
    return [LENS[name]] if name == "env" else [None, LENS[name]]  # (the environment with a user camera only)


def _same_features(a, b):
    return all(np.array_equal(_bits(x), _bits(y)) for x, y in ((a.albedo, b.albedo), (a.normal_depth, b.normal_depth), (a.count, b.count)))


def _twin_frame(pa, twin, w, h, passes, first_pass=0):
    """the twin's frame, and per pixel the number of its samples whose radiance is not black (one-pass frames)"""
    layer = pa.RenderLayer()
    pa.Render(twin, w, h, passes, layer=layer, first_pass=first_pass, seed_seq=SEED)
    lit = np.zeros((h, w), np.uint32)
    one = pa.RenderLayer()
    for p in range(first_pass, first_pass + passes):
        pa.Render(twin, w, h, 1, layer=one, first_pass=p, seed_seq=SEED)
        lit += (one.rgba[..., :3] != 0).any(-1)
    return layer, lit


# ------------------------------------------------------------------------------------------------ the feature pass
@pytest.mark.parametrize("builder", [HOST_SAH, GPU_LBVH_WIDE])
@pytest.mark.parametrize("name", NAMES)
def test_old_buffers_and_emission_layer(pa, name, builder, monkeypatch):
    """1. albedo_hits, normal_depth and count are RenderFeatures' bit for bit.  2. emission.rgb is the rgb of the material-less twin's
    frame bit for bit, emission.w the number of twin samples that saw light -- over both cameras, and with the 4-wide tree switched
    off (PBRHIP_WIDE=0) on the host builder's scene."""
    pair = _scene(pa, name, builder)
    s, twin = pair
    try:
        for cam in _cameras(name):
            _camera(pair, cam)
            for wide in (["1", "0"] if builder == HOST_SAH else ["1"]):
                if wide == "0":
                    monkeypatch.setenv("PBRHIP_WIDE", "0")
                feat, em = pa.RenderFeaturesEmission(s, W, H, PASSES, seed_seq=SEED)
                assert _same_features(feat, pa.RenderFeatures(s, W, H, PASSES, seed_seq=SEED)), (name, builder, cam is None, wide)
                frame, lit = _twin_frame(pa, twin, W, H, PASSES)
                monkeypatch.delenv("PBRHIP_WIDE", raising=False)
                assert (frame.count == PASSES).all() and np.array_equal(feat.count, frame.count)
                assert np.array_equal(_bits(em.emission[..., :3]), _bits(frame.rgba[..., :3])), (name, builder, cam is None, wide)
                assert np.array_equal(em.emission[..., 3], lit.astype(F)), (name, builder, cam is None, wide)
                print(f"{name} builder {builder} {'reference' if cam is None else 'lens'} camera wide {wide}: pixels lit by all / some / none "
                      f"of their samples {(lit == PASSES).sum()} / {((lit > 0) & (lit < PASSES)).sum()} / {(lit == 0).sum()}")
                if cam is not None:
                    # the case is not vacuous: some pixels see the light (or the sky) with all of their samples, some with a part, some not
                    assert (lit == PASSES).sum() > 0 and ((lit > 0) & (lit < PASSES)).sum() > 0 and (lit == 0).sum() > 0, name
                if name == "env":
                    assert ((feat.albedo[..., 3] == 0) & (lit == PASSES)).sum() > 5  # misses that collect the environment
    finally:
        monkeypatch.delenv("PBRHIP_WIDE", raising=False)
        _camera(pair, None)


@pytest.mark.parametrize("name", ["cornell", "hair"])
def test_schedule_independence(pa, name):
    pair = _scene(pa, name)
    s, _ = pair
    _camera(pair, LENS[name])
    try:
        ref_f, ref_e = pa.RenderFeaturesEmission(s, W, H, PASSES, seed_seq=SEED)
        assert ref_e.emission[..., 3].max() > 0

        def same(f, e):
            return _same_features(ref_f, f) and np.array_equal(_bits(ref_e.emission), _bits(e.emission))
        # [0, 2) then [2, 3) on top
        f, e = pa.RenderFeaturesEmission(s, W, H, 2, seed_seq=SEED)
        pa.RenderFeaturesEmission(s, W, H, 1, f, e, first_pass=2, seed_seq=SEED, no_clear=True)
        assert same(f, e)
        # chunks of one pass (three launches), and the smallest chunk there is
        assert same(*pa.RenderFeaturesEmission(s, W, H, PASSES, seed_seq=SEED, max_paths_in_flight=W * H))
        assert same(*pa.RenderFeaturesEmission(s, W, H, PASSES, seed_seq=SEED, max_paths_in_flight=1))
        # two ranks: disjoint pixels, zeros elsewhere: the sum is the frame
        for block in (0, 16):
            parts = [pa.RenderFeaturesEmission(s, W, H, PASSES, seed_seq=SEED, tile_rank=r, tile_world=2, shard_block=block) for r in range(2)]
            assert ((parts[0][0].count > 0) & (parts[1][0].count > 0)).sum() == 0
            tot_f, tot_e = pa.FeatureLayer(W, H), pa.EmissionLayer(W, H)
            for f, e in parts:
                tot_f.albedo += f.albedo
                tot_f.normal_depth += f.normal_depth
                tot_f.count += f.count
                tot_e.emission += e.emission
            assert same(tot_f, tot_e), block
    finally:
        _camera(pair, None)


def test_grid_stride_loop_on_a_large_frame(pa):
    """1056 x 1000 pixels are more than the grid cap's 4096 blocks of 256 lanes: a lane walks more than one pixel"""
    pair = _scene(pa, "cornell")
    s, twin = pair
    _camera(pair, None)
    w, h = 1056, 1000
    assert w * h > 4096 * 256
    feat, em = pa.RenderFeaturesEmission(s, w, h, 1, seed_seq=SEED)
    frame = pa.RenderLayer()
    pa.Render(twin, w, h, 1, layer=frame, seed_seq=SEED)
    assert np.array_equal(_bits(em.emission[..., :3]), _bits(frame.rgba[..., :3]))
    assert np.array_equal(em.emission[..., 3], (frame.rgba[..., :3] != 0).any(-1).astype(F)) and em.emission[..., 3].sum() > 1000
    assert _same_features(feat, pa.RenderFeatures(s, w, h, 1, seed_seq=SEED))


def test_null_buffers_and_states(pa):
    from pbrlab_amd import api, scenes
    s = pa.Scene()
    with pytest.raises(pa.PbrHipError) as e:
        pa.RenderFeaturesEmission(s, 8, 8, 1)
    assert e.value.code == ESTATE  # not committed
    s.close()
    pair = _scene(pa, "cornell")
    s, _ = pair
    _camera(pair, None)
    for w, h, n in ((0, 8, 1), (8, 0, 1), (8, 8, 0)):
        with pytest.raises(pa.PbrHipError) as e:
            pa.RenderFeaturesEmission(s, w, h, n)
        assert e.value.code == EINVAL, (w, h, n)
    full_f, full_e = pa.RenderFeaturesEmission(s, W, H, PASSES, seed_seq=SEED)
    want = (full_f.albedo, full_f.normal_depth, full_f.count, full_e.emission)
    desc = api.RenderDesc(W, H, PASSES, 0, SEED, 0, 1, 0, 0, 0, 0, 0)
    for mask in range(16):  # every subset of the four buffers, the empty one among them; what is given starts dirty
        bufs = [np.full((H, W, 4), 7.0, F), np.full((H, W, 4), 7.0, F), np.full((H, W), 7, np.uint32), np.full((H, W, 4), 7.0, F)]
        args = [b.ctypes.data if mask >> i & 1 else None for i, b in enumerate(bufs)]
        api._chk(s.L.pbrhip_render_features_emission(s.h, C.byref(desc), *args))
        for i, b in enumerate(bufs):
            if mask >> i & 1:
                assert np.array_equal(_bits(b), _bits(want[i])), (mask, i)
            else:
                assert (b == 7).all(), (mask, i)
    # the device entry point: the host's bits
    import torch
    t = [torch.full((H, W, 4), 3.0, dtype=torch.float32, device="cuda:0") for _ in range(3)]
    c = torch.full((H, W), 9, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    pa.RenderFeaturesEmission(s, W, H, PASSES, seed_seq=SEED, device_out=(t[0].data_ptr(), t[1].data_ptr(), c.data_ptr(), t[2].data_ptr()))
    got = (t[0].cpu().numpy(), t[1].cpu().numpy(), c.cpu().numpy().astype(np.uint32), t[2].cpu().numpy())
    assert all(np.array_equal(_bits(g), _bits(x)) for g, x in zip(got, want))
    pa.RenderFeaturesEmission(s, W, H, PASSES, seed_seq=SEED, device_out=(0, 0, 0, t[0].data_ptr()))
    assert np.array_equal(_bits(t[0].cpu().numpy()), _bits(full_e.emission))
    # a stale scene: an edit without its refit
    own = pa.scene_from_desc(_desc("cornell"))
    own.UpdateInstanceTransform(0, scenes.instance_matrix(translate=(0.1, 0.0, 0.0)))
    with pytest.raises(pa.PbrHipError) as e:
        pa.RenderFeaturesEmission(own, W, H, 1)
    assert e.value.code == ESTATE
    own.RefitScene()
    pa.RenderFeaturesEmission(own, W, H, 1)
    own.close()


def test_rendering_is_not_disturbed(pa):
    pair = _scene(pa, "cornell")
    s, _ = pair
    _camera(pair, None)
    a, b = pa.RenderLayer(), pa.RenderLayer()
    pa.Render(s, 64, 48, 2, layer=a)
    pa.RenderFeaturesEmission(s, 50, 70, 3)
    pa.Render(s, 64, 48, 2, layer=b)
    assert np.array_equal(_bits(a.rgba), _bits(b.rgba)) and np.array_equal(a.count, b.count)


# ------------------------------------------------------------------------------------------------ split and merge
def _synthetic(w, h, seed):
    rng = np.random.RandomState(seed)
    count = rng.randint(0, 5, (h, w)).astype(np.uint32)
    k = np.minimum(rng.randint(0, 5, (h, w)), count).astype(np.uint32)  # emitting samples
    le = rng.uniform(0.5, 17.0, (h, w, 3)).astype(F)
    em = np.zeros((h, w, 4), F)
    em[..., :3], em[..., 3] = le * k[..., None].astype(F), k
    rgba = np.zeros((h, w, 4), F)
    rgba[..., :3] = em[..., :3] + (rng.uniform(0, 2, (h, w, 3)) * (count - k)[..., None]).astype(F)
    rgba[..., 3] = count
    lower = rng.rand(h, w) < 0.1  # a colour sum below the emission sum (never from the renderer): clamped at 0
    rgba[lower, :3] *= F(0.5)
    fc = np.where(rng.rand(h, w) < 0.9, count, 0).astype(np.uint32)
    alb = np.zeros((h, w, 4), F)
    hits = np.minimum(fc, count - k)
    alb[..., :3], alb[..., 3] = rng.uniform(0, 1, (h, w, 3)).astype(F) * hits[..., None].astype(F), hits
    filtered = rng.uniform(0, 3, (h, w, 4)).astype(F)
    assert (count == 0).sum() > 20 and ((k == count) & (count > 0)).sum() > 20 and (k == 0).sum() > 20
    return rgba, count, em, alb, fc, filtered


@pytest.mark.parametrize("case", [(67, 45, 1), (131, 23, 2)])
def test_split_and_merge_are_the_model_bit_for_bit(pa, case):
    from pbrlab_amd import _lib
    L = _lib.lib()
    w, h, seed = case
    rgba, count, em, alb, fc, filtered = _synthetic(w, h, seed)
    want_rgba, want_alb = EM.split(rgba, count, em, alb, fc)
    want_merge = EM.merge(filtered, em, count)
    assert not np.array_equal(want_rgba, rgba) and not np.array_equal(want_alb, alb) and not np.array_equal(want_merge, filtered)
    layer = pa.api._bare(pa.RenderLayer, width=w, height=h, rgba=rgba, count=count)
    feat = pa.api._bare(pa.FeatureLayer, width=w, height=h, albedo=alb, normal_depth=np.zeros_like(alb), count=fc)
    # host entry points, with and without the albedo triple
    sl, sf = pa.SplitEmission(layer, pa.api._bare(pa.EmissionLayer, width=w, height=h, emission=em), feat)
    assert np.array_equal(_bits(sl.rgba), _bits(want_rgba)) and np.array_equal(_bits(sf.albedo), _bits(want_alb))
    assert sl.count is count and sf.count is fc and sf.normal_depth is feat.normal_depth
    sl2, none = pa.SplitEmission(layer, em)
    assert none is None and np.array_equal(_bits(sl2.rgba), _bits(want_rgba))
    assert np.array_equal(_bits(pa.MergeEmission(filtered, em, count)), _bits(want_merge))
    # device entry points through tensors
    import torch
    tl = pa.api._bare(pa.RenderLayer, width=w, height=h, rgba=_dev(rgba), count=_dev(count.view(np.int32)))
    tf = pa.api._bare(pa.FeatureLayer, width=w, height=h, albedo=_dev(alb), normal_depth=None, count=_dev(fc.view(np.int32)))
    tem = _dev(em)
    dl, df = pa.SplitEmission(tl, tem, tf)
    assert np.array_equal(_bits(dl.rgba.cpu().numpy()), _bits(want_rgba)) and np.array_equal(_bits(df.albedo.cpu().numpy()), _bits(want_alb))
    dm = pa.MergeEmission(_dev(filtered), tem, tl.count)
    assert np.array_equal(_bits(dm.cpu().numpy()), _bits(want_merge))
    # in place, on the device: out_rgba = rgba, out_albedo_hits = albedo_hits, out_rgba = filtered_rgba
    r, a, f = _dev(rgba), _dev(alb), _dev(filtered)
    torch.cuda.synchronize()
    assert L.pbrhip_emission_split_device(0, w, h, r.data_ptr(), tl.count.data_ptr(), tem.data_ptr(), a.data_ptr(), tf.count.data_ptr(),
                                          r.data_ptr(), a.data_ptr()) == 0
    assert np.array_equal(_bits(r.cpu().numpy()), _bits(want_rgba)) and np.array_equal(_bits(a.cpu().numpy()), _bits(want_alb))
    assert L.pbrhip_emission_merge_device(0, w, h, f.data_ptr(), tem.data_ptr(), tl.count.data_ptr(), f.data_ptr()) == 0
    assert np.array_equal(_bits(f.cpu().numpy()), _bits(want_merge))
    # in place, on the host
    r, a, f = rgba.copy(), alb.copy(), filtered.copy()
    assert L.pbrhip_emission_split(0, w, h, r.ctypes.data, count.ctypes.data, em.ctypes.data, a.ctypes.data, fc.ctypes.data, r.ctypes.data,
                                   a.ctypes.data) == 0
    assert np.array_equal(_bits(r), _bits(want_rgba)) and np.array_equal(_bits(a), _bits(want_alb))
    assert L.pbrhip_emission_merge(0, w, h, f.ctypes.data, em.ctypes.data, count.ctypes.data, f.ctypes.data) == 0
    assert np.array_equal(_bits(f), _bits(want_merge))
    # refusals reach Python as errors
    with pytest.raises(pa.PbrHipError) as e:
        pa.api._chk(L.pbrhip_emission_split(0, w, h, rgba.ctypes.data, count.ctypes.data, em.ctypes.data, alb.ctypes.data, None, r.ctypes.data, None))
    assert e.value.code == EINVAL


def test_split_of_a_rendered_frame_leaves_what_the_twin_does_not_see(pa):
    """on a real frame: the model's bits; the emission sum never exceeds the colour sum (the depth-0 term is the first thing every
    sample's radiance receives, both sums run in pass order and float32 addition is monotone); and merge(split / n) returns the frame's
    mean within the roundings of one subtraction, two divisions and one addition, each relative to at most the mean itself"""
    pair = _scene(pa, "cornell")
    s, _ = pair
    _camera(pair, LENS["cornell"])
    try:
        layer = pa.RenderLayer()
        pa.Render(s, W, H, PASSES, layer=layer, seed_seq=SEED)
        feat, em = pa.RenderFeaturesEmission(s, W, H, PASSES, seed_seq=SEED)
        sl, sf = pa.SplitEmission(layer, em, feat)
        want = EM.split(layer.rgba, layer.count, em.emission, feat.albedo, feat.count)
        assert np.array_equal(_bits(sl.rgba), _bits(want[0])) and np.array_equal(_bits(sf.albedo), _bits(want[1]))
        assert (layer.rgba[..., :3] >= em.emission[..., :3]).all()  # the depth-0 term is part of every sample's radiance
        back = pa.MergeEmission(sl.rgba / F(PASSES), em, layer.count)
        assert np.allclose(back[..., :3], layer.rgba[..., :3] / F(PASSES), rtol=4e-7, atol=0)
    finally:
        _camera(pair, None)


# ------------------------------------------------------------------------------------------------ end to end
def test_orbiting_cornell_sequence_with_albedo(pa):
    """test_svgf_gpu.py::test_orbiting_cornell_sequence's sequence -- scripts/bench_temporal.py's orbit on the Lambert + GGX Cornell box,
    128 x 128, 8 frames at 4 spp, judged on the last frame by that script's rel_mse against 1024 spp -- WITH a FeatureLayer, which that
    test could only record.  "split": SplitEmission -> SvgfAccumulate(layer', motion, history, features', ids) -> SvgfFilter(history,
    features') -> MergeEmission; "plain": the same calls on the unsplit layer and FeatureLayer.  Asserted over the whole frame:
      (a) split filtered < raw;
      (b) split filtered < plain filtered;
      (c) split accumulated < plain accumulated    (accumulated = illumination x this frame's albedo, + the emission for the split).
    Printed beside them, not asserted: the pipeline without a FeatureLayer (albedo 1), whose textures the filter blurs.

    Measured on an MI355X (profiles/README.md "Emission split"): raw 0.0371; split accumulated 0.0071, accumulated + filtered 0.0046;
    plain 155.4 and 237.5; without a FeatureLayer 0.0097 and 0.0051 -- the split is ahead of both on this scene."""
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        import bench_temporal as BT
    finally:
        sys.path.pop(0)
    import _svgf_model as SM
    from pbrlab_amd import scenes
    s = pa.scene_from_desc(scenes.cornell_scene("ggx", seed=1))
    n, spp, size = 8, 4, 128
    layer = pa.RenderLayer()
    h_split = h_plain = h_none = None
    BT.pose(pa, s, 0, n)
    s.RefitScene()
    for k in range(n):
        s.SnapshotPose()
        BT.pose(pa, s, k, n)
        s.RefitScene()
        pa.Render(s, size, size, spp, layer=layer, first_pass=spp * k)
        ml = pa.RenderMotion(s, size, size)
        feat, em = pa.RenderFeaturesEmission(s, size, size, spp, first_pass=spp * k)
        ids = s.ObjectIds(ml, SM.ID_INSTANCE)
        sl, sf = pa.SplitEmission(layer, em, feat)
        h_split = pa.SvgfAccumulate(sl, ml, h_split, sf, ids)
        h_plain = pa.SvgfAccumulate(layer, ml, h_plain, feat, ids)
        h_none = pa.SvgfAccumulate(layer, ml, h_none, None, ids)
    ref = pa.RenderLayer()
    pa.Render(s, size, size, 1024, layer=ref, first_pass=1 << 20)
    truth = ref.rgba[..., :3].astype(np.float64) / 1024
    raw = layer.rgba[..., :3].astype(np.float64) / spp
    em_mean = em.emission[..., :3].astype(np.float64) / spp
    e = dict(raw=BT.rel_mse(raw, truth))
    a_split = EM.clamped_albedo(sf.albedo, sf.count).astype(np.float64)
    e["split_accumulated"] = BT.rel_mse(h_split.illum[..., :3].astype(np.float64) * a_split + em_mean, truth)
    e["split_filtered"] = BT.rel_mse(pa.MergeEmission(pa.SvgfFilter(h_split, sf), em, layer.count)[..., :3].astype(np.float64), truth)
    a_plain = SM.albedo(feat.albedo, feat.count, (size, size))
    e["plain_accumulated"] = BT.rel_mse(h_plain.illum[..., :3].astype(np.float64) * a_plain, truth)
    e["plain_filtered"] = BT.rel_mse(pa.SvgfFilter(h_plain, feat)[..., :3].astype(np.float64), truth)
    e["none_accumulated"] = BT.rel_mse(h_none.illum[..., :3].astype(np.float64), truth)
    e["none_filtered"] = BT.rel_mse(pa.SvgfFilter(h_none)[..., :3].astype(np.float64), truth)
    print(f"frame {n} of the orbit, {size} x {size}, {spp} spp, whole-frame relative MSE against 1024 spp: raw {e['raw']:.5f}")
    for what in ("split", "plain", "none"):
        print(f"  {what:5s}: accumulated {e[what + '_accumulated']:.5f}, accumulated + filtered {e[what + '_filtered']:.5f}")
    assert truth.max() > 0 and em.emission[..., 3].max() == spp
    assert e["split_filtered"] < e["raw"]                        # (a)
    assert e["split_filtered"] < e["plain_filtered"]             # (b)
    assert e["split_accumulated"] < e["plain_accumulated"]       # (c)


def test_cli_split_emission(tmp_path):
    """pbrlab-hip-cli --split-emission: with --aov it writes PREFIX.emission.png beside the three feature images, which stay what they
    are without the flag byte for byte; with --denoise the emitter's pixels come out as the plain frame has them (the emission is added
    back unfiltered), which the plain --denoise does not do; --spp above --feature-spp continues the emission sums alone"""
    import subprocess
    from pbrlab_amd import io_api
    from test_io_gpu import _write_scene_files
    d = str(tmp_path)
    files = _write_scene_files(d, "textured", False)
    w, h = 96, 64
    common = [io_api.CLI_PATH] + files + ["--width", str(w), "--height", str(h), "--spp", "8", "--feature-spp", "4", "--denoise"]
    out = {}
    for name, extra in (("plain", ["--aov", os.path.join(d, "plain")]), ("split", ["--aov", os.path.join(d, "split"), "--split-emission"])):
        r = subprocess.run(common + ["--out", os.path.join(d, name + ".png")] + extra, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        out[name] = io_api.png_decode(open(os.path.join(d, name + ".png"), "rb").read())
    for kind in ("albedo", "normal", "depth"):
        assert open(os.path.join(d, f"plain.{kind}.png"), "rb").read() == open(os.path.join(d, f"split.{kind}.png"), "rb").read(), kind
    assert not os.path.exists(os.path.join(d, "plain.emission.png"))
    em = io_api.png_decode(open(os.path.join(d, "split.emission.png"), "rb").read())
    assert em.shape[:2] == (h, w) and out["plain"].shape == out["split"].shape == (h, w, 4)
    lit = em[..., :3].max(-1) > 0
    assert 0 < lit.sum() < w * h // 4 and not np.array_equal(out["plain"], out["split"])
    # a pixel the light covers with every sample shows the light's colour: the emission image's own value
    full = em[..., :3].min(-1) == em[..., :3].max()
    assert full.sum() > 0 and (out["split"][full][:, :3] >= em[full][:, :3]).all()
