"""GPU (-m gpu): pbrhip_scene_snapshot_pose, pbrhip_render_motion and pbrhip_temporal_accumulate against the float64 model
of tests/_temporal_model.py within derived rounding bounds, their exact properties, the snapshot's state machine, and that a sequence
accumulated across refits is closer to the converged frame than its raw frames.

The scene: a two-triangle plane, a 12-triangle box in front of it as its own instance, a light quad seen edge-on, three hair strands.
Every case is made once (the module's cache) and shared by the tests that read it.  The figures the tests print were measured on an
MI355X; DESIGN.md §16 quotes them."""

import numpy as np
import pytest

import _temporal_model as TM

pytestmark = pytest.mark.gpu

EINVAL, ESTATE = -1, -6
F = np.float32
W, H = 67, 45
BIG = (1056, 1000)  # more than kFeatureGridCap x 256 pixels: the grid-stride loop runs
CAM_A = dict(eye=(0.4, 0.3, 4.5), lookat=(0.0, 0.0, 0.5), up=(0.0, 1.0, 0.0), fov=60.0)
CAM_B = dict(eye=(-0.5, 0.6, 3.0), lookat=(0.1, -0.1, 0.5), up=(0.0, 1.0, 0.0), fov=90.0)  # tan(45 degrees) rounds to 1 in any libm


@pytest.fixture(scope="module")
def pa():
    import pbrlab_amd as pa
    if pa.device_count() < 1:
        pytest.fail("no HIP device: the GPU tests must run on an MI355X (there is no CPU fallback)")
    pa.set_device(0)
    return pa


def _desc():
    from pbrlab_amd import scenes
    b = scenes._Builder()
    b.add("plane", *scenes._quad((-2, -1.5, 0), (2, -1.5, 0), (2, 1.5, 0), (-2, 1.5, 0)), 0)
    c = np.array([[x, y, z] for z in (0.4, 1.2) for y in (-0.4, 0.4) for x in (-0.4, 0.4)], np.float32)
    faces = [(0, 2, 1), (1, 2, 3), (4, 5, 6), (5, 7, 6), (0, 1, 4), (1, 5, 4), (2, 6, 3), (3, 6, 7), (0, 4, 2), (2, 4, 6), (1, 3, 5), (3, 7, 5)]
    b.add("box", c, faces, 0)
    b.add("light", *scenes._quad((2.5, -1, 0.5), (2.5, -1, 2.5), (2.5, 1, 2.5), (2.5, 1, 0.5)), 1)  # faces -x: seen edge-on, lights the rest
    mats = scenes.demo_materials("lambert")[:2]
    strands = []
    for k, x in enumerate((-1.2, -0.9, 1.1)):
        strands += [(x, -1.0, 1.5, 0.09), (x + 0.3, -0.3, 1.7 + 0.1 * k, 0.08), (x - 0.2, 0.4, 1.6, 0.07), (x + 0.1, 1.1, 1.5, 0.06)]
    hair = scenes.CurveShape("hair", np.array(strands, np.float32), np.arange(0, 12, 4, dtype=np.uint32))
    return b.finish(mats, [hair])


PLANE, BOX, LIGHT, HAIR = 0, 1, 2, 3  # mesh ids and instance ids, in build_scene's order


def _edit(pa, s, d, kinds):
    """the three kinds of edit of the issue (and which path the mesh update takes), on a committed scene"""
    from pbrlab_amd import scenes
    if "transform" in kinds:
        s.UpdateInstanceTransform(BOX, scenes.instance_matrix(rotate_deg=(0.0, 20.0, 10.0), translate=(0.3, 0.1, 0.2)))
    if "mesh" in kinds or "mesh_device" in kinds:
        v = d.vertices.copy()
        v[:4, 2] += (0.2, -0.15, 0.1, -0.05)  # the plane's corners
        v[:4, 0] += 0.1
        if "mesh_device" in kinds:
            import torch
            s.UpdateTriangleMeshDevice(PLANE, torch.from_numpy(v).to("cuda:0"))
        else:
            s.UpdateTriangleMesh(PLANE, v)
    if "curves" in kinds:
        v = d.curves[0].vertices.copy()
        v[:, 0] += 0.15
        v[4:8, 2] += 0.4  # (the scene's box grows: the reference's camera moves)
        v[8:, 1] *= 0.9
        s.UpdateCurveMesh(HAIR, v)


def _model_camera(s, cam, w, h):
    if cam is None:
        return TM.reference_camera(*s.FetchSceneAABB(), w, h)
    return TM.user_camera(cam["eye"], cam["lookat"], cam["up"], cam["fov"], w, h)


CASES = {
    "user camera, transform + mesh + curves": dict(size=(W, H), cam0=CAM_A, cam1=CAM_B, edits=("transform", "mesh", "curves")),
    "reference camera through the bounds, device mesh": dict(size=(W, H), cam0=None, cam1=None, edits=("transform", "mesh_device", "curves")),
    "camera set between the frames": dict(size=(W, H), cam0=None, cam1=CAM_A, edits=("transform",)),
    "no edit": dict(size=(W, H), cam0=CAM_B, cam1=CAM_B, edits=()),
    "large frame": dict(size=BIG, cam0=CAM_A, cam1=CAM_B, edits=("transform", "curves")),
}
_MADE = {}


def _case(pa, name, builder=0, **motion_kw):
    """snapshot -> edits -> refit -> RenderMotion, once per (case, builder, shard): everything a test reads"""
    key = (name, builder, tuple(sorted(motion_kw.items())))
    if key not in _MADE:
        c, d = CASES[name], _desc()
        w, h = c["size"]
        s = pa.scene_from_desc(d, bvh_builder=builder)
        if c["cam0"] is not None:
            s.SetCamera(c["cam0"]["eye"], c["cam0"]["lookat"], c["cam0"]["up"], c["cam0"]["fov"])
        slots0, shade0 = s.read_slots()
        cam_prev = _model_camera(s, c["cam0"], w, h)
        s.SnapshotPose()
        _edit(pa, s, d, c["edits"])
        if c["cam1"] is not c["cam0"]:
            s.SetCamera(c["cam1"]["eye"], c["cam1"]["lookat"], c["cam1"]["up"], c["cam1"]["fov"])
        s.RefitScene()
        slots1, shade1 = s.read_slots()
        ml = pa.RenderMotion(s, w, h, **motion_kw)
        _MADE[key] = dict(scene=s, ml=ml, slots0=slots0, shade0=shade0, slots1=slots1, shade1=shade1, cam_prev=cam_prev,
                          cam_now=_model_camera(s, c["cam1"], w, h), size=(w, h))
    return _MADE[key]


# ------------------------------------------------------------------------------------------------ motion against the model
@pytest.mark.parametrize("name", list(CASES))
def test_motion_against_the_float64_model(pa, name):
    """X_prev in float64 from the snapshot's slots and the returned ident, projected through the snapshot's camera; the bound is
    _temporal_model.motion_bound's operation count.  (The large frame: every 97th pixel.)"""
    c = _case(pa, name)
    w, h = c["size"]
    ml = c["ml"]
    want = TM.motion(c["slots0"], c["shade0"], ml.ident, c["cam_prev"], w, h)
    bx, by, bz = TM.motion_bound(c["slots0"], ml.ident, c["cam_prev"], w, h, want)
    pick = np.zeros((h, w), bool)
    pick.reshape(-1)[::97 if (w, h) == BIG else 1] = True
    hit = ml.ident[..., 0] != TM.NONE
    assert hit.mean() > 0.15 and (~hit).any()
    assert np.array_equal(ml.motion[..., 3], want[..., 3].astype(F)), "valid differs from the model's"
    ok = pick & (want[..., 3] != 0)
    assert ok.sum() > 300 and (want[..., 3] == 2).any() and (want[..., 3] == 1).any()
    ex, ey = np.abs(ml.motion[..., 0] - want[..., 0])[ok], np.abs(ml.motion[..., 1] - want[..., 1])[ok]
    ez = (np.abs(ml.motion[..., 2] - want[..., 2]) / np.maximum(want[..., 2], 1e-30))[ok]
    print(f"{name}: {ok.sum()} pixels, max |motion| {np.abs(want[..., :2][ok]).max():.2f} px; max error mx {ex.max():.3e} px (worst error / bound "
          f"{(ex / bx[ok]).max():.3f}), my {ey.max():.3e} px ({(ey / by[ok]).max():.3f}), z_prev {ez.max():.3e} relative ({(ez / bz[ok]).max():.3f})")
    assert (ex <= bx[ok]).all() and (ey <= by[ok]).all() and (ez <= bz[ok]).all()
    if CASES[name]["edits"]:
        assert np.abs(want[..., :2][ok]).max() > 1.0  # something moved by more than a pixel
    assert (ml.motion[~hit] == 0).all()


def test_no_edit_gives_no_motion(pa):
    """a snapshot used with no edit in between: valid = hit, and |mx|, |my| within rounding.  Besides the model's bound there is the
    intersection's own: u and v carry <= 16 u S / |e| each (a dozen operations on coordinates <= S, divided by the determinant), so
    X(u, v) misses the ray by <= 32 u S in the triangle's plane, seen under the angle of incidence; on a curve the hit's point is the
    piece's axis, up to its radius beside the ray."""
    c = _case(pa, "no edit")
    w, h = c["size"]
    ml, cam = c["ml"], c["cam_prev"]
    hit = ml.ident[..., 0] != TM.NONE
    assert np.array_equal(ml.motion[..., 3] != 0, hit)
    want = TM.motion(c["slots0"], c["shade0"], ml.ident, cam, w, h)
    bx, by, _ = TM.motion_bound(c["slots0"], ml.ident, cam, w, h, want)
    S = np.abs(c["slots0"][:, :3, :3]).max() + np.abs(cam["eye"]).max()
    o, d = TM.centre_rays(cam, w, h)
    cos = np.abs((ml.guide[..., :3].astype(np.float64) * d).sum(-1))
    z = np.maximum(ml.motion[..., 2].astype(np.float64), 1e-30)
    px_per_unit = 0.5 * w / float(cam["ha"]) / z * 2.0  # (a unit across the ray at distance z, in pixels; x 2: towards the frame's corner)
    tri = ml.motion[..., 3] == 1
    extra = np.where(tri, 32 * TM.EPS * S / np.maximum(cos, 1e-3), np.abs(c["slots0"][:, :2, 3]).max()) * px_per_unit
    mx, my = np.abs(ml.motion[..., 0]), np.abs(ml.motion[..., 1])
    print(f"no edit: max |mx| {mx[tri].max():.3e}, |my| {my[tri].max():.3e} px on triangles (bound {(bx + extra)[tri].max():.3e}), "
          f"{mx[hit & ~tri].max():.3e} / {my[hit & ~tri].max():.3e} px on curves (their radius: {extra[hit & ~tri].max():.3e} px)")
    assert (mx[hit] <= (bx + extra)[hit]).all() and (my[hit] <= (by + extra)[hit]).all()


# ------------------------------------------------------------------------------------------------ exact properties of motion
@pytest.mark.parametrize("name", ["user camera, transform + mesh + curves", "reference camera through the bounds, device mesh"])
def test_ident_is_trace_closest_of_the_centre_rays(pa, name):
    from pbrlab_amd import api
    c = _case(pa, name)
    w, h = c["size"]
    ml, s = c["ml"], c["scene"]
    o, d = TM.centre_rays(c["cam_now"], w, h)
    rays = np.zeros(w * h, api.RAY_DT)
    rays["org"], rays["dir"], rays["tmin"], rays["tmax"] = o.reshape(-1, 3), d.reshape(-1, 3), 0.0, F(1.844e18)
    hits = s.trace_closest(rays)
    ident = ml.ident.reshape(-1, 4)
    hit = hits["prim_id"] != 0xFFFFFFFF
    assert np.array_equal(ident[:, 0] != TM.NONE, hit) and hit.sum() > 1000
    rec = c["shade1"][ident[hit, 0]]
    for k, f in ((25, "instance_id"), (26, "geom_id"), (27, "prim_id")):
        assert np.array_equal(rec[:, k], hits[f][hit]), f
    for k, f in ((1, "u"), (2, "v"), (3, "t")):
        assert np.array_equal(ident[hit, k], hits[f][hit].view(np.uint32)), f
    # guide.w == t; a miss is zeros, (NONE, 0, 0, 0) in ident
    assert np.array_equal(ml.guide[..., 3].view(np.uint32), np.where(ml.ident[..., 0] != TM.NONE, ml.ident[..., 3], 0))
    miss = ~hit.reshape(h, w)
    assert (ml.guide[miss] == 0).all() and (ml.motion[miss] == 0).all() and (ml.ident[miss] == (TM.NONE, 0, 0, 0)).all()
    # the guide is a unit vector, towards the viewer on triangles
    n = ml.guide[..., :3].astype(np.float64)
    tri = ml.motion[..., 3] == 1
    assert np.abs(np.sqrt((n * n).sum(-1))[~miss] - 1).max() < 8 * TM.EPS and ((n * d).sum(-1)[tri] <= 0).all()


def _canonical(c):
    """(gid, u, v, t bits) per pixel: ident with the builder's slot order taken out"""
    ident = c["ml"].ident.copy()
    hit = ident[..., 0] != TM.NONE
    ident[..., 0][hit] = c["shade1"][ident[..., 0][hit], 24]
    return ident


def test_motion_is_schedule_and_tree_independent(pa, monkeypatch):
    name = "user camera, transform + mesh + curves"
    base = _case(pa, name)
    ml = base["ml"]
    for block in (8, 64):
        parts = [_case(pa, name, tile_rank=r, tile_world=2, shard_block=block)["ml"] for r in (0, 1)]
        for f in ("motion", "guide", "ident"):
            a, b = (getattr(p, f).view(np.uint32) for p in parts)
            assert a.any() and b.any() and not (a.any(-1) & b.any(-1)).any(), (block, f)  # disjoint shards, zero elsewhere
            assert np.array_equal(a | b, getattr(ml, f).view(np.uint32)), (block, f)
    for builder in (1, 2):
        other = _case(pa, name, builder=builder)
        assert np.array_equal(other["ml"].motion.view(np.uint32), ml.motion.view(np.uint32)), builder
        assert np.array_equal(other["ml"].guide.view(np.uint32), ml.guide.view(np.uint32)), builder
        assert np.array_equal(_canonical(other), _canonical(base)), builder
    monkeypatch.setenv("PBRHIP_WIDE", "0")
    w, h = base["size"]
    narrow = pa.RenderMotion(base["scene"], w, h)
    monkeypatch.delenv("PBRHIP_WIDE")
    for f in ("motion", "guide", "ident"):
        assert np.array_equal(getattr(narrow, f).view(np.uint32), getattr(ml, f).view(np.uint32)), f


def test_device_variant_gives_the_host_variants_bits(pa):
    import torch
    c = _case(pa, "user camera, transform + mesh + curves")
    w, h = c["size"]
    out = (torch.zeros((h, w, 4), dtype=torch.float32, device="cuda:0"), torch.zeros((h, w, 4), dtype=torch.float32, device="cuda:0"),
           torch.zeros((h, w, 4), dtype=torch.int32, device="cuda:0"))
    got = pa.RenderMotion(c["scene"], w, h, device_out=out)
    assert got.motion is out[0]
    for f, t in zip(("motion", "guide", "ident"), out):
        assert np.array_equal(t.cpu().numpy().view(np.uint32), getattr(c["ml"], f).view(np.uint32)), f
    only = pa.RenderMotion(c["scene"], w, h, device_out=(None, out[1], None))  # each output may be NULL
    assert only.motion is None and np.array_equal(out[1].cpu().numpy().view(np.uint32), c["ml"].guide.view(np.uint32))


# ------------------------------------------------------------------------------------------------ the snapshot's state machine
def test_snapshot_state_machine(pa):
    from pbrlab_amd import scenes
    d = _desc()
    s = pa.Scene()

    def refused(f):
        with pytest.raises(pa.PbrHipError) as e:
            f()
        assert e.value.code == ESTATE, e.value
    refused(s.SnapshotPose)  # not committed
    s.close()
    s = pa.scene_from_desc(d)
    s.SetCamera(**{k: v for k, v in CAM_A.items()})
    refused(lambda: pa.RenderMotion(s, W, H))  # no snapshot
    before = s.info()["device_bytes"]
    s.SnapshotPose()
    assert s.info()["device_bytes"] == before  # (the scene's own buffers are what they were)
    first = pa.RenderMotion(s, W, H)
    s.UpdateInstanceTransform(BOX, scenes.instance_matrix(translate=(0.5, 0.0, 0.0)))
    refused(s.SnapshotPose)                      # stale
    refused(lambda: pa.RenderMotion(s, W, H))
    s.RefitScene()
    moved = pa.RenderMotion(s, W, H)
    on_box = (moved.ident[..., 0] != TM.NONE) & (np.abs(moved.motion[..., 0]) > 1.0)
    assert on_box.sum() > 20 and np.abs(first.motion[..., :2][first.motion[..., 3] == 1]).max() < 1e-2
    # the snapshot survives a material update, the environment and a camera change; a second snapshot replaces the first
    s.UpdateMaterialParam(0, pa.make_principled(dict(scenes.demo_materials("lambert")[0], base_color=(0.1, 0.2, 0.3))))
    s.SetEnvironment(np.ones((4, 8, 3), np.float32))
    again = pa.RenderMotion(s, W, H)
    assert np.array_equal(again.motion.view(np.uint32), moved.motion.view(np.uint32))
    s.SnapshotPose()
    still = pa.RenderMotion(s, W, H)
    assert np.abs(still.motion[..., :2][still.motion[..., 3] == 1]).max() < 1e-2 and np.array_equal(still.ident, moved.ident)
    # a replica has none; a commit drops it
    r = pa.replicate(s, 0)
    refused(lambda: pa.RenderMotion(r, W, H))
    r.close()
    s.CommitScene()
    refused(lambda: pa.RenderMotion(s, W, H))
    s.SnapshotPose()
    pa.RenderMotion(s, W, H)
    with pytest.raises(pa.PbrHipError) as e:
        pa.RenderMotion(s, W, H, tile_rank=2, tile_world=2)  # pbrhip_render_features' refusals
    assert e.value.code == EINVAL


# ------------------------------------------------------------------------------------------------ accumulation against the model
def _synthetic(pa, w, h, seed, max_history):
    """test_denoise_gpu._synthetic's style: a few planes of distinct normals and depths in the current frame and in the history, moved
    against each other; background regions, count == 0 holes, history holes, motions that leave the frame, a curve region.  Re-drawn
    until no input lies near a decision threshold (_temporal_model.conditioned)."""
    rng = np.random.RandomState(seed)
    params = dict(alpha_min=0.05, sigma_depth=0.1, normal_cos_min=0.9, max_history=max_history)
    normals = np.array([[0, 0, 1], [0.6, 0, 0.8], [0, 1, 0], [0.48, 0.6, 0.64], [-0.6, 0.64, 0.48]], np.float64)
    yy, xx = np.mgrid[0:h, 0:w]
    for _ in range(50):
        region = ((xx * 5) // w + 2 * ((yy * 3) // h)) % 5   # 0 = background
        region_h = (((xx + 3) * 5) // w + 2 * (((yy + 1) * 3) // h)) % 5  # the history's regions, shifted: edges to reject across
        layer = pa.RenderLayer(w, h)
        spp = np.where(rng.rand(h, w) < 0.03, 0, rng.randint(1, 9, (h, w))).astype(np.uint32)
        layer.rgba[..., :3] = rng.uniform(0.0, 2.0, (h, w, 3)) * spp[..., None]
        layer.rgba[..., 3] = spp
        layer.count[...] = spp

        def guide_of(reg):
            n = normals[reg] + 0.02 * rng.normal(size=(h, w, 3))
            n /= np.linalg.norm(n, axis=-1, keepdims=True)
            g = np.concatenate([n, (2.0 + reg + 0.01 * xx + rng.uniform(0, 0.05, (h, w)))[..., None]], -1)
            return np.where((reg == 0)[..., None], 0.0, g).astype(F)
        guide, hist_guide = guide_of(region), guide_of(region_h)
        motion = np.zeros((h, w, 4), F)
        motion[..., 0] = rng.uniform(-4.0, 2.0, (h, w)) + np.where(xx > w - 6, 9.0, 0.0)  # the right columns leave the frame
        motion[..., 1] = rng.uniform(-1.5, 1.5, (h, w)) - np.where(yy < 2, 3.0, 0.0)       # the top rows too
        motion[..., 2] = guide[..., 3] * rng.choice([1.0, 1.0, 1.0, 1.3], (h, w)) + rng.uniform(-0.03, 0.03, (h, w))
        motion[..., 3] = np.where(region == 0, 0.0, np.where(region == 4, 2.0, 1.0))
        for _ in range(100):  # no fractional part of q within 1e-3 of a pixel centre: those pixels are drawn again
            fx, fy = TM._taps(motion, w, h)[:2]
            bad = (np.minimum(fx, 1 - fx) < 2e-3) | (np.minimum(fy, 1 - fy) < 2e-3)
            if not bad.any():
                break
            motion[..., 0][bad] += rng.uniform(0.1, 0.4, bad.sum()).astype(F)
            motion[..., 1][bad] += rng.uniform(0.1, 0.4, bad.sum()).astype(F)
        hist = np.zeros((h, w, 4), F)
        hist[..., :3] = rng.uniform(0.0, 2.0, (h, w, 3))
        hist[..., 3] = np.where(rng.rand(h, w) < 0.05, 0.0, np.where(rng.rand(h, w) < 0.5, max_history, rng.randint(1, max_history + 1, (h, w))))
        margins = []
        TM.accumulate(layer.rgba, layer.count, motion, guide, hist, hist_guide, margins=margins, **params)
        if TM.conditioned(margins):
            return layer, pa.MotionLayer(motion, guide, None), pa.TemporalHistory(hist, hist_guide), params
        rng = np.random.RandomState(rng.randint(1 << 30))
    raise AssertionError("no conditioned input in 50 draws")


@pytest.mark.parametrize("case", [(67, 45, 1, 8), (131, 23, 2, 3)])
def test_accumulation_against_the_float64_model(pa, case):
    """|gpu - model| <= the bound _temporal_model.accumulate derives (the blend is a convex combination; what float32 loses is the
    absolute accuracy of q = x + m, which moves the bilinear weights)"""
    w, h, seed, max_history = case
    layer, ml, hist, params = _synthetic(pa, w, h, seed, max_history)
    bound = []
    want = TM.accumulate(layer.rgba, layer.count, ml.motion, ml.guide, hist.rgba, hist.guide, bound=bound, **params)
    got = pa.TemporalAccumulate(layer, ml, hist, **params)
    err, B = np.abs(got.rgba - want), bound[0]
    kinds = dict(hole=(layer.count == 0), fresh=(want[..., 3] == 1) & (layer.count > 0), blended=want[..., 3] > 1, capped=want[..., 3] == max_history)
    print(f"{w}x{h}: " + ", ".join(f"{k} {v.sum()}" for k, v in kinds.items()) + f"; max error rgb {err[..., :3].max():.3e}, length {err[..., 3].max():.3e}; "
          f"worst error / bound {(err / np.maximum(B, 1e-300))[B > 0].max():.3f}")
    assert all(v.sum() > 10 for v in kinds.values()), {k: int(v.sum()) for k, v in kinds.items()}
    assert (err <= B).all()
    assert got.guide is ml.guide
    # a rejected or history-less pixel: (c, 1) with c = rgb / count bit for bit; a hole: zeros
    with np.errstate(invalid="ignore", divide="ignore"):
        c = (layer.rgba[..., :3] / layer.count[..., None].astype(F)).astype(F)
    fresh = kinds["fresh"]
    assert np.array_equal(got.rgba[fresh][:, :3].view(np.uint32), c[fresh].view(np.uint32)) and (got.rgba[fresh][:, 3] == 1).all()
    assert (got.rgba[kinds["hole"]] == 0).all()
    none = pa.TemporalAccumulate(layer, ml, None, **params)
    live = layer.count > 0
    assert np.array_equal(none.rgba[live][:, :3].view(np.uint32), c[live].view(np.uint32)) and (none.rgba[live][:, 3] == 1).all() and (none.rgba[~live] == 0).all()
    # on tensors: the same bits
    import torch
    dev = lambda a, dt=None: torch.from_numpy(np.ascontiguousarray(a if dt is None else a.view(dt))).to("cuda:0")  # noqa: E731
    tl = type("L", (), dict(rgba=dev(layer.rgba), count=dev(layer.count, np.int32)))()
    on = pa.TemporalAccumulate(tl, pa.MotionLayer(dev(ml.motion), dev(ml.guide), None), pa.TemporalHistory(dev(hist.rgba), dev(hist.guide)), **params)
    assert np.array_equal(on.rgba.cpu().numpy().view(np.uint32), got.rgba.view(np.uint32))


def test_accumulation_exact_properties(pa):
    w, h, K = 33, 21, 5
    guide = np.zeros((h, w, 4), F)
    guide[..., :3], guide[..., 3] = (0.0, 0.6, 0.8), 3.0
    motion = np.zeros((h, w, 4), F)
    motion[..., 2], motion[..., 3] = 3.0, 1.0
    ml = pa.MotionLayer(motion, guide, None)
    layer = pa.RenderLayer(w, h)
    layer.count[...] = 3
    colour = np.array([0.3, 0.6, 0.9], F)
    layer.rgba[..., :3], layer.rgba[..., 3] = colour * F(3), 3
    c = (layer.rgba[0, 0, :3] / F(3)).astype(F)
    hist, lengths = None, []
    for _ in range(K + 3):
        hist = pa.TemporalAccumulate(layer, ml, hist, alpha_min=0.0, max_history=K)
        lengths.append(hist.rgba[..., 3].copy())
        # zero motion, a constant colour: constant to 2 ulp
        assert (np.abs(hist.rgba[..., :3].astype(np.float64) - c) <= 2 * np.spacing(c)).all()
    # the history length goes 1, 2, ..., max_history and stays
    assert [float(a.min()) for a in lengths] == [float(a.max()) for a in lengths] == [min(k + 1, K) for k in range(K + 3)]
    # the same with half a pixel of motion: the interior still counts up, the border column (one tap outside) too
    motion[..., 0] = 0.5
    hist = None
    for k in range(3):
        hist = pa.TemporalAccumulate(layer, ml, hist, alpha_min=0.0, max_history=K)
        assert (hist.rgba[..., 3] == k + 1).all() and (np.abs(hist.rgba[..., :3].astype(np.float64) - c) <= 2 * np.spacing(c)).all()
    # alpha_min caps the window: with alpha_min = 1 the result is the current frame
    loud = pa.TemporalHistory(hist.rgba + F(5.0), hist.guide)
    out = pa.TemporalAccumulate(layer, ml, loud, alpha_min=1.0, max_history=K)
    assert (np.abs(out.rgba[..., :3].astype(np.float64) - c) <= 16 * np.spacing(c + 5)).all()
    # refusals reach Python as errors
    with pytest.raises(pa.PbrHipError) as e:
        pa.TemporalAccumulate(layer, ml, hist, alpha_min=float("nan"))
    assert e.value.code == EINVAL
    # the helper: the accumulated mean as the RenderLayer Denoise takes
    lay = hist.layer()
    assert (lay.count == 1).all() and np.array_equal(lay.rgba[..., :3], hist.rgba[..., :3]) and pa.Denoise(lay).shape == (h, w, 4)


# ------------------------------------------------------------------------------------------------ end to end
def test_accumulated_sequence_beats_its_raw_frames(pa):
    """eight frames of the moving box at 4 spp, 64 x 64: at the last frame the accumulated image is closer (relative MSE against 1024 spp of
    the same pose) than the raw 4-spp frame, on the pixels whose history length is >= 4"""
    from pbrlab_amd import scenes
    d = _desc()
    s = pa.scene_from_desc(d)
    s.SetCamera(CAM_A["eye"], CAM_A["lookat"], CAM_A["up"], CAM_A["fov"])
    n, spp, size = 8, 4, 64
    hist, layer = None, pa.RenderLayer()
    for k in range(n):
        s.SnapshotPose()
        s.UpdateInstanceTransform(BOX, scenes.instance_matrix(rotate_deg=(0.0, 4.0 * k, 0.0), translate=(0.08 * k - 0.3, 0.0, 0.0)))
        s.RefitScene()
        pa.Render(s, size, size, spp, layer=layer, first_pass=spp * k)
        ml = pa.RenderMotion(s, size, size)
        hist = pa.TemporalAccumulate(layer, ml, hist)
    ref = pa.RenderLayer()
    pa.Render(s, size, size, 1024, layer=ref, first_pass=1 << 20)
    truth = ref.rgba[..., :3].astype(np.float64) / 1024
    raw = layer.rgba[..., :3].astype(np.float64) / spp
    old = hist.rgba[..., 3] >= 4
    rel = lambda img: float((((img - truth) ** 2) / (truth ** 2 + 1e-2))[old].mean())  # noqa: E731
    e_raw, e_acc = rel(raw), rel(hist.rgba[..., :3].astype(np.float64))
    print(f"frame {n}: {old.mean():.0%} of the pixels hold >= 4 frames; relative MSE against 1024 spp: raw {spp} spp {e_raw:.4f}, accumulated {e_acc:.4f} "
          f"(x {e_raw / e_acc:.2f})")
    assert old.sum() > 1000 and truth.max() > 0  # (the plane and the box cover two fifths of the frame; the background keeps no history)
    assert e_acc < e_raw
