"""The look-at camera on the GPU, held to the float64 models of tests/_camera_analytic.py.

- Rays: with no camera, pbrhip_camera_rays is the oracle's camera bit for bit; pinhole and thin-lens cameras agree with the float64
  model fed the same draws within a few float32 ulps.
- Radiance through an oblique pinhole (test_analytic_radiance's scenes and statistics), depth of field (an emitter on the focal plane
  is sharp for every lens sample, one at half the focus distance is not), no change for a scene without a camera, the C ABI's checks,
  bit-identity across schedules with a thin lens, the CLI and the C++ shim."""
import os
import subprocess

import numpy as np
import pytest

import _analytic as A
import _camera_analytic as CA
import _env_analytic as EA
import _oracle as O
import test_analytic_radiance as TR
from test_analytic_radiance import _pa
from test_env_gpu import SCHEDULES, _Env, _env, _render, _same, _scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
EPS = 2.0 ** -24
DIR_ULPS = 8    # |d_gpu - d_model| per component of a unit direction, in units of 2^-24
ORG_ULPS = 8    # |o_gpu - o_model| per component, in units of 2^-24 x (max |eye| + lens radius)

CAMERAS = {  # name -> eye, lookat, up, fov, lens radius, focus distance
    "oblique": ((1.2, -1.6, 1.4), (0.0, 0.0, 0.1), (0.0, 0.0, 1.0), 50.0, 0.0, 0.0),
    "facing_x": ((-3.0, 0.25, 0.5), (2.0, 0.25, 0.5), (0.0, 1.0, 0.0), 40.0, 0.0, 0.0),
    "straight_down": ((0.1, 0.2, 4.0), (0.1, 0.2, 0.0), (0.0, 1.0, 0.0), 35.0, 0.0, 0.0),
    "skew_up": ((2.0, 1.0, 3.0), (-0.5, 0.2, 0.0), (0.3, 1.0, 0.4), 70.0, 0.0, 0.0),
    "lens": ((1.2, -1.6, 1.4), (0.0, 0.0, 0.1), (0.0, 0.0, 1.0), 45.0, 0.08, 0.0),
    "lens_focus": ((-3.0, 0.25, 0.5), (2.0, 0.25, 0.5), (0.3, 1.0, -0.2), 30.0, 0.25, 2.5),
}


def _rays(s, W, H, xyp, seed):
    r = s.CameraRays(W, H, xyp, seed_seq=seed)
    return r["org"].astype(np.float64), r["dir"].astype(np.float64), r


@pytest.mark.gpu
def test_default_camera_rays_are_the_oracle_camera():
    pa = _pa()
    S = TR.scene_of("quad_light")
    sg = A.build(pa.Scene(), S, pa.make_principled)
    so = A.build(O.OracleScene(), S, O.make_principled)
    rng = np.random.RandomState(1)
    for (W, H) in ((64, 48), (37, 91)):
        pix = np.stack([rng.randint(0, W, 300), rng.randint(0, H, 300)], 1)
        for p, seed in ((0, 1234567890), (17, 2718281828)):
            want = so.camera_rays(W, H, pix, p=p, seed_seq=seed)
            got = sg.CameraRays(W, H, np.concatenate([pix, np.full((len(pix), 1), p)], 1), seed_seq=seed)
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (W, H, p, seed)
    sg.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CAMERAS))
def test_user_camera_rays_match_the_float64_model(name):
    pa = _pa()
    eye, at, up, fov, lens, focus = CAMERAS[name]
    s = pa.Scene()  # (a user camera needs no committed scene)
    s.SetCamera(eye, at, up, fov, lens, focus)
    rng = np.random.RandomState(7)
    for W, H in ((64, 48), (33, 100)):
        cam = CA.LookAt(eye, at, up, fov, W, H, lens, focus)
        n = 2000
        x, y, p = rng.randint(0, W, n), rng.randint(0, H, n), rng.randint(0, 1 << 20, n)
        for seed in (1234567890, 99):
            o, d, raw = _rays(s, W, H, np.stack([x, y, p], 1), seed)
            assert (raw["tmin"] == 0).all() and (raw["tmax"] == np.float32(1.844e18)).all()
            dr = CA.sample_draws(W, x, y, p, seed, 4)
            mo, md = cam.rays(x, y, dr)
            scale = np.abs(np.asarray(eye, np.float32)).max() + lens
            assert np.abs(d - md).max() <= DIR_ULPS * EPS, (name, np.abs(d - md).max() / EPS)
            assert np.abs(o - mo).max() <= ORG_ULPS * EPS * scale, (name, np.abs(o - mo).max() / (EPS * scale))
            if lens == 0:
                assert (raw["org"] == np.asarray(eye, np.float32)).all()
            # the wrong draw order (lens before jitter) or a flipped axis is far outside the bound
            assert np.abs(cam.rays(x, H - 1 - y, dr)[1] - d).max() > 1e-3
            if lens:
                assert np.abs(cam.rays(x, y, dr[:, [2, 3, 0, 1]])[1] - d).max() > 1e-3
    s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["quad_light", "ggx_metallic"])
def test_radiance_through_an_oblique_camera(case):
    """test_analytic_radiance's statistics with the pinhole moved: GGX is view-dependent, so wo must come from the new camera"""
    pa = _pa()
    eye, at, up, fov, _, _ = CAMERAS["oblique"]
    W, H, K, spp = TR.W, TR.H, TR.K, TR.SPP
    cam = CA.LookAt(eye, at, up, fov, W, H)
    S = TR.scene_of(case)
    cls, val, _ = A.classify_and_expect(S, cam, A.Expectation(S))
    assert (cls == A.PIX_RECEIVER).sum() > 500 and (cls == A.PIX_ZERO).sum() > 0
    sg = A.build(pa.Scene(), S, pa.make_principled)
    sg.SetCamera(eye, at, up, fov)
    rgba, count = [], []
    for k in range(K):
        layer = pa.RenderLayer()
        pa.Render(sg, W, H, spp, layer=layer, first_pass=k * spp, seed_seq=TR.SEED_SEQ)
        rgba.append(np.array(layer.rgba, np.float32).reshape(H, W, 4))
        count.append(np.array(layer.count, np.uint32).reshape(H, W))
    sg.close()
    rgba, count = np.array(rgba), np.array(count)
    assert (count == spp).all() and (rgba[..., 3] == count).all()
    light, zero = cls == A.PIX_LIGHT, cls == A.PIX_ZERO
    want = count[..., None].astype(np.float32) * val.astype(np.float32)[None]
    assert (rgba[:, light, :3] == want[:, light]).all()
    assert (rgba[:, zero, :3] == 0).all()
    means = rgba[..., :3] / count[..., None]
    z, bar = TR.cell_stats(means, cls, val)
    print(f"{case} through the oblique camera: {len(z) - 1} cells, max |z| {np.abs(z).max():.2f} (bar {bar:.2f})")
    assert np.abs(z).max() < bar, (z, bar)
    z1, _ = TR.cell_stats(means, cls, val * 1.01)
    assert np.abs(z1).max() >= bar, ("1.01 E is not rejected", np.abs(z1).max(), bar)


def _plane_quad(cam, dist, a0, a1, b0, b1, Le):
    """an emitter facing the camera on the plane at distance dist along f, spanning sx in [a0, a1], sy in [b0, b1] of the image plane"""
    c = cam.eye + dist * (cam.f + 0.5 * (a0 + a1) * cam.r + 0.5 * (b0 + b1) * cam.u)
    v, f = A.quad(c, 0.5 * dist * (a1 - a0) * cam.r, 0.5 * dist * (b1 - b0) * cam.u)  # normal r x u = -f: towards the camera
    return A.Mesh("light", v, f, A.material(**A.BLACK), emission=np.tile([Le], (2, 1)))


def _coverage(cam, W, H, a0, a1, b0, b1, probe=8):
    """per pixel: the fraction of a probe x probe grid over the slightly widened footprint whose image-plane point is inside the box"""
    py, px = np.mgrid[0:H, 0:W]
    js = np.linspace(-0.02, 1.02, probe)
    jx, jy = np.meshgrid(js, js, indexing="ij")
    sx = (2.0 * (px[..., None] + jx.ravel()) / W - 1.0) * cam.h * W / H
    sy = (1.0 - 2.0 * (py[..., None] + jy.ravel()) / H) * cam.h
    return ((sx > a0) & (sx < a1) & (sy > b0) & (sy < b1)).mean(-1)


@pytest.mark.gpu
def test_depth_of_field():
    """an emitter on the focal plane is sharp for every lens sample; one at half the focus distance is blurred"""
    pa = _pa()
    W, H, spp = 64, 48, 16
    eye, at, up = (0.3, -0.2, 5.0), (0.1, 0.1, 0.0), (0.0, 1.0, 0.0)
    fov, lens = 30.0, 0.15
    cam = CA.LookAt(eye, at, up, fov, W, H, lens, 0.0)
    Le = np.array([2.0, 1.5, 0.5])
    near = (-0.05, 0.2, -0.1, 0.15)  # at half the focus distance: the lower right of the image, sharp edges where a pinhole sees them
    far = (-0.35, -0.05, 0.0, 0.2)   # on the focal plane
    S = A.Scene([_plane_quad(cam, cam.focus, *far, Le), _plane_quad(cam, 0.5 * cam.focus, *near, 2 * Le)], receiver=-1)
    sg = A.build(pa.Scene(), S, pa.make_principled)
    sg.SetCamera(eye, at, up, fov, lens)
    layer = pa.RenderLayer()
    pa.Render(sg, W, H, spp, layer=layer, seed_seq=5)
    img = np.array(layer.rgba, np.float32).reshape(H, W, 4)[..., :3]
    # a lens point lo moves a ray's crossing of the near plane by lo / focus on the unit image plane: the near quad's blur radius
    blur = lens / cam.focus
    cov_far = _coverage(cam, W, H, *far)
    near_wide = _coverage(cam, W, H, near[0] - 2 * blur, near[1] + 2 * blur, near[2] - 2 * blur, near[3] + 2 * blur)
    inside = (cov_far == 1) & (near_wide == 0)
    outside = (cov_far == 0) & (near_wide == 0)
    assert inside.sum() > 50 and outside.sum() > 200
    assert (img[inside] == (spp * Le).astype(np.float32)).all(), "the focal plane is not sharp"
    assert (img[outside] == 0).all()
    # the near quad: a pinhole would give exactly spp * 2 Le inside its image and 0 outside; within half the blur radius of its edge
    # a lens sample misses (hits) it with probability > 0.19, so nearly every such pixel differs from the pinhole's value
    cov_near = _coverage(cam, W, H, *near)
    h = 0.5 * blur
    edge_in = (cov_near == 1) & (_coverage(cam, W, H, near[0] + h, near[1] - h, near[2] + h, near[3] - h) < 1)
    edge_out = (cov_near == 0) & (_coverage(cam, W, H, near[0] - h, near[1] + h, near[2] - h, near[3] + h) > 0) & (cov_far == 0)
    assert edge_in.sum() > 10 and edge_out.sum() > 10
    assert (img[edge_in] < (spp * 2 * Le).astype(np.float32)).any(axis=-1).mean() > 0.8, "the near quad is sharp"
    assert (img[edge_out] > 0).any(axis=-1).mean() > 0.8, "the near quad does not spill past its pinhole image"
    sg.close()


def _lens_camera(s):
    bmin, bmax = (np.array(v, np.float64) for v in s.FetchSceneAABB())
    c, e = 0.5 * (bmin + bmax), bmax - bmin
    eye = c + np.array([0.3, 0.1, 0.45]) * e
    return eye, c - np.array([0.1, 0.05, 0.0]) * e, (0.1, 1.0, 0.0), 55.0, 0.02 * e.max(), 0.0


@pytest.mark.gpu
def test_no_camera_means_no_change():
    pa = _pa()
    s = _scene(pa)
    ref = _render(pa, s)
    eye, at, up, fov, lens, focus = _lens_camera(s)
    s.SetCamera(eye, at, up, fov, lens, focus)
    moved = _render(pa, s)
    assert not _same(moved, ref)
    s.SetCamera(None)
    assert _same(_render(pa, s), ref), "a reset camera changed the image"
    # invalid calls fail and leave the camera as it was
    s.SetCamera(eye, at, up, fov, lens, focus)
    bad = [dict(eye=eye, lookat=eye), dict(up=np.asarray(at) - np.asarray(eye)), dict(up=-3.0 * (np.asarray(at) - np.asarray(eye))),
           dict(fov=0.0), dict(fov=180.0), dict(fov=-5.0), dict(lens_radius=-0.1), dict(focus_distance=-1.0),
           dict(eye=(np.nan, 0, 0)), dict(lookat=(0, np.inf, 0)), dict(up=(0, 0, np.nan)), dict(fov=np.nan), dict(lens_radius=np.inf),
           dict(focus_distance=np.nan), dict(up=(0.0, 0.0, 0.0))]
    for kw in bad:
        args = dict(eye=eye, lookat=at, up=up, fov=fov, lens_radius=lens, focus_distance=focus)
        args.update(kw)
        with pytest.raises(pa.PbrHipError) as e:
            s.SetCamera(**args)
        assert e.value.code == EINVAL, kw
    assert _same(_render(pa, s), moved), "a rejected call changed the camera"
    s.close()


@pytest.mark.gpu
def test_camera_set_before_commit_is_the_camera_set_after():
    pa = _pa()
    S = TR.scene_of("quad_light")
    eye, at, up, fov, lens, focus = CAMERAS["lens"]
    after = A.build(pa.Scene(), S, pa.make_principled)
    after.SetCamera(eye, at, up, fov, lens, focus)
    before = pa.Scene()
    before.SetCamera(eye, at, up, fov, lens, focus)
    A.build(before, S, pa.make_principled)
    la, lb = pa.RenderLayer(), pa.RenderLayer()
    pa.Render(after, 48, 32, 8, layer=la)
    pa.Render(before, 48, 32, 8, layer=lb)
    assert np.array_equal(np.array(la.rgba, np.float32).view(np.uint32), np.array(lb.rgba, np.float32).view(np.uint32))
    assert np.array(la.rgba, np.float32).reshape(-1, 4)[:, :3].sum() > 0
    after.close(), before.close()


@pytest.mark.gpu
def test_thin_lens_is_schedule_independent():
    """hair + SSS + area light + environment through a thin lens: the first rays are stored once and every schedule loads them"""
    pa = _pa()
    s = _scene(pa)
    s.SetEnvironment(_env(), 1.0, EA.Z_UP)
    cam = _lens_camera(s)
    s.SetCamera(*cam)
    ref = _render(pa, s)
    assert ref[0].reshape(-1, 4)[:, :3].sum() > 0
    for kv in SCHEDULES + [dict(PBRHIP_FIRST_DIRECT=0), dict(PBRHIP_TAIL_PATHS=100000000, PBRHIP_SUSP_TURNS=1),
                           dict(PBRHIP_SUSP_TURNS=0, PBRHIP_DIRECT=0)]:
        with _Env(**kv):
            assert _same(_render(pa, s), ref), kv
    W, H, SPP = 48, 36, 8
    # chunked passes; the second half of the passes added to the first with NO_CLEAR
    layer = pa.RenderLayer()
    pa.Render(s, W, H, SPP, layer=layer, max_paths_in_flight=W * H * 3)
    assert _same((np.array(layer.rgba, np.float32), np.array(layer.count, np.uint32)), ref), "chunked"
    from pbrlab_amd import api
    layer = pa.RenderLayer()
    pa.Render(s, W, H, SPP // 2, layer=layer)
    pa.Render(s, W, H, SPP // 2, layer=layer, first_pass=SPP // 2, flags=api.RENDER_NO_CLEAR)
    assert _same((np.array(layer.rgba, np.float32), np.array(layer.count, np.uint32)), ref), "first_pass + NO_CLEAR"
    # shard blocks
    layer = pa.RenderLayer()
    pa.Render(s, W, H, SPP, layer=layer, shard_block=8)
    assert _same((np.array(layer.rgba, np.float32), np.array(layer.count, np.uint32)), ref), "shard_block"
    # the GPU tree builder
    g = _scene(pa, bvh=api.BVH_GPU_LBVH)
    g.SetEnvironment(_env(), 1.0, EA.Z_UP)
    g.SetCamera(*cam)
    assert _same(_render(pa, g), ref), "GPU LBVH"
    g.close()
    # RenderMulti over replicas (tiles of the world): the replica carries the camera
    r = pa.replicate(s, 0)
    layer = pa.RenderLayer()
    pa.RenderMulti([s, r], W, H, SPP, layer=layer)
    assert _same((np.array(layer.rgba, np.float32), np.array(layer.count, np.uint32)), ref), "RenderMulti"
    r.close()
    s.close()


@pytest.mark.gpu
def test_environment_under_rotated_cameras():
    """background pixels whose footprint lies inside one texel hold exactly count x L x scale, looking up, sideways and down"""
    pa = _pa()
    W, H, spp, scale = 48, 36, 4, 1.5
    rgb = EA.sky_map(16, 8, sun=(2, 5), sun_rgb=(40.0, 38.0, 30.0))
    S = EA.floor_scene()
    s = A.build(pa.Scene(), S, pa.make_principled)
    s.SetEnvironment(rgb, scale)
    for eye, at, up in (((0.0, 0.0, 0.5), (0.2, 0.1, 3.0), (0.0, 1.0, 0.0)), ((0.0, 0.0, 0.5), (3.0, 0.5, 0.6), (0.0, 0.0, 1.0)),
                        ((0.0, 0.0, 4.0), (0.0, 0.0, 0.0), (1.0, 0.0, 0.0))):
        cam = CA.LookAt(eye, at, up, 60.0, W, H)
        s.SetCamera(eye, at, up, 60.0)
        layer = pa.RenderLayer()
        pa.Render(s, W, H, spp, layer=layer)
        img = np.array(layer.rgba, np.float32).reshape(H, W, 4)
        r, c = EA.background_texels(S, cam, np.eye(3), rgb.shape[1], rgb.shape[0])
        bg = r >= 0
        assert bg.sum() > 30, (eye, at)
        one = rgb[r[bg], c[bg]] * np.float32(scale)
        want = np.zeros_like(one)
        for _ in range(spp):  # (the passes are added one by one, in float32)
            want = want + one
        assert (img[bg][:, :3] == want).all(), (eye, at)
    s.close()


@pytest.mark.gpu
def test_cli_camera(tmp_path):
    """pbrlab-hip-cli --eye --lookat: the sky sits above the horizon of a sideways camera and the floor below it"""
    from pbrlab_amd import io_api
    cli = os.path.join(ROOT, "pbrlab_amd", "pbrlab-hip-cli")
    obj = tmp_path / "floor.obj"
    (tmp_path / "floor.mtl").write_text("newmtl m\nKd 0.5 0.5 0.5\n")
    obj.write_text("mtllib floor.mtl\nusemtl m\nv -9 -9 0\nv 9 -9 0\nv 9 9 0\nv -9 9 0\nf 1 2 3\nf 1 3 4\n")
    L = 0.25
    hdr = tmp_path / "sky.hdr"
    w, h = 8, 4
    hdr.write_bytes(b"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n-Y %d +X %d\n" % (h, w) + bytes([128, 128, 128, 127]) * (w * h))
    out = tmp_path / "out.png"
    args = [cli, str(obj), "--width", "32", "--height", "24", "--spp", "4", "--env", str(hdr), "--env-scale", "2",
            "--eye", "0,-3,0.5", "--lookat", "0,0,0.5", "--up", "0,0,1", "--fov", "40", "--out", str(out)]
    for extra in ([], ["--gpus", "2"], ["--lens-radius", "0.05", "--focus", "3"]):
        r = subprocess.run(args + extra, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        img = io_api.png_decode(out.read_bytes())
        sky = io_api.layer_to_srgb8(np.array([[[4 * L * 2, 4 * L * 2, 4 * L * 2, 4.0]]], np.float32), np.array([[4]], np.uint32))
        assert img.shape[:2] == (24, 32)
        cam = CA.LookAt((0, -3, 0.5), (0, 0, 0.5), (0, 0, 1), 40.0, 32, 24)
        for y in (0, 1, 2):  # rows well above the horizon: only the sky
            assert cam.dirs(np.arange(32.0), np.full(32, float(y)), 1.0, 1.0)[:, 2].min() > 0.05
            assert (img[y, :, :3] == sky[0, 0, :3]).all(), (extra, y, img[y])
        assert cam.dirs(np.arange(32.0), np.full(32, 23.0), 0.0, 0.0)[:, 2].max() < -0.05
        assert (img[23, :, :3] != sky[0, 0, :3]).any(axis=-1).all(), extra  # the floor
    r = subprocess.run(args + ["--up", "0,1,0"], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "camera" in r.stderr, r.stderr


@pytest.mark.gpu
def test_camera_shim_caller_renders():
    import test_camera_cpu as TC
    TC.test_camera_shim_caller_compiles()
    r = subprocess.run([TC.EXE], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "camera ok" in r.stdout, r.stdout + r.stderr


# ---- the oracle's pinhole (orc_scene_set_camera): the same frame and the same ray, so rays and whole frames are compared bit for bit
PINHOLES = {  # name -> eye, lookat, up, fov
    "head_on": ((0.0, 0.0, 4.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 35.0),
    "oblique": CAMERAS["oblique"][:4],
    "zoom": ((0.031, -0.022, 0.035), (0.0005, 0.0002, -0.0003), (0.1, 0.2, 1.0), 0.35),   # vfov < 1 degree
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(PINHOLES))
def test_pinhole_rays_are_the_oracle_pinhole(name):
    pa = _pa()
    eye, at, up, fov = PINHOLES[name]
    sg, so = pa.Scene(), O.OracleScene()
    sg.SetCamera(eye, at, up, fov)
    so.SetCamera(eye, at, up, fov)
    rng = np.random.RandomState(3)
    for (W, H) in ((64, 48), (37, 91)):
        pix = np.stack([rng.randint(0, W, 300), rng.randint(0, H, 300)], 1)
        for p, seed in ((0, 1234567890), (17, 2718281828)):
            want = so.camera_rays(W, H, pix, p=p, seed_seq=seed)
            got = sg.CameraRays(W, H, np.concatenate([pix, np.full((len(pix), 1), p)], 1), seed_seq=seed)
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (name, W, H, p, seed)
            assert len(np.unique(want["dir"], axis=0)) == len(np.unique(pix, axis=0))  # (float32 still tells the pixels of the zoom apart)
    with pytest.raises(ValueError):
        so.SetCamera(eye, at, up, fov, lens_radius=0.05)
    assert np.array_equal(so.camera_rays(W, H, pix, p=p, seed_seq=seed).view(np.uint32), want.view(np.uint32)), "a refused call changed the camera"
    sg.close()


def _oblique_inside(s):
    """an oblique pinhole inside the scene's box, looking across it"""
    bmin, bmax = (np.array(v, np.float64) for v in s.FetchSceneAABB())
    c, e = 0.5 * (bmin + bmax), bmax - bmin
    return c + np.array([0.31, 0.12, 0.42]) * e, c - np.array([0.12, 0.07, 0.05]) * e, (0.1, 1.0, 0.05), 58.0


@pytest.mark.gpu
@pytest.mark.parametrize("tail", [0xFFFFFFFF, 0])
@pytest.mark.parametrize("name", ["lambert", "hair"])
def test_frames_through_an_oblique_pinhole_are_the_oracle_frames(name, tail):
    """the first user-camera frames compared bit for bit with anything: every kernel behind k_generate_camera against the oracle"""
    from golden.make_golden import golden_scenes
    pa = _pa()
    desc = golden_scenes()[name]
    sg, so = pa.scene_from_desc(desc), O.oracle_scene_from_desc(desc)
    cam = _oblique_inside(so)
    W, H, spp = 64, 48, 4
    layer = pa.RenderLayer()
    plain = pa.RenderLayer()
    pa.Render(sg, W, H, spp, layer=plain, tail_paths=tail)
    sg.SetCamera(*cam)
    so.SetCamera(*cam)
    ok, st = pa.Render(sg, W, H, spp, layer=layer, flags=pa.api.RENDER_STATS, tail_paths=tail)
    assert (st["n_tail"] == 0) == (tail == 0xFFFFFFFF)
    rgba, cnt, ost = so.render(W, H, spp, threads=4, math_mode=O.MATH_DEVICE)
    got = np.array(layer.rgba, np.float32).reshape(H, W, 4)
    assert (cnt == spp).all() and np.array_equal(np.array(layer.count, np.uint32).reshape(H, W), cnt)
    assert np.array_equal(got.view(np.uint32), rgba.view(np.uint32)), int((got != rgba).any(-1).sum())
    assert (st["closest_rays"] + st["tail_closest_rays"] + st["pruned_rays"], st["shadow_rays"] + st["tail_shadow_rays"]) == \
        (ost["closest_rays"], ost["shadow_rays"])
    assert (rgba[..., :3].sum(-1) > 0).mean() > 0.5 and not np.array_equal(got, np.array(plain.rgba, np.float32).reshape(H, W, 4))
    if name == "hair":
        assert ost["curves_tested"] > 0
    so.SetCamera(None)
    fx = np.load(os.path.join(ROOT, "tests", "golden", "oracle_images.npz"))
    back = so.render(64, 64, 4, threads=4, math_mode=O.MATH_LIBM)[0]
    assert np.array_equal(back, fx[f"{name}_libm_rgba"]) or not O.libm_is_glibcf(), "a reset camera is not the reference's camera"
    sg.close()
