"""Rendering along caller-supplied rays and the three projections on the GPU.

- The built-in cameras replayed from their own rays, bit for bit; one list of rays with mixed origins against the oracle's frames.
- Bit-identity across schedules, chunking, pass ranges, shards, builders and the three ways to hand rays over.
- tmin / tmax, inactive rays, the feature buffers over rays.
- The projections against the float64 model of tests/_projection_model.py, a lat-long panorama of an environment texel for texel, the
  CLI and the C++ shim."""
import os
import subprocess

import numpy as np
import pytest

import _env_analytic as EA
import _oracle as O
import _projection_model as PM
import test_features_gpu as TF
from test_analytic_radiance import _pa
from test_camera_gpu import _lens_camera, _oblique_inside
from test_env_gpu import SCHEDULES, _Env, _env
from test_env_gpu import _scene as _rich_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 1234567890
KINF = np.float32(1.844e18)


def _camera_rays(s, W, H, spp, first_pass=0, seed=SEED):
    """the scene's own camera ray of every (pass, y, x): RAY_DT (spp, H, W)"""
    yy, xx = np.mgrid[0:H, 0:W]
    xyp = np.stack([np.broadcast_to(xx, (spp, H, W)), np.broadcast_to(yy, (spp, H, W)),
                    np.broadcast_to(np.arange(first_pass, first_pass + spp)[:, None, None], (spp, H, W))], -1)
    return s.CameraRays(W, H, xyp.reshape(-1, 3), seed_seq=seed).reshape(spp, H, W)


def _out(layer):
    return np.array(layer.rgba, np.float32).copy(), np.array(layer.count, np.uint32).copy()


def _same(a, b):
    return np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and np.array_equal(a[1], b[1])


def _render(pa, s, W, H, spp, **kw):
    layer = pa.RenderLayer()
    pa.Render(s, W, H, spp, layer=layer, **kw)
    return _out(layer)


def _render_rays(pa, s, rays, spp, **kw):
    return _out(pa.RenderRays(s, rays, spp, **kw))


_cache = {}


def _golden(name):
    if name not in _cache:
        from golden.make_golden import golden_scenes
        _cache[name] = _pa().scene_from_desc(golden_scenes()[name])
    return _cache[name]


def _rich(bvh=None):
    """hair + SSS + area light + environment through a thin lens (test_camera_gpu's schedule scene) -> scene, its lens camera"""
    key = ("rich", bvh)
    if key not in _cache:
        s = _rich_scene(_pa(), bvh)
        s.SetEnvironment(_env(), 1.0, EA.Z_UP)
        _cache[key] = s
    s = _cache[key]
    s.SetCamera(*_lens_camera(s))
    return s


# ---------------------------------------------------------------------------------------------------- 1: replay of the built-in cameras
@pytest.mark.gpu
@pytest.mark.parametrize("tail", [0, 0xFFFFFFFF])
@pytest.mark.parametrize("case", ["lambert/reference", "lambert/pinhole", "hair/reference", "hair/pinhole", "rich/lens"])
def test_replay_of_the_built_in_cameras_is_bit_exact(case, tail):
    pa = _pa()
    name, cam = case.split("/")
    if name == "rich":
        s, (W, H, spp), draws = _rich(), (48, 36, 8), 4
    else:
        s, (W, H, spp), draws = _golden(name), (64, 48, 4), 2
        s.SetCamera(*_oblique_inside(s)) if cam == "pinhole" else s.SetCamera(None)
    want = _render(pa, s, W, H, spp, tail_paths=tail)
    rays = _camera_rays(s, W, H, spp)
    s.SetCamera(None)  # (the rays are the camera now)
    got = _render_rays(pa, s, rays, spp, camera_draws=draws, tail_paths=tail)
    assert (got[1] == spp).all() and (got[0][..., :3].sum(-1) > 0).any()
    assert _same(got, want), (case, int((got[0] != want[0]).any(-1).sum()))
    # the draws matter: with the camera's own draws handed to the path again the frame is another one
    assert not _same(_render_rays(pa, s, rays, spp, camera_draws=0, tail_paths=tail), want)


# ---------------------------------------------------------------------------------------------------- 2: mixed origins against the oracle
@pytest.mark.gpu
def test_mixed_origins_give_each_pixel_the_oracle_frame_of_its_camera():
    from golden.make_golden import golden_scenes
    pa = _pa()
    sg, so = _golden("lambert"), O.oracle_scene_from_desc(golden_scenes()["lambert"])
    sg.SetCamera(None)
    W, H, spp = 48, 36, 4
    bmin, bmax = (np.array(v, np.float64) for v in so.FetchSceneAABB())
    c, e = 0.5 * (bmin + bmax), bmax - bmin
    cams = [_oblique_inside(so), (c + np.array([-0.3, 0.25, 0.4]) * e, c + np.array([0.1, -0.1, -0.1]) * e, (0.0, 1.0, 0.1), 50.0),
            (c + np.array([0.1, -0.2, 0.44]) * e, c + np.array([-0.05, 0.15, 0.0]) * e, (0.2, 1.0, 0.0), 66.0)]
    yy, xx = np.mgrid[0:H, 0:W]
    which = (yy * W + xx) % 3
    rays = np.zeros((spp, H, W), pa.api.RAY_DT)
    frames = []
    for k, cam in enumerate(cams):
        so.SetCamera(*cam)
        rgba, cnt, _ = so.render(W, H, spp, threads=4, math_mode=O.MATH_DEVICE)
        assert (cnt == spp).all()
        frames.append(rgba)
        pix = np.stack([xx[which == k], yy[which == k]], 1)
        for p in range(spp):
            rays[p][which == k] = so.camera_rays(W, H, pix, p=p)
    assert len(np.unique(rays["org"].reshape(-1, 3), axis=0)) == 3
    got, count = _render_rays(pa, sg, rays, spp)
    want = np.choose(which[..., None], frames)
    assert (count == spp).all() and (got[..., 3] == spp).all()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), int((got != want).any(-1).sum())
    assert (got[..., :3].sum(-1) > 0).mean() > 0.5
    for k in range(3):  # (the three frames differ where it matters: a pixel of one is not a pixel of another)
        assert not np.array_equal(frames[k][which == k], frames[(k + 1) % 3][which == k])


# ---------------------------------------------------------------------------------------------------- 3: schedule independence
@pytest.mark.gpu
def test_ray_frames_are_schedule_independent():
    import torch
    pa = _pa()
    api = pa.api
    s = _rich()
    W, H, spp = 48, 36, 8
    rays = _camera_rays(s, W, H, spp)
    s.SetCamera(None)
    ref = _render_rays(pa, s, rays, spp, camera_draws=4)
    assert ref[0][..., :3].sum() > 0
    for kv in SCHEDULES + [dict(PBRHIP_FIRST_DIRECT=0), dict(PBRHIP_TAIL_PATHS=100000000, PBRHIP_SUSP_TURNS=1), dict(PBRHIP_SUSP_TURNS=0, PBRHIP_DIRECT=0)]:
        with _Env(**kv):
            assert _same(_render_rays(pa, s, rays, spp, camera_draws=4), ref), kv
    assert _same(_render_rays(pa, s, rays, spp, camera_draws=4, max_paths_in_flight=W * H * 3), ref), "chunked"
    # the two halves of the passes: the second call's buffer starts at its own first pass
    layer = pa.RenderRays(s, rays[:spp // 2], spp // 2, camera_draws=4)
    pa.RenderRays(s, rays[spp // 2:], spp // 2, layer, camera_draws=4, first_pass=spp // 2, flags=api.RENDER_NO_CLEAR)
    assert _same(_out(layer), ref), "first_pass + NO_CLEAR"
    assert _same(_render_rays(pa, s, rays, spp, camera_draws=4, shard_block=8), ref), "shard_block"
    parts = [_render_rays(pa, s, rays, spp, camera_draws=4, tile_rank=r, tile_world=2, shard_block=8) for r in range(2)]
    assert ((parts[0][1] > 0) != (parts[1][1] > 0)).all() and (parts[0][1] > 0).any() and (parts[1][1] > 0).any()
    assert _same((parts[0][0] + parts[1][0], parts[0][1] + parts[1][1]), ref), "tile_world = 2"
    g = _rich(api.BVH_GPU_LBVH)
    g.SetCamera(None)
    assert _same(_render_rays(pa, g, rays, spp, camera_draws=4), ref), "GPU LBVH"
    # the same rays as a float32 host array, behind a device pointer, and as a torch tensor filled on a stream of its own
    flat = rays.view(np.float32).reshape(spp, H, W, 8)
    assert _same(_render_rays(pa, s, flat, spp, camera_draws=4), ref), "float32 host array"
    buf = api.DeviceRays((spp, H, W), s.device).upload(rays)
    assert _same(_render_rays(pa, s, (buf.ptr, (spp, H, W)), spp, camera_draws=4), ref), "device pointer"
    assert _same(_render_rays(pa, s, buf, spp, camera_draws=4), ref), "DeviceRays"
    buf.close()
    side = torch.cuda.Stream()
    pinned = torch.from_numpy(flat.copy()).pin_memory()
    with torch.cuda.stream(side):
        t = torch.zeros((spp, H, W, 8), dtype=torch.float32, device="cuda:0")
        t.copy_(pinned, non_blocking=True)
        got = _render_rays(pa, s, t, spp, camera_draws=4)  # (stream=None: torch's current stream, the side stream)
        rgba = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0")
        count = torch.zeros((H, W), dtype=torch.int32, device="cuda:0")
        side.synchronize()
        pa.RenderRays(s, t, spp, camera_draws=4, device_out=(rgba.data_ptr(), count.data_ptr()))
    assert _same(got, ref), "torch tensor on a side stream"
    assert _same((rgba.cpu().numpy(), count.cpu().numpy().astype(np.uint32)), ref), "device_out"


# ---------------------------------------------------------------------------------------------------- 4: one ray per pixel
@pytest.mark.gpu
def test_one_plane_of_rays_is_that_plane_repeated():
    pa = _pa()
    s = _golden("hair")
    s.SetCamera(*_oblique_inside(s))
    W, H, spp = 48, 36, 6
    plane = _camera_rays(s, W, H, 1, first_pass=3)[0]
    s.SetCamera(None)
    one = _render_rays(pa, s, plane, spp)
    assert one[0][..., :3].sum() > 0 and (one[1] == spp).all()
    assert _same(_render_rays(pa, s, np.broadcast_to(plane, (spp, H, W)).copy(), spp), one)
    assert _same(_render_rays(pa, s, plane[None], spp, max_paths_in_flight=2 * W * H), one), "(1, H, W), chunked"
    # ... under a pass range too: the one plane serves every pass of the call
    layer = pa.RenderRays(s, plane, 2)
    pa.RenderRays(s, plane, spp - 2, layer, first_pass=2, flags=pa.api.RENDER_NO_CLEAR)
    assert _same(_out(layer), one)


# ---------------------------------------------------------------------------------------------------- 5: tmin / tmax, inactive rays
def _set(field, value, k=None):
    def mutate(r):  # r: one ray as a RAY_DT array of length 1
        if k is None:
            r[field][0] = value
        else:
            r[field][0, k] = value
    return mutate


def _empty_interval(r):
    r["tmin"][0], r["tmax"][0] = 2.0, 1.0


# every way for a ray to be inactive: a NaN or an infinity in the origin or the direction, a NaN bound, a negative or infinite tmin, a
# zero direction, tmax < tmin
INACTIVE = ([_set(f, v, k) for f, k in (("org", 0), ("org", 2), ("dir", 1)) for v in (np.nan, np.inf, -np.inf)] +
            [_set("tmin", np.nan), _set("tmax", np.nan), _set("tmin", -1e-3), _set("tmin", np.inf), _set("dir", 0.0), _empty_interval,
             _set("tmax", -np.inf)])


@pytest.mark.gpu
def test_tmin_tmax_and_inactive_rays():
    pa = _pa()
    s = _golden("lambert")
    s.SetCamera(*_oblique_inside(s))
    W, H, spp = 48, 36, 4
    rays = _camera_rays(s, W, H, spp)
    s.SetCamera(None)
    full = _render_rays(pa, s, rays, spp)
    hits = s.trace_closest(rays.reshape(-1)).reshape(spp, H, W)
    hit = hits["instance_id"] != 0xFFFFFFFF
    assert hit.mean() > 0.5
    # rays that end short of their first hit see nothing: no environment here, so exactly 0
    short = rays.copy()
    short["tmax"] = np.where(hit, hits["t"] * np.float32(0.99), np.float32(1.0))
    got = _render_rays(pa, s, short, spp)
    assert (got[0][..., :3] == 0).all() and (got[0][..., 3] == spp).all() and (got[1] == spp).all()
    # ... rays that start just behind it see something else, rays that end just behind it see the same
    longer = rays.copy()
    longer["tmax"] = np.where(hit, hits["t"] * np.float32(1.01), KINF)
    assert _same(_render_rays(pa, s, longer, spp), full)
    behind = rays.copy()
    behind["tmin"] = np.where(hit, hits["t"] * np.float32(1.01), np.float32(0.0))
    assert not _same(_render_rays(pa, s, behind, spp), full)
    # inactive rays of every kind scattered among live ones: (0, 0, 0, spp) there, the frame elsewhere -- with an environment too
    rng = np.random.RandomState(5)
    dead = np.zeros((H, W), bool)
    mixed = rays.copy()
    for i, p in enumerate(rng.choice(W * H, 5 * len(INACTIVE), replace=False)):
        y, x = divmod(int(p), W)
        dead[y, x] = True
        for q in range(spp):  # the pixel's own ray but for the one broken number, another kind in every pass
            r = rays[q, y, x:x + 1].copy()
            INACTIVE[(i + q) % len(INACTIVE)](r)
            mixed[q, y, x] = r[0]
    one_kind = rays.copy()  # a pixel that is dead in two of its four passes holds the other two
    one_kind["dir"][1, 5, 7] = np.nan
    one_kind["tmin"][2, 5, 7] = -1.0
    try:
        for env in (False, True):
            if env:
                s.SetEnvironment(EA.sky_map(16, 8, sun=(2, 5), sun_rgb=(40.0, 38.0, 30.0)), 1.5)
            base = _render_rays(pa, s, rays, spp)
            assert _same(base, full) != env
            got = _render_rays(pa, s, mixed, spp)
            assert (got[0][dead] == np.array([0, 0, 0, spp], np.float32)).all() and (got[1] == spp).all(), env
            assert np.array_equal(got[0][~dead].view(np.uint32), base[0][~dead].view(np.uint32)), env
            assert (base[0][dead][:, :3].sum(-1) > 0).any()
            part = _render_rays(pa, s, one_kind, spp)
            assert part[1][5, 7] == spp and part[0][5, 7, 3] == spp and np.array_equal(np.delete(part[0].reshape(-1, 4), 5 * W + 7, 0), np.delete(base[0].reshape(-1, 4), 5 * W + 7, 0))
            alive = _out(pa.RenderRays(s, rays[0:1], 1))[0][5, 7, :3] + _out(pa.RenderRays(s, rays[3:4], 1, first_pass=3))[0][5, 7, :3]
            assert np.array_equal(part[0][5, 7, :3], alive), (env, part[0][5, 7], alive)
    finally:
        s.SetEnvironment(None)


# ---------------------------------------------------------------------------------------------------- 6: feature buffers
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cornell", "hair"])
def test_feature_buffers_over_a_pinholes_rays_are_render_features(name):
    import torch
    pa = _pa()
    _, s = TF._scene(name)
    eye, at, up, fov = TF.LENS_CAMERAS[name][:4]
    s.SetCamera(eye, at, up, fov)
    W, H, spp = 50, 38, 5
    want = pa.RenderFeatures(s, W, H, spp, first_pass=2)
    rays = _camera_rays(s, W, H, spp, first_pass=2)
    s.SetCamera(None)
    got = pa.RenderFeaturesRays(s, rays, spp, first_pass=2)
    assert want.albedo[..., 3].sum() > 0.2 * spp * W * H
    for a, b in ((got.albedo, want.albedo), (got.normal_depth, want.normal_depth), (got.count, want.count)):
        assert np.array_equal(TF._bits(a), TF._bits(b))
    # chunked, in two calls, and from a tensor into device buffers
    assert TF._same(pa.RenderFeaturesRays(s, rays, spp, first_pass=2, max_paths_in_flight=2 * W * H), want)
    half = pa.RenderFeaturesRays(s, rays[:2], 2, first_pass=2)
    pa.RenderFeaturesRays(s, rays[2:], spp - 2, half, first_pass=4, no_clear=True)
    assert TF._same(half, want)
    t = torch.from_numpy(rays.view(np.float32).reshape(spp, H, W, 8).copy()).to("cuda:0")
    a = torch.full((H, W, 4), 3.0, dtype=torch.float32, device="cuda:0")
    n = torch.full((H, W, 4), 3.0, dtype=torch.float32, device="cuda:0")
    c = torch.full((H, W), 9, dtype=torch.int32, device="cuda:0")
    pa.RenderFeaturesRays(s, t, spp, first_pass=2, device_out=(a.data_ptr(), n.data_ptr(), c.data_ptr()))
    assert np.array_equal(TF._bits(a.cpu().numpy()), TF._bits(want.albedo)) and np.array_equal(TF._bits(n.cpu().numpy()), TF._bits(want.normal_depth))
    assert np.array_equal(c.cpu().numpy().astype(np.uint32), want.count)
    # an inactive ray and a ray cut short are misses
    cut = rays.copy()
    cut["tmax"][:, 0:10] = 1e-3
    cut["dir"][:, 10:20] = np.nan
    f = pa.RenderFeaturesRays(s, cut, spp, first_pass=2)
    assert (f.count == spp).all() and (f.albedo[:20] == 0).all() and (f.normal_depth[:20] == 0).all()
    assert np.array_equal(TF._bits(f.albedo[20:]), TF._bits(want.albedo[20:]))


# ---------------------------------------------------------------------------------------------------- 7: projection rays
CAMERA = ((1.2, -1.6, 1.4), (0.0, 0.0, 0.1), (0.0, 0.0, 1.0), 50.0)
# Each direction component within 2e-6 of the float64 model: the float32 roundings of an angle up to pi (at most four, 1.9e-7 each),
# f_sin / f_cos under one ulp, five roundings in the frame sum.  About 1/50 000 of a pixel's angle at these sizes.
TOL = 2e-6


@pytest.mark.gpu
@pytest.mark.parametrize("size", [(64, 32), (37, 91)])
def test_projection_rays_match_the_float64_model(size):
    pa = _pa()
    W, H = size
    eye, at, up, fov = CAMERA
    s = pa.Scene()  # (a frame needs no committed scene)
    with pytest.raises(pa.PbrHipError) as e:
        s.ProjectionRays("latlong", W, H, 0, 1)
    assert e.value.code == -6
    s.SetCamera(eye, at, up, fov)
    cam = PM.frame(eye, at, up)
    scale = float(np.abs(np.asarray(eye)).max()) + 2.5 * max(1.0, W / H)
    for p in (0, 17):
        jx, jy = PM.jitters(W, H, p)
        for proj, name, param in ((PM.LATLONG, "latlong", 0.0), (PM.FISHEYE, "fisheye", 0.0), (PM.FISHEYE, "fisheye", 180.0),
                                  (PM.FISHEYE, "fisheye", 360.0), (PM.ORTHO, "ortho", 2.5)):
            buf = s.ProjectionRays(name, W, H, p, 1, param)
            got = buf.numpy()[0]
            buf.close()
            org, d, active, rho = PM.rays(proj, cam, W, H, jx, jy, param=param, fov=fov)
            edge = np.abs(rho - 1) <= 1e-5  # fisheye pixels on the image circle itself: either side may call them
            assert edge.mean() < 0.01
            live = (got["dir"] != 0).any(-1)
            assert np.array_equal(live[~edge], active[~edge]), (name, param, p)
            assert (got["tmin"] == 0).all() and (got["tmax"][live] == KINF).all() and (got["tmax"][~live] == 0).all()
            m = live & active
            assert m.mean() > (0.15 if proj == PM.FISHEYE else 0.99)
            err = np.abs(got["dir"][m].astype(np.float64) - d[m]).max()
            oerr = np.abs(got["org"].astype(np.float64) - org).max()
            print(f"{name} {param} {W}x{H} pass {p}: direction error {err:.2e}, origin error {oerr:.2e}")
            assert err <= TOL, (name, param, p, err)
            assert oerr <= TOL * scale, (name, param, p, oerr)
            # a mapping off by a pixel, or mirrored, is far outside the bound
            if proj != PM.ORTHO:
                assert np.abs(PM.rays(proj, cam, W, H, jx + 1, jy, param=param, fov=fov)[1][m] - got["dir"][m]).max() > 1e-3
                assert np.abs(PM.rays(proj, cam, W, H, jx, H - 2.0 * np.arange(H)[:, None] - jy, param=param, fov=fov)[1][m] - got["dir"][m]).max() > 1e-3
    # several passes in one call are the single passes, and a tensor takes them as well
    both = s.ProjectionRays("latlong", W, H, 16, 2).numpy()
    assert np.array_equal(both[1].view(np.uint32), s.ProjectionRays("latlong", W, H, 17, 1).numpy()[0].view(np.uint32))
    import torch
    t = torch.zeros((2, H, W, 8), dtype=torch.float32, device="cuda:0")
    s.ProjectionRays("latlong", W, H, 16, 2, out=t)
    torch.cuda.synchronize()
    assert np.array_equal(t.cpu().numpy().view(np.uint32).reshape(2, H, W, 8), both.view(np.uint32).reshape(2, H, W, 8))
    s.close()


# ---------------------------------------------------------------------------------------------------- 8: a panorama of an environment
@pytest.mark.gpu
def test_latlong_panorama_of_an_environment_is_the_environment():
    """§10's direction -> texel mapping and the lat-long camera are inverses: a panorama as large as the map holds the map"""
    pa = _pa()
    W, H, spp, scale = 48, 24, 4, 1.5
    rng = np.random.RandomState(11)
    blocks = rng.uniform(0.1, 4.0, (H // 3, W // 3, 3)).astype(np.float32)
    rgb = np.repeat(np.repeat(blocks, 3, 0), 3, 1)
    s = pa.Scene()
    v = np.array([[-0.05, -5.0, -0.05, 1], [0.05, -5.0, -0.05, 1], [0.0, -5.0, 0.05, 1]], np.float32)  # straight below: the bottom rows only
    mat = s.AddMaterialParam(pa.make_principled(dict(TF_BLACK)))
    mesh = s.AddTriangleMesh(v, None, None, [[0, 1, 2]], material_ids=[mat])
    ls = s.CreateLocalScene()
    s.AddMeshToLocalScene(ls, mesh)
    s.CreateInstance(ls)
    s.CommitScene()
    s.SetEnvironment(rgb, scale)
    s.SetCamera((0.0, 0.0, 0.0), (0.0, 0.0, -1.0), (0.0, 1.0, 0.0))  # r = +x, u = +y, f = -z
    layer = pa.RenderProjection(s, "latlong", W, H, spp)
    img, count = _out(layer)
    assert (count == spp).all()
    one = blocks * np.float32(scale)
    want = np.zeros_like(one)
    for _ in range(spp):  # (the passes are added one by one, in float32)
        want = want + one
    centres = img[1::3, 1::3]
    free = np.ones((H // 3, W // 3), bool)
    free[-1] = False  # the block row the triangle lies in
    assert np.array_equal(centres[free][:, :3], want[free]) and (centres[..., 3] == spp).all()
    # ... and the whole image but the seams' neighbours, which a jittered sample may cross: every pixel holds a sum of its 3 x 3 blocks' values
    assert (img[:-3, :, :3] > 0).all()
    # chunked by a small ray buffer, the same frame
    from pbrlab_amd import api
    old = api.RAY_BUFFER_BYTES
    api.RAY_BUFFER_BYTES = 32 * W * H + 5
    try:
        assert _same(_out(pa.RenderProjection(s, "latlong", W, H, spp)), (img, count))
    finally:
        api.RAY_BUFFER_BYTES = old
    s.close()


TF_BLACK = dict(base_color=(0.0, 0.0, 0.0), subsurface=0.0, subsurface_radius=(1.0, 1.0, 1.0), subsurface_color=(0.0, 0.0, 0.0), metallic=0.0,
                specular=0.0, specular_tint=0.0, roughness=1.0, anisotropic=0.0, anisotropic_rotation=0.0, sheen=0.0, sheen_tint=0.0,
                clearcoat=0.0, clearcoat_roughness=0.0, ior=1.5, transmission=0.0, transmission_roughness=0.0, base_color_tex_id=0xFFFFFFFF,
                subsurface_color_tex_id=0xFFFFFFFF)


# ---------------------------------------------------------------------------------------------------- 9: CLI and shim
@pytest.mark.gpu
def test_cli_projection(tmp_path):
    """pbrlab-hip-cli --projection: a panorama has the sky in its top rows and the floor in its bottom rows; a fisheye has black corners"""
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
            "--eye", "0,-3,0.5", "--lookat", "0,0,0.5", "--up", "0,0,1", "--out", str(out)]
    sky = io_api.layer_to_srgb8(np.array([[[4 * L * 2, 4 * L * 2, 4 * L * 2, 4.0]]], np.float32), np.array([[4]], np.uint32))[0, 0, :3]
    r = subprocess.run(args + ["--projection", "latlong"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    img = io_api.png_decode(out.read_bytes())
    assert img.shape[:2] == (24, 32)
    assert (img[:10, :, :3] == sky).all(), img[:10]  # above the horizon (row 12), all around: only the sky
    # below it: the floor, 0.5 under the eye and 18 wide.  Albedo 0.5 under a uniform sky: half the sky's radiance on average, though a single
    # pixel's four samples may reach it
    assert (img[16:, :, :3] != sky).any(axis=-1).mean() > 0.9 and img[16:, :, :3].mean() < sky[0] - 5.0
    r = subprocess.run(args + ["--projection", "fisheye", "--fov", "180"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    img = io_api.png_decode(out.read_bytes())
    for y, x in ((0, 0), (0, 31), (23, 0), (23, 31), (2, 3)):  # outside the image circle: no ray, exactly black
        assert (img[y, x, :3] == 0).all(), (y, x, img[y, x])
    assert (img[2, 14:18, :3] == sky).all() and img[20:23, 13:19, :3].mean() < sky[0] - 5.0  # up is sky, down is floor
    down = args[:args.index("--eye")] + ["--eye", "0,0,5", "--lookat", "0,0,0", "--up", "0,1,0", "--out", str(out)]
    r = subprocess.run(down + ["--projection", "ortho", "--ortho-height", "24"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    img = io_api.png_decode(out.read_bytes())
    # straight down on a view 32 x 24 wide: the 18 x 18 floor in the middle, the sky (seen from above, past the floor's edge) around it
    assert (img[:3, :, :3] == sky).all() and (img[21:, :, :3] == sky).all() and (img[:, :6, :3] == sky).all()
    assert (img[4:20, 8:24, :3] != sky).any(axis=-1).mean() > 0.9 and img[4:20, 8:24, :3].mean() < sky[0] - 5.0


@pytest.mark.gpu
def test_rays_shim_caller_renders():
    import test_rays_cpu as TC
    _pa()
    TC.test_rays_shim_caller_compiles()
    r = subprocess.run([TC.EXE], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "rays ok" in r.stdout, (r.returncode, r.stdout + r.stderr)
