"""The environment light on the GPU: exactness, schedules, the C ABI's checks and the CLI.

- An all-black map, and a map set then removed, render bit-identically to the scene that never had one (today's kernels).
- A scene with hair, random-walk SSS, an area light and an environment (every environment kernel reached) renders bit-identically
  across the schedules: PBRHIP_DIRECT, PBRHIP_TAIL_PATHS, PBRHIP_SUSP_TURNS, PBRHIP_WIDE, PBRHIP_GROUPS, PBRHIP_QUAD_RAYS, the GPU
  tree builder, chunked passes, RenderMulti."""
import os
import subprocess

import numpy as np
import pytest

import _env_analytic as EA
from test_analytic_radiance import _pa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, SPP = 48, 36, 8


def _scene(pa, bvh=None):
    from pbrlab_amd import scenes
    s = pa.scene_from_desc(scenes.cornell_hair_scene("sss", n_strands=200, n_segments=5, monkey_subdiv=2, lucy_nu=64, lucy_nv=12),
                           **({} if bvh is None else dict(bvh_builder=bvh)))
    return s


def _render(pa, s, spp=SPP, **kw):
    layer = pa.RenderLayer()
    pa.Render(s, W, H, spp, layer=layer, **kw)
    return np.array(layer.rgba, np.float32).copy(), np.array(layer.count, np.uint32).copy()


def _same(a, b):
    return np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and np.array_equal(a[1], b[1])


def _env():
    return EA.sky_map(16, 8, sun=(2, 5), sun_rgb=(40.0, 38.0, 30.0))


class _Env:
    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        os.environ.update({k: str(v) for k, v in self.kv.items()})

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.mark.gpu
def test_black_or_removed_environment_is_no_environment():
    pa = _pa()
    s = _scene(pa)
    ref = _render(pa, s)
    s.SetEnvironment(np.zeros((8, 16, 3), np.float32))
    assert _same(_render(pa, s), ref), "an all-black map changed the image"
    s.SetEnvironment(_env(), 1.0)
    lit = _render(pa, s)
    assert not _same(lit, ref)
    s.SetEnvironment(None)
    assert _same(_render(pa, s), ref), "a removed environment changed the image"
    s.close()


@pytest.mark.gpu
def test_environment_set_after_commit_takes_effect_and_scales():
    pa = _pa()
    s = _scene(pa)
    s.SetEnvironment(_env(), 1.0)
    a = _render(pa, s)
    s.SetEnvironment(_env(), 2.0)
    b = _render(pa, s)
    assert not _same(a, b) and np.array_equal(b[0].reshape(-1, 4)[:, 3], a[0].reshape(-1, 4)[:, 3])
    assert b[0].reshape(-1, 4)[:, :3].sum() > 1.5 * a[0].reshape(-1, 4)[:, :3].sum()
    s.close()


SCHEDULES = [
    dict(PBRHIP_DIRECT=0), dict(PBRHIP_DIRECT=1), dict(PBRHIP_TAIL_PATHS=0), dict(PBRHIP_TAIL_PATHS=100000000),
    dict(PBRHIP_SUSP_TURNS=0), dict(PBRHIP_SUSP_TURNS=1), dict(PBRHIP_WIDE=0), dict(PBRHIP_WIDE=1), dict(PBRHIP_GROUPS="3,2,3"),
    dict(PBRHIP_QUAD_RAYS=100000000), dict(PBRHIP_SSS_WALK=0),
]


@pytest.mark.gpu
def test_environment_scene_is_schedule_independent():
    pa = _pa()
    s = _scene(pa)
    s.SetEnvironment(_env(), 1.0, EA.Z_UP)
    ref = _render(pa, s)
    assert ref[0].reshape(-1, 4)[:, :3].sum() > 0
    for kv in SCHEDULES:
        with _Env(**kv):
            assert _same(_render(pa, s), ref), kv
    # chunked passes: two halves added into one layer
    layer = pa.RenderLayer()
    pa.Render(s, W, H, SPP, layer=layer, max_paths_in_flight=W * H * 3)
    assert _same((np.array(layer.rgba, np.float32), np.array(layer.count, np.uint32)), ref), "chunked"
    # the GPU tree builder
    from pbrlab_amd import api
    g = _scene(pa, bvh=api.BVH_GPU_LBVH)
    g.SetEnvironment(_env(), 1.0, EA.Z_UP)
    assert _same(_render(pa, g), ref), "GPU LBVH"
    g.close()
    # RenderMulti over replicas on one device: the replica carries the environment
    r = pa.replicate(s, 0)
    layer = pa.RenderLayer()
    pa.RenderMulti([s, r], W, H, SPP, layer=layer)
    assert _same((np.array(layer.rgba, np.float32), np.array(layer.count, np.uint32)), ref), "RenderMulti"
    r.close()
    s.close()


@pytest.mark.gpu
def test_set_environment_rejects_bad_arguments():
    pa = _pa()
    s = _scene(pa)
    good = _env()
    for bad in (lambda: s.SetEnvironment(np.full((2, 2, 3), np.nan, np.float32)),
                lambda: s.SetEnvironment(np.full((2, 2, 3), -1.0, np.float32)),
                lambda: s.SetEnvironment(np.full((2, 2, 3), np.inf, np.float32)),
                lambda: s.SetEnvironment(np.zeros((0, 2, 3), np.float32)),
                lambda: s.SetEnvironment(good, -1.0),
                lambda: s.SetEnvironment(good, 1.0, np.diag([1.0, 2.0, 1.0]))):
        with pytest.raises(pa.PbrHipError) as e:
            bad()
        assert e.value.code == -1
    s.close()


@pytest.mark.gpu
def test_cli_env_background(tmp_path):
    """pbrlab-hip-cli --env: a pixel that sees only the constant sky is the encoded sRGB of L x scale"""
    from pbrlab_amd import io_api
    cli = os.path.join(ROOT, "pbrlab_amd", "pbrlab-hip-cli")
    obj = tmp_path / "floor.obj"
    (tmp_path / "floor.mtl").write_text("newmtl m\nKd 0.5 0.5 0.5\n")
    obj.write_text("mtllib floor.mtl\nusemtl m\nv -1 -1 0\nv 1 -1 0\nv 1 1 0\nv -1 1 0\nv 3 -0.01 0\nv 3.1 -0.01 0\nv 3.1 0.01 0\nf 1 2 3\nf 1 3 4\nf 5 6 7\n")
    L = 0.25
    hdr = tmp_path / "sky.hdr"
    # Radiance RGBE, flat scanlines, every texel 128 / 256 * 2^(127 - 128) = 0.25
    w, h = 8, 4
    m, e = 128, 127
    body = bytes([m, m, m, e]) * (w * h)
    hdr.write_bytes(b"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n-Y %d +X %d\n" % (h, w) + body)
    out = tmp_path / "out.png"
    r = subprocess.run([cli, str(obj), "--width", "32", "--height", "24", "--spp", "4", "--env", str(hdr), "--env-scale", "2",
                        "--out", str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    img = io_api.png_decode(out.read_bytes())
    want = io_api.layer_to_srgb8(np.array([[[4 * L * 2, 4 * L * 2, 4 * L * 2, 4.0]]], np.float32), np.array([[4]], np.uint32))
    assert img.shape[:2] == (24, 32)
    for y, x in ((0, 31), (23, 31), (0, 0)):  # corners beyond the floor: only the sky
        assert tuple(img[y, x, :3]) == tuple(want[0, 0, :3]), (y, x, img[y, x], want)


@pytest.mark.gpu
def test_environment_set_before_commit_and_progressive_passes():
    """SetEnvironment before CommitScene gives the image of SetEnvironment after it; passes rendered in steps (first_pass + NO_CLEAR)
    equal the one-shot render bit for bit"""
    import _analytic as A
    pa = _pa()
    S = EA.floor_scene()
    early = pa.Scene()
    early.SetEnvironment(_env(), 1.5, EA.Z_UP)
    A.build(early, S, pa.make_principled)
    late = A.build(pa.Scene(), S, pa.make_principled)
    late.SetEnvironment(_env(), 1.5, EA.Z_UP)
    ref = _render(pa, late)
    assert ref[0].reshape(-1, 4)[:, :3].sum() > 0
    assert _same(_render(pa, early), ref), "environment set before commit"
    layer = pa.RenderLayer()
    pa.Render(late, W, H, 3, layer=layer, first_pass=0)
    pa.Render(late, W, H, SPP - 3, layer=layer, first_pass=3, flags=pa.api.RENDER_NO_CLEAR)
    assert _same((np.array(layer.rgba, np.float32), np.array(layer.count, np.uint32)), ref), "progressive first_pass"
    early.close()
    late.close()
