"""GPU (-m gpu): every environment kernel against the oracle's restatement of §10, bit for bit.

The environment is this project's own light: the reference leaves a miss black, so only the oracle (oracle/pbr_oracle.c: the miss,
the NEE selection, the environment's estimate and shadow ray, each call site's normal and hemisphere rule, 1 - p_env on the area
lights' NEE and emission-hit MIS) can hold the kernels that carry it -- k_shade_principled<4|5|6>, k_tail<4|5|6, ...>,
k_classify<true>, k_shade_hair<true>, k_sss_step<true> -- to something independent of them.  With the device's arithmetic
(MATH_DEVICE) every pixel's rgba and count must be the oracle's bits, not merely close, and the GPU's closest-hit and shadow ray
counts the oracle's:
  - the five test_gpu_parity scenes x k_tail hand-overs (never / at once / mid-render) x two maps: a constant one on the scene with
    its light quad turned into plain geometry (p_env = 1), and EA.sky_map with its sun, rotated, with the scene's area light
    (p_env = 1/2); each frame once as it renders and once with RENDER_STATS (the ray counts; a k_tail instance of its own);
  - test_env_gpu's hair + random-walk SSS + area light scene, also under suspended rays, path-group plans, chunked passes and
    RenderMulti over a replica;
  - the C3 and C4 benchmark geometry with a map, at 1920 x 1080 x 8 spp: 48 random pixels traced sample by sample."""
import dataclasses

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import _env_analytic as EA  # noqa: E402
import _oracle as O  # noqa: E402
from golden.make_golden import golden_scenes  # noqa: E402
from test_gpu_configs import config_desc, spot_parity  # noqa: E402

NAMES = ["lambert", "ggx", "sss", "hair", "textured"]
W, H, SPP = 64, 64, 4


def _rotation(axis, angle):
    """a world_to_env rotation (Rodrigues), float32"""
    k = np.asarray(axis, np.float64)
    k = k / np.linalg.norm(k)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return (np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K).astype(np.float32)


ROT = _rotation((0.3, 1.0, -0.4), 0.9)
MAPS = {
    "constant": (np.tile(np.float32([0.6, 0.8, 1.1]), (4, 8, 1)), 1.5, None, False),   # rgb, scale, world_to_env, keep the light
    "sky_sun": (EA.sky_map(), 0.25, ROT, True),
}


def _without_lights(desc):
    """the scene with its light quads as plain geometry: no area light, so NEE always samples the environment (p_env = 1)"""
    d = dataclasses.replace(desc, shapes=[dataclasses.replace(s, name="lamp" + s.name[5:]) if s.name[:5] == "light" else s
                                          for s in desc.shapes])
    assert not any(s.name[:5] == "light" for s in d.shapes) and any(s.name[:4] == "lamp" for s in d.shapes)
    return d


@pytest.fixture(scope="module")
def pa():
    import pbrlab_amd as pa
    if pa.device_count() < 1:
        pytest.fail("no HIP device: the GPU tests must run on an MI355X (there is no CPU fallback)")
    pa.set_device(0)
    return pa


def _lit(pa, desc, env):
    rgb, scale, m, keep_light = MAPS[env]
    if not keep_light:
        desc = _without_lights(desc)
    sg, so = pa.scene_from_desc(desc), O.oracle_scene_from_desc(desc)
    sg.SetEnvironment(rgb, scale, m)
    so.SetEnvironment(rgb, scale, m)
    return sg, so


@pytest.fixture(scope="module")
def lit(pa):
    """(name, map) -> (GPU scene, oracle scene, the oracle's frame), built on first use"""
    cache = {}
    scenes = golden_scenes()

    def get(name, env):
        if (name, env) not in cache:
            sg, so = _lit(pa, scenes[name], env)
            cache[(name, env)] = (sg, so, so.render(W, H, SPP, threads=O.oracle_threads(), math_mode=O.MATH_DEVICE))
        return cache[(name, env)]
    yield get
    for sg, _, _ in cache.values():
        sg.close()


def _bits(layer, rgba, count, what):
    nd = int((np.asarray(layer.rgba).view(np.uint32) != rgba.view(np.uint32)).any(axis=2).sum())
    assert nd == 0 and np.array_equal(layer.count, count), (what, f"{nd} pixels differ from the oracle")


def _rays(st):
    return st["closest_rays"] + st["tail_closest_rays"] + st["pruned_rays"], st["shadow_rays"] + st["tail_shadow_rays"]


@pytest.mark.parametrize("env", list(MAPS))
@pytest.mark.parametrize("tail", [0xFFFFFFFF, 0, 3000])
@pytest.mark.parametrize("name", NAMES)
def test_env_render_is_the_oracles(pa, lit, name, tail, env):
    sg, so, (rgba, count, ost) = lit(name, env)
    assert rgba[..., :3].sum() > 0 and count.sum() == W * H * SPP and ost["shadow_rays"] > 0
    layer = pa.RenderLayer()
    ok, _ = pa.Render(sg, W, H, SPP, layer=layer, tail_paths=tail)
    assert ok is True
    _bits(layer, rgba, count, (name, env, tail))
    layer = pa.RenderLayer()
    ok, st = pa.Render(sg, W, H, SPP, layer=layer, flags=pa.api.RENDER_STATS, tail_paths=tail)
    assert (st["n_tail"] == 0) == (tail == 0xFFFFFFFF)
    _bits(layer, rgba, count, (name, env, tail, "stats"))
    assert _rays(st) == (ost["closest_rays"], ost["shadow_rays"]), (name, env, tail, _rays(st), ost)
    assert st["pruned_rays"] == 0  # (no doomed-path pruning with an environment)


def _hair_sss_scene(pa):
    from pbrlab_amd import scenes
    from test_env_gpu import _env, _scene
    desc = scenes.cornell_hair_scene("sss", n_strands=200, n_segments=5, monkey_subdiv=2, lucy_nu=64, lucy_nv=12)
    s, so = _scene(pa), O.oracle_scene_from_desc(desc)
    s.SetEnvironment(_env(), 1.0, EA.Z_UP)
    so.SetEnvironment(_env(), 1.0, EA.Z_UP)
    return s, so


def test_hair_sss_scene_is_the_oracles_under_every_schedule(pa, monkeypatch):
    """test_env_gpu's scene (hair, random-walk SSS, an area light; every environment kernel) against the oracle: as it renders,
    with rays suspended after 1 and 3 turns, under path-group plans, in chunks of passes and over RenderMulti with a replica"""
    from test_env_gpu import H as H2, SPP as SPP2, W as W2
    s, so = _hair_sss_scene(pa)
    rgba, count, ost = so.render(W2, H2, SPP2, threads=O.oracle_threads(), math_mode=O.MATH_DEVICE)
    assert rgba[..., :3].sum() > 0
    layer = pa.RenderLayer()
    ok, st = pa.Render(s, W2, H2, SPP2, layer=layer, flags=pa.api.RENDER_STATS)
    _bits(layer, rgba, count, "stats")
    assert _rays(st) == (ost["closest_rays"], ost["shadow_rays"])
    for kv in (dict(PBRHIP_SUSP_TURNS="1"), dict(PBRHIP_SUSP_TURNS="3"), dict(PBRHIP_GROUPS="3,2,3"), dict(PBRHIP_GROUPS="1,1,1,1,1,1,1,1")):
        for k, v in kv.items():
            monkeypatch.setenv(k, v)
        for tail in (0, 0xFFFFFFFF):
            layer = pa.RenderLayer()
            pa.Render(s, W2, H2, SPP2, layer=layer, tail_paths=tail)
            _bits(layer, rgba, count, (kv, tail))
        for k in kv:
            monkeypatch.delenv(k)
    layer = pa.RenderLayer()
    pa.Render(s, W2, H2, SPP2, layer=layer, max_paths_in_flight=W2 * H2 * 3)
    _bits(layer, rgba, count, "chunked")
    r = pa.replicate(s, 0)
    layer = pa.RenderLayer()
    pa.RenderMulti([s, r], W2, H2, SPP2, layer=layer)
    _bits(layer, rgba, count, "RenderMulti")
    r.close()
    s.close()


@pytest.mark.parametrize("config", ["c3", "c4"])
def test_benchmark_geometry_with_a_map(pa, config):
    """C3 (random-walk SSS) and C4 (hair) at their own 1920 x 1080, 8 spp, under the sun map rotated: 48 random pixels, every sample
    traced by the oracle and summed in pass order, equal as bits"""
    desc = config_desc(config)
    Wc, Hc, S = 1920, 1080, 8
    sg, so = pa.scene_from_desc(desc), O.oracle_scene_from_desc(desc)
    rgb, scale, m, _ = MAPS["sky_sun"]
    sg.SetEnvironment(rgb, scale, m)
    so.SetEnvironment(rgb, scale, m)
    lay = pa.RenderLayer()
    ok, _ = pa.Render(sg, Wc, Hc, S, layer=lay)
    assert ok is True and (lay.count == S).all() and np.isfinite(lay.rgba).all()
    spot_parity(so, lay, Wc, Hc, range(S), 48, seed=7)
    sg.close()
