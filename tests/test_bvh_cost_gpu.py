"""GPU (-m gpu): the cost the host builder and its Q collapse minimise (pbrlab_amd/csrc/bvh_build.cpp, host_scene.h::BvhBuildOptions,
DESIGN.md section 8 "The cost") changes the tree and nothing else.  The reduced Cornell scene (17 688 triangles: wall leaves, mesh
leaves and shadow rays to the light) at 64 x 64, 4 spp, committed with PBRHIP_BVH_COST=0 (the pricing of before), with the defaults and
with PBRHIP_BVH_REINSERT=0 (the defaults' collapse of the builder's own tree): the three frames are the same bits and trace the same
rays; with the defaults the rays visit no more nodes than on the builder's own tree and a shadow ray tests fewer triangles than under
the pricing of before."""
import contextlib
import os

import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pa():
    import pbrlab_amd as pa
    if pa.device_count() < 1:
        pytest.fail("no HIP device: the GPU tests must run on an MI355X (there is no CPU fallback)")
    pa.set_device(0)
    return pa


@contextlib.contextmanager
def env(**kw):
    old = {k: os.environ.get(k) for k in kw}
    os.environ.update(kw)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


@pytest.fixture(scope="module")
def frames(pa):
    """per commit setting: (scene, plain frame, RENDER_STATS frame, its statistics); the knobs are read at commit"""
    from pbrlab_amd import scenes
    desc = scenes.cornell_scene(monkey_subdiv=3, lucy_nu=256, lucy_nv=32)
    out = {}
    for name, kw in (("before", dict(PBRHIP_BVH_COST="0")), ("default", dict(PBRHIP_BVH_COST="1", PBRHIP_BVH_REINSERT="1")), ("no_passes", dict(PBRHIP_BVH_REINSERT="0"))):
        with env(**kw):
            s = pa.scene_from_desc(desc)
        assert s.info()["num_slots"] == 17688 and s.wide_info()["wide_nodes"] > 0
        plain = pa.RenderLayer()
        pa.Render(s, 64, 64, 4, layer=plain)
        # (a frame this small runs in k_tail from the second bounce on, whose rays the counts leave out: this one never hands over)
        counted = pa.RenderLayer()
        _, st = pa.Render(s, 64, 64, 4, layer=counted, flags=pa.api.RENDER_STATS, tail_paths=0xFFFFFFFF)
        out[name] = (s, plain, counted, st)
    return out


def test_same_bits(frames):
    ref = frames["before"]
    assert ref[1].rgba[..., :3].any()
    for name in ("default", "no_passes"):
        for k in (1, 2):
            assert frames[name][k].rgba.tobytes() == ref[k].rgba.tobytes() and frames[name][k].count.tobytes() == ref[k].count.tobytes(), (name, k)
    # (three different trees were walked)
    trees = {name: (f[0].info()["depth"], f[0].wide_info()["wide_nodes"], f[3]["closest_nodes"], f[3]["shadow_nodes"]) for name, f in frames.items()}
    assert len(set(trees.values())) == 3, trees


def test_visits(frames):
    st = {name: f[3] for name, f in frames.items()}
    for name, s in st.items():
        print(f"{name}: " + "; ".join(f"{kind} {s[kind + '_rays']} rays, {s[kind + '_nodes'] / s[kind + '_rays']:.4f} node visits and "
                                      f"{s[kind + '_tris'] / s[kind + '_rays']:.4f} triangle tests per ray" for kind in ("closest", "shadow")))
    for kind in ("closest", "shadow"):
        assert st["before"][kind + "_rays"] == st["default"][kind + "_rays"] == st["no_passes"][kind + "_rays"] > 0, kind
    assert st["default"]["closest_nodes"] + st["default"]["shadow_nodes"] <= st["no_passes"]["closest_nodes"] + st["no_passes"]["shadow_nodes"]
    assert st["default"]["shadow_tris"] / st["default"]["shadow_rays"] < st["before"]["shadow_tris"] / st["before"]["shadow_rays"]
