"""GPU (-m gpu): the host builder's subtree re-insertion (pbrlab_amd/csrc/bvh_build.cpp) changes the tree and nothing
else.  Scenes committed with PBRHIP_BVH_REINSERT=0 (the builder's own tree) and with the default give the same bits: frames and pass
counts of the reduced Cornell scene, closest and any hits of a soup with ties and slivers; a refit of an optimised tree after a
vertex edit gives the frame of a fresh commit.  The ray counts of a RENDER_STATS frame are equal and the rays visit no more nodes
on the optimised tree.  A scene with curves keeps the builder's tree (no hair frames are compared here: the passes do not run there)."""
import contextlib
import copy
import os

import numpy as np
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


def _commit_both(pa, desc):
    """-> (the scene with the builder's own tree, the scene with the passes): the knob is read at commit"""
    with env(PBRHIP_BVH_REINSERT="0"):
        off = pa.scene_from_desc(desc)
    with env(PBRHIP_BVH_REINSERT="1"):
        on = pa.scene_from_desc(desc)
    return off, on


def _frame(pa, s, w, h, spp, **kw):
    layer = pa.RenderLayer()
    _, st = pa.Render(s, w, h, spp, layer=layer, **kw)
    return layer, st


def test_reduced_cornell_frames_and_visits(pa):
    from pbrlab_amd import scenes
    off, on = _commit_both(pa, scenes.cornell_scene(monkey_subdiv=3, lucy_nu=256, lucy_nv=32))
    assert off.info()["num_slots"] == on.info()["num_slots"] == 17688 and on.wide_info()["wide_nodes"] > 0
    a, _ = _frame(pa, off, 96, 64, 8)
    b, _ = _frame(pa, on, 96, 64, 8)
    assert a.rgba.tobytes() == b.rgba.tobytes() and a.count.tobytes() == b.count.tobytes() and a.rgba[..., :3].any()
    # (a frame this small runs in k_tail from the second bounce on, whose rays the node counts leave out: this one never hands over)
    a, sa = _frame(pa, off, 96, 64, 8, flags=pa.api.RENDER_STATS, tail_paths=0xFFFFFFFF)
    b, sb = _frame(pa, on, 96, 64, 8, flags=pa.api.RENDER_STATS, tail_paths=0xFFFFFFFF)
    assert a.rgba.tobytes() == b.rgba.tobytes() and a.count.tobytes() == b.count.tobytes()
    for kind in ("closest", "shadow"):
        print(f"{kind}: {sa[kind + '_rays']} rays, node visits per ray {sa[kind + '_nodes'] / sa[kind + '_rays']:.3f} off, {sb[kind + '_nodes'] / sb[kind + '_rays']:.3f} on; "
              f"triangle tests per ray {sa[kind + '_tris'] / sa[kind + '_rays']:.3f} off, {sb[kind + '_tris'] / sb[kind + '_rays']:.3f} on")
    assert sa["closest_rays"] == sb["closest_rays"] > 0 and sa["shadow_rays"] == sb["shadow_rays"] > 0
    assert sb["closest_nodes"] + sb["shadow_nodes"] <= sa["closest_nodes"] + sa["shadow_nodes"]
    # (the comparison is of two different trees: the passes moved something)
    assert (on.info(), on.wide_info(), sb["closest_nodes"]) != (off.info(), off.wide_info(), sa["closest_nodes"])


def test_soup_with_ties_and_slivers(pa):
    import _soups
    from pbrlab_amd import scenes
    desc, so, _ = _soups.triangle_soup(3, extra_slivers=200)
    off, on = _commit_both(pa, desc)
    rays = scenes.random_rays(so.FetchSceneAABB(), 20000, seed=17)
    ha, hb = off.trace_closest(rays), on.trace_closest(rays)
    assert ha.tobytes() == hb.tobytes() and (ha["prim_id"] != 0xFFFFFFFF).sum() > 1000
    oa, ob = off.trace_any(rays), on.trace_any(rays)
    assert oa.tobytes() == ob.tobytes() and oa.any()


def test_refit_of_an_optimised_tree(pa):
    """a vertex edit on a scene whose tree the passes rearranged, then a refit: the frame of a fresh commit of the edited scene"""
    from pbrlab_amd import scenes
    d0 = scenes.cornell_scene(monkey_subdiv=3, lucy_nu=256, lucy_nv=32)
    with env(PBRHIP_BVH_REINSERT="1"):
        on = pa.scene_from_desc(d0)
    b, _ = _frame(pa, on, 64, 64, 4)
    d1 = copy.deepcopy(d0)
    monkey = [sh.name for sh in d1.shapes].index("monkey")
    ids = np.unique(d1.shapes[monkey].vertex_ids)
    v = d1.vertices.copy()
    p = v[ids, :3]
    v[ids, :3] = (p * (1.0 + 0.25 * np.sin(7.0 * p[:, [1, 2, 0]])) + np.array([0.05, 0.1, -0.05])).astype(np.float32)
    d1.vertices = v
    on.UpdateTriangleMesh(monkey, d1.vertices)
    on.RefitScene()
    fresh = pa.scene_from_desc(d1)
    c, _ = _frame(pa, on, 64, 64, 4)
    d, _ = _frame(pa, fresh, 64, 64, 4)
    assert c.rgba.tobytes() == d.rgba.tobytes() and c.count.tobytes() == d.count.tobytes()
    assert c.rgba.tobytes() != b.rgba.tobytes()


def test_scenes_with_curves_keep_the_builders_tree(pa):
    """the passes are for triangle-only scenes: with curves the knob changes nothing about the committed trees"""
    from pbrlab_amd import scenes
    off, on = _commit_both(pa, scenes.hair_scene(n_strands=300, n_segments=6, head_subdiv=2))
    assert off.info() == on.info() and off.wide_info() == on.wide_info() and on.wide_info()["wide_nodes"] > 0
