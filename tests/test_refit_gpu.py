"""GPU (-m gpu): the refit of a committed scene after vertex and transform edits (pbrlab_amd/csrc/refit_gpu.hip: k_rf_scatter, k_rf_plan,
k_rf_pack, k_rf_bin, k_rf_q; pbrhip_scene_update_* / pbrhip_scene_refit), held to its exact definition and to a fresh commit.

1. The hook against the model, bit for bit (pbrhip_tree_refit, tests/_refit_model.py): binary nodes, Q nodes, triangle words and points on
   every set of _qcollapse_model.all_sets() and once on the large set, for slots moved three ways; unchanged slots give back the input.
2. A scene committed at pose 0, edited to pose 1 and refitted against a scene BUILT at pose 1 and committed with the same builder: hits,
   bounds, frames and feature buffers as bits, builders 0, 1 and 2; refitting back gives the first frame.
3. The states: stale, wrong sizes, refused values, replicas, commits."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import _lbvh_model as M  # noqa: E402
import _qcollapse_model as Q  # noqa: E402
import _refit_model as R  # noqa: E402

SETS = Q.all_sets()
EINVAL, ESIZE, ESTATE = -1, -2, -6
SCENES = ["cornell_ggx", "cornell_sss", "hair", "cornell_hair_sss"]


@pytest.fixture(scope="module")
def pa():
    import pbrlab_amd as pa
    if pa.device_count() < 1:
        pytest.fail("no HIP device: the GPU tests must run on an MI355X (there is no CPU fallback)")
    pa.set_device(0)
    return pa


# ------------------------------------------------------------------------------------------------ 1. the hook against the model
def _pair(pa, lo, hi, kinds):
    lo, hi, kinds, slots = R.case(lo, hi, kinds)
    got = pa.api.qtree_collapse(lo, hi, kinds, slots)
    assert got["fits"] and got["quantised"]
    q = {f: got[f] for f in ("qnodes", "tri", "pts", "hit")}
    return got["nodes"], slots[got["order"]], kinds[got["order"]] != 0, q, got["depth"]


@pytest.mark.parametrize("name", sorted(SETS))
def test_hook_equals_the_model(pa, name):
    nodes, slots, curve, q, depth = _pair(pa, *SETS[name])
    gn, gq = pa.api.tree_refit(slots, nodes, q)
    assert R.differences(gn, gq, nodes, q) == [], "unchanged slots must give back the input bytes"
    for how in R.PERTURBATIONS:
        moved = R.perturb(slots, curve, how)
        gn, gq = pa.api.tree_refit(moved, nodes, q)
        wn, wq = R.refit(nodes, moved, q)
        bad = R.differences(gn, gq, wn, wq)
        print(f"{name} / {how}: n {len(slots)}, {len(q['qnodes'])} Q nodes, parts that differ from the model {bad}")
        assert bad == []
        R.check(gn, moved, gq, depth)
        bn, none = pa.api.tree_refit(moved, nodes)                        # the binary tree alone
        assert none is None and bn.tobytes() == wn.tobytes()


def test_hook_equals_the_model_on_the_large_set(pa):
    """levels that span many blocks"""
    nodes, slots, curve, q, depth = _pair(pa, *M.large_set())
    gn, gq = pa.api.tree_refit(slots, nodes, q)
    assert R.differences(gn, gq, nodes, q) == []
    moved = R.perturb(slots, curve, "jitter")
    gn, gq = pa.api.tree_refit(moved, nodes, q)
    wn, wq = R.refit(nodes, moved, q)
    assert R.differences(gn, gq, wn, wq) == []
    assert gn.tobytes() != nodes.tobytes() and gq["qnodes"].tobytes() != q["qnodes"].tobytes()


def test_device_output_edits_are_noticed(pa):
    """the comparison above can fail: one stale box, one stale record word or one changed reference in the DEVICE's output differs"""
    nodes, slots, curve, q, depth = _pair(pa, *SETS["mixed_500"])
    moved = R.perturb(slots, curve, "far")
    gn, gq = pa.api.tree_refit(moved, nodes, q)
    wn, wq = R.refit(nodes, moved, q)
    assert R.differences(gn, gq, wn, wq) == []
    i = int(np.flatnonzero((gn["lo"] != nodes["lo"]).any(axis=(1, 2)))[0])
    e = gn.copy()
    e["lo"][i] = nodes["lo"][i]
    assert R.differences(e, gq, wn, wq) == ["nodes"]
    for part in ("qnodes", "tri", "pts"):
        k = int(np.flatnonzero(np.ascontiguousarray(gq[part]).view(np.uint8).reshape(len(gq[part]), -1) !=
                               np.ascontiguousarray(q[part]).view(np.uint8).reshape(len(q[part]), -1))[0])
        e = dict(gq, **{part: gq[part].copy()})
        e[part].view(np.uint8).reshape(-1)[k] = np.ascontiguousarray(q[part]).view(np.uint8).reshape(-1)[k]
        assert R.differences(gn, e, wn, wq) == [part]
    e = dict(gq, qnodes=gq["qnodes"].copy())
    e["qnodes"]["c"][0, 0] ^= 8
    assert R.differences(gn, e, wn, wq) == ["qnodes"]


# ------------------------------------------------------------------------------------------------ 2. a scene against a fresh commit
def _desc(name):
    from pbrlab_amd import scenes
    if name.startswith("cornell"):
        kw = dict(monkey_subdiv=2, lucy_nu=64, lucy_nv=12)
        d = scenes.cornell_hair_scene("sss", n_strands=200, n_segments=5, **kw) if "hair" in name else scenes.cornell_scene(name.split("_")[1], **kw)
        for sh in d.shapes:                                               # the instance transforms of tests/test_features_gpu.py
            if sh.name == "monkey":
                sh.transform = scenes.instance_matrix((20.0, 35.0, -10.0), (1.3, 0.8, 1.1), (0.2, 0.25, 0.3))
            elif sh.name == "lucy":
                sh.transform = scenes.instance_matrix((0.0, 50.0, 15.0), (0.9, 1.2, 0.9), (-0.15, 0.1, 0.35))
            elif sh.name == "box":
                sh.transform = scenes.instance_matrix((10.0, 30.0, 25.0), (1.5, 2.0, 1.2), (0.1, 0.9, -0.5))
            elif sh.name == "back":
                sh.transform = scenes.instance_matrix((0.0, 0.0, 0.0), (0.8, 0.8, 1.0), (0.0, 0.0, 0.0))
        return d
    return scenes.hair_scene(n_strands=1500, n_segments=6, head_subdiv=2)


def _pose1(d0):
    """pose 1 of a description: one mesh deformed (with new normals), one instance moved out of its old bounds, the curves swayed, the
    light quad lowered -> (description, the edits as (kind, shape or curve index))"""
    import copy
    from pbrlab_amd import scenes
    d = copy.deepcopy(d0)
    names = [sh.name for sh in d.shapes]
    v, nrm = d.vertices.copy(), d.normals.copy()
    body = names.index("monkey" if "monkey" in names else "head")
    ids = np.unique(d.shapes[body].vertex_ids)
    p = v[ids, :3]
    v[ids, :3] = (p * (1.0 + 0.25 * np.sin(7.0 * p[:, [1, 2, 0]])) + np.array([0.05, 0.1, -0.05])).astype(np.float32)
    nids = np.unique(d.shapes[body].normal_ids)
    q = nrm[nids, :3] + 0.3 * np.sin(5.0 * nrm[nids][:, [2, 0, 1]])
    nrm[nids, :3] = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)
    light = names.index("light")
    v[np.unique(d.shapes[light].vertex_ids), 1] -= np.float32(0.2)
    d.vertices, d.normals = v, nrm
    moved = names.index("lucy" if "lucy" in names else "back")
    d.shapes[moved].transform = scenes.instance_matrix((15.0, -40.0, 30.0), (0.7, 1.1, 1.3), (-0.9, 0.6, 1.4))
    edits = [("mesh+normals", body), ("mesh", light), ("transform", moved)]
    for c, cs in enumerate(d.curves):
        cv = cs.vertices.copy()
        cv[:, 0] += (0.08 * np.sin(6.0 * cv[:, 1] + 1.0)).astype(np.float32)
        cv[:, 2] += (0.05 * cv[:, 1] * cv[:, 1]).astype(np.float32)
        cs.vertices = cv.astype(np.float32)
        edits.append(("curves", c))
    return d, edits


def _apply(s, d, edits):
    """the edits of _pose1 through the update calls: mesh i is shape i (then the curve meshes), and so is instance i"""
    for kind, i in edits:
        if kind == "mesh+normals":
            s.UpdateTriangleMesh(i, d.vertices, d.normals)
        elif kind == "mesh":
            s.UpdateTriangleMesh(i, d.vertices)
        elif kind == "transform":
            s.UpdateInstanceTransform(i, d.shapes[i].transform)
        else:
            s.UpdateCurveMesh(len(d.shapes) + i, d.curves[i].vertices)


def _observe(pa, s, rays):
    hits, occ = s.trace_closest(rays), s.trace_any(rays)
    layer = pa.RenderLayer()
    pa.Render(s, 64, 64, 8, layer=layer)
    f = pa.api.RenderFeatures(s, 64, 64, 4)
    lo, hi = s.FetchSceneAABB()
    return dict(hits=hits.tobytes(), any=occ.tobytes(), aabb=lo.tobytes() + hi.tobytes(), rgba=layer.rgba.tobytes(), count=layer.count.tobytes(),
                albedo=f.albedo.tobytes(), normal_depth=f.normal_depth.tobytes(), fcount=f.count.tobytes(), lit=bool(layer.rgba[..., :3].any()),
                nhits=int((hits["prim_id"] != 0xFFFFFFFF).sum()))


def _differ(a, b):
    return [k for k in a if a[k] != b[k] and k not in ("lit", "nhits")]


@pytest.fixture(scope="module")
def poses():
    out = {}
    for name in SCENES:
        d0 = _desc(name)
        d1, edits = _pose1(d0)
        out[name] = (d0, d1, edits)
    return out


@pytest.mark.parametrize("builder", [0, 1, 2])
@pytest.mark.parametrize("name", SCENES)
def test_refit_equals_a_fresh_commit(pa, poses, name, builder):
    from pbrlab_amd import scenes
    d0, d1, edits = poses[name]
    a, b = pa.scene_from_desc(d0, bvh_builder=builder), pa.scene_from_desc(d1, bvh_builder=builder)
    rays = np.concatenate([scenes.random_rays(a.FetchSceneAABB(), 10000, seed=3), scenes.random_rays(b.FetchSceneAABB(), 10000, seed=4)])
    info, wide = a.info(), a.wide_info()
    first = _observe(pa, a, rays)
    want = _observe(pa, b, rays)
    assert _differ(first, want) != [] and want["lit"] and want["nhits"] > 2000
    _apply(a, d1, edits)
    a.RefitScene()
    got = _observe(pa, a, rays)
    print(f"{name}, builder {builder}: {info}, {wide}; after the refit these differ from a fresh commit: {_differ(got, want)}")
    assert _differ(got, want) == []
    assert a.info() == info and a.wide_info() == wide                     # nodes, depth, stack need: topology alone
    assert (wide["wide_nodes"] > 0) == (builder != 1)
    # ... and back to pose 0
    _apply(a, d0, edits)
    a.RefitScene()
    assert _differ(_observe(pa, a, rays), first) == []


# ------------------------------------------------------------------------------------------------ 3. states
def _code(pa, f, *args):
    with pytest.raises(pa.PbrHipError) as e:
        f(*args)
    return e.value.code, str(e.value)


def test_states(pa, poses):
    from pbrlab_amd import scenes
    d0, d1, edits = poses["cornell_hair_sss"]
    s = pa.scene_from_desc(d0)
    rays = scenes.random_rays(s.FetchSceneAABB(), 2000, seed=6)
    first = _observe(pa, s, rays)
    info, wide = s.info(), s.wide_info()
    s.RefitScene()                                                        # a clean scene: nothing happens
    assert _differ(_observe(pa, s, rays), first) == [] and s.wide_info() == wide and s.info() == info
    monkey, hair = [sh.name for sh in d0.shapes].index("monkey"), len(d0.shapes)      # mesh ids: the shapes, then the curve mesh
    # refused calls change nothing and leave the scene usable
    assert _code(pa, s.UpdateTriangleMesh, monkey, d0.vertices[:-1])[0] == ESIZE
    assert _code(pa, s.UpdateTriangleMesh, monkey, d0.vertices, d0.normals[:-1])[0] == ESIZE
    assert _code(pa, s.UpdateCurveMesh, hair, d0.curves[0].vertices[:-4])[0] == ESIZE
    bad = d0.vertices.copy()
    bad[5, 1] = np.nan
    assert _code(pa, s.UpdateTriangleMesh, monkey, bad)[0] == EINVAL
    badc = d0.curves[0].vertices.copy()
    badc[3, 3] = np.inf
    assert _code(pa, s.UpdateCurveMesh, hair, badc)[0] == EINVAL
    assert _code(pa, s.UpdateCurveMesh, monkey, d0.curves[0].vertices)[0] == EINVAL           # a mesh of the other kind
    assert _code(pa, s.UpdateTriangleMesh, hair, d0.vertices)[0] == EINVAL
    assert _code(pa, s.UpdateTriangleMesh, 999, d0.vertices)[0] == EINVAL
    singular = scenes.instance_matrix(scale=(1.0, 0.0, 1.0))
    assert _code(pa, s.UpdateInstanceTransform, 1, singular)[0] == EINVAL
    nanm = np.eye(4, dtype=np.float32)
    nanm[3, 0] = np.nan
    assert _code(pa, s.UpdateInstanceTransform, 1, nanm)[0] == EINVAL
    assert _code(pa, s.UpdateInstanceTransform, 999, None)[0] == EINVAL
    assert _differ(_observe(pa, s, rays), first) == []
    # an accepted edit: stale until the refit
    s.UpdateInstanceTransform(monkey, d0.shapes[monkey].transform)        # (the same values: still an edit)
    layer = pa.RenderLayer()
    for f, args in ((pa.Render, (s, 16, 16, 1, None, layer)), (pa.api.RenderFeatures, (s, 16, 16, 1)), (s.trace_closest, (rays,)), (s.trace_any, (rays,)),
                    (s.FetchSceneAABB, ()), (s.CameraRays, (16, 16, [[0, 0, 0]])), (pa.api.replicate, (s, 0))):
        code, msg = _code(pa, f, *args)
        assert code == ESTATE and "pbrhip_scene_refit" in msg, (f, msg)
    s.RefitScene()
    assert _differ(_observe(pa, s, rays), first) == []
    # a commit on a stale scene rebuilds from the model and clears the state
    _apply(s, d1, edits)
    assert _code(pa, s.trace_any, rays)[0] == ESTATE
    s.CommitScene()
    fresh = pa.scene_from_desc(d1)
    assert _differ(_observe(pa, s, rays), _observe(pa, fresh, rays)) == []
    # a replica holds no geometry
    r = pa.api.replicate(s, 0)
    assert _code(pa, r.UpdateTriangleMesh, monkey, d0.vertices)[0] == ESTATE
    assert _code(pa, r.UpdateCurveMesh, hair, d0.curves[0].vertices)[0] == ESTATE
    assert _code(pa, r.UpdateInstanceTransform, 0, None)[0] == ESTATE
    code, msg = _code(pa, r.RefitScene)
    assert code == ESTATE and "replicate" in msg
    assert _differ(_observe(pa, r, rays), _observe(pa, fresh, rays)) == []
    # an uncommitted scene cannot be refitted; edits before the first commit only edit the model
    u = pa.Scene()
    assert _code(pa, u.RefitScene)[0] == ESTATE


def test_edits_before_the_first_commit(pa, poses):
    """a scene built at pose 0, edited to pose 1 BEFORE it is committed, equals a scene built at pose 1"""
    from pbrlab_amd import scenes
    d0, d1, edits = poses["cornell_hair_sss"]

    class Late:                                                           # build_scene commits at its end: hold that back
        def __init__(self, s):
            self.s = s

        def __getattr__(self, k):
            return (lambda: None) if k == "CommitScene" else getattr(self.s, k)
    s = pa.Scene()
    scenes.build_scene(Late(s), d0, pa.make_principled, pa.make_hair)
    _apply(s, d1, edits)
    assert _code(pa, s.RefitScene)[0] == ESTATE
    s.CommitScene()
    fresh = pa.scene_from_desc(d1)
    rays = scenes.random_rays(fresh.FetchSceneAABB(), 5000, seed=8)
    assert _differ(_observe(pa, s, rays), _observe(pa, fresh, rays)) == []
