"""GPU (-m gpu): signed distance on top of the nearest-point queries.

Scenes: the six closed shapes of tests/_sdf_model.py, two instances of the cube (one rotated, one scaled non-uniformly), a small Cornell
box and a small hair scene.  Held to: ident and closest equal NearestPointDevice's as bytes under every builder and tree, the host
variant equals the device variant; the pseudonormal table stays within the rounding bound of the float64 model and is bit-identical,
keyed by canonical id, across builders; sd equals the float32 model evaluated with the device's own table bit for bit; the sign equals
the float64 winding number; a refit (host and device updates) equals a fresh commit; Cornell's walls and boundary edges; curve winners;
refusals; the grid.

Scenes are committed once per module; the float32 model of a scene (2000 points against at most a few hundred primitives) is computed
once and shared."""
import dataclasses
import functools
import os

import numpy as np
import pytest

import _query_model as QM
import _sdf_model as SM

pytestmark = pytest.mark.gpu

F = np.float32
NONE = 0xFFFFFFFF
HOST_SAH, GPU_LBVH, GPU_LBVH_WIDE = 0, 1, 2
TREES = ((HOST_SAH, None), (HOST_SAH, "0"), (GPU_LBVH, None), (GPU_LBVH_WIDE, None), (GPU_LBVH_WIDE, "0"))
SHAPES = sorted(SM.SHAPES)
ALL = SHAPES + ["cubes", "cornell", "hair"]
U = 2.0 ** -24
# the largest |row - float64 model| of the table over ALL, in units of 2^-24, as measured on an MI355X (DESIGN.md §20 records it per
# scene); the test asserts twice that, beside the derived bound (tests/_sdf_model.py::pseudonormal_bounds)
TABLE_MEASURED_U = 3.76


@pytest.fixture(scope="module")
def pa():
    import pbrlab_amd as pa
    if pa.device_count() < 1:
        pytest.fail("no HIP device: the GPU tests must run on an MI355X (there is no CPU fallback)")
    pa.set_device(0)
    return pa


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _host(t):
    return t.cpu().numpy()


class wide_env:
    """PBRHIP_WIDE for the calls inside (read per call): "0" walks the binary tree, None leaves the variable as it is"""

    def __init__(self, value):
        self.value = value

    def __enter__(self):
        self.before = os.environ.get("PBRHIP_WIDE")
        if self.value is not None:
            os.environ["PBRHIP_WIDE"] = self.value

    def __exit__(self, *exc):
        if self.before is None:
            os.environ.pop("PBRHIP_WIDE", None)
        else:
            os.environ["PBRHIP_WIDE"] = self.before


# ------------------------------------------------------------------------------------------------ scenes
def _mat():
    from pbrlab_amd import scenes
    return dict(scenes.PRINCIPLED_DEFAULTS, kind="principled", name="m")


def _mesh_desc(v, f, transforms=(None,)):
    from pbrlab_amd import scenes
    v4 = np.concatenate([np.asarray(v, F), np.ones((len(v), 1), F)], axis=1)
    shapes = [scenes.Shape(f"s{i}", np.asarray(f, np.uint32), None, np.zeros(len(f), np.uint32), transform=m) for i, m in enumerate(transforms)]
    return scenes.SceneDesc(v4, np.zeros((0, 4), F), [_mat()], shapes)


@functools.lru_cache(maxsize=None)
def _desc(name):
    from pbrlab_amd import scenes
    if name in SM.SHAPES:
        return _mesh_desc(*SM.shape(name))
    if name == "cubes":
        ms = (scenes.instance_matrix((25.0, -40.0, 15.0), (1.0, 1.0, 1.0), (-1.2, 0.1, 0.2)), scenes.instance_matrix((0.0, 0.0, 0.0), (1.6, 0.5, 0.9), (1.4, -0.2, 0.1)))
        return _mesh_desc(*SM.shape("cube"), transforms=ms)
    if name == "cornell":
        return scenes.cornell_scene("ggx", monkey_subdiv=1, lucy_nu=32, lucy_nv=8)
    if name == "hair":  # 24 ribbons above a two-triangle floor
        rng = np.random.RandomState(31)
        nc = 24
        cp = np.zeros((nc, 4, 4), F)
        cp[:, 0, :3] = rng.rand(nc, 3) * [2, 2, 0.2] - [1, 1, 0]
        cp[:, 1:, :3] = cp[:, :1, :3] + np.cumsum((rng.rand(nc, 3, 3) - [0.5, 0.5, 0.0]) * 0.3, axis=1)
        cp[..., 3] = 0.01
        curve = scenes.CurveShape("c", cp.reshape(-1, 4), (np.arange(nc, dtype=np.uint32) * 4))
        tv = np.array([[-1, -1, -0.5, 1], [1, -1, -0.5, 1], [1, 1, -0.5, 1], [-1, 1, -0.5, 1]], F)
        return scenes.SceneDesc(tv, np.zeros((0, 4), F), [_mat()], [scenes.Shape("floor", np.array([[0, 1, 2], [0, 2, 3]], np.uint32), None, np.zeros(2, np.uint32))], [curve])
    raise KeyError(name)


_SCENES = {}


def scene(pa, name, builder=HOST_SAH):
    """-> (scene, slots, shade), committed once per module"""
    if (name, builder) not in _SCENES:
        s = pa.scene_from_desc(_desc(name), bvh_builder=builder)
        _SCENES[name, builder] = (s,) + tuple(s.read_slots())
    return _SCENES[name, builder]


def slot_topology(desc, shade):
    """-> (triangle (n,) bool, idx (n, 3), obj (n,)) per slot from the description: instance i is shape i with one geometry"""
    tri = ((shade[:, 3] >> 24) & QM.SLOT_IS_CURVE) == 0
    idx, obj = np.zeros((len(shade), 3), np.int64), shade[:, 25].astype(np.int64)
    for k in np.nonzero(tri)[0]:
        idx[k] = desc.shapes[obj[k]].vertex_ids[shade[k, 27]]
    return tri, idx, obj


@functools.lru_cache(maxsize=None)
def points(name):
    """the query set of a scene: the CPU test's points for a shape; else 2000 points, a quarter on vertices, centroids and near centroids
    of the slots (tests/_query_model.py::soup_points) and the rest uniform in 1.5 x the box, every third with a bound"""
    if name in SM.SHAPES:
        return SM.ground_truth(name)[0]
    import pbrlab_amd as pa
    _, slots, shade = scene(pa, name)
    tris = slots[:, :3, :3].copy()
    curve = ((shade[:, 3] >> 24) & QM.SLOT_IS_CURVE) != 0
    tris[curve, 2] = tris[curve, 1]
    near = QM.soup_points(tris, 9, 1000)[:500]
    rng = np.random.RandomState(12)
    lo, hi = tris.reshape(-1, 3).min(axis=0), tris.reshape(-1, 3).max(axis=0)
    box = 0.5 * (lo + hi) + (rng.rand(1500, 3) - 0.5) * 1.5 * (hi - lo)
    md = np.full((1500, 1), np.inf)
    md[::3] = 0.25
    return np.ascontiguousarray(np.concatenate([near, np.concatenate([box, md], axis=1).astype(F)]), F)


_MODEL = {}


def model(pa, name):
    """-> the float32 model's answer (tests/_sdf_model.py::signed_model) on the HOST_SAH scene's slots with the device's own table"""
    if name not in _MODEL:
        s, slots, shade = scene(pa, name)
        _MODEL[name] = SM.signed_model(points(name), slots, shade, s.read_pseudonormals())
    return _MODEL[name]


def signed_device(s, pts):
    ident, closest, sd = s.SignedDistanceDevice(_dev(pts))
    return _host(ident).view(np.uint32), _host(closest), _host(sd)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def by_gid(table, shade):
    return table[np.argsort(shade[:, 24], kind="stable")]


# ------------------------------------------------------------------------------------------------ 1. the unsigned part
@pytest.mark.parametrize("name", ALL)
def test_ident_and_closest_equal_the_nearest_point_query(pa, name):
    pts = points(name)
    d = _dev(pts)
    for builder, wide in TREES:
        s, slots, shade = scene(pa, name, builder)
        with wide_env(wide):
            ident, closest, sd = s.SignedDistanceDevice(d)
            want_ident, want_closest = s.NearestPointDevice(d)
        assert _host(ident).tobytes() == _host(want_ident).tobytes() and _host(closest).tobytes() == _host(want_closest).tobytes(), (name, builder, wide)
    s, slots, shade = scene(pa, name)
    hi, hc, hs = s.SignedDistance(pts)
    gi, gc, gs = signed_device(s, pts)
    assert np.array_equal(hi, gi) and np.array_equal(bits(hc), bits(gc)) and np.array_equal(bits(hs), bits(gs))
    # each output alone
    import torch
    only = s.SignedDistanceDevice(d, sd=torch.zeros((len(pts), 4), dtype=torch.float32, device="cuda:0"))
    assert only[0] is None and only[1] is None and np.array_equal(bits(_host(only[2])), bits(gs))
    only = s.SignedDistanceDevice(d, ident=torch.zeros((len(pts), 4), dtype=torch.int32, device="cuda:0"))
    assert only[1] is None and only[2] is None and np.array_equal(_host(only[0]).view(np.uint32), gi)


# ------------------------------------------------------------------------------------------------ 2. the table
def table_error(pa, name):
    """-> (largest |row - float64 model| in units of 2^-24 over the rows with a bound, largest ratio to the derived bound)"""
    s, slots, shade = scene(pa, name)
    table = s.read_pseudonormals()
    tri, idx, obj = slot_topology(_desc(name), shade)
    assert table.shape == (len(slots), 7, 4) and (table[..., 3] == 0).all() and (table[~tri] == 0).all()
    corners = slots[tri][:, :3, :3].astype(np.float64)
    want = SM.pseudonormals64(corners, idx[tri], obj[tri])
    bound = SM.pseudonormal_bounds(corners, idx[tri], obj[tri])
    err = np.linalg.norm(table[tri][..., :3].astype(np.float64) - want, axis=2) / U
    ok = np.isfinite(bound)
    assert ok.mean() > 0.99
    # unit length, or zero
    ln = np.linalg.norm(table[tri][..., :3].astype(np.float64), axis=2)
    assert (np.abs(ln[ok] - 1.0) < 1e-6).all()
    return float(err[ok].max()), float((err[ok] / bound[ok]).max()), int(np.bincount(obj[tri]).max())


@pytest.mark.parametrize("name", ALL)
def test_table_is_within_the_rounding_bound_of_the_float64_model(pa, name):
    err, ratio, _ = table_error(pa, name)
    print(f"{name}: largest table error {err:.2f} x 2^-24, {ratio:.4f} of the derived bound")
    assert ratio <= 1.0
    assert err <= 2.0 * TABLE_MEASURED_U


@pytest.mark.parametrize("name", ["l_prism", "torus", "cubes", "cornell", "hair"])
def test_table_keyed_by_gid_does_not_depend_on_builder_or_tree(pa, name):
    first = None
    for builder in (HOST_SAH, GPU_LBVH, GPU_LBVH_WIDE):
        s, slots, shade = scene(pa, name, builder)
        got = by_gid(s.read_pseudonormals(), shade)
        first = got if first is None else first
        assert np.array_equal(bits(got), bits(first)), (name, builder)
        info = s.SignedDistanceInfo()
        tri, idx, obj = slot_topology(_desc(name), shade)
        want = SM.topology_report(idx[tri], obj[tri])
        assert {k: info[k] for k in want} == want, (name, builder, info)
        assert info["table_bytes"] > 0 or not tri.any()


# ------------------------------------------------------------------------------------------------ 3. sd against the float32 model
@pytest.mark.parametrize("name", ALL)
def test_sd_equals_the_float32_model_with_the_device_table(pa, name):
    s, slots, shade = scene(pa, name)
    pts, m = points(name), model(pa, name)
    print(f"{name}: {len(slots)} slots, {int(m['res']['found'].sum())} of {len(pts)} found, features", np.bincount(m["feature"], minlength=8))
    for wide in (None, "0"):
        with wide_env(wide):
            ident, closest, sd = signed_device(s, pts)
        assert np.array_equal(ident, m["ident"]) and np.array_equal(bits(closest), bits(m["closest"])), (name, wide)
        bad = np.nonzero((bits(sd) != bits(m["sd"])).any(axis=1))[0]
        assert len(bad) == 0, (name, wide, len(bad), bad[:5], sd[bad[:3]], m["sd"][bad[:3]], m["feature"][bad[:3]])
    # the sizes around a wave and a block
    for n in (1, 63, 64, 65, 257):
        got = signed_device(s, pts[:n])
        assert np.array_equal(bits(got[2]), bits(m["sd"][:n])) and np.array_equal(got[0], m["ident"][:n])


# ------------------------------------------------------------------------------------------------ 4. the sign
@pytest.mark.parametrize("name", SHAPES)
def test_sign_equals_the_winding_number(pa, name):
    s, slots, shade = scene(pa, name)
    pts, inside, dist, diam = SM.ground_truth(name)
    sd = signed_device(s, pts)[2]
    held = dist > SM.NEAR * diam
    assert (~held).sum() <= 0.01 * len(pts)
    bad = np.nonzero(held & ((sd[:, 3] < 0) != inside))[0]
    assert len(bad) == 0, (name, len(bad), pts[bad[:5]], sd[bad[:5]])
    assert np.allclose(np.abs(sd[:, 3]), dist, rtol=1e-5, atol=1e-6 * diam)


def test_sign_on_the_instanced_cubes(pa):
    s, slots, shade = scene(pa, "cubes")
    tri = slots[:, :3, :3].astype(np.float64)
    rng = np.random.RandomState(3)
    lo, hi = tri.reshape(-1, 3).min(axis=0), tri.reshape(-1, 3).max(axis=0)
    p = (0.5 * (lo + hi) + (rng.rand(2000, 3) - 0.5) * 1.5 * (hi - lo)).astype(F)
    pts = np.concatenate([p, np.full((len(p), 1), np.inf, F)], axis=1)
    inside = np.rint(SM.winding_number(p.astype(np.float64), tri)) == 1
    dist = SM.dist64(p.astype(np.float64), tri)
    held = dist > SM.NEAR * np.linalg.norm(hi - lo)
    sd = signed_device(s, pts)[2]
    print("instanced cubes:", int(inside.sum()), "of", len(p), "points inside,", int((~held).sum()), "not held")
    assert inside.sum() > 50 and (~held).sum() <= 0.01 * len(p)
    assert np.array_equal((sd[:, 3] < 0)[held], inside[held])
    info = s.SignedDistanceInfo()
    assert (info["triangles"], info["vertices"], info["edges_manifold"], info["edges_boundary"]) == (24, 16, 36, 0)


# ------------------------------------------------------------------------------------------------ 5. refits
def _by_ids(ident, closest, sd, shade):
    found = ident[:, 0] != NONE
    sl = np.where(found, ident[:, 0], 0)
    ids = np.where(found[:, None], shade[sl][:, 25:28], NONE).astype(np.uint32)
    return np.concatenate([ids, ident[:, 1:], bits(closest), bits(sd)], axis=1)


@pytest.mark.parametrize("device_update", [False, True])
@pytest.mark.parametrize("builder", [HOST_SAH, GPU_LBVH_WIDE])
def test_after_a_refit_table_and_answers_equal_a_fresh_commit(pa, builder, device_update):
    desc = _desc("torus")
    rng = np.random.RandomState(17)
    moved = desc.vertices.copy()
    moved[:, :3] += ((rng.rand(len(moved), 3) - 0.5) * 0.1).astype(F)
    s = pa.scene_from_desc(desc, bvh_builder=builder)
    pts = points("torus")
    before = s.SignedDistance(pts)
    table_before = s.read_pseudonormals()
    if device_update:
        s.UpdateTriangleMeshDevice(0, _dev(moved))
    else:
        s.UpdateTriangleMesh(0, moved)
    with pytest.raises(pa.PbrHipError) as e:  # stale until the refit
        s.SignedDistance(pts)
    assert e.value.code == -6 and "refit" in str(e.value)
    s.RefitScene()
    fresh = pa.scene_from_desc(dataclasses.replace(desc, vertices=moved), bvh_builder=builder)
    sh, fsh = s.read_slots()[1], fresh.read_slots()[1]
    table = s.read_pseudonormals()
    assert np.array_equal(bits(by_gid(table, sh)), bits(by_gid(fresh.read_pseudonormals(), fsh)))
    assert not np.array_equal(bits(table), bits(table_before))  # the edit shows
    want = _by_ids(*fresh.SignedDistance(pts), fsh)
    for wide in (None, "0"):
        with wide_env(wide):
            assert np.array_equal(_by_ids(*signed_device(s, pts), sh), want), wide
    assert np.array_equal(_by_ids(*s.SignedDistance(pts), sh), want)
    assert not np.array_equal(_by_ids(*before, sh), want)
    # ... and the refitted scene equals the model on its own slots and table
    m = SM.signed_model(pts, s.read_slots()[0], sh, table)
    assert np.array_equal(bits(signed_device(s, pts)[2]), bits(m["sd"]))


# ------------------------------------------------------------------------------------------------ 6. Cornell
def test_cornell_reports_its_boundary_edges_and_a_wall_has_two_sides(pa):
    s, slots, shade = scene(pa, "cornell")
    desc = _desc("cornell")
    tri, idx, obj = slot_topology(desc, shade)
    want = SM.topology_report(idx[tri], obj[tri])
    info = s.SignedDistanceInfo()
    print("cornell:", info)
    assert {k: info[k] for k in want} == want and info["edges_boundary"] >= 6 * 4 and info["edges_nonmanifold"] == 0
    back = [sh.name for sh in desc.shapes].index("back")
    pts = np.array([[-0.1, 0.6, -0.9, np.inf], [-0.1, 0.6, -1.1, np.inf]], F)  # in front of the back wall (in the room), and behind it
    ident, closest, sd = signed_device(s, pts)
    assert (shade[ident[:, 0], 25] == back).all()
    assert np.array_equal(sd[:, :3], np.array([[0, 0, 1], [0, 0, 1]], F))      # the wall faces the room (+z)
    assert sd[0, 3] > 0 and sd[1, 3] < 0 and np.allclose(np.abs(sd[:, 3]), 0.1, atol=1e-6)


# ------------------------------------------------------------------------------------------------ 7. curves
def test_a_curve_winner_is_outside_and_has_no_normal(pa):
    s, slots, shade = scene(pa, "hair")
    pts = points("hair")
    ident, closest, sd = signed_device(s, pts)
    found = ident[:, 0] != NONE
    curve = np.zeros(len(pts), bool)
    curve[found] = ((shade[ident[found, 0], 3] >> 24) & QM.SLOT_IS_CURVE) != 0
    print("hair:", int(curve.sum()), "curve winners,", int((found & ~curve).sum()), "triangle winners of", len(pts))
    assert curve.sum() > 200 and (found & ~curve).sum() > 50
    assert (sd[curve, :3] == 0).all() and np.array_equal(bits(sd[curve, 3]), ident[curve, 3]) and not np.signbit(sd[curve, 3]).any()
    assert (sd[~found] == 0).all() and (bits(sd[~found]) == 0).all()
    info = s.SignedDistanceInfo()
    assert info["triangles"] == 2 and info["edges_boundary"] == 4 and info["edges_manifold"] == 1


# ------------------------------------------------------------------------------------------------ 8. refusals
def test_inactive_points_miss_with_zeros(pa):
    s, slots, shade = scene(pa, "cube")
    good = points("cube")[:200]
    bad = np.array([[np.nan, 0, 0, 1], [0, np.nan, 0, np.inf], [0, 0, np.inf, 1], [-np.inf, 0, 0, 1], [0, 0, 0, np.nan], [0, 0, 0, -1.0], [5, 5, 5, 0.5]], F)
    want = model(pa, "cube")
    for at in (0, 200, 77):
        mixed = np.concatenate([good[:at], bad, good[at:]])
        keep = np.ones(len(mixed), bool)
        keep[at:at + len(bad)] = False
        for wide in (None, "0"):
            with wide_env(wide):
                ident, closest, sd = signed_device(s, mixed)
            assert (ident[~keep] == (NONE, 0, 0, 0)).all() and (bits(closest[~keep]) == 0).all() and (bits(sd[~keep]) == 0).all()
            assert np.array_equal(bits(sd[keep]), bits(want["sd"][:200])) and np.array_equal(ident[keep], want["ident"][:200])


def test_refusals(pa):
    import torch
    from pbrlab_amd import api
    s, slots, shade = scene(pa, "cube")
    L = s.L
    # n = 0: nothing to do
    assert L.pbrhip_signed_distance(s.h, None, 0, None, None, None) == 0 and L.pbrhip_signed_distance_device(s.h, None, 0, None, None, None, None) == 0
    assert tuple(s.SignedDistanceGridDevice((0, 0, 0), (1, 1, 1), (4, 0, 3)).shape) == (3, 0, 4)
    # a misaligned pointer, no output, NULL points: refused before any device work (the outputs keep their contents)
    pts = _dev(np.concatenate([points("cube")[:8].reshape(-1), np.zeros(4, F)]))
    out = torch.full((8, 4), 7.0, dtype=torch.float32, device="cuda:0")
    for call in (lambda: s.SignedDistanceDevice((pts.data_ptr() + 4, 8), sd=out.data_ptr()), lambda: s.SignedDistanceDevice((pts.data_ptr(), 8), sd=out.data_ptr() + 4),
                 lambda: s.SignedDistanceDevice((pts.data_ptr(), 8)), lambda: s.SignedDistanceDevice((None, 8), sd=out.data_ptr()),
                 lambda: s.SignedDistanceGridDevice((0, 0, 0), (1, 1, 1), (2, 2, 2), out=out.data_ptr() + 2)):
        with pytest.raises(api.PbrHipError) as e:
            call()
        assert e.value.code == -1
    assert bool((out == 7.0).all())
    # shapes, dtypes and sizes are checked before any C call
    with pytest.raises(ValueError):
        s.SignedDistance(np.zeros((4, 3), F))
    with pytest.raises((ValueError, TypeError)):
        s.SignedDistanceDevice(torch.zeros((4, 4), dtype=torch.float64, device="cuda:0"))
    with pytest.raises(ValueError):
        s.SignedDistanceGridDevice((0, 0, 0), (1, 1, 1), (2048, 2048, 1024))
    with pytest.raises(ValueError):
        s.SignedDistanceGridDevice((0, 0, 0), (1, 1), (2, 2, 2))
    # an uncommitted scene, a replica
    fresh = api.Scene()
    for call in (lambda: fresh.SignedDistance(np.zeros((4, 4), F)), lambda: fresh.SignedDistanceInfo(), lambda: fresh.read_pseudonormals()):
        with pytest.raises(api.PbrHipError) as e:
            call()
        assert e.value.code == -6
    twin = pa.replicate(s, 0)
    assert np.array_equal(_host(twin.NearestPointDevice(pts[:32].reshape(8, 4))[0]), _host(s.NearestPointDevice(pts[:32].reshape(8, 4))[0]))
    for call in (lambda: twin.SignedDistanceDevice((pts.data_ptr(), 8), sd=out.data_ptr()), lambda: twin.SignedDistance(points("cube")[:8]),
                 lambda: twin.SignedDistanceInfo(), lambda: twin.SignedDistanceGridDevice((0, 0, 0), (1, 1, 1), (2, 2, 1), out=out.data_ptr())):
        with pytest.raises(api.PbrHipError) as e:
            call()
        assert e.value.code == -6 and "replica" in str(e.value)
    assert bool((out == 7.0).all())


# ------------------------------------------------------------------------------------------------ 9. the grid
@pytest.mark.parametrize("name,dims", [("cube", (7, 5, 3)), ("cube", (33, 1, 9)), ("hair", (1, 17, 4)), ("tetrahedron", (128, 128, 65))])
def test_grid_equals_the_point_query_at_its_points(pa, name, dims):
    import torch
    s, slots, shade = scene(pa, name)
    lo, hi = slots[:, :3, :3].reshape(-1, 3).min(axis=0), slots[:, :3, :3].reshape(-1, 3).max(axis=0)
    # 1.6 x the box, an axis of one point through the middle of the box; the cube with a bound that leaves the far corners (0.3
    # diameters away) empty and still reaches its inside points next to the surface
    origin = np.where(np.array(dims) > 1, lo - F(0.3) * (hi - lo), F(0.5) * (lo + hi)).astype(F)
    spacing = (F(1.6) * (hi - lo) / np.maximum(np.array(dims, F) - 1, 1)).astype(F)
    max_dist = F(0.15) * np.linalg.norm(hi - lo).astype(F) if name == "cube" else F(np.inf)
    if dims[0] * dims[1] * dims[2] > 4096 * 256:
        print("grid of", dims, "=", dims[0] * dims[1] * dims[2], "points: more than one pass of the", 4096 * 256, "lanes of a launch")
    grid = s.SignedDistanceGridDevice(origin, spacing, dims, max_dist)
    assert tuple(grid.shape) == (dims[2], dims[1], dims[0]) and grid.dtype == torch.float32
    k, j, i = np.meshgrid(np.arange(dims[2]), np.arange(dims[1]), np.arange(dims[0]), indexing="ij")
    p = np.stack([origin[a] + x.astype(F) * spacing[a] for a, x in enumerate((i, j, k))], axis=-1).astype(F)  # multiply, then add, each rounded once
    pts = np.concatenate([p.reshape(-1, 3), np.full((p.size // 3, 1), max_dist, F)], axis=1)
    sd = s.SignedDistanceDevice(_dev(pts))[2]
    assert torch.equal(grid.reshape(-1).view(torch.int32), sd[:, 3].contiguous().view(torch.int32))
    got = _host(grid)
    assert (got < 0).any() or name == "hair"
    if name == "cube":
        assert (got == 0).any() and (got > 0).any()  # the bound leaves the far corners empty
    # written in place into a tensor and through a pointer
    out = torch.zeros_like(grid)
    assert s.SignedDistanceGridDevice(origin, spacing, dims, max_dist, out=out) is out and torch.equal(out.view(torch.int32), grid.view(torch.int32))
    out.zero_()
    s.SignedDistanceGridDevice(origin, spacing, dims, max_dist, out=out.data_ptr())
    assert torch.equal(out.view(torch.int32), grid.view(torch.int32))
