"""GPU (-m gpu): ray and nearest-point queries from device memory.

Ray queries: pbrhip_trace_closest_device's hits against pbrhip_trace_closest's as bytes, its ident against (slot, u, v, t) of those,
pbrhip_trace_any_device against pbrhip_trace_any on tmax == hit distance rays, for every builder and tree; inactive rays; ObjectIds of
the ident; rays produced on a side stream.

Nearest point: the device and the host variant against the brute force of tests/_query_model.py over the scene's own slots, bit for bit
and with no query left out -- slot, D2, sqrtf(D2), u, v and q --, on seven scenes, at the sizes 1, 63, 64, 65, 257 and 3000, under every
builder and tree, after a refit, across the grid stride, and for inactive queries.  The seventh scene, the depth-64 comb, is committed
with the GPU builders (its Morton tree is the chain) and queried from its deep end, so that the spill part of the stack is walked.

Scenes are committed once per module; a model brute force (3000 points against a few hundred primitives) is computed once per scene."""
import dataclasses
import functools
import os

import numpy as np
import pytest

import _query_model as QM

pytestmark = pytest.mark.gpu

F = np.float32
NONE = 0xFFFFFFFF
HOST_SAH, GPU_LBVH, GPU_LBVH_WIDE = 0, 1, 2
SOUP_SEED = 3  # the seed on which the validation bound changes candidates (tests/test_query_cpu.py)
SIZES = (1, 63, 64, 65, 257, 3000)


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
    """PBRHIP_WIDE for the calls inside (read per call): "0" walks the binary tree, None leaves the variable as it is.  The value the
    suite was started with comes back on exit."""

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
@functools.lru_cache(maxsize=None)
def soup():
    import _soups
    desc, so, rays = _soups.triangle_soup(SOUP_SEED, 30)
    return desc, rays


@functools.lru_cache(maxsize=None)
def curve_soup():
    """tests/_soups.py::curve_soup, seed 0 (tests/test_gpu_parity.py::test_curve_soup's scenes): 300 cubic ribbons incl. duplicates,
    degenerate, zero-radius, straight and grid-aligned ones, two triangles behind them; random rays and axis-aligned rays at control
    points"""
    import _soups
    desc, so, rays = _soups.curve_soup(0)
    return desc, rays


def _desc(name):
    from pbrlab_amd import scenes
    mat = dict(scenes.PRINCIPLED_DEFAULTS, kind="principled", name="m")
    if name == "soup":
        return soup()[0]
    if name == "curves":
        return curve_soup()[0]
    if name == "triangle":
        v = np.array([[0.1, -0.2, 0.3, 1], [1.3, 0.1, -0.4, 1], [0.2, 0.9, 0.6, 1]], F)
        return scenes.SceneDesc(v, np.zeros((0, 4), F), [mat], [scenes.Shape("t", np.array([[0, 1, 2]], np.uint32), None, np.zeros(1, np.uint32))])
    if name == "curve":
        cp = np.array([[0, 0, 0, 0.02], [0.3, 0.5, 0.1, 0.03], [0.7, 0.4, -0.2, 0.02], [1.0, 0.0, 0.1, 0.01]], F)
        return scenes.SceneDesc(np.zeros((0, 4), F), np.zeros((0, 4), F), [], [], [scenes.CurveShape("c", cp, np.array([0], np.uint32))])
    if name == "empty":
        return scenes.SceneDesc(np.zeros((0, 4), F), np.zeros((0, 4), F), [mat], [])
    if name == "instanced":  # the soup's two meshes under two non-trivial transforms
        d = soup()[0]
        ms = (scenes.instance_matrix((20.0, -35.0, 10.0), (1.3, 0.7, 1.1), (0.4, -0.2, 0.3)), scenes.instance_matrix((-50.0, 15.0, 80.0), (0.6, 1.2, 0.9), (-0.3, 0.5, 0.1)))
        return dataclasses.replace(d, shapes=[dataclasses.replace(s, transform=m) for s, m in zip(d.shapes, ms)])
    if name == "comb":  # 64 deep as a Morton tree (the GPU builders): test_comb_reaches_the_spill_part_of_the_stack commits it with them
        from test_lbvh_gpu import comb_scene
        return comb_scene(1)[0]
    raise KeyError(name)


_SCENES = {}


def scene(pa, name, builder=HOST_SAH):
    """-> (scene, slots, shade), committed once per module"""
    if (name, builder) not in _SCENES:
        s = pa.scene_from_desc(_desc(name), bvh_builder=builder)
        _SCENES[name, builder] = (s,) + tuple(s.read_slots())
    return _SCENES[name, builder]


def points_for(name, slots, shade, seed=0, n=3000):
    """the query set of a scene: tests/_query_model.py::soup_points over the soup's triangles in the order of its description (the recipe
    aims at its duplicates), else over the scene's slots (a curve piece as the triangle (a, b, b)); an empty scene: points in a box"""
    if name == "soup":
        return QM.soup_points(soup()[0].vertices[:, :3].reshape(-1, 3, 3), SOUP_SEED, n)
    if len(slots) == 0:
        rng = np.random.RandomState(77)
        return np.concatenate([rng.rand(n, 3) * 2 - 1, np.full((n, 1), np.inf)], axis=1).astype(F)
    tris = slots[:, :3, :3].copy()
    curve = ((shade[:, 3] >> 24) & QM.SLOT_IS_CURVE) != 0
    tris[curve, 2] = tris[curve, 1]
    return QM.soup_points(tris, seed, n)


_MODEL = {}


def model(pa, name, builder=HOST_SAH):
    """-> (points, brute force, expected ident, expected closest) for a scene's own slots"""
    if (name, builder) not in _MODEL:
        _, slots, shade = scene(pa, name, builder)
        pts = points_for(name, slots, shade)
        res = QM.brute_force(pts, slots, shade)
        _MODEL[name, builder] = (pts, res) + QM.expected_buffers(res)
    return _MODEL[name, builder]


def nearest_device(s, pts):
    ident, closest = s.NearestPointDevice(_dev(pts))
    return _host(ident).view(np.uint32), _host(closest)


def assert_nearest_equal(got, want, what=""):
    (gi, gc), (wi, wc) = got, want
    bad = np.nonzero((gi != wi).any(axis=1) | (gc.view(np.uint32) != wc.view(np.uint32)).any(axis=1))[0]
    assert len(bad) == 0, (what, len(bad), bad[:5], gi[bad[:3]], wi[bad[:3]], gc[bad[:3]], wc[bad[:3]])


# ------------------------------------------------------------------------------------------------ ray queries
INACTIVE = [  # one of each kind (org, tmin, dir, tmax)
    ((np.nan, 0, 0), 0.0, (0, 0, 1), 1e30), ((0, 0, 0), np.nan, (0, 0, 1), 1e30), ((0, 0, 0), 0.0, (0, np.nan, 1), 1e30), ((0, 0, 0), 0.0, (0, 0, 1), np.nan),
    ((np.inf, 0, 0), 0.0, (0, 0, 1), 1e30), ((0, 0, 0), 0.0, (0, -np.inf, 1), 1e30), ((0, 0, 0), 0.0, (0, 0, 0), 1e30), ((0, 0, 3), -1.0, (0, 0, -1), 1e30),
    ((0, 0, 3), 2.0, (0, 0, -1), 1.0),
]


def _ident_of(hits, slots_of_hits):
    ident = np.zeros((len(hits), 4), np.uint32)
    miss = hits["instance_id"] == NONE
    ident[:, 0] = np.where(miss, NONE, slots_of_hits)
    for k, f in ((1, "u"), (2, "v"), (3, "t")):
        ident[:, k] = np.where(miss, 0, hits[f].view(np.uint32))
    return ident


def _check_rays(pa, s, shade, rays):
    """the device calls against the host hooks on `rays` -> (hits, ident) of the device call"""
    want = s.trace_closest(rays)
    d_rays = _dev(rays.view(F).reshape(-1, 8))
    ident, hits = s.TraceClosestDevice(d_rays)
    ident, hits = _host(ident).view(np.uint32), _host(hits).view(pa.api.HIT_DT).reshape(-1)
    assert hits.tobytes() == want.tobytes()
    # the ident's slot names the primitive the hit names, and carries the hit's u, v, t
    hit = want["instance_id"] != NONE
    assert (ident[~hit] == (NONE, 0, 0, 0)).all() and (ident[hit, 0] < len(shade)).all()
    sl = ident[hit, 0]
    for word, f in ((25, "instance_id"), (26, "geom_id"), (27, "prim_id")):
        assert np.array_equal(shade[sl, word], want[f][hit]), f
    assert np.array_equal(ident, _ident_of(want, ident[:, 0]))
    # each output alone
    only_ident, none = s.TraceClosestDevice(d_rays, ident=_dev(np.zeros((len(rays), 4), np.int32)))
    assert none is None and np.array_equal(_host(only_ident).view(np.uint32), ident)
    none, only_hits = s.TraceClosestDevice(d_rays, hits=_dev(np.zeros((len(rays), 9), np.int32)))
    assert none is None and _host(only_hits).tobytes() == want.tobytes()
    short = rays.copy()
    short["tmax"] = np.where(np.isfinite(want["t"]) & hit, want["t"], 1.0)  # tmax == hit distance: accepted (t <= tmax)
    occ = _host(s.TraceAnyDevice(_dev(short.view(F).reshape(-1, 8))))
    assert np.array_equal(occ, s.trace_any(short)) and occ[hit].all()
    return hits, ident


@pytest.mark.parametrize("name", ["soup", "curves"])
@pytest.mark.parametrize("builder,wide", [(HOST_SAH, None), (HOST_SAH, "0"), (GPU_LBVH, None), (GPU_LBVH_WIDE, None)])
def test_ray_queries_equal_the_host_hooks(pa, name, builder, wide):
    rays = soup()[1] if name == "soup" else curve_soup()[1]
    s, slots, shade = scene(pa, name, builder)
    with wide_env(wide):
        hits, _ = _check_rays(pa, s, shade, rays)
    assert (hits["instance_id"] != NONE).sum() > 1500


def test_ray_queries_on_small_and_empty_scenes(pa):
    from pbrlab_amd import scenes
    rays = scenes.random_rays((np.array([-1, -1, -1], F), np.array([1.5, 1, 1], F)), 257, seed=5)
    for name in ("triangle", "curve", "empty"):
        s, slots, shade = scene(pa, name)
        for wide in (None, "0"):
            with wide_env(wide):
                _check_rays(pa, s, shade, rays)


def test_inactive_rays_miss_and_leave_their_neighbours_alone(pa):
    rays = soup()[1][:2000]
    bad = np.zeros(len(INACTIVE), pa.api.RAY_DT)
    for r, (o, tmin, d, tmax) in zip(bad, INACTIVE):
        r["org"], r["tmin"], r["dir"], r["tmax"] = o, tmin, d, tmax
    s, slots, shade = scene(pa, "soup")
    want = s.trace_closest(rays)
    want_any = s.trace_any(rays)
    for at in (0, len(rays), 997):  # the first, the last and a middle index
        mixed = np.concatenate([rays[:at], bad, rays[at:]])
        keep = np.ones(len(mixed), bool)
        keep[at:at + len(bad)] = False
        for wide in (None, "0"):
            with wide_env(wide):
                d_rays = _dev(mixed.view(F).reshape(-1, 8))
                ident, hits = s.TraceClosestDevice(d_rays)
                occ = _host(s.TraceAnyDevice(d_rays))
            ident, hits = _host(ident).view(np.uint32), _host(hits).view(pa.api.HIT_DT).reshape(-1)
            assert (ident[~keep] == (NONE, 0, 0, 0)).all() and (hits["instance_id"][~keep] == NONE).all() and (occ[~keep] == 0).all()
            assert (hits["geom_id"][~keep] == NONE).all() and (hits["prim_id"][~keep] == NONE).all()
            assert hits[keep].tobytes() == want.tobytes() and np.array_equal(occ[keep], want_any)
            assert np.array_equal(ident[keep][:, 1:], _ident_of(want, 0)[:, 1:])


def test_object_ids_take_the_ident(pa):
    """pbrhip_scene_object_ids_device reads the ident as it is: instance and geometry ids equal the hits'; the primitive id it returns is
    the canonical one (ShadeRec word 24) of the slot whose word 27 is the hit's prim_id"""
    import torch
    from pbrlab_amd import api
    rays = curve_soup()[1]
    s, slots, shade = scene(pa, "curves")
    ident, hits = s.TraceClosestDevice(_dev(rays.view(F).reshape(-1, 8)))
    h = _host(hits).view(api.HIT_DT).reshape(-1)
    assert ident.dtype == torch.int32
    img = ident.reshape(1, -1, 4)
    for what, f in ((api.ID_INSTANCE, "instance_id"), (api.ID_GEOM, "geom_id")):
        assert np.array_equal(_host(s.ObjectIds(img, what)).view(np.uint32).reshape(-1), h[f])
    gid = _host(s.ObjectIds(img, api.ID_PRIMITIVE)).view(np.uint32).reshape(-1)
    sl = _host(ident).view(np.uint32)[:, 0]
    hit = sl != NONE
    assert np.array_equal(gid[hit], shade[sl[hit], 24]) and (gid[~hit] == NONE).all() and np.array_equal(shade[sl[hit], 27], h["prim_id"][hit])
    # the host path of ObjectIds takes the downloaded ident as well
    assert np.array_equal(s.ObjectIds(_host(ident).view(np.uint32).reshape(1, -1, 4), api.ID_INSTANCE).reshape(-1), h["instance_id"])


def test_rays_and_points_made_on_a_side_stream_are_read_after_it(pa):
    import torch
    rays = soup()[1]
    s, slots, shade = scene(pa, "soup")
    pts = model(pa, "soup")[0]
    want, want_near = s.trace_closest(rays), s.NearestPoint(pts)
    src, psrc = _dev(rays.view(F).reshape(-1, 8)), _dev(pts)
    busy = torch.ones((2048, 2048), device="cuda:0")
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    d_rays, d_pts = torch.zeros_like(src), torch.full_like(psrc, float("nan"))  # (read too early: inactive rays and queries, all misses)
    with torch.cuda.stream(side):
        for _ in range(20):  # work in front of the kernels that make the arrays
            busy = busy @ busy * 1e-4
        d_rays.copy_(src * 1.0)
        d_pts.copy_(psrc * 1.0)
        ident, hits = s.TraceClosestDevice(d_rays)                   # torch's current stream: the side stream
    ident2, hits2 = s.TraceClosestDevice(d_rays, stream=side)        # ... and named
    occ = s.TraceAnyDevice(d_rays, stream=side.cuda_stream)
    near = s.NearestPointDevice(d_pts, stream=side)
    assert _host(hits).tobytes() == want.tobytes() and _host(hits2).tobytes() == want.tobytes() and torch.equal(ident, ident2)
    assert np.array_equal(_host(occ), s.trace_any(rays))
    assert_nearest_equal((_host(near[0]).view(np.uint32), _host(near[1])), want_near)


def test_pointer_pairs_are_accepted(pa):
    rays = soup()[1][:500]
    s, slots, shade = scene(pa, "soup")
    d_rays = _dev(rays.view(F).reshape(-1, 8))
    hits, occ = _dev(np.zeros((500, 9), np.int32)), _dev(np.zeros(500, np.uint8))
    got = s.TraceClosestDevice((d_rays.data_ptr(), 500), hits=hits.data_ptr())
    assert got == (None, hits.data_ptr()) and _host(hits).tobytes() == s.trace_closest(rays).tobytes()
    s.TraceAnyDevice((d_rays.data_ptr(), 500), out=occ.data_ptr())
    assert np.array_equal(_host(occ), s.trace_any(rays))
    pts = model(pa, "soup")[0][:500]
    d_pts, ident = _dev(pts), _dev(np.zeros((500, 4), np.int32))
    s.NearestPointDevice((d_pts.data_ptr(), 500), ident=ident.data_ptr())
    assert np.array_equal(_host(ident).view(np.uint32), model(pa, "soup")[2][:500])


def test_state_and_empty_calls(pa):
    from pbrlab_amd import api
    s, slots, shade = scene(pa, "triangle")
    L = s.L
    assert L.pbrhip_trace_closest_device(s.h, None, 0, None, None, None) == 0 and L.pbrhip_nearest_point(s.h, None, 0, None, None) == 0
    assert L.pbrhip_trace_any_device(s.h, None, 0, None, None) == 0 and L.pbrhip_nearest_point_device(s.h, None, 0, None, None, None) == 0
    fresh = api.Scene()  # not committed
    pts = np.zeros((4, 4), F)
    with pytest.raises(api.PbrHipError) as e:
        fresh.NearestPoint(pts)
    assert e.value.code == -6
    with pytest.raises(api.PbrHipError) as e:
        fresh.TraceClosestDevice(_dev(np.zeros((4, 8), F)))
    assert e.value.code == -6


def test_a_stale_scene_is_refused_until_it_is_refit(pa):
    desc = _desc("triangle")
    s = pa.scene_from_desc(desc)
    d_rays, d_pts = _dev(np.array([[0.5, 0.2, 3, 0, 0, 0, -1, 1e30]], F)), _dev(np.array([[0.5, 0.2, 1, np.inf]], F))
    before = s.NearestPoint(_host(d_pts))
    moved = desc.vertices.copy()
    moved[:, 2] += F(0.5)
    s.UpdateTriangleMesh(0, moved)  # pending geometry edits: every query is PBRHIP_ESTATE until the refit
    for call in (lambda: s.TraceClosestDevice(d_rays), lambda: s.TraceAnyDevice(d_rays), lambda: s.NearestPoint(_host(d_pts)),
                 lambda: s.NearestPointDevice(d_pts)):
        with pytest.raises(pa.PbrHipError) as e:
            call()
        assert e.value.code == -6 and "refit" in str(e.value)
    s.RefitScene()
    after = s.NearestPointDevice(d_pts)
    assert _host(after[0])[0, 0] == 0 and _host(after[1])[0, 3] != before[1][0, 3]
    assert _host(s.TraceAnyDevice(d_rays))[0] == 1 and _host(s.TraceClosestDevice(d_rays)[0])[0, 0] == 0


# ------------------------------------------------------------------------------------------------ nearest point
@pytest.mark.parametrize("name", ["soup", "curves", "triangle", "curve", "empty", "instanced"])
def test_nearest_point_equals_the_brute_force(pa, name):
    s, slots, shade = scene(pa, name)
    pts, res, want_ident, want_closest = model(pa, name)
    print(f"{name}: {len(slots)} slots, {int(res['found'].sum())} of {len(pts)} found, {int((res['ties'] >= 2).sum())} shared minima, {res['clamped']} clamped candidates")
    if name == "empty":
        assert len(slots) == 0 and not res["found"].any()
    else:
        assert res["found"][1::3].all()  # no bound: always found
    for wide in (None, "0"):
        with wide_env(wide):
            assert_nearest_equal(nearest_device(s, pts), (want_ident, want_closest), (name, wide, "device"))
            assert_nearest_equal(s.NearestPoint(pts), (want_ident, want_closest), (name, wide, "host"))


@pytest.mark.parametrize("builder", [GPU_LBVH, GPU_LBVH_WIDE])
def test_comb_reaches_the_spill_part_of_the_stack(pa, builder):
    """The comb of tests/test_lbvh_gpu.py::comb_scene(1) is a chain 64 deep as a Morton tree, so it is committed with the GPU builders
    (the host's SAH tree over 65 triangles is shallow).  A query near the origin end without a bound walks down the whole chain before
    it tests its first leaf, pushing the far child at every node: the model's walk over the model's tree (tests/_lbvh_model.py, which
    the GPU's tree equals bit for bit) counts 62 live stack entries, past the kSimpleLdsStack = 40 that live in LDS.  Every fourth of
    those queries has a bound that prunes the chain at once.  The answers equal the brute force on both trees; so do the ray queries."""
    import _lbvh_model as M
    from pbrlab_amd import scenes
    from test_lbvh_gpu import comb_scene
    desc, lo, hi, rays = comb_scene(1)
    s, slots, shade = scene(pa, "comb", builder)
    nodes, order, depth, _ = M.build(lo, hi, np.zeros(len(lo), np.uint8))
    info = s.info()
    print(builder, info, s.wide_info())
    assert depth == 64 and info["num_slots"] == 65
    if builder == GPU_LBVH:
        assert info["depth"] == 64 and info["num_nodes"] == 64
    tri = M.comb_triangles(1)[0]
    assert np.array_equal(slots[:, :3, :3], tri[order]) and np.array_equal(shade[:, 27], order)  # the scene's leaf order is the model tree's
    rng = np.random.RandomState(3)
    near = np.concatenate([rng.rand(64, 3) * 0.6 - 0.3, np.full((64, 1), np.inf)], axis=1).astype(F)
    near[1::4, 3] = 0.4
    pts = np.concatenate([near, points_for("comb", slots, shade)])
    res = QM.brute_force(pts, slots, shade)
    want = QM.expected_buffers(res)
    d2 = QM.candidates(near, slots, shade)[0]
    walks = [QM.binary_walk(nodes, near[i], d2[i]) for i in range(len(near))]
    peaks = [w[0] for w in walks]
    print("live stack entries of the model's walk, queries near the origin end:", sorted(set(peaks)))
    assert max(peaks) > 40 and min(peaks) == 0
    assert all(w[1] == res["d2"][i] for i, w in enumerate(walks) if res["found"][i]) and res["found"][:64][0::4].all()
    for wide in (None, "0"):
        with wide_env(wide):
            assert_nearest_equal(nearest_device(s, pts), want, (builder, wide, "device"))
            assert_nearest_equal(s.NearestPoint(pts), want, (builder, wide, "host"))
            assert_nearest_equal(nearest_device(s, near[:1]), (want[0][:1], want[1][:1]), (builder, wide, "one query"))
            _check_rays(pa, s, shade, rays)


def test_nearest_point_sizes_and_single_outputs(pa):
    import torch
    s, slots, shade = scene(pa, "soup")
    pts, res, want_ident, want_closest = model(pa, "soup")
    for n in SIZES:
        for wide in (None, "0"):
            with wide_env(wide):
                assert_nearest_equal(nearest_device(s, pts[:n]), (want_ident[:n], want_closest[:n]), (n, wide))
        assert_nearest_equal(s.NearestPoint(pts[:n]), (want_ident[:n], want_closest[:n]), n)
    d = _dev(pts[:257])
    ident, none = s.NearestPointDevice(d, ident=torch.zeros((257, 4), dtype=torch.int32, device="cuda:0"))
    assert none is None and np.array_equal(_host(ident).view(np.uint32), want_ident[:257])
    none, closest = s.NearestPointDevice(d, closest=torch.zeros((257, 4), dtype=torch.float32, device="cuda:0"))
    assert none is None and _host(closest).tobytes() == want_closest[:257].tobytes()


def _by_gid(ident, closest, shade):
    """(gid, bits of u, v, sqrt(D2), q, D2) per query: what does not depend on the slot order"""
    found = ident[:, 0] != NONE
    gid = np.where(found, shade[np.where(found, ident[:, 0], 0), 24] if len(shade) else 0, NONE).astype(np.uint32)
    return np.concatenate([gid[:, None], ident[:, 1:], closest.view(np.uint32)], axis=1)


@pytest.mark.parametrize("name", ["soup", "curves"])
def test_nearest_point_does_not_depend_on_builder_or_tree(pa, name):
    pts = model(pa, name)[0]
    first = None
    for builder, wide in ((HOST_SAH, None), (HOST_SAH, "0"), (GPU_LBVH, None), (GPU_LBVH_WIDE, None), (GPU_LBVH_WIDE, "0")):
        s, slots, shade = scene(pa, name, builder)
        with wide_env(wide):
            ident, closest = nearest_device(s, pts)
        got = _by_gid(ident, closest, shade)
        if first is None:
            first = got
            assert np.array_equal(ident, model(pa, name)[2])
        assert np.array_equal(got, first), (builder, wide, np.nonzero((got != first).any(axis=1))[0][:5])


def _by_ids(ident, closest, shade):
    found = ident[:, 0] != NONE
    sl = np.where(found, ident[:, 0], 0)
    ids = np.where(found[:, None], shade[sl][:, 25:28], NONE).astype(np.uint32)
    return np.concatenate([ids, ident[:, 1:3], closest.view(np.uint32)[:, 3:]], axis=1)  # instance, geom, prim, u, v, D2


@pytest.mark.parametrize("builder", [HOST_SAH, GPU_LBVH_WIDE])
def test_nearest_point_after_a_refit_equals_a_fresh_commit(pa, builder):
    desc = soup()[0]
    rng = np.random.RandomState(11)
    moved = desc.vertices.copy()
    moved[:, :3] += ((rng.rand(len(moved), 3) - 0.5) * 0.2).astype(F)
    moved[300:360] = desc.vertices[300:360]                                          # triangles 100 .. 119 stay duplicates of 60 .. 79 where both moved alike
    moved[180:240] = desc.vertices[180:240]
    s = pa.scene_from_desc(desc, bvh_builder=builder)
    pts = QM.soup_points(moved[:, :3].reshape(-1, 3, 3), 5)
    before = s.NearestPoint(pts)
    for mesh in range(len(desc.shapes)):
        s.UpdateTriangleMesh(mesh, moved)
    s.RefitScene()
    fresh = pa.scene_from_desc(dataclasses.replace(desc, vertices=moved), bvh_builder=builder)
    want = _by_ids(*fresh.NearestPoint(pts), fresh.read_slots()[1])
    for wide in (None, "0"):
        with wide_env(wide):
            got = _by_ids(*nearest_device(s, pts), s.read_slots()[1])
            assert np.array_equal(got, want), (wide, np.nonzero((got != want).any(axis=1))[0][:5])
            assert np.array_equal(_by_ids(*s.NearestPoint(pts), s.read_slots()[1]), want)
    assert not np.array_equal(_by_ids(*before, s.read_slots()[1]), want)             # the edit shows
    # ... and the refitted scene equals the model on its own slots
    sl, sh = s.read_slots()
    assert_nearest_equal(nearest_device(s, pts), QM.expected_buffers(QM.brute_force(pts, sl, sh)), "refit")


def test_nearest_point_across_the_grid_stride(pa):
    """more queries than one full grid of the launch holds (4096 blocks of 256): every copy of the query set equals the first"""
    import torch
    s, slots, shade = scene(pa, "soup")
    pts, res, want_ident, want_closest = model(pa, "soup")
    copies = 4096 * 256 // len(pts) + 2
    assert copies * len(pts) > 4096 * 256 + len(pts)
    d = _dev(pts).repeat(copies, 1)
    for wide in (None, "0"):
        with wide_env(wide):
            ident, closest = s.NearestPointDevice(d)
        ident, closest = ident.reshape(copies, len(pts), 4), closest.reshape(copies, len(pts), 4).view(torch.int32)
        assert bool((ident == ident[:1]).all()) and bool((closest == closest[:1]).all())
        assert_nearest_equal((_host(ident[0]).view(np.uint32), _host(closest[0]).view(F)), (want_ident, want_closest), wide)


def test_inactive_queries_miss(pa):
    s, slots, shade = scene(pa, "soup")
    pts = model(pa, "soup")[0][:300].copy()
    pts[:, 3] = np.inf
    bad = np.array([[np.nan, 0, 0, 1], [0, np.nan, 0, np.inf], [0, 0, np.inf, 1], [-np.inf, 0, 0, 1], [0, 0, 0, np.nan], [0, 0, 0, -1.0], [0, 0, 0, -np.inf]], F)
    for at in (0, 300, 131):
        mixed = np.concatenate([pts[:at], bad, pts[at:]])
        keep = np.ones(len(mixed), bool)
        keep[at:at + len(bad)] = False
        want = QM.expected_buffers(QM.brute_force(mixed, slots, shade))
        assert (want[0][~keep] == (NONE, 0, 0, 0)).all() and (want[0][keep, 0] != NONE).all()
        for wide in (None, "0"):
            with wide_env(wide):
                assert_nearest_equal(nearest_device(s, mixed), want, (at, wide))
                assert_nearest_equal(s.NearestPoint(mixed), want, (at, wide))
    # max_dist = 0 finds what the point lies on, +0 and -0 alike
    on = np.concatenate([slots[:50, 0, :3], np.zeros((50, 1), F)], axis=1)
    on[::2, 3] = -0.0
    want = QM.expected_buffers(QM.brute_force(on, slots, shade))
    assert (want[0][:, 0] != NONE).all()
    assert_nearest_equal(nearest_device(s, on), want, "max_dist 0")
