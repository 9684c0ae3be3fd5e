"""GPU (-m gpu): k-nearest queries.

pbrhip_k_nearest_device against the brute force of tests/_knearest_model.py over the scene's own slots, count, ident and closest as
bytes: the adversarial soup (430 triangles, 3000 queries at the radii 0.05, 0.25 and none; tests/test_knearest_cpu.py shows that it
truncates at K = 1, 4 and 32 with ties of D2 across each cut and has queries without a primitive in reach) for K in {1, 4, 32} with
count, without count and count only, with and without closest, under the three builders and both trees, and after a vertex edit and a
refit; curve, single-primitive, empty and instanced scenes; entry 0 against pbrhip_nearest_point_device; the depth-64 comb, whose walk
reaches the spill part of the stack; inactive queries; placements at world scales; the host variant; stream ordering; the grid stride;
refusals.

Scenes are committed once per module and shared with tests/test_query_gpu.py; a model brute force is computed once per scene."""
import dataclasses

import numpy as np
import pytest

import _knearest_model as KM
import _query_model as QM
import test_knearest_cpu as KC
import test_query_gpu as TQ
from test_query_gpu import GPU_LBVH, GPU_LBVH_WIDE, HOST_SAH, pa, wide_env  # noqa: F401  (pa: the module's fixture)

pytestmark = pytest.mark.gpu

F = np.float32
NONE = 0xFFFFFFFF
CONFIGS = [(HOST_SAH, None), (HOST_SAH, "0"), (GPU_LBVH, None), (GPU_LBVH_WIDE, None), (GPU_LBVH_WIDE, "0")]  # tests/test_allhits_gpu.py::CONFIGS
KS = (1, 4, 32)


def _u32(t):
    return None if t is None else TQ._host(t).view(np.uint32)


def knn(s, d_pts, k, count=True, ident=True, closest=False):
    """-> (count, ident, closest) as uint32 words, None where not asked for"""
    return tuple(_u32(t) for t in s.KNearestDevice(d_pts, k, count=count, ident=ident, closest=closest))


def assert_rows_equal(got, want, what=""):
    want = np.ascontiguousarray(want).view(np.uint32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.nonzero((got != want).reshape(len(got), -1).any(axis=1))[0]
    assert len(bad) == 0, (what, len(bad), bad[:5], got[bad[:2]], want[bad[:2]])


def check_against_model(s, d_pts, want, ks=KS, what=""):
    """count, ident and closest as bytes for every K: count with the list, the list only, count only -- the lists with and without closest"""
    for k in ks:
        for closest in (False, True):
            c, i, q = knn(s, d_pts, k, closest=closest)
            assert_rows_equal(c, want["count"], (what, k, closest, "count"))
            assert_rows_equal(i, want["ident"][:, :k], (what, k, closest, "ident with count"))
            c, i, q2 = knn(s, d_pts, k, count=False, closest=closest)
            assert c is None and (q is None) == (q2 is None) == (not closest)
            assert_rows_equal(i, want["ident"][:, :k], (what, k, closest, "ident without count"))
            if closest:
                assert_rows_equal(q, want["closest"][:, :k], (what, k, "closest with count"))
                assert_rows_equal(q2, want["closest"][:, :k], (what, k, "closest without count"))
        c, i, q = knn(s, d_pts, k, ident=False)
        assert i is None and q is None
        assert_rows_equal(c, want["count"], (what, k, "count only"))
    c, i, q = knn(s, d_pts, 0)
    assert i is None and q is None
    assert_rows_equal(c, want["count"], (what, "max_k 0"))


def points_for(name, slots, shade):
    """the soup: tests/test_knearest_cpu.py's query set; another scene: tests/test_query_gpu.py's with the same three radii"""
    if name == "soup":
        return KC.soup_points(TQ.soup()[0].vertices[:, :3].reshape(-1, 3, 3), TQ.SOUP_SEED)
    pts = TQ.points_for(name, slots, shade)
    pts[1::3, 3] = F(0.25)
    return pts


_MODEL = {}


def model(pa, name, builder=HOST_SAH):
    """-> (points, the model with 32 listed) on the scene's own slots"""
    if (name, builder) not in _MODEL:
        _, slots, shade = TQ.scene(pa, name, builder)
        pts = points_for(name, slots, shade)
        _MODEL[name, builder] = (pts, KM.brute_force(pts, slots, shade, 32))
    return _MODEL[name, builder]


# ------------------------------------------------------------------------------------------------ against the model
@pytest.mark.parametrize("builder,wide", CONFIGS)
def test_soup_equals_the_model(pa, builder, wide):
    s, slots, shade = TQ.scene(pa, "soup", builder)
    pts, want = model(pa, "soup", builder)
    count = want["count"]
    print(f"{len(pts)} queries, {len(slots)} slots: {int((count == 0).sum())} with count 0, {int((count > 32).sum())} above 32, {int((count == len(slots)).sum())} with every slot")
    assert len(pts) == 3000 and len(slots) == 430
    assert (count == 0).sum() >= 100 and (count > 4).sum() >= 100 and ((count > 32) & (count < 430)).sum() >= 10 and (count == 430).sum() == 1000
    with wide_env(wide):
        check_against_model(s, TQ._dev(pts), want, what=(builder, wide))


@pytest.mark.parametrize("name", ["curves", "curve", "triangle", "empty", "instanced"])
def test_other_scenes_equal_the_model(pa, name):
    s, slots, shade = TQ.scene(pa, name)
    pts, want = model(pa, name)
    count = want["count"]
    print(f"{name}: {len(slots)} slots, count up to {count.max()}, {int((count == 0).sum())} queries with count 0")
    if name == "empty":
        assert len(slots) == 0 and not count.any()
    else:
        assert (count[2::3] == len(slots)).all()  # no bound: every slot
    for wide in (None, "0"):
        with wide_env(wide):
            check_against_model(s, TQ._dev(pts), want, ks=(1, 32) if name != "curves" else KS, what=(name, wide))


@pytest.mark.parametrize("builder", [HOST_SAH, GPU_LBVH_WIDE])
def test_two_pieces_at_a_joint_are_listed_by_sub(pa, builder):
    """A straight cubic along the x axis with control points at x = 0, 1, 2, 3: its pieces meet in joints that float32 holds exactly
    (asserted on the scene's own slots).  A query on the normal through a joint has the two pieces there at equal D2 and u: the smaller
    sub comes first, on both trees, whatever the slot order -- a committed scene numbers its units in (instance, geometry, primitive,
    sub) order, so the gid decides (asserted too).  The curve soup does not hold the case, since x + (y - x) is rarely y."""
    from pbrlab_amd import scenes
    cp = np.array([[0, 0, 0, 0.125], [1, 0, 0, 0.125], [2, 0, 0, 0.125], [3, 0, 0, 0.125]], F)
    desc = scenes.SceneDesc(np.zeros((0, 4), F), np.zeros((0, 4), F), [], [], [scenes.CurveShape("c", cp, np.array([0], np.uint32))])
    s = pa.scene_from_desc(desc, bvh_builder=builder)
    slots, shade = s.read_slots()
    sub = KM.sub_of(slots, shade)
    assert sorted(sub.tolist()) == [0, 1, 2, 3] and np.array_equal(np.argsort(shade[:, 24]), np.argsort(sub)) and len(set(shade[:, 27].tolist())) == 1
    by_sub = slots[np.argsort(sub)]
    a, b = by_sub[:, 0, :3], by_sub[:, 1, :3]
    print("joints:", a[:, 0].tolist(), b[-1, 0])
    assert np.array_equal(b[:-1], a[1:]) and np.array_equal(a + (b - a), b) and not a[:, 1:].any() and not b[:, 1:].any()
    pts = []
    for j in a[1:, 0]:
        pts += [[j, 1.0, 0.0, np.inf], [j, 0.0, -0.5, np.inf], [j, 1.0, 0.0, 1.0], [j, 0.0, 0.5, 0.5], [j, 0.0, 0.0, 0.0]]
    pts = np.array(pts, F)
    want = KM.brute_force(pts, slots, shade, 4)
    d2, first = want["closest"][:, :, 3], sub[want["ident"][:, :2, 0]]
    assert (d2[:, 0] == d2[:, 1]).all() and (first[:, 1] == first[:, 0] + 1).all() and (want["ident"][:, 0, 1] == want["ident"][:, 1, 1]).all()
    assert want["count"].reshape(-1, 5)[:, 2:].tolist() == [[2, 2, 2]] * 3 and (want["count"].reshape(-1, 5)[:, :2] == 4).all()
    for wide in (None, "0"):
        with wide_env(wide):
            check_against_model(s, TQ._dev(pts), want, ks=(1, 2, 4), what=(builder, wide))


# ------------------------------------------------------------------------------------------------ entry 0, builders and trees
@pytest.mark.parametrize("name", ["soup", "instanced", "curves"])
def test_entry_0_is_the_nearest_point(pa, name):
    s, slots, shade = TQ.scene(pa, name)
    pts = model(pa, name)[0]
    d = TQ._dev(pts)
    for wide in (None, "0"):
        with wide_env(wide):
            ident, closest = TQ.nearest_device(s, pts)
            for k in (1, 4):
                for count in (True, False):
                    c, i, q = knn(s, d, k, count=count, closest=True)
                    # all bytes, on curves too: a tie of D2 goes to the smaller gid in both queries, and no two units share one
                    assert i[:, 0].tobytes() == ident.tobytes() and q[:, 0].tobytes() == closest.tobytes(), (name, wide, k, count)
                    assert c is None or np.array_equal(c > 0, ident[:, 0] != NONE)


def _by_gid(ident, closest, slots, shade):
    """(gid, sub, bits of u, v, sqrt(D2), q, D2) per entry: what does not depend on the slot order"""
    found = ident[..., 0] != NONE
    sl = np.where(found, ident[..., 0], 0)
    gid = np.where(found, shade[sl, 24] if len(shade) else 0, NONE).astype(np.uint32)
    sub = np.where(found, KM.sub_of(slots, shade)[sl] if len(shade) else 0, 0).astype(np.uint32)
    return np.concatenate([gid[..., None], sub[..., None], ident[..., 1:], closest], axis=-1)


@pytest.mark.parametrize("name", ["soup", "curves"])
def test_does_not_depend_on_builder_or_tree(pa, name):
    pts = model(pa, name)[0]
    first = None
    for builder, wide in CONFIGS:
        s, slots, shade = TQ.scene(pa, name, builder)
        with wide_env(wide):
            c, i, q = knn(s, TQ._dev(pts), 8, closest=True)
        got = _by_gid(i, q, slots, shade)
        if first is None:
            first = (c, got)
        assert np.array_equal(c, first[0]) and np.array_equal(got, first[1]), (builder, wide, np.nonzero((got != first[1]).reshape(len(got), -1).any(axis=1))[0][:5])


@pytest.mark.parametrize("builder", [HOST_SAH, GPU_LBVH_WIDE])
def test_after_a_refit_equals_the_model_on_the_edited_slots(pa, builder):
    desc = TQ.soup()[0]
    rng = np.random.RandomState(11)
    moved = desc.vertices.copy()
    moved[:, :3] += ((rng.rand(len(moved), 3) - 0.5) * 0.2).astype(F)
    moved[300:360] = desc.vertices[300:360]  # triangles 100 .. 119 stay duplicates of 60 .. 79 (tests/test_query_gpu.py's edit)
    moved[180:240] = desc.vertices[180:240]
    s = pa.scene_from_desc(desc, bvh_builder=builder)
    pts = KC.soup_points(moved[:, :3].reshape(-1, 3, 3), 5)
    d = TQ._dev(pts)
    before = knn(s, d, 4)
    for mesh in range(len(desc.shapes)):
        s.UpdateTriangleMesh(mesh, moved)
    with pytest.raises(pa.PbrHipError) as e:  # pending geometry edits: PBRHIP_ESTATE until the refit
        s.KNearestDevice(d, 4)
    assert e.value.code == -6 and "refit" in str(e.value)
    with pytest.raises(pa.PbrHipError) as e:
        s.KNearest(pts[:8], 4)
    assert e.value.code == -6
    s.RefitScene()
    slots, shade = s.read_slots()
    want = KM.brute_force(pts, slots, shade, 32)
    assert not np.array_equal(want["count"], before[0])  # the edit shows
    for wide in (None, "0"):
        with wide_env(wide):
            check_against_model(s, d, want, ks=(4, 32), what=("refit", builder, wide))
    # ... and equals a fresh commit of the edited model, primitive by primitive
    fresh = pa.scene_from_desc(dataclasses.replace(desc, vertices=moved), bvh_builder=builder)
    got, ref = knn(s, d, 4, closest=True), knn(fresh, d, 4, closest=True)
    assert np.array_equal(got[0], ref[0]) and np.array_equal(_by_gid(got[1], got[2], slots, shade), _by_gid(ref[1], ref[2], *fresh.read_slots()))


# ------------------------------------------------------------------------------------------------ the spill part of the stack
@pytest.mark.parametrize("builder", [GPU_LBVH, GPU_LBVH_WIDE])
def test_comb_reaches_the_spill_part_of_the_stack(pa, builder):
    """The depth-64 comb of tests/test_query_gpu.py::test_comb_reaches_the_spill_part_of_the_stack, committed with the GPU builders (its
    Morton tree is the chain), with tests/test_knearest_cpu.py's queries near the origin end: without a bound and with K = 32 the
    model's walk over the model's tree (tests/_lbvh_model.py, which the GPU's tree equals bit for bit) holds 62 live stack entries, past
    the kSimpleLdsStack = 40 that live in LDS; every fourth query has a bound that prunes the chain at once."""
    import _lbvh_model as M
    from test_lbvh_gpu import comb_scene
    desc, lo, hi, rays = comb_scene(1)
    s, slots, shade = TQ.scene(pa, "comb", builder)
    nodes, order, depth, _ = M.build(lo, hi, np.zeros(len(lo), np.uint8))
    info = s.info()
    assert depth == 64 and info["num_slots"] == 65
    if builder == GPU_LBVH:
        assert info["depth"] == 64 and info["num_nodes"] == 64
    assert np.array_equal(slots[:, :3, :3], M.comb_triangles(1)[0][order]) and np.array_equal(shade[:, 27], order)  # the scene's leaf order is the model tree's
    near = KC.comb_queries()
    pts = np.concatenate([near, points_for("comb", slots, shade)])
    want = KM.brute_force(pts, slots, shade, 32)
    d2 = QM.candidates(near, slots, shade)[0]
    peaks = [KM.binary_walk_k(nodes, near[i], d2[i], shade[:, 24], 32)[0] for i in range(len(near))]
    print("live stack entries of the model's walk with K = 32, queries near the origin end:", sorted(set(peaks)))
    assert max(peaks) > 40 and min(peaks) == 0 and (want["count"][:64][0::4] == 65).all()
    for wide in (None, "0"):
        with wide_env(wide):
            check_against_model(s, TQ._dev(pts), want, ks=(4, 32), what=(builder, wide))
            check_against_model(s, TQ._dev(near[:1]), {k: v[:1] for k, v in want.items()}, ks=(32,), what=(builder, wide, "one query"))


# ------------------------------------------------------------------------------------------------ inactive queries, placements
def test_inactive_queries_have_nothing_and_leave_their_neighbours_alone(pa):
    s, slots, shade = TQ.scene(pa, "soup")
    pts, full = model(pa, "soup")
    pts = pts[:300]
    want = {k: v[:300] for k, v in full.items()}
    bad = np.array([[np.nan, 0, 0, 1], [0, np.nan, 0, np.inf], [0, 0, np.inf, 1], [-np.inf, 0, 0, 1], [0, 0, 0, np.nan], [0, 0, 0, -1.0], [0, 0, 0, -np.inf]], F)
    for at in (0, 300, 131):  # the first, the last and a middle index
        mixed = np.concatenate([pts[:at], bad, pts[at:]])
        keep = np.ones(len(mixed), bool)
        keep[at:at + len(bad)] = False
        for wide in (None, "0"):
            with wide_env(wide):
                for k, count in ((4, True), (4, False), (32, True)):
                    c, i, q = knn(s, TQ._dev(mixed), k, count=count, closest=True)
                    assert (i[~keep] == (NONE, 0, 0, 0)).all() and not q[~keep].any() and (c is None or (c[~keep] == 0).all())
                    assert_rows_equal(i[keep], want["ident"][:, :k], (at, wide, k))
                    assert_rows_equal(q[keep], want["closest"][:, :k], (at, wide, k))
                    assert c is None or np.array_equal(c[keep], want["count"])
    # max_dist = 0 lists what the point lies on, +0 and -0 alike
    sel = np.nonzero(shade[:, 24] < 100)[0]  # (triangles 60 .. 79 have exact duplicates: two primitives at distance 0)
    on = np.concatenate([slots[sel, 0, :3], np.zeros((len(sel), 1), F)], axis=1)
    on[::2, 3] = -0.0
    want = KM.brute_force(on, slots, shade, 32)
    twins = (shade[sel, 24] >= 60) & (shade[sel, 24] < 80)
    assert (want["count"] >= 1).all() and twins.sum() == 20 and (want["count"][twins] >= 2).all()
    check_against_model(s, TQ._dev(on), want, ks=(4,), what="max_dist 0")


@pytest.mark.parametrize("name", ["scale_1e-6", "scale_3e7", "offset_4096"])
def test_placed_soup_equals_the_model(pa, name):
    """a small and a large uniform scale and an offset of tests/_soups.py::PLACEMENTS, all inside §19's stated domain; the radii scale
    with the scene"""
    import _soups
    import test_placements_cpu as PC
    assert name in _soups.PLACEMENTS
    desc = _soups.placed_soup(3, 30, name)[0]
    tris, _, _, pts = PC.placed_points(3, name)
    assert np.array_equal(desc.vertices[:, :3].reshape(-1, 3, 3), tris)
    pts[1::3, 3] = F(0.25) * np.median(np.abs(_soups.placement(name)[0]))
    for builder in (HOST_SAH, GPU_LBVH_WIDE):
        s = pa.scene_from_desc(desc, bvh_builder=builder)
        slots, shade = s.read_slots()
        want = KM.brute_force(pts, slots, shade, 4)
        count = want["count"]
        assert (count == 0).sum() >= 100 and ((count > 4) & (count < 430)).sum() >= 100 and (count[2::3] == 430).all(), (name, np.bincount(np.minimum(count, 5)))
        for wide in (None, "0"):
            with wide_env(wide):
                check_against_model(s, TQ._dev(pts), want, ks=(4,), what=(name, builder, wide))


# ------------------------------------------------------------------------------------------------ host variant, streams, sizes, refusals
@pytest.mark.parametrize("name", ["soup", "curves"])
def test_host_variant_equals_the_device_variant(pa, name):
    s, slots, shade = TQ.scene(pa, name)
    pts, want = model(pa, name)
    for k in (0, 1, 4, 32):
        count, ident, closest = s.KNearest(pts, k)
        assert count.dtype == np.uint32 and ident.dtype == np.uint32 and closest.dtype == F and ident.shape == closest.shape == (len(pts), k, 4)
        assert_rows_equal(count, want["count"], k)
        assert_rows_equal(ident, want["ident"][:, :k], k)
        assert_rows_equal(closest.view(np.uint32), want["closest"][:, :k], k)
    rec = np.zeros(len(pts), pa.api.POINT_DT)
    rec["p"], rec["max_dist"] = pts[:, :3], pts[:, 3]
    count, ident, closest = s.KNearest(rec, 4)  # POINT_DT records
    assert_rows_equal(ident, want["ident"][:, :4], "records")


def test_points_made_on_a_side_stream_are_read_after_it(pa):
    import torch
    s, slots, shade = TQ.scene(pa, "soup")
    pts, want = model(pa, "soup")
    src = TQ._dev(pts)
    busy = torch.ones((2048, 2048), device="cuda:0")
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    d = torch.full_like(src, float("nan"))  # (read too early: inactive queries, nothing listed)
    with torch.cuda.stream(side):
        for _ in range(20):  # work in front of the kernel that makes the array
            busy = busy @ busy * 1e-4
        d.copy_(src * 1.0)
        count, ident, _ = s.KNearestDevice(d, 4)                           # torch's current stream: the side stream
    count2, ident2, closest2 = s.KNearestDevice(d, 4, closest=True, stream=side)  # ... and named
    count3, _, _ = s.KNearestDevice(d, 0, stream=side.cuda_stream)
    assert_rows_equal(_u32(ident), want["ident"][:, :4])
    assert_rows_equal(_u32(count), want["count"])
    assert_rows_equal(_u32(closest2), want["closest"][:, :4])
    assert torch.equal(ident, ident2) and torch.equal(count, count2) and torch.equal(count, count3)


def test_sizes_outputs_in_place_and_pointer_pairs(pa):
    import torch
    s, slots, shade = TQ.scene(pa, "soup")
    pts, want = model(pa, "soup")
    for n in TQ.SIZES:
        assert n in (1, 63, 64, 65, 257, 3000)
        for wide in (None, "0"):
            with wide_env(wide):
                c, i, q = knn(s, TQ._dev(pts[:n]), 3, closest=True)
            assert_rows_equal(c, want["count"][:n], (n, wide))
            assert_rows_equal(i, want["ident"][:n, :3], (n, wide))
            assert_rows_equal(q, want["closest"][:n, :3], (n, wide))
    d = TQ._dev(pts[:500])
    count, ident = torch.zeros((500,), dtype=torch.int32, device="cuda:0"), torch.zeros((500, 4, 4), dtype=torch.int32, device="cuda:0")
    closest = torch.zeros((500, 4, 4), dtype=torch.float32, device="cuda:0")
    assert s.KNearestDevice(d, 4, count=count, ident=ident, closest=closest) == (count, ident, closest)
    assert_rows_equal(_u32(ident), want["ident"][:500, :4])
    assert_rows_equal(_u32(closest), want["closest"][:500, :4])
    count.zero_(), ident.zero_(), closest.zero_()
    got = s.KNearestDevice((d.data_ptr(), 500), 4, count=count.data_ptr(), ident=ident.data_ptr(), closest=closest.data_ptr())
    assert got == (count.data_ptr(), ident.data_ptr(), closest.data_ptr())
    assert_rows_equal(_u32(count), want["count"][:500])
    assert_rows_equal(_u32(ident), want["ident"][:500, :4])
    assert_rows_equal(_u32(closest), want["closest"][:500, :4])
    with pytest.raises(ValueError):
        s.KNearestDevice(d, 4, ident=torch.zeros((500, 3, 4), dtype=torch.int32, device="cuda:0"))  # another K's rows
    with pytest.raises(TypeError):
        s.KNearestDevice(d, 4, closest=torch.zeros((500, 4, 4), dtype=torch.int32, device="cuda:0"))  # not float32


def test_across_the_grid_stride(pa):
    """more queries than one full grid of the launch holds (4096 blocks of 256), K = 2, the list only: every copy of the query set equals
    the first"""
    s, slots, shade = TQ.scene(pa, "soup")
    pts, want = model(pa, "soup")
    copies = 4096 * 256 // len(pts) + 2
    assert copies * len(pts) > 4096 * 256 + len(pts)
    d = TQ._dev(pts).repeat(copies, 1)
    for wide in (None, "0"):
        with wide_env(wide):
            count, ident, closest = s.KNearestDevice(d, 2, count=False)
        assert count is None and closest is None
        ident = ident.reshape(copies, len(pts), 2, 4)
        assert bool((ident == ident[:1]).all())
        assert_rows_equal(_u32(ident[0]), want["ident"][:, :2], wide)


def test_state_and_empty_calls(pa):
    from pbrlab_amd import api
    s, slots, shade = TQ.scene(pa, "triangle")
    L = s.L
    assert L.pbrhip_k_nearest_device(s.h, None, 0, 4, None, None, None, None) == 0 and L.pbrhip_k_nearest(s.h, None, 0, 0, None, None, None) == 0
    count, ident, closest = s.KNearest(np.zeros((0, 4), F), 4)
    assert count.shape == (0,) and ident.shape == (0, 4, 4) and closest.shape == (0, 4, 4)
    # max_k == 0 ignores ident and closest: a closest pointer beside a NULL ident is then no error, and nothing is written to it
    pts = np.array([[0.5, 0.2, 0.1, np.inf], [0.5, 0.2, 0.1, 0.0]], F)
    count, closest = np.full(2, 9, np.uint32), np.full((2, 4), 7.0, F)
    assert L.pbrhip_k_nearest(s.h, pts.ctypes.data, 2, 0, count.ctypes.data, None, closest.ctypes.data) == 0
    assert count.tolist() == [1, 0] and (closest == 7.0).all()
    # a replica is refused, on the scene's own device too; the source scene goes on answering
    twin = pa.replicate(s, 0)
    for call in (lambda: twin.KNearest(pts, 4), lambda: twin.KNearestDevice(TQ._dev(pts), 4), lambda: twin.KNearestDevice(TQ._dev(pts), 0)):
        with pytest.raises(api.PbrHipError) as e:
            call()
        assert e.value.code == -6 and "replica" in str(e.value)
    assert s.KNearest(pts, 4)[0].tolist() == [1, 0]
    fresh = api.Scene()  # not committed
    for call in (lambda: fresh.KNearest(np.zeros((4, 4), F), 4), lambda: fresh.KNearestDevice(TQ._dev(np.zeros((4, 4), F)), 4)):
        with pytest.raises(api.PbrHipError) as e:
            call()
        assert e.value.code == -6
