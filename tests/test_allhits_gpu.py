"""GPU (-m gpu): all-hits ray queries.

pbrhip_trace_all_device against the brute force of tests/_allhits_model.py over the scene's own slots, count and ident as bytes: the
adversarial soup (430 triangles, 11 000 rays; tests/test_allhits_cpu.py shows that it truncates at K = 4, has ties in t and rays
without a hit) for K in {1, 4, 32} with count, without count and count only, under the three builders and both trees, and after a vertex
edit and a refit; entry 0 against pbrhip_trace_closest_device's ident; inactive rays; a curve scene against peeling with the unchanged
closest-hit query; the depth-64 comb and its fat twin, whose walk reaches the spill part of the stack; the host variant; stream ordering;
the grid stride; refusals.

Scenes are committed once per module and shared with tests/test_query_gpu.py; a model brute force is computed once per scene."""
import dataclasses
import functools

import numpy as np
import pytest

import _allhits_model as AM
import test_query_gpu as TQ
from test_query_gpu import GPU_LBVH, GPU_LBVH_WIDE, HOST_SAH, pa, wide_env  # noqa: F401  (pa: the module's fixture)

pytestmark = pytest.mark.gpu

F = np.float32
NONE = 0xFFFFFFFF
CONFIGS = [(HOST_SAH, None), (HOST_SAH, "0"), (GPU_LBVH, None), (GPU_LBVH_WIDE, None), (GPU_LBVH_WIDE, "0")]
ZRAY = np.array([[0, 0, -10, 0, 0, 0, 1, np.inf]], F)  # up the z axis: through the origin's triangle and the 21 teeth on that axis


def _dev(rays):
    return TQ._dev(AM.as_rays(rays))


def _u32(t):
    return None if t is None else TQ._host(t).view(np.uint32)


def trace_all(s, d_rays, k, count=True, ident=True):
    c, i = s.TraceAllDevice(d_rays, k, count=count, ident=ident)
    return _u32(c), _u32(i)


def assert_rows_equal(got, want, what=""):
    bad = np.nonzero((got != want).reshape(len(got), -1).any(axis=1))[0]
    assert got.shape == want.shape and len(bad) == 0, (what, len(bad), bad[:5], got[bad[:2]], want[bad[:2]])


def check_against_model(s, d_rays, want, ks=(1, 4, 32), what=""):
    """count and ident as bytes for every K: with count, without count, count only"""
    for k in ks:
        c, i = trace_all(s, d_rays, k)
        assert_rows_equal(c, want["count"], (what, k, "count"))
        assert_rows_equal(i, want["ident"][:, :k], (what, k, "ident with count"))
        c, i = trace_all(s, d_rays, k, count=False)
        assert c is None
        assert_rows_equal(i, want["ident"][:, :k], (what, k, "ident without count"))
        c, i = trace_all(s, d_rays, k, ident=False)
        assert i is None
        assert_rows_equal(c, want["count"], (what, k, "count only"))
    c, i = trace_all(s, d_rays, 0)
    assert i is None
    assert_rows_equal(c, want["count"], (what, "max_hits 0"))


_MODEL = {}


def soup_model(pa, builder):
    if builder not in _MODEL:
        _, slots, shade = TQ.scene(pa, "soup", builder)
        _MODEL[builder] = AM.brute_force(TQ.soup()[1], slots, shade, 32)
    return _MODEL[builder]


# ------------------------------------------------------------------------------------------------ the soup against the model
@pytest.mark.parametrize("builder,wide", CONFIGS)
def test_soup_equals_the_model(pa, builder, wide):
    rays = TQ.soup()[1]
    s, slots, shade = TQ.scene(pa, "soup", builder)
    want = soup_model(pa, builder)
    count = want["count"]
    print(f"{len(rays)} rays, {len(slots)} slots, |H| up to {count.max()}, {int((count > 4).sum())} rays above 4, {int((want['ties'] > 0).sum())} with a tie, {int((count == 0).sum())} without a hit")
    assert len(rays) == 11000 and len(slots) == 430
    assert (count > 4).sum() >= 100 and (want["ties"] > 0).sum() >= 100 and (count == 0).sum() >= 100 and count.max() <= 32
    with wide_env(wide):
        check_against_model(s, _dev(rays), want, what=(builder, wide))


@pytest.mark.parametrize("builder", [HOST_SAH, GPU_LBVH_WIDE])
def test_soup_after_a_refit_equals_the_model_on_the_edited_slots(pa, builder):
    desc, rays = TQ.soup()
    rng = np.random.RandomState(11)
    moved = desc.vertices.copy()
    moved[:, :3] += ((rng.rand(len(moved), 3) - 0.5) * 0.2).astype(F)
    moved[300:360] = desc.vertices[300:360]  # triangles 100 .. 119 stay duplicates of 60 .. 79 (tests/test_query_gpu.py's edit)
    moved[180:240] = desc.vertices[180:240]
    s = pa.scene_from_desc(desc, bvh_builder=builder)
    d_rays = _dev(rays)
    before = trace_all(s, d_rays, 4)
    for mesh in range(len(desc.shapes)):
        s.UpdateTriangleMesh(mesh, moved)
    with pytest.raises(pa.PbrHipError) as e:  # pending geometry edits: PBRHIP_ESTATE until the refit
        s.TraceAllDevice(d_rays, 4)
    assert e.value.code == -6 and "refit" in str(e.value)
    with pytest.raises(pa.PbrHipError) as e:
        s.TraceAll(rays[:8], 4)
    assert e.value.code == -6
    s.RefitScene()
    slots, shade = s.read_slots()
    want = AM.brute_force(rays, slots, shade, 32)
    assert (want["ties"] > 0).sum() >= 100 and not np.array_equal(want["count"], before[0])  # the edit shows, the duplicates stay
    for wide in (None, "0"):
        with wide_env(wide):
            check_against_model(s, d_rays, want, ks=(4, 32), what=("refit", builder, wide))
    # ... and equals a fresh commit of the edited model, primitive by primitive
    fresh = pa.scene_from_desc(dataclasses.replace(desc, vertices=moved), bvh_builder=builder)
    got, ref = trace_all(s, d_rays, 4), trace_all(fresh, d_rays, 4)
    assert np.array_equal(got[0], ref[0]) and np.array_equal(_by_gid(got[1], shade), _by_gid(ref[1], fresh.read_slots()[1]))


def _by_gid(ident, shade):
    """(gid, bits of u, v, t) per entry: what does not depend on the slot order"""
    found = ident[..., 0] != NONE
    out = ident.copy()
    out[..., 0] = np.where(found, shade[np.where(found, ident[..., 0], 0), 24], NONE)
    return out


# ------------------------------------------------------------------------------------------------ entry 0, ObjectIds, inactive rays
@pytest.mark.parametrize("name", ["soup", "curves"])
@pytest.mark.parametrize("builder,wide", [(HOST_SAH, None), (HOST_SAH, "0"), (GPU_LBVH_WIDE, None)])
def test_entry_0_is_the_closest_hit_and_object_ids_take_the_rows(pa, name, builder, wide):
    from pbrlab_amd import api
    rays = TQ.soup()[1] if name == "soup" else TQ.curve_soup()[1]
    s, slots, shade = TQ.scene(pa, name, builder)
    d_rays = _dev(rays)
    with wide_env(wide):
        closest = _u32(s.TraceClosestDevice(d_rays)[0])
        assert (closest[:, 0] != NONE).sum() > 1500
        for k in (1, 4):
            for count in (True, False):
                c, ident = s.TraceAllDevice(d_rays, k, count=count)
                assert ident.shape == (len(rays), k, 4)
                assert _u32(ident)[:, 0].tobytes() == closest.tobytes(), (k, count)
        # the (n * K, 4) view of ident as it is: the canonical primitive id of every entry, NONE past the count
        gid = _u32(s.ObjectIds(ident.reshape(1, -1, 4), api.ID_PRIMITIVE)).reshape(len(rays), k)
        ident = _u32(ident)
        assert np.array_equal(gid, _by_gid(ident, shade)[..., 0]) and ((gid == NONE) == (ident[..., 0] == NONE)).all()


def test_inactive_rays_have_no_hits_and_leave_their_neighbours_alone(pa):
    rays = TQ.soup()[1][:2000]
    bad = np.zeros(len(TQ.INACTIVE), pa.api.RAY_DT)
    for r, (o, tmin, d, tmax) in zip(bad, TQ.INACTIVE):
        r["org"], r["tmin"], r["dir"], r["tmax"] = o, tmin, d, tmax
    assert not AM.ray_active(AM.as_rays(bad)).any() and AM.ray_active(AM.as_rays(rays)).all()
    s, slots, shade = TQ.scene(pa, "soup")
    want = {k: v[:2000] for k, v in soup_model(pa, HOST_SAH).items()}
    for at in (0, len(rays), 997):  # the first, the last and a middle index
        mixed = np.concatenate([rays[:at], bad, rays[at:]])
        keep = np.ones(len(mixed), bool)
        keep[at:at + len(bad)] = False
        for wide in (None, "0"):
            with wide_env(wide):
                for k, count in ((4, True), (4, False), (32, True)):
                    c, ident = trace_all(s, _dev(mixed), k, count=count)
                    assert (ident[~keep] == (NONE, 0, 0, 0)).all() and (c is None or (c[~keep] == 0).all())
                    assert_rows_equal(ident[keep], want["ident"][:, :k], (at, wide, k))
                    assert c is None or np.array_equal(c[keep], want["count"])


# ------------------------------------------------------------------------------------------------ curves against peeling
def _peel(s, d_rays, most):
    """pbrhip_trace_closest_device with tmin advanced to the last t until every ray has missed -> ident (n, steps, 4) of the steps"""
    import torch
    r = d_rays.clone()
    rows = []
    for _ in range(most + 2):
        ident = s.TraceClosestDevice(r, ident=torch.empty((len(r), 4), dtype=torch.int32, device=r.device))[0]
        hit = ident[:, 0] != -1
        if not bool(hit.any()):
            break
        rows.append(ident)
        r[:, 3] = torch.where(hit, ident[:, 3].contiguous().view(torch.float32), r[:, 3])  # (a ray that has missed misses again)
    else:
        raise AssertionError("peeling did not end")
    return TQ._host(torch.stack(rows, dim=1)).view(np.uint32)


@functools.lru_cache(maxsize=None)
def _curve_rays():
    """tests/test_query_gpu.py's curve soup (300 cubics with duplicates, degenerate, zero-radius and grid-aligned ones, two triangles
    behind them): its first 2000 random rays and its first 1000 axis-aligned ones"""
    rays = TQ.curve_soup()[1]
    return np.concatenate([rays[:2000], rays[5000:6000]])


def test_curves_equal_peeling_with_the_closest_hit_query(pa):
    rays = _curve_rays()
    first = None
    for builder, wide in CONFIGS:
        s, slots, shade = TQ.scene(pa, "curves", builder)
        d_rays = _dev(rays)
        with wide_env(wide):
            count, ident = trace_all(s, d_rays, 32)
            _, ident_nc = trace_all(s, d_rays, 32, count=False)
            peel = _peel(s, d_rays, 32) if first is None else None
        assert count.max() <= 32 and np.array_equal(ident, ident_nc)
        n, k = ident.shape[:2]
        listed = np.arange(k)[None, :] < count[:, None]
        assert np.array_equal(listed, ident[:, :, 0] != NONE)
        by_gid = _by_gid(ident, shade)
        if first is not None:  # identical across builders and trees, primitive by primitive
            assert np.array_equal(count, first[0]) and np.array_equal(by_gid, first[1]), (builder, wide)
            continue
        first = (count, by_gid)
        t = ident[:, :, 3].view(F)
        new = listed & np.concatenate([np.ones((n, 1), bool), t[:, 1:] != t[:, :-1]], axis=1)  # the first entry of every distinct t
        steps = new.sum(axis=1)
        curve = ((shade[:, 3] >> 24) & AM.SLOT_IS_CURVE) != 0
        on_curve = listed & curve[np.where(listed, ident[:, :, 0], 0)]
        print(f"{n} rays: |H| up to {count.max()}, {int(on_curve.sum())} of {int(listed.sum())} hits on curve pieces, {int((steps < count).sum())} rays with a tie in t, {int((count == 0).sum())} without a hit")
        assert (on_curve.sum(axis=1) >= 2).sum() >= 100 and (steps < count).sum() >= 10 and (count == 0).any() and (count >= 5).any()
        # the distinct t of the list, in order, are the peel's
        assert np.array_equal((peel[:, :, 0] != NONE).sum(axis=1), steps) and peel.shape[1] == steps.max()
        for j in range(peel.shape[1]):
            rows = np.nonzero(steps > j)[0]
            col = np.argmax(np.cumsum(new[rows], axis=1) == j + 1, axis=1)
            assert np.array_equal(ident[rows, col], peel[rows, j]), j  # (a tie's first entry is the smaller id: the closest hit's)
        # where all t of a ray are distinct the rows are the peel's rows and count is the number of steps
        plain = np.nonzero(steps == count)[0]
        assert len(plain) >= 1000
        pad = np.zeros((len(plain), k, 4), np.uint32)
        pad[:, :, 0] = NONE
        pad[:, :peel.shape[1]] = peel[plain]
        assert pad.tobytes() == ident[plain].tobytes()


# ------------------------------------------------------------------------------------------------ the spill part of the stack
@functools.lru_cache(maxsize=None)
def _fat_comb():
    """-> (desc, triangles, lo, hi, rays): tests/_allhits_model.py::fat_comb_triangles as one mesh (tests/test_lbvh_gpu.py::comb_scene's
    way); rays along the z axis -- up and down, ending on and starting from the plane z = 0 the fat teeth share -- and random ones near
    the origin end"""
    from pbrlab_amd import scenes
    tri, lo, hi = AM.fat_comb_triangles()
    n = len(tri)
    verts = np.concatenate([tri.reshape(-1, 3), np.ones((3 * n, 1), F)], 1)
    mat = dict(scenes.PRINCIPLED_DEFAULTS, kind="principled", name="m")
    desc = scenes.SceneDesc(verts, np.zeros((0, 4), F), [mat], [scenes.Shape("comb", np.arange(3 * n, dtype=np.uint32).reshape(n, 3), None, np.zeros(n, np.uint32))])
    z = np.repeat(ZRAY, 6, axis=0)
    z[1, 7] = 10.0                      # ends ON the plane z = 0
    z[2, 3] = 10.0                      # starts ON it
    z[3, 2], z[3, 6] = 3000000.0, -1.0  # down the axis: the far end first
    z[4, 0:3], z[4, 4:7] = (0.125, 0.0625, -2.0), (0.0, 0.0, 0.5)
    z[5, 0:3], z[5, 4:7] = (-4, -3, -5), (4, 3, 5)  # through the origin, oblique
    rnd = AM.as_rays(scenes.random_rays((np.array([-1, -1, -1], F), np.array([3, 3, 3], F)), 250, seed=7))
    return desc, tri, lo, hi, np.concatenate([z, rnd])


@pytest.mark.parametrize("builder", [GPU_LBVH, GPU_LBVH_WIDE])
@pytest.mark.parametrize("name", ["comb", "fat"])
def test_combs_reach_the_spill_part_of_the_stack(pa, name, builder):
    """The depth-64 comb of tests/test_query_gpu.py::test_comb_reaches_the_spill_part_of_the_stack, committed with the GPU builders (its
    Morton tree is the chain), and a ray up the z axis with count on, which crosses every tooth a line can cross: count and rows equal
    the model's.  By the model's own walk (tests/_allhits_model.py::binary_walk_all over tests/_lbvh_model.py's tree, which the GPU's tree
    equals bit for bit) that ray holds 20 live stack entries -- the comb's teeth are thin, and only the 22 leaves on the z axis lie on the
    ray; a nearest-point query reaches 62 because every box is within its bound, a ray only pushes boxes it crosses.  So the spill part
    -- more than kSimpleLdsStack = 40 live entries -- is reached on the FAT comb: the same box centres, hence the same chain, with the
    teeth on x and y grown to cover the origin.  There the ray crosses 63 leaf boxes on its way down the chain, holds 62 entries, and
    meets 43 triangles at one t in the plane z = 0, ordered by gid; 64 hits against K = 32."""
    import _lbvh_model as M
    from test_lbvh_gpu import comb_scene
    if name == "comb":
        _, lo, hi, rays = comb_scene(1)
        tri = M.comb_triangles(1)[0]
        s, slots, shade = TQ.scene(pa, "comb", builder)
        rays = np.concatenate([ZRAY, AM.as_rays(rays)])
    else:
        desc, tri, lo, hi, rays = _fat_comb()
        s = pa.scene_from_desc(desc, bvh_builder=builder)
        slots, shade = s.read_slots()
    nodes, order, depth, _ = M.build(lo, hi, np.zeros(len(lo), np.uint8))
    info = s.info()
    print(name, builder, info, s.wide_info())
    assert depth == 64 and info["num_slots"] == 65
    if builder == GPU_LBVH:
        assert info["depth"] == 64 and info["num_nodes"] == 64
    assert np.array_equal(slots[:, :3, :3], tri[order]) and np.array_equal(shade[:, 27], order)  # the scene's leaf order is the model tree's
    want = AM.brute_force(rays, slots, shade, 32)
    peak, hits = AM.binary_walk_all(nodes, ZRAY, slots, shade)
    print(f"the ray up the z axis: {hits} hits, {peak} live stack entries in the model's walk; |H| up to {want['count'].max()}")
    assert hits == want["count"][0]
    if name == "comb":
        assert (peak, hits) == (20, 22)
    else:
        assert peak == 62 and peak > 40 and hits == 64 and want["ties"][0] >= 40
    for wide in (None, "0"):
        with wide_env(wide):
            check_against_model(s, _dev(rays), want, ks=(4, 32), what=(name, builder, wide))
            check_against_model(s, _dev(rays[:1]), {k: v[:1] for k, v in want.items()}, ks=(32,), what=(name, builder, wide, "one ray"))


# ------------------------------------------------------------------------------------------------ host variant, streams, sizes, refusals
@pytest.mark.parametrize("name", ["soup", "curves"])
def test_host_variant_equals_the_device_variant(pa, name):
    rays = TQ.soup()[1] if name == "soup" else _curve_rays()
    s, slots, shade = TQ.scene(pa, name)
    for k in (0, 1, 4, 32):
        count, ident = s.TraceAll(rays, k)
        assert count.dtype == np.uint32 and ident.dtype == np.uint32 and ident.shape == (len(rays), k, 4)
        c, i = trace_all(s, _dev(rays), k)
        assert count.tobytes() == c.tobytes() and (k == 0 or ident.tobytes() == i.tobytes()), k
    count, ident = s.TraceAll(AM.as_rays(rays), 4)  # (n, 8) rows
    assert ident.tobytes() == i[:, :4].tobytes()
    if name == "soup":
        assert_rows_equal(ident, soup_model(pa, HOST_SAH)["ident"][:, :4])


def test_rays_made_on_a_side_stream_are_read_after_it(pa):
    import torch
    rays = TQ.soup()[1]
    s, slots, shade = TQ.scene(pa, "soup")
    want = soup_model(pa, HOST_SAH)
    src = _dev(rays)
    busy = torch.ones((2048, 2048), device="cuda:0")
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    d_rays = torch.zeros_like(src)  # (read too early: inactive rays, no hits)
    with torch.cuda.stream(side):
        for _ in range(20):  # work in front of the kernel that makes the array
            busy = busy @ busy * 1e-4
        d_rays.copy_(src * 1.0)
        count, ident = s.TraceAllDevice(d_rays, 4)                      # torch's current stream: the side stream
    count2, ident2 = s.TraceAllDevice(d_rays, 4, stream=side)           # ... and named
    count3, _ = s.TraceAllDevice(d_rays, 0, stream=side.cuda_stream)
    assert_rows_equal(_u32(ident), want["ident"][:, :4])
    assert_rows_equal(_u32(count), want["count"])
    assert torch.equal(ident, ident2) and torch.equal(count, count2) and torch.equal(count, count3)


def test_sizes_outputs_in_place_and_pointer_pairs(pa):
    import torch
    rays = TQ.soup()[1]
    s, slots, shade = TQ.scene(pa, "soup")
    want = soup_model(pa, HOST_SAH)
    for n in (1, 63, 64, 65, 257):
        for wide in (None, "0"):
            with wide_env(wide):
                c, i = trace_all(s, _dev(rays[:n]), 3)
            assert_rows_equal(c, want["count"][:n], (n, wide))
            assert_rows_equal(i, want["ident"][:n, :3], (n, wide))
    d = _dev(rays[:500])
    count, ident = torch.zeros((500,), dtype=torch.int32, device="cuda:0"), torch.zeros((500, 4, 4), dtype=torch.int32, device="cuda:0")
    assert s.TraceAllDevice(d, 4, count=count, ident=ident) == (count, ident)
    assert_rows_equal(_u32(ident), want["ident"][:500, :4])
    count.zero_(), ident.zero_()
    got = s.TraceAllDevice((d.data_ptr(), 500), 4, count=count.data_ptr(), ident=ident.data_ptr())
    assert got == (count.data_ptr(), ident.data_ptr())
    assert_rows_equal(_u32(count), want["count"][:500])
    assert_rows_equal(_u32(ident), want["ident"][:500, :4])
    with pytest.raises(ValueError):
        s.TraceAllDevice(d, 4, ident=torch.zeros((500, 3, 4), dtype=torch.int32, device="cuda:0"))  # another K's rows


def test_across_the_grid_stride(pa):
    """more rays than one full grid of the launch holds (4096 blocks of 256): every copy of the ray set equals the first"""
    rays = TQ.soup()[1][:3000]
    s, slots, shade = TQ.scene(pa, "soup")
    want = soup_model(pa, HOST_SAH)
    copies = 4096 * 256 // len(rays) + 2
    assert copies * len(rays) > 4096 * 256 + len(rays)
    d = _dev(rays).repeat(copies, 1)
    for wide in (None, "0"):
        with wide_env(wide):
            count, ident = s.TraceAllDevice(d, 2)
        count, ident = count.reshape(copies, len(rays)), ident.reshape(copies, len(rays), 2, 4)
        assert bool((count == count[:1]).all()) and bool((ident == ident[:1]).all())
        assert_rows_equal(_u32(ident[0]), want["ident"][:3000, :2], wide)
        assert_rows_equal(_u32(count[0]), want["count"][:3000], wide)


def test_state_and_empty_calls(pa):
    from pbrlab_amd import api
    rays = TQ.soup()[1][:257]
    for name in ("triangle", "curve", "empty"):
        s, slots, shade = TQ.scene(pa, name)
        for wide in (None, "0"):
            with wide_env(wide):
                c, i = trace_all(s, _dev(rays), 4)
                closest = _u32(s.TraceClosestDevice(_dev(rays))[0])
            assert i[:, 0].tobytes() == closest.tobytes() and np.array_equal(c > 0, closest[:, 0] != NONE)
            if name == "empty":
                assert not c.any() and (i == (NONE, 0, 0, 0)).all()
    s, slots, shade = TQ.scene(pa, "triangle")
    L = s.L
    assert L.pbrhip_trace_all_device(s.h, None, 0, 4, None, None, None) == 0 and L.pbrhip_trace_all(s.h, None, 0, 0, None, None) == 0
    count, ident = s.TraceAll(np.zeros((0, 8), F), 4)
    assert count.shape == (0,) and ident.shape == (0, 4, 4)
    fresh = api.Scene()  # not committed
    for call in (lambda: fresh.TraceAll(np.zeros((4, 8), F), 4), lambda: fresh.TraceAllDevice(_dev(np.zeros((4, 8), F)), 4)):
        with pytest.raises(api.PbrHipError) as e:
            call()
        assert e.value.code == -6
