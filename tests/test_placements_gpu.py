"""GPU (-m gpu): the ray, all-hits, refit, nearest-point, signed-distance and whole-frame contracts away from the unit box.

tests/test_placements_cpu.py shows on the CPU that the references stay inside their contracts at the placements of tests/_soups.py
(scales 1e-10 .. 1e10, offsets of 4096, 1e5 and 1e7, anisotropic, flat, collapsed to a line and to a point) and that none of them is
vacuous.  Here every GPU tree is asked the same, one placement per test:

* rays: trace_closest, trace_any (tmax == hit distance) and TraceClosestDevice equal the oracle's brute force as bytes under the host SAH
  builder (Q tree and PBRHIP_WIDE=0), the GPU LBVH and its wide collapse, each with the default traversal, PBRHIP_SIMPLE_TRAVERSAL=1 and
  PBRHIP_QUAD=1 + PBRHIP_QUAD_RAYS; FetchSceneAABB equals the oracle's;
* all hits: TraceAll at K = 4 equals tests/_allhits_model.py over the scene's own slots, count and rows as bytes, under the three builders;
* refit: the unit soup, committed once per builder, is moved to the placement (UpdateTriangleMesh + RefitScene, and once through
  UpdateTriangleMeshDevice): hits and bounds equal a fresh commit's and the brute force;
* nearest point: NearestPointDevice and NearestPoint equal tests/_query_model.py over the scene's slots bit for bit, no query left out, on
  the triangle soup at 10^k, k in {-8, -6, -3, 3, 6, 9}, and on the offset, anisotropic and flat placements, and on the curve soup at
  1e-3, 1e3 and the offset 4096; three builders; sizes 1, 65 and 3000;
* signed distance: on the six shapes at 10^k, k in {-8, -6, -3, 3, 6, 9}, and at the offset (4096, -300, 1e4) the GPU equals the float32
  model with the device's own table bit for bit, that table is within tests/_sdf_model.py::pseudonormal_bounds of the float64 one, and
  the sign equals the winding number at every held point.  k = -8 and k = 9 are the ends of the domain DESIGN.md §20 states: the table's
  dot(n, n) is fourth order in edge length, as the query's is;
* frames: the golden scenes lambert, sss, hair and textured at 48 x 32 x 4 spp at scale 100 + offset (1000, -500, 2000), at scale 0.01
  and at the offset (4096, 4096, -4096): rgba and count equal the oracle's as bytes with tail_paths 0 and 0xFFFFFFFF."""
import functools
import os

import numpy as np
import pytest

import _allhits_model as AM
import _oracle as O
import _query_model as QM
import _sdf_model as SM
import _soups
import test_placements_cpu as PC

pytestmark = pytest.mark.gpu

F = np.float32
NONE = 0xFFFFFFFF
HOST_SAH, GPU_LBVH, GPU_LBVH_WIDE = 0, 1, 2
BUILDERS = (HOST_SAH, GPU_LBVH, GPU_LBVH_WIDE)
TREES = ((HOST_SAH, None), (HOST_SAH, "0"), (GPU_LBVH, None), (GPU_LBVH_WIDE, None))  # (builder, PBRHIP_WIDE)
TRAVERSALS = ({}, {"PBRHIP_SIMPLE_TRAVERSAL": "1"}, {"PBRHIP_QUAD": "1", "PBRHIP_QUAD_RAYS": str(1 << 30)})
NEAREST_AT = tuple(f"scale_1e{k}" for k in (-8, -6, -3, 3, 6, 9)) + PC.ELSEWHERE
CURVES_AT = (("scale_1e-3", 1e-3, (0.0, 0.0, 0.0)), ("scale_1e3", 1e3, (0.0, 0.0, 0.0)), ("offset_4096", 1.0, (4096.0, -4096.0, 4096.0)))
SD_AT = tuple(f"scale_1e{k}" for k in (-8, -6, -3, 3, 6, 9)) + ("sd_offset",)
FRAMES_AT = (("scale_100_offset", 100.0, (1000.0, -500.0, 2000.0)), ("scale_0.01", 0.01, (0.0, 0.0, 0.0)), ("offset_4096", 1.0, (4096.0, 4096.0, -4096.0)))
SIZES = (1, 65, 3000)
U = 2.0 ** -24


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


class env:
    """environment switches for the calls inside (read per call); a value of None leaves a variable alone; what the suite was started
    with comes back on exit"""

    def __init__(self, **values):
        self.values = {k: v for k, v in values.items() if v is not None}

    def __enter__(self):
        self.before = {k: os.environ.get(k) for k in self.values}
        os.environ.update(self.values)

    def __exit__(self, *exc):
        for k, v in self.before.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def assert_hits_equal(a, b, what=""):
    for f in ("instance_id", "geom_id", "prim_id"):
        assert np.array_equal(a[f], b[f]), (what, f, np.nonzero(a[f] != b[f])[0][:5])
    for f in ("t", "u", "v", "normal_g"):
        x, y = (np.ascontiguousarray(h[f]).view(np.uint32) for h in (a, b))
        assert np.array_equal(x, y), (what, f, np.nonzero((x != y).reshape(len(x), -1).any(axis=1))[0][:5])


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ------------------------------------------------------------------------------------------------ rays
@functools.lru_cache(maxsize=2)
def placed(name):
    """-> (desc, rays, the oracle's brute-force hits, tmax == hit distance rays, the oracle's brute-force occlusion, the oracle's bounds)"""
    desc, so, rays = _soups.placed_soup(PC.SOUP_SEED, PC.SLIVERS, name)
    hb = so.trace_closest(rays, brute_force=True)
    short = rays.copy()
    short["tmax"] = np.where(hb["instance_id"] != NONE, hb["t"], 1.0)
    return desc, rays, hb, short, so.trace_any(short, brute_force=True), so.FetchSceneAABB()


def check_rays(pa, s, name, what):
    """every way of tracing the placement's rays through the committed scene s against the oracle's brute force"""
    desc, rays, hb, short, ob, (lo, hi) = placed(name)
    glo, ghi = s.FetchSceneAABB()
    assert np.array_equal(bits(lo), bits(glo)) and np.array_equal(bits(hi), bits(ghi)), (what, lo, glo, hi, ghi)
    d_rays = _dev(rays.view(F).reshape(-1, 8))
    for switches in TRAVERSALS:
        with env(**switches):
            assert_hits_equal(s.trace_closest(rays), hb, (what, switches))
            assert np.array_equal(s.trace_any(short), ob), (what, switches)
            hits = _host(s.TraceClosestDevice(d_rays)[1]).view(pa.api.HIT_DT).reshape(-1)
            assert_hits_equal(hits, hb, (what, switches, "device"))


@pytest.mark.parametrize("name", list(_soups.PLACEMENTS))
def test_rays_equal_the_oracles_brute_force(pa, name):
    desc, rays, hb = placed(name)[:3]
    hit = hb["instance_id"] != NONE
    assert len(rays) == 16000 and (hit.mean() >= 0.25 if _soups.kept_dimensions(name) >= 2 else not hit.any())
    scenes = {}
    for builder, wide in TREES:
        if builder not in scenes:
            scenes[builder] = pa.scene_from_desc(desc, bvh_builder=builder)
        with env(PBRHIP_WIDE=wide):
            check_rays(pa, scenes[builder], name, (name, builder, wide))


# ------------------------------------------------------------------------------------------------ all hits
@pytest.mark.parametrize("name", list(_soups.PLACEMENTS))
def test_all_hits_equal_the_model(pa, name):
    desc, rays = placed(name)[:2]
    for builder in BUILDERS:
        s = pa.scene_from_desc(desc, bvh_builder=builder)
        slots, shade = s.read_slots()
        want = AM.brute_force(rays, slots, shade, 4)
        count, ident = s.TraceAll(rays, 4)
        bad = np.nonzero((count != want["count"]) | (ident != want["ident"]).reshape(len(rays), -1).any(axis=1))[0]
        assert len(bad) == 0, (name, builder, len(bad), bad[:5], count[bad[:3]], want["count"][bad[:3]], ident[bad[:2]], want["ident"][bad[:2]])


# ------------------------------------------------------------------------------------------------ refit
@pytest.mark.parametrize("name", list(_soups.PLACEMENTS))
def test_refit_to_the_placement_equals_a_fresh_commit(pa, name):
    unit = _soups.triangle_soup(PC.SOUP_SEED, PC.SLIVERS)[0]
    desc, rays, hb = placed(name)[:3]
    for builder, device_update in ((HOST_SAH, False), (GPU_LBVH, False), (GPU_LBVH_WIDE, False), (GPU_LBVH_WIDE, True)):
        s = pa.scene_from_desc(unit, bvh_builder=builder)
        for mesh in range(len(unit.shapes)):
            if device_update:
                s.UpdateTriangleMeshDevice(mesh, _dev(desc.vertices))
            else:
                s.UpdateTriangleMesh(mesh, desc.vertices)
        s.RefitScene()
        check_rays(pa, s, name, (name, builder, "refit", device_update))
        fresh = pa.scene_from_desc(desc, bvh_builder=builder)
        for a, b in zip(s.FetchSceneAABB(), fresh.FetchSceneAABB()):
            assert np.array_equal(bits(a), bits(b)), (name, builder)
        assert_hits_equal(s.trace_closest(rays), fresh.trace_closest(rays), (name, builder, "fresh"))


# ------------------------------------------------------------------------------------------------ nearest point
def check_nearest(s, pts, what):
    slots, shade = s.read_slots()
    want = QM.expected_buffers(QM.brute_force(pts, slots, shade))
    d_pts = _dev(pts)
    for n in SIZES:
        ident, closest = s.NearestPointDevice(d_pts[:n].contiguous())
        for got in ((_host(ident).view(np.uint32), _host(closest)), s.NearestPoint(pts[:n])):
            bad = np.nonzero((got[0] != want[0][:n]).any(axis=1) | (bits(got[1]) != bits(want[1][:n])).any(axis=1))[0]
            assert len(bad) == 0, (what, n, len(bad), bad[:5], got[0][bad[:3]], want[0][bad[:3]], got[1][bad[:3]], want[1][bad[:3]])
    return want


@pytest.mark.parametrize("name", NEAREST_AT)
def test_nearest_point_on_the_placed_soup_equals_the_model(pa, name):
    tris, _, _, pts = PC.placed_points(3, name)  # seed 3: the soup on which the validation bound changes candidates (tests/test_query_cpu.py)
    assert len(pts) == 3000 and np.isfinite(pts[1::3, 3]).sum() == 0 and np.isfinite(pts[::3, 3]).all()  # every third keeps a max_dist
    desc = _soups.placed_desc(_soups.triangle_soup(3, 30)[0], name)
    assert np.array_equal(desc.vertices[:, :3].reshape(-1, 3, 3), tris)
    for builder in BUILDERS:
        want = check_nearest(pa.scene_from_desc(desc, bvh_builder=builder), pts, (name, builder))
    found = want[0][:, 0] != NONE
    assert found[1::3].all() and found[::3].any() and not found[::3].all(), (int(found[::3].sum()),)  # the bound decides either way


@pytest.mark.parametrize("name,scale,offset", CURVES_AT)
def test_nearest_point_on_the_placed_curve_soup_equals_the_model(pa, name, scale, offset):
    # the points of the unit curve soup's own slots (a piece as the triangle (a, b, b)), placed with it; max_dist scales
    slots, shade = pa.scene_from_desc(_soups.curve_soup(0)[0]).read_slots()
    tris = slots[:, :3, :3].copy()
    curve = ((shade[:, 3] >> 24) & QM.SLOT_IS_CURVE) != 0
    assert curve.sum() >= 1000
    tris[curve, 2] = tris[curve, 1]
    pts = QM.soup_points(tris, 0, 3000)
    s, t = np.full(3, scale, F), np.array(offset, F)
    pts[:, :3], pts[:, 3] = _soups.place(pts[:, :3], s, t), pts[:, 3] * F(scale)
    desc = _soups.curve_soup(0, scale, offset)[0]
    for builder in BUILDERS:
        want = check_nearest(pa.scene_from_desc(desc, bvh_builder=builder), pts, (name, builder))
    found = want[0][:, 0] != NONE
    assert found[1::3].all() and found[::3].any() and not found[::3].all()


# ------------------------------------------------------------------------------------------------ signed distance
def _mesh_desc(v, f):
    from pbrlab_amd import scenes
    v4 = np.concatenate([np.asarray(v, F), np.ones((len(v), 1), F)], axis=1)
    mat = dict(scenes.PRINCIPLED_DEFAULTS, kind="principled", name="m")
    return scenes.SceneDesc(v4, np.zeros((0, 4), F), [mat], [scenes.Shape("s", np.asarray(f, np.uint32), None, np.zeros(len(f), np.uint32))])


@pytest.mark.parametrize("shape", sorted(SM.SHAPES))
@pytest.mark.parametrize("name", SD_AT)
def test_signed_distance_on_the_placed_shapes(pa, name, shape):
    v, f, pts, inside, dist, diam = PC.placed_shape(shape, name)
    assert np.array_equal(v.astype(F).astype(np.float64), v)  # the scene holds exactly the vertices of the ground truth
    s = pa.scene_from_desc(_mesh_desc(v, f))
    slots, shade = s.read_slots()
    table = s.read_pseudonormals()
    # 1. the GPU equals the float32 model with the device's own table, bit for bit
    m = SM.signed_model(pts, slots, shade, table)
    ident, closest, sd = s.SignedDistanceDevice(_dev(pts))
    ident, closest, sd = _host(ident).view(np.uint32), _host(closest), _host(sd)
    assert m["res"]["found"].all()
    assert np.array_equal(ident, m["ident"]) and np.array_equal(bits(closest), bits(m["closest"])), (shape, name)
    bad = np.nonzero((bits(sd) != bits(m["sd"])).any(axis=1))[0]
    assert len(bad) == 0, (shape, name, len(bad), bad[:5], sd[bad[:3]], m["sd"][bad[:3]], m["feature"][bad[:3]])
    # 2. the table is within the derived rounding bound of the float64 one
    idx = f[shade[:, 27]]
    corners = slots[:, :3, :3].astype(np.float64)
    want = SM.pseudonormals64(corners, idx)
    bound = SM.pseudonormal_bounds(corners, idx)
    err = np.linalg.norm(table[..., :3].astype(np.float64) - want, axis=2) / U
    ok = np.isfinite(bound)
    print(f"{shape} at {name}: largest table error {err[ok].max():.2f} x 2^-24, {(err[ok] / bound[ok]).max():.4f} of the derived bound")
    assert ok.all() and np.isfinite(table).all() and (err <= bound).all(), (shape, name, float((err / bound).max()))
    # 3. the sign equals the winding number at every held point
    near = PC.sd_offset_near(v) / diam if name == "sd_offset" else SM.NEAR
    held = dist > near * diam
    wrong = held & ((sd[:, 3] < 0) != inside)
    print(f"{shape} at {name}: {int((~held).sum())} of {len(pts)} points not held, {int(wrong.sum())} held points with the wrong sign")
    assert (~held).sum() <= 0.01 * len(pts) and inside.sum() > 100 and (~inside).sum() > 100
    assert not wrong.any(), (shape, name, pts[wrong][:5], sd[wrong][:5])
    big = np.abs(v).max() + dist
    assert (np.abs(np.abs(sd[:, 3].astype(np.float64)) - dist) <= PC.MODEL_ERR_UNITS * U * big).all()


# ------------------------------------------------------------------------------------------------ frames
@functools.lru_cache(maxsize=None)
def golden():
    from golden.make_golden import golden_scenes
    return golden_scenes()


@pytest.mark.parametrize("scene", ["lambert", "sss", "hair", "textured"])
@pytest.mark.parametrize("name,scale,offset", FRAMES_AT)
def test_frames_equal_the_oracles(pa, name, scale, offset, scene):
    desc = _soups.placed_scene(golden()[scene], scale, offset)
    sg, so = pa.scene_from_desc(desc), O.oracle_scene_from_desc(desc)
    for a, b in zip(sg.FetchSceneAABB(), so.FetchSceneAABB()):
        assert np.array_equal(bits(a), bits(b))
    rgba, count, _ = so.render(48, 32, 4, threads=4, math_mode=O.MATH_DEVICE)
    lit = float((rgba[..., :3].sum(axis=2) > 0).mean())
    assert np.isfinite(rgba).all() and 0.4 <= lit <= 0.7, lit  # the frame shows the scene (measured: 45 to 65 % of the pixels)
    for tail in (0, 0xFFFFFFFF):
        layer = pa.RenderLayer()
        pa.Render(sg, 48, 32, 4, layer=layer, tail_paths=tail)
        assert np.array_equal(layer.count, count) and layer.rgba.tobytes() == rgba.tobytes(), (scene, name, tail, int((bits(layer.rgba) != bits(rgba)).any(axis=2).sum()))
