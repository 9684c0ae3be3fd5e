"""The ray, all-hits, nearest-point and signed-distance contracts away from the unit box, without a GPU.

Every other test of them works in one place of float32 space: inside [-1, 1]^3, around the origin, with triangle edges of about 0.3.
tests/_soups.py::PLACEMENTS puts the same adversarial soup elsewhere -- uniform scales from 1e-10 to 1e10, offsets of 4096, 1e5 and 1e7,
anisotropic scales, flattened into a plane, collapsed to a line and to a point -- and adds rays that share coordinates exactly with
vertices: axis-parallel ones through a vertex and rays with one zero direction component inside a vertex's coordinate plane.

* The oracle's tree equals its brute force as bytes on every placement (closest hit, and any-hit with tmax == hit distance); no placement
  is vacuous: where two or more dimensions are kept at least 25 % of each ray family hit, on the line and the point nothing does.
* tests/_allhits_model.py's brute force equals the oracle's there: entry 0 and count.
* The float32 nearest-point model (tests/_query_model.py) stays within MODEL_ERR_UNITS of tests/test_query_cpu.py of the float64 distance
  at every uniform scale 10^k, k = -8 .. 9, and on the offset, anisotropic and flat placements, on all four seeds; at k = -9 and k = 10 it
  does not, so the domain stated in DESIGN.md §19 is the measured one.  Measured (all four seeds, 3000 points, 1.29 M candidates each): the
  largest error is 5.10 units over k = -8 .. 9 and 1.97 on the other placements; 95 to 212 units per seed at k = -9; infinities at k =
  10.  With the plane term written (h * h) / nn, as it was, the same sweep gives 128 units at k = -5, 5.3e4 at k = -6 and 2.5e6 at k = 7.
* The signed-distance model's sign equals the float64 winding number on the six shapes of tests/_sdf_model.py at the same scales and at
  the offset (4096, -300, 1e4)."""
import functools

import numpy as np
import pytest

import _allhits_model as AM
import _query_model as QM
import _sdf_model as SM
import _soups
from test_query_cpu import MODEL_ERR_UNITS

F = np.float32
NONE = 0xFFFFFFFF
SOUP_SEED, SLIVERS = 1, 30                                    # the soup of the ray tests: 430 triangles, 16 000 rays
DECADES = tuple(f"scale_1e{k}" for k in range(-8, 10))        # the nearest-point and signed-distance domain, uniform scales
OUTSIDE = ("scale_1e-9", "scale_1e10")
ELSEWHERE = ("offset_4096", "offset_1e5", "scale_1e3_offset_1e7", "anisotropic", "anisotropic_2", "flat_z", "flat_z_1000", "flat_x")
SD_OFFSET = (4096.0, -300.0, 1e4)


def sd_offset_near(v):
    """The distance, in the scene's units, below which a point is not held to the ground truth at SD_OFFSET.  The sign is that of
    dot(p - q, N), and the closest point q is a float32 position: each of its coordinates is rounded by up to half an ulp of the largest
    coordinate (2^-10 at 1e4, against 2^-24 around the origin), so p - q is off by up to sqrt(3) / 2 ulp and means nothing below that.
    That is 8.5e-4, between 19 and 40 times SM.NEAR diameters on the six shapes.  (A flat 1e3 x SM.NEAR = 1e-2 diameters cannot stand
    beside the condition that at most 1 % of the points are not held: the points displaced by 1e-3 and 1e-2 diameters, a quarter of the
    set, lie within it by construction.)"""
    return np.sqrt(3.0) / 2.0 * float(np.spacing(F(np.abs(v).max())))


# ------------------------------------------------------------------------------------------------ rays
@functools.lru_cache(maxsize=4)
def placed(name):
    """-> (desc, oracle scene, rays, the oracle's brute-force closest hits)"""
    desc, so, rays = _soups.placed_soup(SOUP_SEED, SLIVERS, name)
    return desc, so, rays, so.trace_closest(rays, brute_force=True)


@pytest.mark.parametrize("name", list(_soups.PLACEMENTS))
def test_oracle_tree_equals_oracle_brute_force(name):
    desc, so, rays, hb = placed(name)
    assert len(desc.vertices) == 3 * 430 and len(rays) == 16000
    assert so.trace_closest(rays).tobytes() == hb.tobytes()
    hit = hb["instance_id"] != NONE
    assert np.isfinite(hb["t"][hit]).all()
    short = rays.copy()
    short["tmax"] = np.where(hit, hb["t"], 1.0)               # tmax == hit distance: accepted (t <= tmax)
    ob = so.trace_any(short, brute_force=True)
    assert np.array_equal(so.trace_any(short), ob) and ob[hit].all()
    share = {k: float(hit[v].mean()) for k, v in _soups.ray_families(rays).items()}
    print(name, {k: f"{100 * v:.1f} %" for k, v in share.items()})
    if _soups.kept_dimensions(name) >= 2:
        assert min(share.values()) >= 0.25, share
    else:
        assert not hit.any()                                  # every triangle is degenerate: the scene still commits, nothing is hit


def test_unit_placement_is_the_soup():
    desc, so, rays = _soups.triangle_soup(SOUP_SEED, SLIVERS)
    pdesc, _, prays, _ = placed("unit")
    assert pdesc.vertices.tobytes() == desc.vertices.tobytes() and prays[:len(rays)].tobytes() == rays.tobytes()
    fam = _soups.ray_families(prays)
    a, b = prays[fam["axis-parallel"]], prays[fam["in-plane"]]
    v = desc.vertices[:, :3]
    # an axis-parallel ray has two zero direction components of either sign and shares those two coordinates with a vertex, exactly
    assert ((a["dir"] == 0).sum(axis=1) == 2).all() and np.signbit(a["dir"][a["dir"] == 0]).any() and not np.signbit(a["dir"][a["dir"] == 0]).all()
    keys = {tuple(x) for k in range(3) for x in np.concatenate([np.full((len(v), 1), k), np.delete(v, k, axis=1)], axis=1).tolist()}
    ax = np.argmax(a["dir"] != 0, axis=1)
    assert all((int(k),) + tuple(np.delete(o, k).tolist()) in keys for k, o in zip(ax, a["org"]))
    # an in-plane ray has one, and its origin has that coordinate of a vertex
    assert ((b["dir"] == 0).sum(axis=1) == 1).all() and np.signbit(b["dir"][b["dir"] == 0]).any()
    ax = np.argmax(b["dir"] == 0, axis=1)
    assert all(o[k] in v[:, k] for k, o in zip(ax, b["org"]))


@pytest.mark.parametrize("name", list(_soups.PLACEMENTS))
def test_allhits_model_equals_the_oracle(name):
    """entry 0 and count of the model's brute force against the oracle's, as tests/test_allhits_cpu.py holds them at unit scale"""
    desc, so, rays, want = placed(name)
    tris = np.ascontiguousarray(desc.vertices[:, :3].reshape(-1, 3, 3), F)
    n = len(tris)
    slots, shade = np.zeros((n, 4, 4), F), np.zeros((n, 32), np.uint32)
    slots[:, :3, :3], shade[:, 24] = tris, np.arange(n)
    res = AM.brute_force(rays, slots, shade, 1)
    first = res["ident"][:, 0]
    hit = want["instance_id"] != NONE
    assert np.array_equal(hit, first[:, 0] != NONE) and np.array_equal(hit, res["count"] > 0)
    for word, f in ((1, "u"), (2, "v"), (3, "t")):
        assert np.array_equal(first[hit, word], want[f][hit].view(np.uint32)), f
    assert (first[~hit] == (NONE, 0, 0, 0)).all()
    assert np.array_equal(first[hit, 0], want["instance_id"][hit] * 250 + want["prim_id"][hit])


# ------------------------------------------------------------------------------------------------ nearest point
def placed_points(seed, name, n=3000):
    """-> (tris, slots, shade, points) of the soup with 30 extra slivers at a placement: triangles and the points of
    tests/_query_model.py::soup_points go through the same v * s + t, so a point on a vertex stays on it; max_dist scales with the
    middle one of the three axes"""
    s, t, _ = _soups.placement(name)
    unit = np.ascontiguousarray(_soups.triangle_soup(seed, 30)[0].vertices[:, :3].reshape(-1, 3, 3), F)
    pts = QM.soup_points(unit, seed, n)
    tris = _soups.place(unit, s, t)
    pts[:, :3], pts[:, 3] = _soups.place(pts[:, :3], s, t), pts[:, 3] * np.median(np.abs(s))
    m = len(tris)
    slots, shade = np.zeros((m, 4, 4), F), np.zeros((m, 32), np.uint32)
    slots[:, :3, :3], shade[:, 24] = tris, np.arange(m)
    return tris, slots, shade, pts


def model_error(seed, name):
    """-> (largest |sqrt(D2) - d64| over all candidates in units of 2^-24 (largest |coordinate| + d64), inf when a candidate is not
    finite; largest | |p - q| - sqrt(D2) | of the winners; the coordinate bound that figure is held against)"""
    tris, slots, shade, pts = placed_points(seed, name)
    D2, U, V, Q, clamped = cand = QM.candidates(pts, slots, shade)
    res = QM.brute_force(pts, slots, shade, cand)
    p = pts[:, None, :3]
    d64 = QM.tri_dist64(p, tris[None, :, 0], tris[None, :, 1], tris[None, :, 2])
    big = np.maximum(np.abs(p).max(axis=-1), np.abs(tris).reshape(len(tris), 9).max(axis=1)[None, :])
    with np.errstate(all="ignore"):
        err = np.abs(np.sqrt(D2.astype(np.float64)) - d64) / (2.0 ** -24 * (big + d64))
    finite = all(np.isfinite(a).all() for a in (D2, U, V, Q))
    f = res["found"]
    d = (pts[f, :3] - res["q"][f]).astype(np.float64)
    gap = np.abs(np.sqrt((d * d).sum(axis=1)) - np.sqrt(res["d2"][f].astype(np.float64))).max()
    s, t, _ = _soups.placement(name)
    return (float(err.max()) if finite and np.isfinite(err).all() else np.inf), float(gap), 4.0 * float(np.abs(s).max()) + float(np.abs(t).max())


@pytest.mark.parametrize("seed", range(4))
@pytest.mark.parametrize("name", DECADES + ELSEWHERE)
def test_nearest_model_is_close_to_float64(name, seed):
    err, gap, coord = model_error(seed, name)
    print(f"{name} seed {seed}: largest |sqrt(D2) - d64| = {err:.3f} units; winners' | |p - q| - sqrt(D2) | = {gap / (2.0 ** -24 * coord):.3f} units of the coordinate bound")
    assert err <= MODEL_ERR_UNITS
    # the closest point is where the distance says (test_query_cpu.py holds this with the coordinate bound 4 of the unit soup)
    assert gap <= MODEL_ERR_UNITS * 2.0 ** -24 * coord


@pytest.mark.parametrize("name", OUTSIDE)
def test_nearest_model_domain_ends_where_it_is_said_to(name):
    """one decade past either end the model is NOT within the bar: (h / nn) * h still divides by the fourth power of an edge"""
    errs = [model_error(seed, name)[0] for seed in range(4)]
    print(name, errs)
    assert min(errs) > MODEL_ERR_UNITS


# ------------------------------------------------------------------------------------------------ signed distance
def placed_shape(shape, name):
    """-> (vertices as float32 rounded, in float64; faces; points (n, 4) float32; inside; float64 distance; diameter) of a shape of
    tests/_sdf_model.py at a placement or at SD_OFFSET ("sd_offset")"""
    v, f = SM.shape(shape)
    s, t = (np.ones(3, F), np.array(SD_OFFSET, F)) if name == "sd_offset" else _soups.placement(name)[:2]
    vp = _soups.place(v, s, t).astype(np.float64)
    pts = SM.sample_points(vp, f, sorted(SM.SHAPES).index(shape))
    p = pts[:, :3].astype(np.float64)
    return vp, f, pts, np.rint(SM.winding_number(p, vp[f])) == 1, SM.dist64(p, vp[f]), SM.diameter(vp)


@pytest.mark.parametrize("shape", sorted(SM.SHAPES))
@pytest.mark.parametrize("name", DECADES + ("sd_offset",))
def test_signed_model_sign_equals_the_winding_number(name, shape):
    """tests/test_sdf_cpu.py::test_model_sign_equals_the_winding_number's conditions, placed"""
    v, f, pts, inside, dist, diam = placed_shape(shape, name)
    slots, shade = SM.mesh_slots(v, f)
    m = SM.signed_model(pts, slots, shade, SM.pseudonormals64(v[f], f).astype(F))
    assert m["res"]["found"].all()
    near = sd_offset_near(v) / diam if name == "sd_offset" else SM.NEAR
    held = dist > near * diam
    n = len(inside)
    big = np.abs(v).max() + dist
    err = np.abs(np.abs(m["sd"][:, 3].astype(np.float64)) - dist) / (2.0 ** -24 * big)
    print(f"{shape} at {name}: {n} points, {int(inside.sum())} inside, {int((~held).sum())} nearer than {near:.2e} diameters, distance within {err.max():.2f} units")
    assert 1900 <= n <= 2100 and (~held).sum() <= 0.01 * n
    assert inside.sum() > 100 and (~inside).sum() > 100
    bad = np.nonzero(held & ((m["sd"][:, 3] < 0) != inside))[0]
    assert len(bad) == 0, (shape, name, len(bad), bad[:5], m["sd"][bad[:5]], m["feature"][bad[:5]])
    count = np.bincount(m["feature"], minlength=8)
    assert count[0:3].sum() > 0 and count[3:6].sum() > 0 and count[6] > 0 and count[7] == 0
    assert err.max() <= MODEL_ERR_UNITS
