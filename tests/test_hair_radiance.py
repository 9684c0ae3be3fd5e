"""The hair shader against float64 integrals (tests/_hair_analytic.py): what should a pixel on a strand converge to?

HairShader -- ParamToBsdf, the tangent frame, NEE with hemisphere = false and Q3 on the tangent, the MIS weights on both sides, the
curve path of the tracer feeding v into h -- is restated by the oracle, by k_shade_hair and by k_tail from one reading, and bit-parity
between them cannot see a mistake they share.  Here one straight strand under one emitting quad is rendered through a look-at pinhole
that zooms until the strand fills more than half of the columns, and every pixel on it is held to the model's expectation with
test_analytic_radiance's statistics, on the oracle and on the HIP renderer.

Why a strand pixel has a single-bounce closed form here (asserted by test_strand_conditions, from the model alone):
  (a) curve_test accepts t > tmin only and continuation / shadow rays start at tmin = 1e-3 (Q9).  A ray that leaves a straight strand of
      radius r at an angle psi to its axis finds the nearest axis point at a depth <= r (1 + cot psi); with r = 3.5e-5 that is <= 1e-3 for
      psi >= 2.08 degrees.  Every direction from the seen part of the strand to the light is further from the axis: no self-shadowing.
  (b) the density of the BSDF sampler, integrated over the two cones psi < 2.08 degrees, is <= 1e-4 for every seen (wo, h): camera
      paths that meet the strand twice carry at most 1e-4 of E.  The oracle's ray counts are held to that.
  The quad and the strand are >= 0.028 apart, 28 x the 1e-3 offsets; the quad is black, so a path ends on it.

Statistics: K = 64 batches of SPP_OF[case] samples per pixel; groups = 8 bands of h plus the whole strand; the Student-t / Bonferroni
bar of test_analytic_radiance.  A pixel counts when the 4 nodes of its 2 x 2 footprint rule lie on the strand with |h| <= 0.95.
Each case must reject 1.01 E and the mutations of the model listed in ALT_OF.

What the cases pin: rgb_side -- the frame, the sign of h (the R highlight sits on h ~ -0.6 only) and, through the edge of the TT lobe on
h > 0.75, the MIS weights (Q3 on the tangent); melanin_tinted_oblique -- melanin -> sigma_a, the tint order, the alpha rotation and the
longitudinal terms at theta_o = 35 degrees; blond_backlit -- the TT lobe, where the BSDF-sampled path carries a third of E;
light_facing_away -- NEE through the quad's back (hemisphere = false) with w_nee only: its quad stands behind the strand, where the
TT lobe sends most BSDF samples, so emission hits through the back would add > 5 %.
Why the quads of rgb_side and light_facing_away stand where the TT lobe reaches them: under a quad of 0.44 sr (edge 0.02 at 0.03)
the MIS weights of the R and TRT lobes alone sum to 1 within 0.3 %, which no affordable sample count tells from 1; the TT lobe's do not."""
import numpy as np
import pytest

import _analytic as A
import _camera_analytic as CA
import _hair_analytic as HA
import _oracle as O
import test_analytic_radiance as TR
from pbrlab_amd import scenes
from test_geometry_f64 import Geometry

W, H, K = TR.W, TR.H, TR.K
# samples per pixel and batch, per case: enough that 1.01 E is rejected on the whole-strand mean (its relative standard error must be
# below 1 % / bar = 1.6e-3) and no more than keeps that standard error above HA.MODEL_D, so that the model's own deviation from
# the leaf can move no z by more than 1
SPP_OF = {"rgb_side": 32, "melanin_tinted_oblique": 16, "blond_backlit": 16, "light_facing_away": 32}
MAX_NAN = 4                   # Q19: (batch, pixel) entries that may be NaN, per case
R = 3.5e-5                    # the strand's radius: the largest round value at which every case meets (b)
EYE_DIST = 0.05
VFOV = 0.107                  # degrees: 64 columns span 2.49e-3 rad, the strand (2 r at 0.05) 1.4e-3 of them = 36 columns
LIGHT_DIST, LIGHT_HALF = 0.03, 0.01
LE = (3.0, 2.5, 2.0)
H_MAX = 0.95
BANDS = 8
RETRACE_BOUND = 1e-4          # (b)
EYE, LOOKAT, UP = (0.0, 0.0, EYE_DIST), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0)

RGB_SIDE = dict(scenes.HAIR_DEFAULTS, kind="hair", name="hair", coloring_hair=0, base_color=(0.6, 0.4, 0.2), roughness=0.3,
                azimuthal_roughness=0.3, ior=1.55, shift=2.0)
MELANIN = dict(scenes.HAIR_DEFAULTS, kind="hair", name="hair", coloring_hair=1, melanin=0.5, melanin_redness=0.6, roughness=0.3,
               azimuthal_roughness=0.3, ior=1.55, shift=5.0, specular_tint=(1.0, 0.8, 0.6), transmission_tint=(0.7, 1.0, 0.7),
               second_specular_tint=(0.6, 0.8, 1.0))
BLOND = dict(RGB_SIDE, base_color=(0.9, 0.85, 0.7))
# case -> material, the strand's tilt out of the image plane (degrees), the light's direction from the origin, its winding reversed
CASES = {
    # on the camera's side (z > 0) and nearly level with the strand: the R highlight falls on h ~ -0.6, the edge of the TT lobe on h > 0.75
    "rgb_side": (RGB_SIDE, 10.0, (1.0, -0.3, 0.1), False),
    # the R highlight (theta_i = -25 degrees) inside the light, Q17's jump of the R lobe (|theta_i| = 45.6 degrees) outside it
    "melanin_tinted_oblique": (MELANIN, 35.0, (-0.8, -0.5, 0.4), False),
    "blond_backlit": (BLOND, 10.0, (0.25, -0.1, -1.0), False),
    # behind the strand, where the TT lobe sends most BSDF samples, its back to it
    "light_facing_away": (RGB_SIDE, 10.0, (-0.3, 0.15, -1.0), True),
}
ALT_OF = {"rgb_side": ("flip_h", "physical_mis"), "melanin_tinted_oblique": ("flip_h", "swap_tints"), "blond_backlit": ("flip_h", "physical_mis"),
          "light_facing_away": ("count_emission",)}
PIX_OTHER, PIX_STRAND, PIX_ZERO, PIX_LIGHT = 0, 1, 2, 3


def scene_of(case):
    """(SceneDesc, axis, light triangles (2,3,3)): the strand's control points equally spaced along `axis`, from -0.019 to 0.029 (half
    length 0.024; the origin lies inside the second of the ribbon's four pieces, 5e-3 from its ends), the quad facing the origin"""
    mat, tilt, ldir, reverse = CASES[case]
    t = np.radians(tilt)
    axis = np.array([0.0, np.cos(t), np.sin(t)])
    cp = np.concatenate([np.linspace(-0.019, 0.029, 4)[:, None] * axis, np.full((4, 1), R)], 1).astype(np.float32)
    c = np.asarray(ldir, np.float64)
    c = LIGHT_DIST * c / np.linalg.norm(c)
    n = -c / np.linalg.norm(c)                         # towards the strand
    a = np.cross(n, [0.0, 1.0, 0.0])
    a = LIGHT_HALF * a / np.linalg.norm(a)
    bb = np.cross(n, a)                                # a x bb = n |a|^2: scenes._quad's normal (p1 - p0) x (p2 - p0) is along n
    p = [c - a - bb, c + a - bb, c + a + bb, c - a + bb]
    if reverse:
        p = p[::-1]
    b = scenes._Builder()
    v, f = scenes._quad(*p)
    b.add("light", v, f, 0)
    black = dict(scenes.PRINCIPLED_DEFAULTS, kind="principled", name="black", **A.BLACK)
    desc = b.finish([black], [scenes.CurveShape("strand", cp, np.zeros(1, np.uint32), material=mat)])
    desc.light_emission = LE
    tris = desc.vertices[:, :3].astype(np.float64)[desc.shapes[0].vertex_ids.astype(np.int64)]
    want = -n if reverse else n
    assert np.allclose(np.cross(tris[0, 1] - tris[0, 0], tris[0, 2] - tris[0, 0]) / (4 * LIGHT_HALF ** 2), want, atol=1e-5)
    return desc, cp[3, :3].astype(np.float64) - cp[0, :3].astype(np.float64), tris


_expect = {}
ANCHORS = (0, H, 2 * H - 1)   # the row nodes at which E is integrated; between them it is a parabola to 1e-7 (test_quadrature_converged)


def expected(case):
    """per case, once per session (both back ends use it): the scene, the pixel classes, E and its mutations per pixel, the nodes.

    The nodes of the 2 x 2 footprint rule form a grid of 2 W column nodes x 2 H row nodes.  Along a column node h moves by < 1 % and
    the hit point by < 3e-4 (1 % of the light's distance): E is integrated at three row nodes of every column node and interpolated
    by the parabola through them in between."""
    if case in _expect:
        return _expect[case]
    desc, axis, tris = scene_of(case)
    axis = axis / np.linalg.norm(axis)
    geo = Geometry(desc)
    cam = CA.LookAt(EYE, LOOKAT, UP, VFOV, W, H)
    ex = HA.StrandExpectation(CASES[case][0], axis, tris, LE, alts=ALT_OF[case])
    g, gw = A.gauss_legendre01(2)
    cx = (np.arange(W)[:, None] + g[None]).ravel()             # column nodes: image x of node 2 px + i
    ry = (np.arange(H)[:, None] + g[None]).ravel()             # row nodes
    d = cam.dirs(cx[:, None], ry[None, :], 0.0, 0.0)           # (2W, 2H, 3)
    on, x, h, _ = HA.strand_hits(geo, cam.org, d.reshape(-1, 3))
    on, h, x = on.reshape(2 * W, 2 * H), h.reshape(2 * W, 2 * H), x.reshape(2 * W, 2 * H, 3)
    ok = on & (np.abs(h) <= H_MAX)
    pix_ok = ok.reshape(W, 2, H, 2).all((1, 3)).T              # (H, W): all four nodes on the strand with |h| <= H_MAX
    pix_on = on.reshape(W, 2, H, 2).all((1, 3)).T
    cols = np.nonzero(ok.any(1))[0]
    assert on[cols].all(), "a column node of a counted pixel leaves the strand"
    a = np.asarray(ANCHORS)
    va = ex(x[cols][:, a].reshape(-1, 3), -d[cols][:, a].reshape(-1, 3), h[cols][:, a].reshape(-1)).reshape(len(cols), 3, -1)
    lag = np.stack([np.prod([(ry - ry[a[m]]) / (ry[a[k]] - ry[a[m]]) for m in range(3) if m != k], 0) for k in range(3)], 1)   # (2H, 3)
    node_val = np.zeros((2 * W, 2 * H, ex.channels))
    node_val[cols] = np.einsum("rk,ckn->crn", lag, va)
    val = np.einsum("xiyjn,i,j->yxn", node_val.reshape(W, 2, H, 2, -1), gw, gw)
    val[~pix_ok] = 0.0
    # off the strand: no node of a probe grid over the slightly widened footprint touches the ribbon
    py, px = (v.ravel().astype(np.float64) for v in np.mgrid[0:H, 0:W])
    js = np.linspace(-0.02, 1.02, 6)
    jx, jy = (v.ravel() for v in np.meshgrid(js, js, indexing="ij"))
    dp = cam.dirs(px[:, None], py[:, None], jx, jy).reshape(-1, 3)
    touched = HA.strand_hits(geo, cam.org, dp, margin=-0.02)[0].reshape(-1, 36).any(1)
    S = A.Scene([A.Mesh("light", desc.vertices[:, :3].astype(np.float64), desc.shapes[0].vertex_ids.astype(np.int64), {},
                        emission=np.tile([LE], (2, 1)))])
    mesh, _, _, front = A.cast(S, cam.org, dp)
    mesh, front = mesh.reshape(-1, 36), front.reshape(-1, 36)
    cls = np.full(W * H, PIX_OTHER)
    cls[~touched & ((mesh < 0) | ~front).all(1)] = PIX_ZERO
    cls[~touched & ((mesh == 0) & front).all(1)] = PIX_LIGHT
    cls = cls.reshape(H, W)
    assert not (pix_ok & (cls != PIX_OTHER)).any()
    cls[pix_ok] = PIX_STRAND
    val[cls == PIX_LIGHT] = np.tile(LE, 1 + len(ex.alts))
    sel = ok.copy()
    sel[~np.repeat(np.repeat(pix_ok.T, 2, 0), 2, 1)] = False   # the nodes of the counted pixels
    nodes = dict(x=x[sel], wo=-d[sel], h=h[sel], val=node_val[sel])
    out = dict(desc=desc, axis=axis, tris=tris, cam=cam, ex=ex, cls=cls, val=val[..., :3], nodes=nodes,
               h=h.reshape(W, 2, H, 2).mean((1, 3)).T, on_strand=int(pix_on.sum()), columns=int(pix_ok.any(0).sum()),
               alt={n: val[..., 3 * k + 3:3 * k + 6] for k, n in enumerate(ex.alts)})
    _expect[case] = out
    return out


def groups_of(e):
    """BANDS equal bands of h over [-1, 1] that hold pixels, then the whole strand"""
    on = e["cls"] == PIX_STRAND
    band = np.clip(((e["h"] + 1.0) * 0.5 * BANDS).astype(int), 0, BANDS - 1)
    g = [on & (band == k) for k in range(BANDS)]
    return [m for m in g if m.sum() >= TR.MIN_CELL_PIXELS] + [on]


def build(case, backend, pa=None):
    desc = expected(case)["desc"]
    s = O.oracle_scene_from_desc(desc) if backend == "oracle" else pa.scene_from_desc(desc)
    s.SetCamera(EYE, LOOKAT, UP, VFOV)
    return s


_rendered = {}


def render_batches(case, backend):
    """K batches of SPP_OF[case] passes each, once per session and back end: (K,H,W,4) rgba, (K,H,W) count, the oracle's Stats per batch"""
    if (case, backend) in _rendered:
        return _rendered[case, backend]
    spp = SPP_OF[case]
    pa = TR._pa() if backend == "gpu" else None
    s = build(case, backend, pa)
    out, stats = [], []
    if backend == "oracle":
        th = O.oracle_threads()
        for k in range(K):
            rgba, cnt, st = s.render(W, H, spp, first_pass=k * spp, seed_seq=TR.SEED_SEQ, threads=th)
            out.append((rgba, cnt)), stats.append(st)
    else:
        for k in range(K):
            layer = pa.RenderLayer()
            pa.Render(s, W, H, spp, layer=layer, first_pass=k * spp, seed_seq=TR.SEED_SEQ)
            out.append((np.array(layer.rgba, np.float32).reshape(H, W, 4), np.array(layer.count, np.uint32).reshape(H, W)))
        # batch 0 through the wavefront kernels alone and through k_tail: k_shade_hair and k_tail both stand behind the statistic
        both = []
        for tail in (0xFFFFFFFF, 0):
            layer = pa.RenderLayer()
            ok, st = pa.Render(s, W, H, spp, layer=layer, first_pass=0, seed_seq=TR.SEED_SEQ, flags=pa.api.RENDER_STATS, tail_paths=tail)
            assert (st["n_tail"] == 0) == (tail == 0xFFFFFFFF)
            both.append(np.array(layer.rgba, np.float32).reshape(H, W, 4))
        assert np.array_equal(both[0].view(np.uint32), both[1].view(np.uint32)), "k_shade_hair and k_tail disagree on batch 0"
        assert np.array_equal(both[0].view(np.uint32), out[0][0].view(np.uint32))
        s.close()
    _rendered[case, backend] = np.stack([o[0] for o in out]), np.stack([o[1] for o in out]), stats
    return _rendered[case, backend]


def batch_means(case, backend):
    """(K,H,W,3) batch means with Q19's entries set to NaN, after the checks every frame must pass exactly"""
    e = expected(case)
    cls, val = e["cls"], e["val"]
    rgba, count, _ = render_batches(case, backend)
    assert (count == SPP_OF[case]).all() and (rgba[..., 3] == count).all()
    light, zero, on = cls == PIX_LIGHT, cls == PIX_ZERO, cls == PIX_STRAND
    want = count[..., None].astype(np.float32) * val.astype(np.float32)[None]
    assert (rgba[:, light, :3] == want[:, light]).all(), "a pixel on the quad's front, off the strand, is not exactly count * Le"
    assert (rgba[:, zero, :3] == 0).all(), "a pixel off the strand that sees the quad's back or nothing is not exactly 0"
    assert light.sum() + zero.sum() > 500 and (light.sum() > 500) == (case == "blond_backlit")
    # Q19: NEE hands the leaf's f cos_i / |wi . ex| (hair-shader.cc:197) to shader-utils.h:192-207, whose pdf_sigma divides by the same
    # wi . ex: a light sample exactly perpendicular to the tangent in float32 (about 1 in 1e7 where the light straddles that plane)
    # gives inf * weight(inf, pdf) / inf = NaN for the sample and for its pixel.  Such entries are counted, bounded and left out.
    bad = ~np.isfinite(rgba[..., :3]).all(-1)
    assert bad.sum() <= MAX_NAN and not bad[:, ~on].any() and np.isnan(rgba[bad][:, :3]).all(), (int(bad.sum()), np.argwhere(bad))
    means = rgba[..., :3] / count[..., None]
    means[bad] = np.nan
    return means, int(bad.sum())


@pytest.mark.parametrize("backend", TR.BACKENDS)
@pytest.mark.parametrize("case", sorted(CASES))
def test_hair_radiance(case, backend):
    """Measured (oracle; the HIP renderer's figures agree to the digits printed): the whole-strand mean is within 0.12 % of E on every
    case (relative standard errors 8e-4 .. 1.3e-3), max |z| over the bands 0.96 .. 2.42 under a bar of 6.27; 1.01 E reaches 7.4 .. 37,
    h -> -h more than 7000, swapped tints 53, MIS weights summing to 1 11.6 (rgb_side) and 288 (blond_backlit), emission through the
    quad's back 673, the hemisphere rule 1248.  No NaN entry (Q19) occurred in these runs; one did at another light position."""
    e = expected(case)
    cls, val = e["cls"], e["val"]
    on = cls == PIX_STRAND
    means, n_nan = batch_means(case, backend)
    groups = groups_of(e)
    assert len(groups) - 1 >= 8 and on.sum() >= (2.0 / 3.0) * e["on_strand"], (len(groups) - 1, on.sum(), e["on_strand"])
    assert e["columns"] >= 30
    stat = lambda v: TR.group_stats(means, groups, v, skip_nan=True)  # noqa: E731
    z, bar = stat(val)
    whole = np.nanmean(means[:, on], 1)
    rel_se = (whole.std(0, ddof=1) / np.sqrt(K)) / val[on].mean(0)
    print(f"{case} [{backend}]: {on.sum()} pixels in {len(groups) - 1} bands, {n_nan} NaN entries, max |z| {np.abs(z).max():.2f} (bar {bar:.2f}), "
          f"whole-strand rel err {' '.join(f'{r:+.1e}' for r in whole.mean(0) / val[on].mean(0) - 1)}, rel SE {' '.join(f'{r:.1e}' for r in rel_se)}")
    assert np.abs(z).max() < bar, (z, bar)
    assert rel_se.min() >= HA.MODEL_D, ("the model's deviation from the leaf could move a z by more than 1", rel_se, HA.MODEL_D)
    z1, _ = stat(val * 1.01)
    print(f"{case} [{backend}]: max |z| against 1.01 E {np.abs(z1).max():.2f}")
    assert np.abs(z1).max() >= bar, ("1.01 E is not rejected", np.abs(z1).max(), bar)
    for name, alt in e["alt"].items():
        za, _ = stat(alt)
        print(f"{case} [{backend}]: max |z| against {name}: {np.abs(za).max():.2f}")
        assert np.abs(za).max() >= bar, (f"{name} is not rejected", np.abs(za).max(), bar)
    if case == "light_facing_away":
        # the hemisphere rule (shader-utils.h:195 with hemisphere = true) would leave the strand black
        assert val[on].min() > 0
        z0, _ = stat(np.zeros_like(val))
        print(f"{case} [{backend}]: max |z| against the hemisphere rule (E = 0): {np.abs(z0).max():.2f}")
        assert np.abs(z0).max() >= bar


def test_paths_meet_the_strand_once():
    """(b) on the oracle's own ray counts, batch 0 of every case: off the strand a camera path is 1 closest-hit ray (a miss, or the black
    quad, whose shader returns a black throughput); on it 2, plus what meets the strand again: at most 10 x RETRACE_BOUND per path"""
    pix = np.stack([a.ravel() for a in np.mgrid[0:W, 0:H]], 1)
    for case in sorted(CASES):
        st = render_batches(case, "oracle")[2][0]
        s = build(case, "oracle")
        n_strand = 0
        for p in range(SPP_OF[case]):
            n_strand += int((s.trace_closest(s.camera_rays(W, H, pix, p=p, seed_seq=TR.SEED_SEQ))["instance_id"] == 1).sum())  # (the quad is instance 0)
        extra = st["closest_rays"] - st["samples"] - n_strand
        print(f"{case}: {n_strand} camera paths on the strand in batch 0, {extra} closest-hit rays beyond 2 per path")
        assert st["samples"] == W * H * SPP_OF[case] and n_strand > 0.4 * st["samples"]
        assert extra <= 10 * RETRACE_BOUND * n_strand, (case, extra, n_strand)


def test_strand_conditions():
    """(a) and (b), from the model alone, for every case"""
    psi = HA.self_hit_angle(R)
    assert R * (1.0 + 1.0 / np.tan(psi)) <= HA.TMIN * (1 + 1e-12) and np.degrees(psi) < 2.09
    g, gw = np.polynomial.legendre.leggauss(24)
    for case in sorted(CASES):
        e = expected(case)
        n = e["nodes"]
        # (a): the angle between the axis and every direction from a seen point to the light's corners (the extremes: the quad is convex)
        corners = e["tris"].reshape(-1, 3)
        d = corners[None] - n["x"][:, None]
        cosang = np.abs(np.sum(d * e["axis"], -1)) / np.linalg.norm(d, axis=-1)
        # the quad does not cross the axis, so the smallest angle to a convex quad is reached on its boundary; the boundary's edges are
        # checked at 33 points each
        tt = np.linspace(0, 1, 33)[:, None]
        quad = np.concatenate([e["tris"][0], e["tris"][1][2:]])
        edge = np.concatenate([quad[k] + tt * (quad[(k + 1) % 4] - quad[k]) for k in range(4)])
        de = edge[None] - n["x"][::50, None]
        cose = np.abs(np.sum(de * e["axis"], -1)) / np.linalg.norm(de, axis=-1)
        worst = np.degrees(np.arccos(max(cosang.max(), cose.max())))
        assert worst >= np.degrees(psi), (case, worst)
        assert np.linalg.norm(d, axis=-1).min() >= 10 * HA.TMIN and np.linalg.norm(corners - np.asarray(EYE), axis=-1).min() >= 10 * HA.TMIN
        # the camera rays themselves are further than psi from the axis (no kAmbiguous branch, and the tilt is >= 5 degrees)
        assert np.degrees(np.arcsin(np.abs(n["wo"] @ e["axis"]).min())) >= 5.0 - 0.2
        # (b): the sampler's density over the two cones psi' < psi about +-axis, 24 x 24 Gauss-Legendre each, on a spread of nodes
        i = np.linspace(0, len(n["x"]) - 1, 120).astype(int)
        ex = e["axis"]
        wo = n["wo"][i]
        ey = np.cross(np.cross(wo, ex), ex)
        ey /= np.linalg.norm(ey, axis=-1, keepdims=True)
        wol = np.stack([wo @ ex, np.sum(wo * ey, -1), np.zeros(len(i))], -1)[:, None, None]
        mu = 1.0 - (1.0 - np.cos(psi)) * 0.5 * (g + 1)                      # cos psi' over [cos psi, 1]
        ph = np.pi * (g + 1)
        wq = np.outer((1.0 - np.cos(psi)) * 0.5 * gw, np.pi * gw)
        st = np.sqrt(1.0 - mu * mu)[:, None]
        mass = 0.0
        for sgn in (1.0, -1.0):
            wil = np.stack(np.broadcast_arrays(sgn * mu[:, None], st * np.cos(ph), st * np.sin(ph)), -1)[None]
            b = HA.hair_param_to_bsdf(CASES[case][0], n["h"][i][:, None, None])
            mass = mass + (HA.hair_sample_density(wil, wol, b) * wq).sum((1, 2))
        print(f"{case}: the light stays {worst:.1f} degrees off the axis (psi_min {np.degrees(psi):.2f}); sampler mass inside the cones <= {mass.max():.1e}")
        assert mass.max() <= RETRACE_BOUND, (case, mass.max())


def test_quadrature_converged():
    """doubling the Gauss-Legendre order moves E and its mutations by < 1e-5 relative, on 200 nodes of every case.  (Q17 makes the leaf
    jump by a factor 2.7 where cos theta_i cos theta_o / v crosses 7.5; every case keeps its light inside that cone for the R lobe and
    far from it for the others, or this would not converge.)"""
    for case in sorted(CASES):
        e = expected(case)
        n = e["nodes"]
        i = np.random.RandomState(3).choice(len(n["x"]), 200, replace=False)
        a = e["ex"](n["x"][i], n["wo"][i], n["h"][i])
        b = e["ex"](n["x"][i], n["wo"][i], n["h"][i], order=2 * e["ex"].order)
        assert np.abs(b).max() > 0 and np.abs(a - b).max() < 1e-5 * np.abs(b).max(), (case, np.abs(a - b).max() / np.abs(b).max())
        # the parabola along a column node (expected) against the integral itself
        assert np.abs(n["val"][i] - a).max() < 1e-6 * np.abs(a).max(), (case, np.abs(n["val"][i] - a).max() / np.abs(a).max())


def test_expectation_sees_the_case():
    """the geometry does what each case claims"""
    for case in ("rgb_side", "melanin_tinted_oblique", "blond_backlit"):
        e = expected(case)
        on = e["cls"] == PIX_STRAND
        assert np.abs(e["alt"]["flip_h"][on] / e["val"][on] - 1).max() > 1.0, case       # E(h) != E(-h), by far
    e = expected("light_facing_away")
    on = e["cls"] == PIX_STRAND
    assert (e["alt"]["count_emission"][on] > 1.05 * e["val"][on]).mean() > 0.3             # emission hits would add > 5 % on many pixels
    assert (e["cls"] == PIX_LIGHT).sum() == 0                                            # the camera sees the quad's back
    e = expected("blond_backlit")
    on = e["cls"] == PIX_STRAND
    assert e["val"][on].mean() > 20 * expected("rgb_side")["val"][expected("rgb_side")["cls"] == PIX_STRAND].mean()   # the TT lobe
