"""Radiance against float64 integrals (tests/_analytic.py): what should a pixel converge to?

Every other radiance test compares the HIP renderer with the oracle sample by sample; a misreading the two share (a pdf
missing a cosine, a CDF off by one, emission on the wrong face) passes them all.  Here the expectation of each pixel is
derived independently, in float64, as an integral over the lights that models the reference's quirks (SURVEY §8(a'),
Q1-Q3, Q9, Q10, Q15), and both back ends are held to it statistically.  The same test runs on the oracle (CPU) and on
the HIP renderer (the `gpu` parameter).

Statistics.  K = 64 batches of 16 spp each (64 for the occluder and the grazing view), first_pass = spp * k and a fixed seed_seq, so every run is the same run.  The
image is cut into 8x8-pixel cells; a cell counts when it holds >= 16 pixels whose whole footprint sees the receiver.  Per
cell and channel, the K batch means of those pixels give the mean M and its standard error SE = sd / sqrt(K) (sd with
K - 1 degrees of freedom); z = (M - E) / SE, E = the mean of the pixels' float64 expectations.  The whole-receiver mean is
tested the same way.  The bar: |z| < t, t = Student's t quantile with K - 1 = 63 dof at two-sided 1e-6 / n_tests (Bonferroni
over 3 channels x (cells + 1)), e.g. t = 6.70 for 150 tests -- a correct renderer fails with probability < 1e-6 (the
normal approximation of each batch mean is good: every batch mean averages >= 16 x 16 = 256 samples).
Power, inside the tests: the same statistic against 1.01 E must fail, and in case 1 also against the physically consistent
expectation (w_nee + w_bsdf replaced by 1) -- so the test pins Q3 and is not merely loose.

The closure mix (MIX, GRAZING): receivers that enable several closures at once, so that ParamToBsdf, the selection weights,
EvalBsdf's sum and SampleBsdf's pick -- which kernel and oracle restate from the same reading -- are held to the float64 model of
tests/_analytic.py (closure_set / selection_weights / lobes), itself written from the reference's text and held to the
reference's compiled leaves (test_gtr1_f64_matches_reference_leaf, test_ggx_sampler_density_matches_model).  What these cases
cannot see: selection weights that are wrong in the same way in the pick and in the pdf leave the estimator unbiased and cost
variance only; bit-parity with the oracle covers that.

Exact pixels: a pixel whose whole footprint sees an emitter's front face holds exactly count * Le, one that sees only black
geometry, back faces of emitters or nothing holds exactly 0, and alpha == count == spp everywhere."""
import numpy as np
import pytest

import _analytic as A
import _oracle as O

W, H = 64, 48
K, SPP = 64, 16
# the shadow makes NEE's estimator noisier, and so does a narrow lobe seen at grazing angles: 4x the samples keep 1.01 E rejected
SPP_OF = {"occluder": 64, "grazing": 64}
SEED_SEQ = 2718281828
CELL = 8
MIN_CELL_PIXELS = 16
P_FAIL = 1e-6
LAMBERT = dict(base_color=(0.7, 0.5, 0.3), specular=0.0)

# The principled closure mix (cycles-principled-shader.cc:244-412): receivers that enable more than one closure, so that the
# selection weights (Q7) enter both pdfs; between them they use every parameter of the non-subsurface set
PLASTIC = dict(base_color=(0.7, 0.5, 0.3), specular=0.5, roughness=0.6)
DARK_THREE_LOBES = dict(base_color=(0.1, 0.08, 0.05), specular=1.0, specular_tint=0.5, roughness=0.5, clearcoat=1.0, clearcoat_roughness=0.3)
MIX = {
    "plastic": PLASTIC,
    "tinted_half_metal": dict(base_color=(0.8, 0.4, 0.2), specular=0.8, specular_tint=0.7, metallic=0.5, roughness=0.5, transmission=0.4),
    "clearcoat_diffuse": dict(base_color=(0.3, 0.5, 0.7), specular=0.0, clearcoat=1.0, clearcoat_roughness=0.5),
    "dark_three_lobes": DARK_THREE_LOBES,
    "anisotropic": dict(PLASTIC, anisotropic=0.8, metallic=0.3),
}
GRAZING = dict(base_color=(0.1, 0.08, 0.05), specular=0.5, roughness=0.4)
T_GRAZE = np.radians(72.0)

TH = np.radians(55.0)
N_TILT = np.array([np.sin(TH), 0.0, -np.cos(TH)])            # the tilted light's normal: down and towards +x


def _floor(flip=False, **mat):
    v, f = A.quad((0, 0, 0), (1.0, 0, 0), (0, 0.75, 0))       # z = 0, normal +z
    return A.Mesh("floor", v, f[:, ::-1] if flip else f, A.material(**(mat or LAMBERT)))


def _tilted_light(normals=None):
    """1.0 x 0.5 quad tilted 55 degrees, its low edge 0.095 above the floor: grazing cos_p over most of the floor"""
    v, f = A.quad((-0.35, 0.0, 0.30), (0.0, 0.45, 0.0), (0.25 * np.cos(TH), 0.0, 0.25 * np.sin(TH)))
    n = None if normals is None else np.tile(normals, (4, 1))
    return A.Mesh("light", v, f, A.material(**A.BLACK), emission=np.full((2, 3), 3.0), normals=n)


def _fan(center, radii, z):
    """a fan of unequal triangles around `center` in the plane z, wound to face -z"""
    ang = np.radians([0, 80, 150, 215, 290])
    rim = [(center[0] + r * np.cos(a), center[1] + r * np.sin(a), z) for r, a in zip(radii, ang)]
    v = np.array([(center[0], center[1], z)] + rim)
    f = np.array([[0, 1 + (k + 1) % 5, 1 + k] for k in range(5)])
    return v, f


def scene_of(case):
    if case == "quad_light":
        return A.Scene([_floor(), _tilted_light()])
    if case == "floor_reversed":
        return A.Scene([_floor(flip=True), _tilted_light()])
    if case == "occluder":
        # a black plate parallel to the light, 0.2 in front of it: umbra + penumbra on the floor
        c = np.array([-0.35, 0.0, 0.30]) + 0.2 * N_TILT
        pv, pf = A.quad(c, (0.0, 0.3, 0.0), 0.17 * np.array([np.cos(TH), 0.0, np.sin(TH)]))
        return A.Scene([_floor(), _tilted_light(), A.Mesh("plate", pv, pf, A.material(**A.BLACK))], occluders=[2])
    if case == "two_lights":
        # coplanar (z = 0.35, facing down) so neither shadows the other; different Le and area; the fan's faces are unequal
        # and carry two emissions with different max(Le)
        qv, qf = A.quad((-0.45, 0.25, 0.35), (0.2, 0.0, 0.0), (0.0, -0.15, 0.0))
        fv, ff = _fan((0.35, -0.2), (0.25, 0.12, 0.2, 0.15, 0.22), 0.35)
        fe = np.array([[1.0, 2.5, 0.5], [2.0, 0.6, 1.2]] * 3)[:5]
        return A.Scene([_floor(), A.Mesh("light_a", qv, qf, A.material(**A.BLACK), emission=np.tile([[4.0, 3.0, 2.0]], (2, 1))),
                        A.Mesh("light_b", fv, ff, A.material(**A.BLACK), emission=fe)])
    if case == "tilted_shading_normal":
        n = N_TILT + np.array([0.0, 0.9, 0.0])
        return A.Scene([_floor(), _tilted_light(normals=n / np.linalg.norm(n))])
    if case == "light_facing_away":
        v, f = A.quad((-0.2, 0.1, 0.3), (0.3, 0.0, 0.0), (0.0, 0.2, 0.0))    # normal +z: towards the camera, away from the floor
        return A.Scene([_floor(), A.Mesh("light", v, f, A.material(**A.BLACK), emission=np.full((2, 3), 3.0))])
    if case == "ggx_metallic":
        return A.Scene([_floor(base_color=(0.9, 0.6, 0.3), metallic=1.0, roughness=0.7, specular=0.5, anisotropic=0.0),
                        _tilted_light()])
    if case in MIX:
        return A.Scene([_floor(**MIX[case]), _tilted_light()])
    if case == "grazing":
        # The camera looks down -z at a receiver tilted 72 degrees (view cosines 0.32 .. 0.61) and the emitter sits around the
        # mirror direction of the view: dot(h, wo) gets small, so the Fresnel tint of SpecularColor (and with it `ior`) matters
        c, s_ = np.cos(T_GRAZE), np.sin(T_GRAZE)
        rv, rf = A.quad((0, 0, 0), (c, 0, s_), (0, 0.75, 0))
        n = np.array([-s_, 0.0, c])
        r = 2.0 * n[2] * n - np.array([0.0, 0.0, 1.0])
        ev, ef = A.quad(1.2 * r, (0, 0.4, 0), 0.3 * np.array([r[2], 0.0, -r[0]]))
        ng = np.cross(ev[1] - ev[0], ev[2] - ev[0])
        assert np.allclose(np.cross(rv[1] - rv[0], rv[2] - rv[0]) / (4 * 0.75), n) and np.dot(ng, -r) > 0.999 * np.linalg.norm(ng), \
            "the emitter's geometric normal must point back at the receiver"
        return A.Scene([A.Mesh("slope", rv, rf, A.material(**GRAZING)),
                        A.Mesh("light", ev, ef, A.material(**A.BLACK), emission=np.full((2, 3), 3.0))])
    raise KeyError(case)


CASES = ["quad_light", "floor_reversed", "occluder", "two_lights", "tilted_shading_normal", "light_facing_away", "ggx_metallic",
         "plastic", "tinted_half_metal", "clearcoat_diffuse", "dark_three_lobes", "anisotropic", "grazing"]
# Quadrature per case (test_quadrature_converged holds each to the same 1e-5): the Gauss-Legendre order, and for narrow lobes the
# refinement of the light's triangles by the lobe's width (A.Expectation)
QUAD_OF = {"dark_three_lobes": dict(lobe=3.0), "anisotropic": dict(order=8), "grazing": dict(order=6, lobe=1.0)}
# Mutations of the model itself that a case must reject (like `phys` for case 1): the expectation with p_true := q_rep pins Q15
# and the clearcoat's GTR2 sampler together, the clearcoat without its 0.25 pins Q8
ALT_OF = {"dark_three_lobes": ("honest_pdf", "clearcoat_unscaled"), "anisotropic": ("honest_pdf",)}
MIN_CELLS = 12            # every mix case keeps at least this many cells ...
MAX_MIXED = 1.0 / 3.0     # ... and drops at most this share of the pixels whose footprint lies on the receiver

_expect = {}


def expected(case):
    """(scene, cls, value[, physical value]) per case, computed once per session (both back ends use it)"""
    if case not in _expect:
        S = scene_of(case)
        so = A.build(O.OracleScene(), S, O.make_principled)
        cam = A.Camera(*so.FetchSceneAABB(), W, H)
        ex = A.Expectation(S, alts=ALT_OF.get(case, ()), **QUAD_OF.get(case, {}))
        cls, val, (pts, wo) = A.classify_and_expect(S, cam, ex)
        out = dict(S=S, cam=cam, ex=ex, cls=cls, val=val[..., :3], pts=pts, wo=wo)
        out["alt"] = {name: val[..., 3 * k + 3:3 * k + 6] for k, name in enumerate(ex.alts)}
        if case in MIX or case == "grazing":
            on = A.on_receiver(S, cam)
            out["mixed"] = 1.0 - (cls == A.PIX_RECEIVER).sum() / on.sum()
        if case == "quad_light":
            out["phys"] = A.classify_and_expect(S, cam, A.Expectation(S, physical_mis=True))[1]
        _expect[case] = out
    return _expect[case]


def render_batches(backend, S, pa=None, spp=SPP):
    """K batches of spp passes each: (K,H,W,4) rgba, (K,H,W) count"""
    if backend == "oracle":
        so = A.build(O.OracleScene(), S, O.make_principled)
        th = O.oracle_threads()
        out = [so.render(W, H, spp, first_pass=k * spp, seed_seq=SEED_SEQ, threads=th)[:2] for k in range(K)]
    else:
        sg = A.build(pa.Scene(), S, pa.make_principled)
        out = []
        for k in range(K):
            layer = pa.RenderLayer()
            pa.Render(sg, W, H, spp, layer=layer, first_pass=k * spp, seed_seq=SEED_SEQ)
            out.append((np.array(layer.rgba, np.float32).reshape(H, W, 4), np.array(layer.count, np.uint32).reshape(H, W)))
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def group_stats(means, groups, val, skip_nan=False):
    """z per (group of pixels, channel) and the Bonferroni t bar.  means: (K,H,W,3) batch means, groups: (H,W) bool masks.
    skip_nan: a batch mean leaves out the pixels that are NaN in that batch (the caller bounds and explains their number)."""
    z = []
    for g in groups:
        bm = np.nanmean(means[:, g], 1) if skip_nan else means[:, g].mean(1)                                   # (K,3)
        se = bm.std(0, ddof=1) / np.sqrt(len(means))
        d = bm.mean(0) - val[g].mean(0)
        # a cell no light reaches (every batch mean 0, SE 0) passes only when E is 0 there as well
        z.append(np.where(se > 0, d / np.where(se > 0, se, 1.0), np.where(d == 0, 0.0, np.inf)))
    z = np.array(z)                                                # (groups, 3)
    bar = A.student_t_bar(P_FAIL / z.size, len(means) - 1)
    return z, bar


def cell_groups(cls):
    """the judged groups of pixels: every 8x8 cell's PIX_RECEIVER pixels where there are >= MIN_CELL_PIXELS, then the whole receiver"""
    rec = cls == A.PIX_RECEIVER
    groups = []
    for cy in range(0, H, CELL):
        for cx in range(0, W, CELL):
            m = np.zeros_like(rec)
            m[cy:cy + CELL, cx:cx + CELL] = rec[cy:cy + CELL, cx:cx + CELL]
            if m.sum() >= MIN_CELL_PIXELS:
                groups.append(m)
    groups.append(rec)
    return groups


def cell_stats(means, cls, val):
    """z per (cell, channel) and for the whole receiver, and the Bonferroni t bar.  means: (K,H,W,3) batch means."""
    return group_stats(means, cell_groups(cls), val)


def _pa():
    import pbrlab_amd as pa
    if pa.device_count() < 1:
        pytest.fail("no HIP device: the GPU tests must run on an MI355X (there is no CPU fallback)")
    pa.set_device(0)
    return pa


BACKENDS = ["oracle", pytest.param("gpu", marks=pytest.mark.gpu)]


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("case", CASES)
def test_analytic_radiance(case, backend):
    e = expected(case)
    cls, val = e["cls"], e["val"]
    spp = SPP_OF.get(case, SPP)
    rgba, count = render_batches(backend, e["S"], _pa() if backend == "gpu" else None, spp)
    # exact pixels, batch by batch
    assert (count == spp).all() and (rgba[..., 3] == count).all()
    light, zero = cls == A.PIX_LIGHT, cls == A.PIX_ZERO
    want = count[..., None].astype(np.float32) * val.astype(np.float32)[None]
    assert (rgba[:, light, :3] == want[:, light]).all(), "a pixel on an emitter's front face is not exactly count * Le"
    assert (rgba[:, zero, :3] == 0).all(), "a pixel on black geometry / an emitter's back / nothing is not exactly 0"
    assert zero.sum() > 0
    if case == "light_facing_away":
        assert light.sum() > 100
        rec = cls == A.PIX_RECEIVER
        assert rec.sum() > 500 and (rgba[:, rec, :3] == 0).all(), "light reaches the floor from an emitter facing away"
        return
    means = rgba[..., :3] / count[..., None]
    z, bar = cell_stats(means, cls, val)
    floor_rel = means.mean(0)[cls == A.PIX_RECEIVER].mean(0) / val[cls == A.PIX_RECEIVER].mean(0) - 1
    print(f"{case} [{backend}]: {len(z) - 1} cells, max |z| {np.abs(z).max():.2f} (bar {bar:.2f}), whole-receiver rel err "
          f"{' '.join(f'{r:+.1e}' for r in floor_rel)}")
    assert np.abs(z).max() < bar, (z, bar)
    # power: 1 % more light must be caught
    z1, _ = cell_stats(means, cls, val * 1.01)
    assert np.abs(z1).max() >= bar, ("1.01 E is not rejected", np.abs(z1).max(), bar)
    print(f"{case} [{backend}]: max |z| against 1.01 E {np.abs(z1).max():.2f}")
    if case == "quad_light":
        zp, _ = cell_stats(means, cls, e["phys"])
        assert np.abs(zp).max() >= bar, ("MIS weights summing to 1 are not rejected: Q3 is not pinned", np.abs(zp).max(), bar)
    if "mixed" in e:
        assert len(z) - 1 >= MIN_CELLS and e["mixed"] <= MAX_MIXED, (len(z) - 1, e["mixed"])
    for name, alt in e["alt"].items():
        za, _ = cell_stats(means, cls, alt)
        print(f"{case} [{backend}]: max |z| against {name}: {np.abs(za).max():.2f}")
        assert np.abs(za).max() >= bar, (f"{name} is not rejected", np.abs(za).max(), bar)


def test_quadrature_converged(cases=CASES, expected=expected):
    """doubling the Gauss-Legendre order changes E by < 1e-5 relative, on every case's receiver points (a sample of 400)
    (tests/test_texture_radiance.py runs it on its own cases)"""
    for case in cases:
        e = expected(case)
        rng = np.random.RandomState(3)
        i = rng.choice(len(e["pts"]), min(400, len(e["pts"])), replace=False)
        a = e["ex"](e["pts"][i], e["wo"][i])
        b = e["ex"](e["pts"][i], e["wo"][i], order=2 * e["ex"].order)
        scale = np.abs(b).max()
        if scale == 0:
            assert case == "light_facing_away"
            continue
        assert np.abs(a - b).max() < 1e-5 * scale, (case, np.abs(a - b).max() / scale)


class _ClosedForms(A.Expectation):
    """The two closed forms Expectation held before it modelled the closure set, inline: a Lambert receiver (f = rho / pi, q =
    cos / pi, the BSDF path carries f cos) and a metallic isotropic GGX one (f = F G1o G1i D / (4 cos_o cos_i), q = G1o D /
    (4 cos_o cos_i), the BSDF path carries f cos^2: Q15)."""

    def _lobes(self, wi, wo):
        m = self.S.meshes[self.S.receiver].material
        base = np.asarray(m["base_color"], np.float64)
        ci, co = wi[..., 2], wo[..., 2]
        if m["metallic"] == 0.0:
            assert m["specular"] == 0.0
            q = ci / np.pi
            return (base / np.pi) * np.ones(ci.shape + (1,)), q, q, 0.0
        assert m["metallic"] == 1.0 and m["anisotropic"] == 0.0
        a2 = float(m["roughness"]) ** 4
        h = wi + wo
        h = h / np.linalg.norm(h, axis=-1, keepdims=True)
        c2 = h[..., 2] ** 2
        D = a2 / (np.pi * c2 * c2 * (a2 + (1 - c2) / c2) ** 2)
        g1 = lambda c: 2 / (1 + np.sqrt(1 + a2 * (1 - c * c) / (c * c)))  # noqa: E731
        ior = 2.0 / (1.0 - np.sqrt(0.08 * float(m["specular"]))) - 1.0
        f0 = A.fresnel_dielectric_cos(1.0, ior)
        fh = (A.fresnel_dielectric_cos(np.sum(h * wo, -1), ior) - f0) / (1.0 - f0)
        q = g1(co) * D / (4 * co * ci)
        return (base * (1 - fh[..., None]) + fh[..., None]) * (g1(ci) * q)[..., None], q, q * ci, 0.0


def test_closure_set_model_keeps_the_closed_forms():
    """the closure-set model reduces to the closed forms it replaced: on the seven single-closure cases E moves by < 1e-12
    relative (300 receiver points each; Lambert is the special case p_true / q_rep = 1, metallic GGX the case cos_i)"""
    for case in CASES[:7]:
        e = expected(case)
        i = np.random.RandomState(5).choice(len(e["pts"]), min(300, len(e["pts"])), replace=False)
        a = e["ex"](e["pts"][i], e["wo"][i])
        b = _ClosedForms(e["S"])(e["pts"][i], e["wo"][i])
        assert a.shape == b.shape and np.abs(a - b).max() <= 1e-12 * np.abs(b).max(), (case, np.abs(a - b).max(), np.abs(b).max())
        assert case == "light_facing_away" or np.abs(b).max() > 0


def test_untextured_expectations_are_unchanged():
    """Expectation resolves the receiver's base colour per point for textured receivers (tests/_texture_model.py); for the thirteen
    untextured cases it returns, bit for bit, the float64 values it returned before it could: E and every alternative on 300 receiver
    points per case, recorded by tests/golden/make_analytic_golden.py at the commit before"""
    import os
    gold = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "analytic_expectations.npz"))
    for case in CASES:
        e = expected(case)
        i = np.random.RandomState(5).choice(len(e["pts"]), min(300, len(e["pts"])), replace=False)
        assert np.array_equal(e["pts"][i], gold[case + "/pts"]) and np.array_equal(e["wo"][i], gold[case + "/wo"]), case
        got = e["ex"](gold[case + "/pts"], gold[case + "/wo"])
        assert got.dtype == np.float64 and got.shape == gold[case + "/E"].shape and got.tobytes() == gold[case + "/E"].tobytes(), \
            (case, np.abs(got - gold[case + "/E"]).max())
    assert len(CASES) == 13


def test_student_t_bar():
    """the t quantiles the bar uses, against tabulated values: (two-sided p, dof) -> x"""
    for p, dof, x in ((0.05, 63, 1.998341), (0.01, 10, 3.169273), (0.05, 1, 12.706205), (1e-6, 63, 5.420030), (1e-6 / 150, 63, 6.699101)):
        assert abs(A.student_t_bar(p, dof) - x) < 1e-6 * x, (p, dof, A.student_t_bar(p, dof), x)
    assert abs(A.student_t_two_sided(1.998341, 63) - 0.05) < 1e-6


def test_pixel_rule_converged():
    """the footprint rule (2 x 2 Gauss-Legendre; steep pixels left out) agrees with 8 x 8 to < 1e-4 of the brightest pixel
    (30x below the smallest per-cell standard error)
    (the 100 steepest and 100 random receiver pixels of case 1)"""
    e = expected("quad_light")
    ys, xs = np.nonzero(e["cls"] == A.PIX_RECEIVER)
    v = e["val"][ys, xs, 0]
    gy, gx = np.gradient(e["val"][..., 0])
    steep = np.argsort(-np.hypot(gx, gy)[ys, xs])[:100]
    i = np.concatenate([steep, np.random.RandomState(4).choice(len(ys), 100, replace=False)])
    fine = A.pixel_mean(e["S"], e["cam"], e["ex"], xs[i], ys[i], 8)
    err = np.abs(fine - e["val"][ys[i], xs[i]]).max()
    assert err < 1e-4 * v.max(), err / v.max()


def test_expectation_sees_the_case():
    """the geometry does what each case claims: Q3's weight sum departs from 1, the occluder casts umbra and penumbra,
    the tilted shading normal switches kFront off over part of the light, two lights each light the floor"""
    e = expected("quad_light")
    rec = e["cls"] == A.PIX_RECEIVER
    rec &= e["phys"][..., 0] > 0
    ratio = e["val"][rec][:, 0] / e["phys"][rec][:, 0]
    assert ratio.max() - ratio.min() > 0.05, (ratio.min(), ratio.max())
    # occluder: some receiver points fully in umbra (E == 0 where the open light gives E > 0), many partly shadowed
    o, q = expected("occluder"), expected("quad_light")
    pts, wo = q["pts"][::3], q["wo"][::3]
    vo, vq = o["ex"](pts, wo)[:, 0], q["ex"](pts, wo)[:, 0]
    lit = vq > 0
    r = vo[lit] / vq[lit]
    assert (r == 0).sum() > 0 and ((r > 0.05) & (r < 0.95)).sum() > 100 and (r == 1).sum() > 100, ((r == 0).sum(), ((r > 0.05) & (r < 0.95)).sum(), (r == 1).sum())
    # tilted n_s: some visible light pieces are not kFront from some receiver points
    t = expected("tilted_shading_normal")
    ex = t["ex"]
    n_back = sum(1 for x in t["pts"][::97] for fc in ex.faces for _, fr in ex._pieces(x, np.array([0, 0, 1.0]), fc) if not fr)
    assert n_back > 0
    tl = expected("two_lights")
    assert len(tl["ex"].faces) == 7 and len({round(f["pA"], 9) for f in tl["ex"].faces}) >= 3


def test_ggx_f64_matches_reference_leaf():
    """the float64 GGX eval reproduces the reference's leaf outputs (ggx2/eval: f and pdf) before it is trusted as an
    integrand: where the float32 inputs are well conditioned (alpha >= 0.05 and both cosines >= 0.05: 144 of the 1500
    inputs) the relative difference is < 5e-5 everywhere and < 1e-5 for 95 % of them (measured: 4.6e-5 and 6e-7)"""
    from test_oracle_vs_reference_leaf import _in_ggx
    from test_oracle_vs_reference_leaf import _ref_ggx
    want = O.ref_outputs("ggx2", lambda R: _ref_ggx(R, 2))["eval"]
    wo, wi, alphas, _ = _in_ggx(2)
    f, pdf = A.ggx_eval(wi.astype(np.float64), wo.astype(np.float64), alphas[:, 0].astype(np.float64), alphas[:, 1].astype(np.float64))
    ok = (alphas.min(1) >= 0.05) & (wo[:, 2] >= 0.05) & (wi[:, 2] >= 0.05)
    assert ok.sum() > 100
    for k, got in enumerate((f, pdf)):
        rel = np.abs(got[ok] / want[ok, k] - 1)
        assert rel.max() < 5e-5 and np.quantile(rel, 0.95) < 1e-5, (k, rel.max(), np.quantile(rel, 0.95))
    below = (wi[:, 2] <= 0) | (wo[:, 2] <= 0)
    assert below.any() and (f[below] == 0).all() and (want[below, 0] == 0).all()


def test_gtr1_f64_matches_reference_leaf():
    """the float64 clearcoat eval (distrib = 1: GTR1 D, alpha^2 = 0.0625 inside G, the extra 0.25; the anisotropic GTR2 branch
    where alpha_x != alpha_y) reproduces the reference's leaf outputs (ggx1/eval: f and pdf), on test_ggx_f64_matches_reference_leaf's
    conditioning filter and with its bars"""
    from test_oracle_vs_reference_leaf import _in_ggx
    from test_oracle_vs_reference_leaf import _ref_ggx
    want = O.ref_outputs("ggx1", lambda R: _ref_ggx(R, 1))["eval"]
    wo, wi, alphas, _ = _in_ggx(1)
    f, pdf = A.ggx_eval(wi.astype(np.float64), wo.astype(np.float64), alphas[:, 0].astype(np.float64), alphas[:, 1].astype(np.float64), 1)
    ok = (alphas.min(1) >= 0.05) & (wo[:, 2] >= 0.05) & (wi[:, 2] >= 0.05)
    iso = alphas[:, 0] == alphas[:, 1]
    assert ok.sum() > 100 and (ok & iso).sum() > 30 and (ok & ~iso).sum() > 30 and (ok & iso & (alphas[:, 0] < 1)).sum() > 20
    for k, got in enumerate((f, pdf)):
        rel = np.abs(got[ok] / want[ok, k] - 1)
        print(f"ggx1 eval[{k}]: max rel {rel.max():.1e}, 95 % {np.quantile(rel, 0.95):.1e}")
        assert rel.max() < 5e-5 and np.quantile(rel, 0.95) < 1e-5, (k, rel.max(), np.quantile(rel, 0.95))
    below = (wi[:, 2] <= 0) | (wo[:, 2] <= 0)
    assert below.any() and (f[below] == 0).all() and (want[below, 0] == 0).all()


SAMPLER_BAR = 0.005      # half of the 1 % the radiance tests detect


def test_ggx_sampler_density_matches_model():
    """p_true, the density the expectations assume for MicrofacetGGXSample (A.ggx_vndf_pdf: the GTR2 density of visible normals
    mirrored, for distrib = 1 as well), explains where the reference's own sampler puts wi: a jittered 1024 x 1024 grid of
    (u0, u1) per setting (isotropic 0.25, anisotropic (0.6, 0.15), clearcoat 0.09 with distrib = 1) and wo (cos_o 0.9 and 0.45),
    wi binned on 16 (cos theta) x 32 (phi) bins, against the float64 integral of p_true over each bin (32 x 32 Gauss-Legendre).
    Bins expecting >= 1e4 samples are judged: |count / expected - 1| < 0.5 % (half of what the radiance tests detect), or the
    bin's own counting noise where that is larger (normal quantile at 1e-6 / bins, binomial sd: an upper bound, the grid is
    stratified).  The share of draws that land below the surface is held to the model's as well.  The slope sampler's slope_y
    is a rational fit (microfacet-ggx.h:113-117), so exact agreement is not expected.
    The same bins merged 4 x 4 (those expecting >= 1e5 samples) are held to the flat 0.5 %: there the counting noise is below it.
    Measured: over the 127 judged bins max |rel| 0.88 % (a bin expecting 1.0e4 draws: 0.9 of its Poisson sd; no judged bin
    departs by more than 1.02 Poisson sd, rms 0.14 .. 0.47), over the 14 merged bins 0.17 %; below the surface the model is
    within 0.5 % for alpha >= 0.15 and 5 % high (430 of 1e6 draws) for the clearcoat's 0.09.  So nothing here raises the
    factor the radiance cases must detect above 1.01."""
    from statistics import NormalDist
    import test_oracle_vs_reference_leaf as T
    got = O.ref_outputs("ggx_sample_hist", T._ref_ggx_hist, needs=("ref_ggx_sample_n",))
    n_total = T.GGX_HIST_N ** 2
    nc, nph = T.GGX_HIST_BINS
    g, gw = A.gauss_legendre01(32)
    ce, pe = np.linspace(0.0, 1.0, nc + 1), np.linspace(-np.pi, np.pi, nph + 1)
    mu = (ce[:-1, None] + g[None] * np.diff(ce)[:, None])                     # (nc, 32)
    ph = (pe[:-1, None] + g[None] * np.diff(pe)[:, None])                     # (nph, 32)
    wq = (gw * np.diff(ce)[:, None])[:, None, :, None] * (gw * np.diff(pe)[:, None])[None, :, None, :]
    M, PH = mu[:, None, :, None], ph[None, :, None, :]
    st = np.sqrt(1.0 - M * M)
    wi = np.stack(np.broadcast_arrays(st * np.cos(PH), st * np.sin(PH), M), -1)   # (nc, nph, 32, 32, 3)
    worst = 0.0
    case = 0
    for ax, ay, distrib in T.GGX_HIST_SETTINGS:
        for k in range(len(T.GGX_HIST_WO)):
            wo = T._ggx_hist_wo(k).astype(np.float64)
            wo /= np.linalg.norm(wo)
            expect = (A.ggx_vndf_pdf(wi, wo, ax, ay) * wq).sum((2, 3)) * n_total
            counts = got["counts"][case]
            judged = expect >= 1e4
            zq = NormalDist().inv_cdf(1.0 - 0.5 * P_FAIL / judged.sum())
            rel = counts[judged] / expect[judged] - 1.0
            noise = zq * np.sqrt((1.0 - expect[judged] / n_total) / expect[judged])
            # the rest of the unit mass lies below the surface (or, a hair of it, in wi.z + wo.z <= 0 where the density is 0)
            below_model = n_total - expect.sum()
            print(f"ggx sampler alpha ({ax}, {ay}) distrib {distrib} cos_o {T.GGX_HIST_WO[k][0]}: {judged.sum()} judged bins hold "
                  f"{counts[judged].sum() / n_total:.3f} of the draws, max |rel| {np.abs(rel).max():.2e} (noise bar there "
                  f"{noise[np.argmax(np.abs(rel))]:.2e}), below the surface {got['below'][case]} (model {below_model:.0f})")
            assert judged.sum() >= 8
            assert (np.abs(rel) < np.maximum(SAMPLER_BAR, noise)).all(), (ax, ay, distrib, k, np.abs(rel).max())
            em, cm = expect.reshape(nc // 4, 4, nph // 4, 4).sum((1, 3)), counts.reshape(nc // 4, 4, nph // 4, 4).sum((1, 3))
            big = em >= 1e5
            assert big.any() and (np.abs(cm[big] / em[big] - 1.0) < SAMPLER_BAR).all(), (ax, ay, distrib, k, cm[big] / em[big] - 1.0)
            assert abs(got["below"][case] - below_model) < max(SAMPLER_BAR * below_model, zq * np.sqrt(max(below_model, 1.0)) + 1.0)
            assert counts.sum() + got["below"][case] == n_total
            worst = max(worst, np.abs(rel).max())
            case += 1
    print(f"ggx sampler: max |rel| over all judged bins {worst:.2e}")
