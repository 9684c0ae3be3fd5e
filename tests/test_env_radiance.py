"""The environment light's radiance against float64 expectations (tests/_env_analytic.py), on both back ends:
every case runs on the HIP renderer under its own name (marked gpu) and on the oracle, which restates §10 (oracle/pbr_oracle.c),
on the CPU (test_env_case_on_the_oracle[case]).

A Lambert floor with nothing above it, lit by a lat-long map only (furnace, rotated sun map), with a black occluder, with an area
light as well; a white Lambert box open to a constant sky, whose paths bounce many times (k_tail's environment instances); a metallic
GGX floor under a constant sky (the skewed GGX pdf of Q15 on the BSDF side).  Same statistics as test_analytic_radiance.py: K seeded
batches, per 8x8 cell and channel a Student-t bar with Bonferroni correction (a correct renderer fails with probability < 1e-6), plus
the whole receiver; 1.01 E must be rejected, and each case's plausible mistake as well.  Background pixels whose footprint lies
inside one texel are exact: count x L x scale."""
import numpy as np
import pytest

import _analytic as A
import _env_analytic as EA
import _oracle as O
from test_analytic_radiance import CELL, MIN_CELL_PIXELS, P_FAIL, _pa

W, H = 64, 48
K, SPP = 48, 16
SEED_SEQ = 1414213562


def _render(backend, S, env, scale, m):
    """K batches of SPP passes: (K,H,W,4) rgba, (K,H,W) count, the camera and the closest-hit rays per sample (oracle; None on the GPU)"""
    if backend == "oracle":
        so = A.build(O.OracleScene(), S, O.make_principled)
        so.SetEnvironment(env, scale, m)
        th = O.oracle_threads()
        out = [so.render(W, H, SPP, first_pass=k * SPP, seed_seq=SEED_SEQ, threads=th) for k in range(K)]
        rays = sum(o[2]["closest_rays"] for o in out) / sum(o[2]["samples"] for o in out)
        return np.stack([o[0] for o in out]), np.stack([o[1] for o in out]), A.Camera(*so.FetchSceneAABB(), W, H), rays
    pa = _pa()
    sg = A.build(pa.Scene(), S, pa.make_principled)
    sg.SetEnvironment(env, scale, m)
    rgba, count = [], []
    for k in range(K):
        layer = pa.RenderLayer()
        pa.Render(sg, W, H, SPP, layer=layer, first_pass=k * SPP, seed_seq=SEED_SEQ)
        rgba.append(np.array(layer.rgba, np.float32).reshape(H, W, 4))
        count.append(np.array(layer.count, np.uint32).reshape(H, W))
    cam = A.Camera(*sg.FetchSceneAABB(), W, H)
    sg.close()
    return np.stack(rgba), np.stack(count), cam, None


def _receiver(S, cam, probe=6):
    py, px = np.mgrid[0:H, 0:W]
    js = np.linspace(-0.02, 1.02, probe)
    jx, jy = np.meshgrid(js, js, indexing="ij")
    d = cam.dirs(px[..., None].astype(np.float64), py[..., None].astype(np.float64), jx.ravel(), jy.ravel()).reshape(-1, 3)
    mesh = A.cast(S, cam.org, d)[0].reshape(H, W, -1)
    return np.all(mesh == S.receiver, -1)


def _z(means, rec, E):
    groups = []
    for cy in range(0, H, CELL):
        for cx in range(0, W, CELL):
            g = np.zeros_like(rec)
            g[cy:cy + CELL, cx:cx + CELL] = rec[cy:cy + CELL, cx:cx + CELL]
            if g.sum() >= MIN_CELL_PIXELS:
                groups.append(g)
    groups.append(rec)
    z = []
    for g in groups:
        bm = means[:, g].mean(1)
        se = bm.std(0, ddof=1) / np.sqrt(K)
        z.append((bm.mean(0) - E) / se)
    z = np.array(z)
    return z, A.student_t_bar(P_FAIL / z.size, K - 1)


def _check(case, means, rec, E, also_reject=()):
    z, bar = _z(means, rec, E)
    rel = means.mean(0)[rec].mean(0) / E - 1
    print(f"env {case}: {len(z) - 1} cells, max |z| {np.abs(z).max():.2f} (bar {bar:.2f}), whole-floor rel err "
          f"{' '.join(f'{r:+.1e}' for r in rel)}")
    assert np.abs(z).max() < bar, (case, z, bar)
    for name, alt in (("1.01 E", 1.01 * E),) + tuple(also_reject):
        za, _ = _z(means, rec, alt)
        assert np.abs(za).max() >= bar, (case, f"{name} is not rejected", np.abs(za).max(), bar)


def _case_furnace_constant_sky(backend):
    """A Lambert floor under a constant sky converges to rho L (the environment's two MIS weights sum to 1); the skewed NEE
    weight of Q3 is rejected; the background is exactly count x L x scale"""
    S = EA.floor_scene()
    L = np.array([0.75, 1.25, 0.5])
    scale = 2.0
    env = np.tile(L.astype(np.float32), (4, 8, 1))
    rgba, count, cam, _ = _render(backend, S, env, scale, None)
    assert (count == SPP).all() and (rgba[..., 3] == count).all()
    rec = _receiver(S, cam)
    assert rec.sum() > 1000
    bg_r, _ = EA.background_texels(S, cam, np.eye(3), 8, 4)
    bg = bg_r >= 0
    assert bg.sum() > 100
    assert (rgba[:, bg, :3] == (SPP * L * scale).astype(np.float32)).all(), "a background pixel is not count x L x scale"
    means = rgba[..., :3] / count[..., None]
    E = EA.constant_expectation(L * scale)
    _check("furnace", means, rec, E, (("Q3-skewed NEE weight", EA.skewed_constant_expectation(L * scale)),))


def _case_hdr_map_rotated_sun(backend):
    """A 32 x 16 sky with one bright sun texel, rotated so that env-up is the floor's normal: the horizon is a row boundary
    and E = (rho / pi) sum_t L_t (phi1 - phi0)(sin^2 theta1 - sin^2 theta0) / 2; background pixels inside one texel are exact"""
    S = EA.floor_scene()
    rgb = EA.sky_map()
    scale = 0.5
    rgba, count, cam, _ = _render(backend, S, rgb, scale, EA.Z_UP)
    assert (count == SPP).all() and (rgba[..., 3] == count).all()
    rec = _receiver(S, cam)
    r, c = EA.background_texels(S, cam, EA.Z_UP, rgb.shape[1], rgb.shape[0])
    bg = r >= 0
    assert bg.sum() > 100
    one = rgb[r[bg], c[bg]] * np.float32(scale)
    want = np.zeros_like(one)
    for _ in range(SPP):  # (the passes are added one by one, in float32)
        want = want + one
    assert (rgba[:, bg, :3] == want[None]).all(), "a background pixel inside one texel is not count x L x scale"
    means = rgba[..., :3] / count[..., None]
    E = EA.map_expectation(rgb, scale)
    # the sun alone is most of E: a sampler that ignored it (uniform over the sky) would be far noisier than the bar allows
    sun_only = EA.map_expectation(np.where(np.arange(16)[:, None, None] == 3, rgb * (np.arange(32)[None, :, None] == 21), 0), scale)
    assert sun_only[0] > 0.5 * E[0]
    _check("hdr_map", means, rec, E)


def _per_pixel(S, cam, expectation, rec):
    """E averaged over each receiver pixel's footprint (2 x 2 Gauss-Legendre, as test_analytic_radiance.py); pixels where E is steep on
    the scale of a pixel are left out"""
    ys, xs = np.nonzero(rec)
    e, ev, _, _ = A.pixel_mean(S, cam, expectation, xs, ys, 2, nodes=True)
    steep = (ev.max(1) - ev.min(1)).max(1) > A.STEEP * np.abs(e).max(1)
    val = np.zeros((H, W, 3))
    val[ys, xs] = e
    keep = rec.copy()
    keep[ys[steep], xs[steep]] = False
    return val, keep


def _zv(means, rec, val):
    """_z with a per-pixel expectation: the cells' means of E"""
    groups = []
    for cy in range(0, H, CELL):
        for cx in range(0, W, CELL):
            g = np.zeros_like(rec)
            g[cy:cy + CELL, cx:cx + CELL] = rec[cy:cy + CELL, cx:cx + CELL]
            if g.sum() >= MIN_CELL_PIXELS:
                groups.append(g)
    groups.append(rec)
    z = []
    for g in groups:
        bm = means[:, g].mean(1)
        se = bm.std(0, ddof=1) / np.sqrt(K)
        z.append((bm.mean(0) - val[g].mean(0)) / se)
    z = np.array(z)
    return z, A.student_t_bar(P_FAIL / z.size, K - 1)


def _check_v(case, means, rec, val, also_reject=()):
    z, bar = _zv(means, rec, val)
    rel = means.mean(0)[rec].mean(0) / val[rec].mean(0) - 1
    print(f"env {case}: {len(z) - 1} cells, max |z| {np.abs(z).max():.2f} (bar {bar:.2f}), whole-floor rel err "
          f"{' '.join(f'{r:+.1e}' for r in rel)}")
    assert np.abs(z).max() < bar, (case, z, bar)
    for name, alt in (("1.01 E", 1.01 * val),) + tuple(also_reject):
        za, _ = _zv(means, rec, alt)
        assert np.abs(za).max() >= bar, (case, f"{name} is not rejected", np.abs(za).max(), bar)


def _case_occluder_form_factor(backend):
    """A constant sky, the floor and a black plate above it: E(x) = rho L (1 - F(x)), F = the point-to-polygon form factor of the
    plate (Lambert's formula).  Pins the environment's shadow rays: an occluded NEE sample adds nothing, an escaped BSDF ray does."""
    S0 = EA.floor_scene()
    pv, pf = A.quad((0.1, -0.05, 0.3), (0.25, 0.0, 0.0), (0.0, 0.18, 0.0))
    S = A.Scene([S0.meshes[0], A.Mesh("plate", pv, pf, A.material(**A.BLACK)), S0.meshes[1]])
    L = np.array([0.75, 1.25, 0.5])
    env = np.tile(L.astype(np.float32), (4, 8, 1))
    rgba, count, cam, _ = _render(backend, S, env, 1.0, None)
    assert (count == SPP).all() and (rgba[..., 3] == count).all()
    rec = _receiver(S, cam)
    val, keep = _per_pixel(S, cam, EA.SkyExpectation(L, [pv]), rec)
    assert keep.sum() > 1000 and val[keep, 0].min() < 0.85 * val[keep, 0].max()  # (the plate hides up to a fifth of the sky)
    means = rgba[..., :3] / count[..., None]
    _check_v("occluder", means, keep, val)


def _case_area_light_and_sky(backend):
    """test_analytic_radiance's tilted quad light plus a constant sky: NEE picks the sky with p_env = 1/2, so the light's pdf carries
    1 - p_env on the NEE and on the emission-hit side.  E = _analytic.Expectation with every face's pA x 1/2 (Q3's skew kept for the
    area part) + rho L_env (1 - F_light(x)).  The expectation without the 1/2 must be rejected."""
    from test_analytic_radiance import _tilted_light
    S0 = EA.floor_scene()
    light = _tilted_light()
    S = A.Scene([S0.meshes[0], light, S0.meshes[1]])
    L = np.array([0.2, 0.25, 0.15])
    env = np.tile(L.astype(np.float32), (4, 8, 1))
    rgba, count, cam, _ = _render(backend, S, env, 1.0, None)
    assert (count == SPP).all() and (rgba[..., 3] == count).all()
    rec = _receiver(S, cam)
    half = A.Expectation(S)
    for fc in half.faces:
        fc["pA"] = fc["pA"] * 0.5
    val, keep = _per_pixel(S, cam, EA.SkyExpectation(L, [light.verts], half), rec)
    alt, _ = _per_pixel(S, cam, EA.SkyExpectation(L, [light.verts], A.Expectation(S)), rec)
    assert keep.sum() > 800
    means = rgba[..., :3] / count[..., None]
    _check_v("area_light_and_sky", means, keep, val, (("pA without 1 - p_env", alt),))


def _case_white_furnace_deep_box(backend):
    """A white Lambert box (albedo 1, no specular) three times as deep as it is wide, open to a constant sky and nothing else: a
    furnace, every pixel converges to L x scale at any depth.  Paths bounce many times before they escape (Q1: the roulette never
    ends a throughput of 1), so every bounce's NEE, its escaped BSDF rays and their MIS weights are summed over long paths -- on the
    GPU through k_tail's environment instances.  0.99 L must be rejected; sky pixels are exact."""
    S = EA.deep_box_scene()
    L = np.array([0.75, 1.25, 0.5])
    scale = 2.0
    env = np.tile(L.astype(np.float32), (4, 8, 1))
    rgba, count, cam, rays = _render(backend, S, env, scale, None)
    assert (count == SPP).all() and (rgba[..., 3] == count).all()
    sky = EA.sky_pixels(S, cam)
    assert sky.sum() > 500
    assert (rgba[:, sky, :3] == (SPP * L * scale).astype(np.float32)).all(), "a sky pixel is not count x L x scale"
    box = _receiver(S, cam)
    assert box.sum() > 2000
    if rays is not None:
        print(f"deep box [{backend}]: {rays:.2f} closest-hit rays per sample")
        assert rays > 8, rays
    means = rgba[..., :3] / count[..., None]
    E = L * scale
    _check(f"deep_box [{backend}]", means, box, E, (("0.99 L", 0.99 * E),))


def _case_ggx_metallic_constant_sky(backend):
    """test_analytic_radiance's metallic GGX receiver under a constant sky, no area light (p_env = 1).  Q15 stays in the BSDF branch:
    the environment's NEE integrates f L cos_i w_env, the BSDF side f L cos_i^2 w_bsdf, both weights on the skewed pdf
    (EA.GGXSkyExpectation, hemisphere quadrature per pixel footprint).  1.01 E and the Q15-free expectation int f L cos_i must be
    rejected."""
    S = EA.ggx_floor_scene()
    L = np.array([0.6, 0.9, 1.2])
    env = np.tile(L.astype(np.float32), (4, 8, 1))
    rgba, count, cam, _ = _render(backend, S, env, 1.0, None)
    assert (count == SPP).all() and (rgba[..., 3] == count).all()
    sky = EA.sky_pixels(S, cam)
    want = np.zeros(3, np.float32)
    for _ in range(SPP):  # (the passes are added one by one, in float32)
        want = want + L.astype(np.float32)
    assert sky.sum() > 100 and (rgba[:, sky, :3] == want).all(), "a sky pixel is not count x L"
    rec = _receiver(S, cam)
    val, keep = _per_pixel(S, cam, EA.GGXSkyExpectation(S, L), rec)
    free, _ = _per_pixel(S, cam, EA.GGXSkyExpectation(S, L, q15=False), rec)
    assert keep.sum() > 1000
    means = rgba[..., :3] / count[..., None]
    _check_v(f"ggx_sky [{backend}]", means, keep, val, (("Q15-free", free),))


def _mix_constant_sky(backend, name):
    """A receiver of test_analytic_radiance's closure mix (MIX[name]) as the floor under a constant sky, no area light: k_shade_principled<4>
    with solid-angle pdfs on both MIS sides.  E = int f L (cos_i w_env + cos_i (p_true / q_rep) w_bsdf) dw with the selection weights
    (Q7) inside both pdfs, plus what the GGX samplers send below the floor (EA.GGXSkyExpectation).  1.01 E and the expectation
    with p_true := q_rep (int f L cos_i) must be rejected; the three-lobe floor, where the rays below the floor take more than 1 %
    of E away, must reject the expectation without them as well."""
    from test_analytic_radiance import MIX
    S = EA.ggx_floor_scene(MIX[name])
    L = np.array([0.6, 0.9, 1.2])
    env = np.tile(L.astype(np.float32), (4, 8, 1))
    rgba, count, cam, _ = _render(backend, S, env, 1.0, None)
    assert (count == SPP).all() and (rgba[..., 3] == count).all()
    sky = EA.sky_pixels(S, cam)
    want = np.zeros(3, np.float32)
    for _ in range(SPP):  # (the passes are added one by one, in float32)
        want = want + L.astype(np.float32)
    assert sky.sum() > 100 and (rgba[:, sky, :3] == want).all(), "a sky pixel is not count x L"
    rec = _receiver(S, cam)
    val, keep = _per_pixel(S, cam, EA.GGXSkyExpectation(S, L), rec)
    free, _ = _per_pixel(S, cam, EA.GGXSkyExpectation(S, L, q15=False), rec)
    assert keep.sum() > 1000
    means = rgba[..., :3] / count[..., None]
    reject = (("p_true := q_rep", free),)
    if name == "dark_three_lobes":
        above = _per_pixel(S, cam, EA.GGXSkyExpectation(S, L, below=False), rec)[0]
        assert (above[keep, 0] > 1.01 * val[keep, 0]).all()      # (red: the channel the tinted lobe weighs most)
        reject += (("nothing below the floor", above),)
    _check_v(f"{name}_sky [{backend}]", means, keep, val, reject)


def _case_plastic_constant_sky(backend):
    """diffuse + specular at specular = 0.5 (the material nearly every scene uses) under a constant sky: _mix_constant_sky"""
    _mix_constant_sky(backend, "plastic")


def _case_dark_three_lobes_constant_sky(backend):
    """a dark base under a tinted specular lobe and a clearcoat (all three closures, the clearcoat's GTR2 sampler): _mix_constant_sky"""
    _mix_constant_sky(backend, "dark_three_lobes")


# Every case on both back ends: the GPU under the case's own name (marked gpu), the oracle's restatement of §10 on the CPU.
ORACLE_CASES = {n: globals()["_case_" + n] for n in (
    "furnace_constant_sky", "hdr_map_rotated_sun", "occluder_form_factor", "area_light_and_sky", "white_furnace_deep_box",
    "ggx_metallic_constant_sky", "plastic_constant_sky", "dark_three_lobes_constant_sky")}


@pytest.mark.parametrize("case", list(ORACLE_CASES))
def test_env_case_on_the_oracle(case):
    ORACLE_CASES[case]("oracle")


@pytest.mark.gpu
def test_env_furnace_constant_sky():
    _case_furnace_constant_sky("gpu")


@pytest.mark.gpu
def test_env_hdr_map_rotated_sun():
    _case_hdr_map_rotated_sun("gpu")


@pytest.mark.gpu
def test_env_occluder_form_factor():
    _case_occluder_form_factor("gpu")


@pytest.mark.gpu
def test_env_area_light_and_sky():
    _case_area_light_and_sky("gpu")


@pytest.mark.gpu
def test_env_white_furnace_deep_box():
    _case_white_furnace_deep_box("gpu")


@pytest.mark.gpu
def test_env_ggx_metallic_constant_sky():
    _case_ggx_metallic_constant_sky("gpu")


@pytest.mark.gpu
def test_env_plastic_constant_sky():
    _case_plastic_constant_sky("gpu")


@pytest.mark.gpu
def test_env_dark_three_lobes_constant_sky():
    _case_dark_three_lobes_constant_sky("gpu")


def test_ggx_sky_quadrature_converged():
    """doubling both orders of GGXSkyExpectation's hemisphere rule changes E by < 1e-6 relative over the view cosines the floor
    shows, for the metallic floor and for the two floors of the closure mix (the part below the floor included); the grid's
    linear interpolation is within 1e-6 as well"""
    from test_analytic_radiance import MIX
    co = np.array([0.5, 0.8, 0.9, 0.97, 1.0])
    for mat in (None, MIX["plastic"], MIX["dark_three_lobes"]):
        S = EA.ggx_floor_scene(mat)
        ex = EA.GGXSkyExpectation(S, (1.0, 1.0, 1.0))
        a, b = ex.at(co), ex.at(co, 2 * ex.n_mu, 2 * ex.n_phi)
        assert np.abs(a - b).max() < 1e-6 * np.abs(b).max(), np.abs(a - b).max() / np.abs(b).max()
        mid = np.array([0.8123, 0.9071, 0.9977])
        wo = np.stack([np.sqrt(1 - mid * mid), np.zeros(3), mid], -1)
        c = ex(np.zeros((3, 3)), wo)
        assert np.abs(c - ex.at(mid)).max() < 1e-6 * np.abs(b).max()
        # Q15 matters here: the skewed BSDF branch loses a visible share of the light (the mix: at least twice the 1 % the
        # radiance tests detect)
        free = EA.GGXSkyExpectation(S, (1.0, 1.0, 1.0), q15=False).at(co)
        assert (a < (0.97 if mat is None else 0.98) * free).all(), a / free
        if mat is not None:
            # ... and so does what the GGX samplers send below the floor: a negative share of E that the tests can see
            up = ex.at(co, lower=False)
            assert ((up - a) > 0.004 * a).all(), (up - a) / a
