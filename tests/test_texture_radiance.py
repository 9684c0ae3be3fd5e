"""Textured shading against float64 integrals, on both back ends: what should a pixel of a textured receiver converge to?

Every other test of a textured frame compares the HIP renderer with the oracle, or either with the reference's fetch as a leaf; a
misreading the two share between the hit and the texel (which corner u weights, texcoords looked up through the vertex ids, a transposed
image, a 1 - v, a half-texel offset, repeat instead of clamp, the closure set built from the base_color parameter) passes them all.
Here the base colour of every receiver point comes from tests/_texture_model.py, written from the reference's text, and
tests/_analytic.py::Expectation builds the closure set, the selection weights and both pdfs from it per point.  Statistics, sizes, seeds
and bars are test_analytic_radiance.py's: K = 64 seeded batches of 16 spp at 64 x 48, 8 x 8 cells, Student's t with Bonferroni
correction; 1.01 E must be rejected, and so must every mutant of the model listed for the case (MUTANTS_OF).

The floor and the light are quad_light's.  The textures are 4 x 3 texels (W != H, so a transposition shows) with values in [0.15, 0.9]
drawn once from numpy's RandomState (seeds 1324 / 12 / 7) and written out below; all three channels differ and every row and column
has a pair of neighbours whose luminance differs 2 : 1.  Every textured material's base_color PARAMETER is a decoy far from the
texture's mean.

What these cases cannot see: selection weights that are wrong alike in the pick and in the pdf (test_analytic_radiance.py says why);
a textured subsurface walk, textures under instance transforms and hair (no texture slot) are out of scope."""
import time

import numpy as np
import pytest

import _analytic as A
import _env_analytic as EA
import _oracle as O
import _texture_model as TM
import test_analytic_radiance as R
from test_analytic_radiance import BACKENDS, H, K, MAX_MIXED, MIN_CELLS, MIX, PLASTIC, SEED_SEQ, SPP, W, _pa, cell_groups, cell_stats, render_batches

NONE = TM.NONE
DECOY = (0.9, 0.1, 0.9)
TEX_RGB = np.array([[[0.89, 0.71, 0.50], [0.38, 0.84, 0.65], [0.21, 0.89, 0.20], [0.26, 0.21, 0.46]],
                    [[0.66, 0.22, 0.70], [0.20, 0.27, 0.87], [0.55, 0.21, 0.56], [0.26, 0.88, 0.90]],
                    [[0.17, 0.36, 0.39], [0.83, 0.85, 0.21], [0.39, 0.70, 0.89], [0.20, 0.52, 0.77]]])
TEX_MONO = np.array([[0.27, 0.71, 0.35, 0.55],
                     [0.16, 0.84, 0.83, 0.18],
                     [0.87, 0.25, 0.36, 0.60]])
ALPHA_DECOY = np.array([[0.21, 0.73, 0.48, 0.69],
                        [0.88, 0.55, 0.53, 0.20],
                        [0.35, 0.52, 0.66, 0.75]])
SSS_DECOY = np.array([[[0.44, 0.20, 0.37], [0.83, 0.31, 0.49], [0.85, 0.17, 0.60], [0.86, 0.32, 0.56]],
                      [[0.83, 0.25, 0.54], [0.71, 0.65, 0.50], [0.30, 0.52, 0.43], [0.51, 0.42, 0.78]],
                      [[0.73, 0.39, 0.58], [0.36, 0.49, 0.41], [0.64, 0.43, 0.49], [0.69, 0.46, 0.83]]])
TEX_RGBA = np.concatenate([TEX_RGB, ALPHA_DECOY[..., None]], -1)

# The floor's vertices are (-1, -.75), (1, -.75), (1, .75), (-1, .75) and its faces (0, 1, 2), (0, 2, 3).  Every texcoord array is
# ordered differently from the vertices, so texcoord_ids != vertex_ids.
IDS = np.array([[1, 3, 0], [1, 0, 2]], np.uint32)
TC_UNIT = np.array([[1.0, 1.0], [0.0, 0.0], [0.0, 1.0], [1.0, 0.0]])                 # u along x, v along y, (0,0) .. (1,1)
TC_CLAMPED = np.array([[1.25, -0.25], [-0.25, 1.25], [1.25, 1.25], [-0.25, -0.25]])  # a quarter turn: u along y, v along -x
# triangle 0 has texcoords of its own (a skewed map); triangle 1 lacks one corner's id and reads its barycentrics (the two ids it
# keeps point at decoys)
TC_FALLBACK = np.array([[0.8, 0.95], [0.05, 0.1], [0.3, 0.3], [0.9, 0.2]])
IDS_FALLBACK = np.array([[1, 3, 0], [1, NONE, 2]], np.uint32)

LAMBERT = dict(specular=0.0)
CASES = ["lambert_unit", "lambert_clamped", "lambert_fallback", "plastic_textured", "tinted_half_metal_textured"]
SETUP = {  # case: (material, texture, texcoords, texcoord ids)
    "lambert_unit": (LAMBERT, TEX_RGB, TC_UNIT, IDS),
    "lambert_clamped": (LAMBERT, TEX_RGBA, TC_CLAMPED, IDS),
    "lambert_fallback": (LAMBERT, TEX_MONO, TC_FALLBACK, IDS_FALLBACK),
    "plastic_textured": (PLASTIC, TEX_RGB, TC_UNIT, IDS),
    "tinted_half_metal_textured": (MIX["tinted_half_metal"], TEX_RGB, TC_UNIT, IDS),
}
# the mutants of tests/_texture_model.py each case must reject; one a case cannot see is not listed for it.  fallback_whole_mesh: the
# fallback to the barycentrics applied to the wrong triangle (to triangle 0 as well, because its mesh has a face without texcoords)
MUTANTS_OF = {
    "lambert_unit": ("half_texel", "swap_uv", "flip_v", "vertex_indexed", "weights_transposed", "nearest", "param_color"),
    "lambert_clamped": ("wrap", "half_texel", "swap_uv"),
    "lambert_fallback": ("corner_order", "fallback_whole_mesh"),
    "plastic_textured": ("param_color", "half_texel"),
    "tinted_half_metal_textured": ("param_color", "half_texel"),
}
SPP_OF = {}          # (every case rejects its mutants at 16 spp)


def textured_floor(mat, tc, ids, extra=()):
    v, f = A.quad((0, 0, 0), (1.0, 0, 0), (0, 0.75, 0))
    m = A.material(**dict(mat, base_color=DECOY, base_color_tex_id=0, **dict(extra)))
    return A.Mesh("floor", v, f, m, texcoords=tc, texcoord_ids=ids)


def scene_of(case):
    mat, tex, tc, ids = SETUP[case]
    return A.Scene([textured_floor(mat, tc, ids), R._tilted_light()], textures=[tex])


_expect = {}


def expected(case):
    """test_analytic_radiance.expected for the textured cases, computed once per session: classes, E and every mutant's expectation"""
    if case not in _expect:
        S = scene_of(case)
        so = A.build(O.OracleScene(), S, O.make_principled)
        cam = A.Camera(*so.FetchSceneAABB(), W, H)
        ex = A.Expectation(S, alts=MUTANTS_OF[case])
        t0 = time.time()
        cls, val, (pts, wo) = A.classify_and_expect(S, cam, ex)
        on = A.on_receiver(S, cam)
        out = dict(S=S, cam=cam, ex=ex, cls=cls, val=val[..., :3], pts=pts, wo=wo, on=on, seconds=time.time() - t0,
                   mixed=1.0 - (cls == A.PIX_RECEIVER).sum() / on.sum())
        out["alt"] = {name: val[..., 3 * k + 3:3 * k + 6] for k, name in enumerate(ex.alts)}
        print(f"{case}: expectation in {out['seconds']:.1f} s, {100 * out['mixed']:.1f} % of the on-receiver pixels left out")
        _expect[case] = out
    return _expect[case]


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("case", CASES)
def test_texture_radiance(case, backend):
    e = expected(case)
    cls, val = e["cls"], e["val"]
    spp = SPP_OF.get(case, SPP)
    rgba, count = render_batches(backend, e["S"], _pa() if backend == "gpu" else None, spp)
    # exact pixels, batch by batch (test_analytic_radiance's)
    assert (count == spp).all() and (rgba[..., 3] == count).all()
    light, zero = cls == A.PIX_LIGHT, cls == A.PIX_ZERO
    want = count[..., None].astype(np.float32) * val.astype(np.float32)[None]
    assert (rgba[:, light, :3] == want[:, light]).all(), "a pixel on an emitter's front face is not exactly count * Le"
    assert zero.sum() > 0 and (rgba[:, zero, :3] == 0).all(), "a pixel on black geometry / an emitter's back / nothing is not exactly 0"
    if case == "lambert_fallback":
        # a one-channel texture: FetchFloat3 reads 0 for G and B, on both triangles and on the pixels the statistics leave out
        assert e["on"].sum() > 1500 and (rgba[:, e["on"], 0] > 0).any() and (rgba[:, e["on"], 1:3] == 0).all(), "G or B is not exactly 0"
    means = rgba[..., :3] / count[..., None]
    z, bar = cell_stats(means, cls, val)
    print(f"{case} [{backend}]: {len(z) - 1} cells, max |z| {np.abs(z).max():.2f} (bar {bar:.2f}), {100 * e['mixed']:.1f} % left out")
    assert np.abs(z).max() < bar, (z, bar)
    z1, _ = cell_stats(means, cls, val * 1.01)
    print(f"{case} [{backend}]: max |z| against 1.01 E {np.abs(z1).max():.2f}")
    assert np.abs(z1).max() >= bar, ("1.01 E is not rejected", np.abs(z1).max(), bar)
    assert len(z) - 1 >= MIN_CELLS and e["mixed"] <= MAX_MIXED, (len(z) - 1, e["mixed"])
    assert tuple(e["alt"]) == MUTANTS_OF[case]
    for name, alt in e["alt"].items():
        za, _ = cell_stats(means, cls, alt)
        print(f"{case} [{backend}]: max |z| against {name}: {np.abs(za).max():.2f}")
        assert np.abs(za).max() >= bar, (f"{name} is not rejected", np.abs(za).max(), bar)


@pytest.mark.parametrize("case", CASES)
def test_mutants_are_visible_by_design(case):
    """no rendering: every listed mutant's float64 expectation departs from E by more than 5 % (in some channel) in at least a quarter
    of the judged cells, so that a later edit of the textures cannot quietly make a mutant invisible"""
    e = expected(case)
    cells = cell_groups(e["cls"])[:-1]
    assert len(cells) >= MIN_CELLS
    for name, alt in e["alt"].items():
        E = np.array([e["val"][g].mean(0) for g in cells])
        M = np.array([alt[g].mean(0) for g in cells])
        far = (np.abs(M - E) > 0.05 * np.abs(E)).any(1)
        print(f"{case}: {name} departs by > 5 % in {far.sum()} of {len(cells)} cells")
        assert far.mean() >= 0.25, (case, name, far.mean())


def test_texture_quadrature_converged():
    """test_analytic_radiance.test_quadrature_converged (1e-5) on the textured cases"""
    R.test_quadrature_converged(CASES, lambda case: dict(expected(case), ex=A.Expectation(expected(case)["S"])))   # (E alone)


def _near_texel_lines(e, n):
    """the n PIX_RECEIVER pixels whose centres lie nearest to a texel line, in texels"""
    ys, xs = np.nonzero(e["cls"] == A.PIX_RECEIVER)
    d = e["cam"].dirs(xs.astype(np.float64), ys.astype(np.float64), 0.5, 0.5)
    _, _, t, _ = A.cast(e["S"], e["cam"].org, d)
    tx = e["ex"].textured
    tu, tv = tx.coords(e["cam"].org + t[:, None] * d)
    h, w = tx.tex.shape[:2]
    dist = np.minimum(np.where((tu > 0) & (tu < 1), np.abs(w * tu - np.rint(w * tu)), np.minimum(np.abs(w * tu), np.abs(w * tu - w))),
                      np.where((tv > 0) & (tv < 1), np.abs(h * tv - np.rint(h * tv)), np.minimum(np.abs(h * tv), np.abs(h * tv - h))))
    return np.argsort(dist)[:n], xs, ys


@pytest.mark.parametrize("case", CASES[:3])
def test_texture_pixel_rule_converged(case):
    """test_pixel_rule_converged's textured twin: a bilinear texture kinks along texel lines, so footprints are cut along them
    (A.texel_pieces) before the rule is applied.  The footprint means agree with an 8 x 8 rule to < 1e-4 of the brightest pixel on the 100
    pixels nearest to texel lines plus 100 random ones; and on the 8 nearest, with a rule that knows nothing of texel lines (a 32 x 32
    midpoint rule; its own error across a kink is < 1e-4 of the change of slope there, 1e-5 of the texel contrast) -- so the cuts are in
    the right place."""
    e = expected(case)
    ex = A.Expectation(e["S"])                               # (E alone: the mutants' expectations are not under test here)
    near, xs, ys = _near_texel_lines(e, 100)
    i = np.concatenate([near, np.random.RandomState(4).choice(len(ys), 100, replace=False)])
    top = e["val"][ys, xs].max()
    fine = A.pixel_mean(e["S"], e["cam"], ex, xs[i], ys[i], 8)
    err = np.abs(fine[:, :3] - e["val"][ys[i], xs[i]]).max()
    pieces, affine = A.texel_pieces(ex.textured, e["S"], e["cam"], xs[i], ys[i])
    assert affine.all() and len(pieces) >= 30, len(pieces)
    j = near[:8]
    m = (np.arange(32) + 0.5) / 32
    jx, jy = (a.ravel() for a in np.meshgrid(m, m, indexing="ij"))
    d = e["cam"].dirs(xs[j, None].astype(np.float64), ys[j, None].astype(np.float64), jx, jy).reshape(-1, 3)
    _, _, t, _ = A.cast(e["S"], e["cam"].org, d)
    brute = ex(e["cam"].org + t[:, None] * d, -d).reshape(len(j), -1, 3).mean(1)
    err_b = np.abs(brute - e["val"][ys[j], xs[j]]).max()
    print(f"{case}: footprint rule against 8 x 8: {err / top:.1e}, against 32 x 32 midpoints: {err_b / top:.1e} of the brightest pixel; "
          f"{len(pieces)} of the {len(i)} footprints are cut")
    assert err < 1e-4 * top and err_b < 1e-4 * top, (err / top, err_b / top)


def test_texture_model_edges():
    """the model's own quirks, as the reference's lines give them: the first texel alone only at u = 0, the last column flat over
    u in [(W-1)/W, 1], clamping outside [0, 1], rows follow v, missing channels read 0, a fourth is dropped"""
    t = TEX_RGB
    assert np.array_equal(TM.fetch(t, 0.0, 0.0), t[0, 0]) and np.array_equal(TM.fetch(t, -3.0, -0.1), t[0, 0])
    assert np.array_equal(TM.fetch(t, 0.75, 0.0), t[0, 3]) and np.allclose(TM.fetch(t, 0.9, 0.0), t[0, 3], atol=1e-15) and np.array_equal(TM.fetch(t, 7.0, 0.0), t[0, 3])
    assert np.allclose(TM.fetch(t, 0.125, 0.0), 0.5 * (t[0, 0] + t[0, 1]), atol=1e-15)           # px = 0.5: halfway, no half-texel offset
    assert np.allclose(TM.fetch(t, 0.0, 0.5), 0.5 * (t[1, 0] + t[2, 0]), atol=1e-15)             # py = 1.5: rows follow v
    assert np.allclose(TM.fetch(t, 0.3, 1.0), TM.fetch(t, 0.3, 0.7), atol=1e-15)                          # the last row is flat as well
    assert np.array_equal(TM.fetch(TEX_RGBA, 0.3, 0.4), TM.fetch(t, 0.3, 0.4))
    assert np.array_equal(TM.fetch(TEX_MONO, 0.3, 0.4)[1:], [0.0, 0.0]) and TM.fetch(TEX_MONO, 0.3, 0.4)[0] == TM.fetch(TEX_MONO[..., None], 0.3, 0.4)[0]
    floor = scene_of("lambert_fallback").meshes[0]
    assert [float(c[0]) for c in TM.texcoord(floor, np.array([1]), np.array([0.25]), np.array([0.5]))] == [0.25, 0.5]
    tu, tv = TM.texcoord(floor, np.array([0, 0, 0]), np.array([0.0, 1.0, 0.0]), np.array([0.0, 0.0, 1.0]))
    assert np.array_equal(np.stack([tu, tv], -1), TC_FALLBACK[[1, 3, 0]])


# ----------------------------------------------------------------------------------------------- the constant sky: kShadeFull | kShadeEnv
SKY_L, SKY_SCALE = np.array([0.75, 1.25, 0.5]), 2.0        # test_env_radiance's furnace sky


def _sky_scene():
    """lambert_unit's floor and _env_analytic.floor_scene's sliver (it widens the scene's box, so the camera sees the background too)"""
    return A.Scene([textured_floor(LAMBERT, TC_UNIT, IDS), EA.floor_scene().meshes[1]], textures=[TEX_RGB])


def _case_lambert_unit_sky(backend):
    """lambert_unit's floor, no quad light, under test_env_radiance's constant sky (its furnace case, batches and statistics): a Lambert
    floor converges to rho(x) L with rho(x) the texel colour; 1.01 E, the half-texel offset and the base_color parameter are rejected"""
    from test_env_radiance import SPP as ESPP, _check_v, _per_pixel, _receiver, _render
    S, L, scale = _sky_scene(), SKY_L, SKY_SCALE
    rgba, count, cam, _ = _render(backend, S, np.tile(L.astype(np.float32), (4, 8, 1)), scale, None)
    assert (count == ESPP).all() and (rgba[..., 3] == count).all()
    rec = _receiver(S, cam)
    assert rec.sum() > 1000
    bg = EA.background_texels(S, cam, np.eye(3), 8, 4)[0] >= 0
    assert bg.sum() > 100 and (rgba[:, bg, :3] == (ESPP * L * scale).astype(np.float32)).all(), "a background pixel is not count x L x scale"
    val, keep = _per_pixel(S, cam, _Albedo(S, L * scale), rec)
    alts = tuple((m, _per_pixel(S, cam, _Albedo(S, L * scale, m), rec)[0]) for m in ("half_texel", "param_color"))
    assert keep.sum() > 1000 and 1.0 - keep.sum() / rec.sum() <= MAX_MIXED
    _check_v(f"lambert_unit_sky [{backend}]", rgba[..., :3] / count[..., None], keep, val, alts)


class _Albedo:
    """E(x) = the float64 texel colour at x (times a constant radiance): the albedo layer's expectation, and a Lambert floor's under a
    constant sky.  mutant: the same through one of the texture model's mutants."""

    def __init__(self, S, scale=1.0, mutant=None):
        m = S.meshes[S.receiver]
        self.textured, self.scale, self.mutant = A.Textured(m, S.textures[m.material["base_color_tex_id"]]), np.asarray(scale, np.float64), mutant

    def __call__(self, x, wo, order=None):
        return self.textured.base_color(x, self.mutant) * self.scale


@pytest.mark.parametrize("backend", BACKENDS)
def test_texture_lambert_unit_sky(backend):
    _case_lambert_unit_sky(backend)


# ----------------------------------------------------------------------------------------------- the albedo layer
@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES[:3])
def test_texture_albedo_layer(case):
    """RenderFeatures' albedo sum / count per pixel over the same K batches against the footprint mean of the float64 texel colour alone:
    dfirsthit.h's fetch held to the model with far less noise than the radiance has.  1.01 x and the half-texel offset are rejected.
    Where the texture is flat over a whole cell (the clamped borders, the last column) every batch mean is the same number and SE = 0:
    there the mean must equal E to float32 rounding, (spp + 2) eps relative (the texel's conversion and spp additions in float32),
    which is also let off |M - E| before it is divided by SE elsewhere -- 2e-6 relative, against the 1e-2 the test must see."""
    pa = _pa()
    e = expected(case)
    S = e["S"]
    cls, val, _ = A.classify_and_expect(S, e["cam"], _Albedo(S))
    half = A.classify_and_expect(S, e["cam"], _Albedo(S, mutant="half_texel"))[1]
    sg = A.build(pa.Scene(), S, pa.make_principled)
    means = []
    for k in range(K):
        layer = pa.RenderFeatures(sg, W, H, SPP, first_pass=k * SPP, seed_seq=SEED_SEQ)
        assert (layer.count == SPP).all() and (layer.albedo[e["on"], 3] == SPP).all()
        means.append(layer.albedo[..., :3] / layer.count[..., None])
    sg.close()
    means = np.stack(means)
    groups = cell_groups(cls)
    tol = (SPP + 2) * float(np.finfo(np.float32).eps)

    def stats(v):
        bm = np.array([means[:, g].mean(1) for g in groups])                                # (groups, K, 3)
        E = np.array([v[g].mean(0) for g in groups])
        se = bm.std(1, ddof=1) / np.sqrt(K)
        d = np.maximum(np.abs(bm.mean(1) - E) - tol * np.abs(E), 0.0)
        return np.where(se > 0, d / np.where(se > 0, se, 1.0), np.where(d == 0, 0.0, np.inf))
    z = stats(val)
    bar = A.student_t_bar(R.P_FAIL / z.size, K - 1)
    z1, zh = stats(1.01 * val), stats(half)
    flat = int((np.array([means[:, g].mean(1) for g in groups]).std(1) == 0).any(1).sum())
    top = lambda v: v[np.isfinite(v)].max()  # noqa: E731  (inf: a flat cell off by more than float32 rounding)
    print(f"{case} albedo [gpu]: {len(groups) - 1} cells ({flat} of them flat in a channel: SE = 0), max |z| {z.max():.2f} (bar {bar:.2f}), against 1.01 x "
          f"{top(z1):.0f} ({int(np.isinf(z1).any(1).sum())} flat cells off), against half_texel {top(zh):.0f} ({int(np.isinf(zh).any(1).sum())} flat cells off)")
    assert len(groups) - 1 >= MIN_CELLS
    assert z.max() < bar, (z, bar)
    assert z1.max() >= bar and zh.max() >= bar, (z1.max(), zh.max(), bar)


# ----------------------------------------------------------------------------------------------- frames that must be identical
def _first_batch(backend, S, spp=SPP, device_math=False, env=None):
    """the first of render_batches' K batches: (rgba, count); env: SetEnvironment's arguments"""
    if backend == "oracle":
        so = A.build(O.OracleScene(), S, O.make_principled)
        if env is not None:
            so.SetEnvironment(*env)
        return so.render(W, H, spp, first_pass=0, seed_seq=SEED_SEQ, threads=O.oracle_threads(),
                         math_mode=O.MATH_DEVICE if device_math else O.MATH_LIBM)[:2]
    pa = _pa()
    sg = A.build(pa.Scene(), S, pa.make_principled)
    if env is not None:
        sg.SetEnvironment(*env)
    layer = pa.RenderLayer()
    pa.Render(sg, W, H, spp, layer=layer, first_pass=0, seed_seq=SEED_SEQ)
    out = np.array(layer.rgba, np.float32).reshape(H, W, 4), np.array(layer.count, np.uint32).reshape(H, W)
    sg.close()
    return out


def _same_frame(a, b):
    return a[0][..., :3].any() and np.array_equal(a[1], b[1]) and a[0].tobytes() == b[0].tobytes()


@pytest.mark.parametrize("backend", BACKENDS)
def test_subsurface_color_map_does_nothing_without_subsurface(backend):
    """lambert_unit with a decoy subsurface_color_tex_id and subsurface = 0 renders lambert_unit's frame, as bytes:
    mixed_ss_base_color = subsurface_color * 0 + base_color * 1 (cycles-principled-shader.cc:334-335)"""
    S = scene_of("lambert_unit")
    D = A.Scene([textured_floor(LAMBERT, TC_UNIT, IDS, dict(subsurface_color_tex_id=1, subsurface=0.0)), S.meshes[1]], textures=[TEX_RGB, SSS_DECOY])
    assert _same_frame(_first_batch(backend, S), _first_batch(backend, D)), "a subsurface colour map changes a frame without subsurface"


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("name", ["plastic", "tinted_half_metal"])
def test_one_texel_at_zero_texcoords_is_the_untextured_material(name, backend):
    """a 1 x 1 texture holding exactly the material's base_color, texcoords (0, 0) at every vertex (dx = dy = 0: the fetch returns the
    texel itself) and a decoy base_color parameter: the untextured material's frame, as bytes.  On the GPU this sets the per-hit
    closure set of k_shade_principled<2> / k_tail<2> against the committed one of <0> on the closure mix."""
    plain = A.Scene([R._floor(**MIX[name]), R._tilted_light()])
    floor = textured_floor(MIX[name], np.zeros((4, 2)), plain.meshes[0].faces.astype(np.uint32))
    one = A.Scene([floor, plain.meshes[1]], textures=[np.asarray(MIX[name]["base_color"], np.float32).reshape(1, 1, 3)])
    assert _same_frame(_first_batch(backend, plain), _first_batch(backend, one)), "the texel and the parameter render different frames"


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES + ["lambert_unit_sky"])
def test_texture_gpu_matches_oracle(case):
    """the first batch of every case: the HIP renderer and the oracle (device math), equal as bytes"""
    if case == "lambert_unit_sky":
        S, spp, env = _sky_scene(), SPP, (np.tile(SKY_L.astype(np.float32), (4, 8, 1)), SKY_SCALE, None)
    else:
        S, spp, env = scene_of(case), SPP_OF.get(case, SPP), None
    assert _same_frame(_first_batch("gpu", S, spp, env=env), _first_batch("oracle", S, spp, device_math=True, env=env)), case
