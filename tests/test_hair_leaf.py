"""The float64 hair BSDF of tests/_hair_analytic.py against the reference's own leaves, and the hair sampler against the model.

The model is what tests/test_hair_radiance.py integrates, so it is held here first: to the outputs of the reference's header compiled
unmodified (the inputs of test_oracle_vs_reference_leaf._in_hair() and those of tests/golden/ref_leaf_kats.npz), and -- its sampling
density -- to where EnergyConservingHairSample really puts wi, on the oracle and on the device."""
import os
from statistics import NormalDist

import numpy as np
import pytest

import _analytic as A
import _hair_analytic as HA
import _oracle as O
import test_hair_radiance as TH

P_FAIL = 1e-6
N_DRAWS = 1 << 20
BINS = (16, 32)               # sin(theta) = wi.x over [-1, 1] x phi = atan2(wi.z, wi.y) over [-pi, pi]: the polar axis is the tangent
MIN_EXPECT = 50
MAX_REST = 0.02
MAX_NOT_UNIT = 8              # of 2^20 (Q20)


def _unit(v):
    v = np.asarray(v, np.float64)
    return (v / np.linalg.norm(v)).astype(np.float32)


# two (wo, h, material) settings: the radiance cases' materials, one of them at |h| = 0.8
SETTINGS = [(_unit([0.3, 0.5, 0.81]), 0.35, TH.RGB_SIDE), (_unit([-0.55, 0.1, 0.83]), -0.8, TH.MELANIN)]


def _deviation(p, wo, wi, want):
    f, pdf = HA.hair_eval(wi.astype(np.float64), wo.astype(np.float64), HA.bsdf_from_leaf_params(p[:, :23]))
    got, want = np.concatenate([f, pdf[:, None]], 1), want.astype(np.float64)
    scale = np.abs(want).max(1)
    assert (scale > 0).all() and np.isfinite(got).all()
    return np.abs(got - want).max(1) / scale


def test_model_matches_the_reference_leaf():
    """D, the model's largest deviation from the reference's outputs, relative to each case's largest channel (f cos_i per channel and the
    pdf together): over EnergyConservingHairBsdfCosPdf at the 1500 inputs of _in_hair() and the 256 of ref_leaf_kats.npz, and over the
    f cos_i and pdf EnergyConservingHairSample returns with the wi it drew, evaluated by the model at that (float32) wi.

    Measured: D = 5.8e-4 (a sampled wi of a lobe with v = 4e-4, where the leaf's own float32 exponent -- terms of 2500 that cancel --
    is good to 5e-4; eval alone 2.6e-4, on outputs of 1e-43; median 6e-7, 99 % below 2.4e-4).  With exact exp / log / asin / atan2 in
    place of fast_math's polynomials D is 1.3e-2 on the sampled directions (FastAsin's 4.5e-5 moves Phi by a visible share of a narrow
    azimuthal lobe) and 1 in the far tails, so the polynomials are restated (HA.FAST).
    The bound HA.MODEL_D = 6e-4 is what test_hair_radiance holds every case's whole-strand relative standard error above (measured
    there: 8e-4 .. 1.3e-3), so that the model itself can move no z by more than 1."""
    import test_oracle_vs_reference_leaf as T
    want = O.ref_outputs("hair", T._ref_hair)
    cases = T._in_hair()
    p, wo, wi = (np.array([c[k] for c in cases]) for k in range(3))
    kat = np.load(os.path.join(O.ROOT, "tests", "golden", "ref_leaf_kats.npz"))
    d_eval = max(_deviation(p, wo, wi, want["eval"]).max(), _deviation(kat["hair_params"], kat["hair_wo"], kat["hair_wi"], kat["hair_eval"]).max())
    d_sample = max(_deviation(p, wo, want["sample"][:, :3], want["sample"][:, 3:]).max(),
                   _deviation(kat["hair_params"], kat["hair_wo"], kat["hair_sample"][:, :3], kat["hair_sample"][:, 3:]).max())
    print(f"hair model against the reference leaf: D = {max(d_eval, d_sample):.2e} (eval {d_eval:.2e}, at sampled directions {d_sample:.2e})")
    assert max(d_eval, d_sample) <= HA.MODEL_D
    HA.FAST = False
    try:
        d_exact = _deviation(p, wo, want["sample"][:, :3], want["sample"][:, 3:]).max()
    finally:
        HA.FAST = True
    print(f"with exact exp / log / asin / atan2: {d_exact:.2e}")
    assert d_exact > HA.MODEL_D, "fast_math's polynomials need no restating"


def test_param_to_bsdf_model():
    """hair_param_to_bsdf against the oracle's ParamToBsdf (bit-equal to nothing but its own reading: this is the independent one) for
    both colourings: relative 1e-6 on every one of the 23 values, and the tint ORDER -- specular, transmission, second specular, 1"""
    L = O.lib()
    for mat in (TH.RGB_SIDE, TH.MELANIN, TH.BLOND):
        par = np.zeros(23, np.float32)
        L.orc_kat_hair_param_to_bsdf(O.make_hair(mat), np.float32(0.4), O._ptr(par))
        b = HA.hair_param_to_bsdf(mat, 0.4)
        mine = np.concatenate([[0.4], b["v"], [b["s"]], b["sigma_a"], [b["eta"], b["alpha"]], b["tints"].ravel(), [1.0]])[:23]
        assert np.abs(mine - par).max() <= 1e-6 * np.abs(par).max(), (mat["coloring_hair"], mine, par)
    b = HA.hair_param_to_bsdf(TH.MELANIN, 0.0)
    assert np.allclose(b["tints"], [TH.MELANIN["specular_tint"], TH.MELANIN["transmission_tint"], TH.MELANIN["second_specular_tint"], (1, 1, 1)])
    assert len({tuple(t) for t in b["tints"]}) == 4


_model_bins = {}


def _bins(k):
    """the model's two densities integrated over each bin (24 x 24 Gauss-Legendre inside it): the pdf the leaf returns and the density
    the sampler draws from, (16, 32) each"""
    if k not in _model_bins:
        wo, h, mat = SETTINGS[k]
        nc, nph = BINS
        g, gw = A.gauss_legendre01(24)
        ce, pe = np.linspace(-1, 1, nc + 1), np.linspace(-np.pi, np.pi, nph + 1)
        M = (ce[:-1, None] + g[None] * np.diff(ce)[:, None])[:, None, :, None]
        PH = (pe[:-1, None] + g[None] * np.diff(pe)[:, None])[None, :, None, :]
        wq = (gw * np.diff(ce)[:, None])[:, None, :, None] * (gw * np.diff(pe)[:, None])[None, :, None, :]
        st = np.sqrt(1 - M * M)
        wi = np.stack(np.broadcast_arrays(M, st * np.cos(PH), st * np.sin(PH)), -1)
        _, pdf, dens = HA.hair_eval(wi, wo.astype(np.float64), HA.hair_param_to_bsdf(mat, h), density=True)
        _model_bins[k] = (pdf * wq).sum((2, 3)), (dens * wq).sum((2, 3))
    return _model_bins[k]


def _leaf_params(k):
    wo, h, mat = SETTINGS[k]
    par = np.zeros(23, np.float32)
    O.lib().orc_kat_hair_param_to_bsdf(O.make_hair(mat), np.float32(h), O._ptr(par))
    return par


def _uniforms(k):
    return np.random.RandomState(11 + k).rand(N_DRAWS, 4).astype(np.float32)


def _oracle_sampler(k):
    out = np.zeros((N_DRAWS, 7), np.float32)
    O.lib().orc_kat_hair_sample_n(O._ptr(SETTINGS[k][0]), O._ptr(_leaf_params(k)), O._ptr(_uniforms(k)), N_DRAWS, O._ptr(out))
    return out


def _gpu_sampler(k):
    import test_analytic_radiance as TR
    api = TR._pa().api
    us, par, wo = _uniforms(k), _leaf_params(k), SETTINGS[k][0]
    out = []
    for c0 in range(0, N_DRAWS, 1 << 18):
        u = us[c0:c0 + (1 << 18)]
        out.append(api.leaf_eval(api.LEAF_HAIR_SAMPLE, np.hstack([np.tile(wo, (len(u), 1)), np.tile(par, (len(u), 1)), u]), 7))
    return np.concatenate(out)


def _check_sampler(k, out):
    wo, h, mat = SETTINGS[k]
    nc, nph = BINS
    wi = out[:, :3].astype(np.float64)
    # Q20: FastSin / FastCos return 0 where their polynomial rounds above 1 (pbrlab_math.h:160, :183), so a phi_i within ~3e-4 of a
    # multiple of pi / 2 can lose a component: about one wi in 1e6 is not a unit vector.  Counted, bounded, binned like the rest.
    unit = np.abs(np.linalg.norm(wi, axis=1) - 1) < 1e-5
    assert np.isfinite(out).all() and (~unit).sum() <= MAX_NOT_UNIT, int((~unit).sum())
    ic = np.minimum((0.5 * (np.clip(wi[:, 0], -1, 1) + 1) * nc).astype(int), nc - 1)
    ip = np.minimum(((np.arctan2(wi[:, 2], wi[:, 1]) + np.pi) / (2 * np.pi) * nph).astype(int), nph - 1)
    counts = np.bincount(ic * nph + ip, minlength=nc * nph).reshape(nc, nph)
    p_pdf, p_dens = _bins(k)
    assert abs(p_dens.sum() - 1) < 1e-5, p_dens.sum()

    def z_of(p):
        """binomial z per bin expecting >= MIN_EXPECT draws, the rest merged into one bin (its probability: what is left of 1)"""
        big = N_DRAWS * p >= MIN_EXPECT
        pp = np.append(p[big], 1.0 - p[big].sum())
        cc = np.append(counts[big], counts[~big].sum())
        return (cc - N_DRAWS * pp) / np.sqrt(N_DRAWS * pp * (1 - pp)), pp[-1]
    z, rest = z_of(p_dens)
    bar = NormalDist().inv_cdf(1.0 - 0.5 * P_FAIL / len(z))
    zq, _ = z_of(p_pdf / p_pdf.sum())
    print(f"hair sampler, setting {k} (h = {h}): {len(z) - 1} bins + the rest ({rest:.4f} of the mass), max |z| {np.abs(z).max():.2f} (bar {bar:.2f}), "
          f"rms z {np.sqrt((z * z).mean()):.2f}; against the RETURNED pdf (mass {p_pdf.sum():.3f}, normalised) max |z| {np.abs(zq).max():.1f}")
    assert rest <= MAX_REST
    assert np.abs(z).max() < bar, (k, np.abs(z).max(), bar)
    # Q18: the pdf the leaf returns is not that density -- it does not even integrate to 1 -- and the counts tell the two apart
    assert abs(p_pdf.sum() - 1) > 0.02 and np.abs(zq).max() >= bar
    # the pdf returned with each drawn wi is the model's pdf there
    _, pdf = HA.hair_eval(wi, wo.astype(np.float64), HA.hair_param_to_bsdf(mat, h))
    rel = (np.abs(pdf - out[:, 6]) / out[:, 6])[unit]
    print(f"hair sampler, setting {k}: returned pdf against the model's, max rel {rel.max():.1e}")
    assert (out[:, 6] > 0).all() and rel.max() <= 4 * HA.MODEL_D, rel.max()


def test_settings_fill_the_bins():
    """a condition on the chosen settings, from the model alone: bins expecting fewer than 50 of the 2^20 draws hold <= 2 % of the mass"""
    assert any(abs(h) == 0.8 for _, h, _ in SETTINGS)
    for k in range(len(SETTINGS)):
        p = _bins(k)[1]
        assert p[N_DRAWS * p < MIN_EXPECT].sum() + (1.0 - p.sum()) <= MAX_REST, (k, p[N_DRAWS * p < MIN_EXPECT].sum())
        assert (N_DRAWS * p >= MIN_EXPECT).sum() >= 100


@pytest.mark.parametrize("k", range(len(SETTINGS)))
def test_hair_sampler_density_matches_model(k):
    """where orc_kat_hair_sample puts wi for 2^20 quadruples of uniforms, binned 16 x 32 in (sin theta, phi), against N x the integral of
    the model's SAMPLING density (Q18: hair_sample_density, not the pdf the leaf returns) over each bin: binomial z under a Bonferroni
    bar at 1e-6.  Measured: max |z| 2.7 and 4.5 (bar 5.86), rms 0.96 and 0.99; against the returned pdf 25 and 153."""
    _check_sampler(k, _oracle_sampler(k))


@pytest.mark.gpu
@pytest.mark.parametrize("k", range(len(SETTINGS)))
def test_hair_sampler_density_matches_model_gpu(k):
    """the same for the device's sampler: the hair-sample op of pbrhip_leaf_eval on the same uniforms"""
    _check_sampler(k, _gpu_sampler(k))
