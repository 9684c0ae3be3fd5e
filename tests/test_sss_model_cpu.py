"""The float64 model of the random-walk subsurface closure (tests/_sss_analytic.py) proves itself on the CPU, and the
oracle's leaves are held to it.

Solver.  The slab solver is checked five ways before any radiance test trusts it: R + T + A = 1 (R and T come from the escape kernels, A
from the density), n against 2 n, the half-space limit against Chandrasekhar's H function, the thin limit A = (1 - a) 2 tau0, and a
seeded analog Monte Carlo that knows nothing of exponential integrals.

Leaves.  orc_kat_sss_medium and orc_kat_scatter_distance (oracle/pbr_oracle.c) run the functions the oracle's walk runs.  Flags and
the channel picked must equal the model's; values agree within bounds counted in float32 roundings (eps = 2^-24, the relative error
of one rounding to nearest), every count taken along the longest dependency path and multiplied by the condition number of the step
it passes through:

  medium (MEDIUM_BOUND = 67 eps = 4.0e-6), longest path sigma_s = sigma_t a:
    A = sc s + base (1 - s)                           4      (1 - s, two products, one sum of positives)
    l = 0.25 (1 / pi) (r s)                           4      (r s, float pi, 1 / pi, the product)
    s5 = 1.85 - A + 7 |A - 0.8|^3                     8 + 8  (two inexact constants, 6 operations; A's 4 x |A s5' / s5| <= 2)
    d = l / s5                                        1
    s6 = 1.9 - A + 3.5 (A - 0.8)^2                    7 + 4  (two inexact constants, 5 operations; A's 4 x |A s6' / s6| <= 1)
    sigma_t = 1 / max(d s6, 1e-16)                    2                                         -> 34
    x = A (c0 + A (c1 - A c2))                        8 + 4  (three constants, 5 operations; A's 4), |x e^x / (1 - e^x)| <= 1
    a = 1 - exp(x)                                    2 x 9.5 + 1   (exp is correct to 1 ulp = 2 eps; at A = 0.02, x = -0.10 and the
                                                      subtraction magnifies it by e^x / (1 - e^x) = 9.5)   -> 32
    sigma_s = sigma_t a                               1                                         -> 67
  scatter distance (DISTANCE_BOUND = 7 eps = 4.2e-7): the channel pdf is 5 (sigma_s / sigma_t, the product, two sums of positives, the
    quotient); t = -log(1 - u1) / sigma_t is the quotient's 1 (1 - u1 is exact for a draw, a multiple of 2^-23) + log's 1 ulp = 2 eps: 3 eps.

Measured maxima (oracle against model; the device gives the same, tests/test_sss_leaf_gpu.py): medium 6.1 eps = 3.6e-7 of 67, t 1.7 eps
of 3, channel pdf 4.0 eps = 2.4e-7 of 7; no u0 within 1e-6 of a boundary.  DESIGN.md §15 holds the same figures."""
import ctypes as C

import numpy as np
import pytest

import _analytic as A
import _oracle as O
import _sss_analytic as S

EPS = 2.0 ** -24
MEDIUM_BOUND = 67 * EPS
DISTANCE_BOUND = 7 * EPS
BOUNDARY = 1e-6            # items whose u0 lies this close to a selection boundary are left out of the channel check ...
MAX_NEAR = 0.01            # ... at most this share of them

def _used():
    """(a, tau0) per case and channel of tests/test_sss_radiance.py, and of its plate variant's cut slab"""
    import test_sss_radiance as R
    out = set()
    for mat, _, _ in R.CASES.values():
        m = S.medium(mat)
        for st, ss in zip(m["sigma_t"], m["sigma_s"]):
            out.add((round(float(ss / st), 12), round(float(st * R.THICKNESS), 9)))
            out.add((round(float(ss / st), 12), round(float(st * R.PLATE_DEPTH), 9)))
    return sorted(out)


USED = _used()


# ------------------------------------------------------------------------------------------------- the solver
@pytest.mark.parametrize("a,tau0", USED + [(0.8, 40.0), (0.5, 1e-3), (0.99, 4.0)])
def test_slab_conserves_walks(a, tau0):
    R, T, Ab = S.slab(a, tau0)
    assert abs(R + T + Ab - 1.0) < 1e-8, (R, T, Ab)
    assert R > 0 and T > 0 and Ab > 0


def test_slab_converged():
    worst = 0.0
    for a, tau0 in USED:
        r1, r2 = S.slab(a, tau0, 24), S.slab(a, tau0, 48)
        worst = max(worst, max(abs(x - y) for x, y in zip(r1, r2)))
        assert max(abs(x - y) for x, y in zip(r1, r2)) < 1e-6, (a, tau0, r1, r2)
    print(f"slab: n = 24 against 48, max difference {worst:.1e}")


@pytest.mark.parametrize("a", [0.3, 0.8, 0.95])
def test_thick_slab_is_chandrasekhars_half_space(a):
    R, T, _ = S.slab(a, 40.0)
    assert T < 1e-6
    assert abs(R - S.chandrasekhar_R(a)) < 1e-5, (R, S.chandrasekhar_R(a))


def test_h_function():
    """the H iteration itself: conservative scattering reflects everything, and H's zeroth moment obeys Chandrasekhar's identity
    (a / 2) int H dmu = 1 - sqrt(1 - a)"""
    assert abs(S.chandrasekhar_R(1.0 - 1e-12) - 1.0) < 1e-5
    a = 0.8
    x, w = np.polynomial.legendre.leggauss(256)
    mu, w = 0.5 * (x + 1.0), 0.5 * w
    H = np.ones_like(mu)
    for _ in range(400):
        H = 1.0 / (np.sqrt(1.0 - a) + 0.5 * a * ((w * mu * H)[None] / (mu[:, None] + mu[None])).sum(1))
    assert abs(0.5 * a * (w * H).sum() - (1.0 - np.sqrt(1.0 - a))) < 1e-10


@pytest.mark.parametrize("tau0", [1e-3, 1e-4])
def test_thin_slab_absorbs_to_first_order(tau0):
    """a cosine-distributed beam's mean path through a thin slab is 2 tau0: A = (1 - a) 2 tau0 (1 + O(tau0 log tau0))"""
    for a in (0.2, 0.9):
        _, _, Ab = S.slab(a, tau0)
        assert abs(Ab / ((1.0 - a) * 2.0 * tau0) - 1.0) < 10.0 * tau0 * abs(np.log(tau0)), (a, tau0, Ab)


@pytest.mark.parametrize("a,tau0", [(0.5, 2.0), (0.9, 0.5), (0.95, 10.0), (0.2, 8.0)])
def test_slab_agrees_with_analog_monte_carlo(a, tau0):
    R, T, _ = S.slab(a, tau0)
    mc = S.slab_mc(a, tau0, 1000000, seed=7)
    print(f"slab({a}, {tau0}): R {R:.6f} (MC {mc['R']:.6f} +- {mc['se_R']:.1e}), T {T:.6f} (MC {mc['T']:.6f} +- {mc['se_T']:.1e})")
    assert abs(mc["R"] - R) < 4.0 * mc["se_R"] and abs(mc["T"] - T) < 4.0 * mc["se_T"], (R, T, mc)


# ------------------------------------------------------------------------------------------------- inputs of the leaf tests
def medium_inputs(n=600, seed=11):
    """seeded random materials: subsurface 1 / 0.5 / 0.05, colours in [0.02, 0.98], radii over four decades (1e-3 .. 10), radii below
    1e-8 in one, two and three channels (every eighth item), a transmission and a metallic now and then"""
    rng = np.random.RandomState(seed)
    mats = []
    for i in range(n):
        s = (1.0, 0.5, 0.05)[i % 3]
        r = 10.0 ** rng.uniform(-3.0, 1.0, 3)
        if i % 8 == 7:
            k = 1 + (i // 8) % 3
            r[rng.permutation(3)[:k]] = 10.0 ** rng.uniform(-12.0, -9.0, k) / s        # (r s stays a decade below 1e-8)
        mats.append(A.material(subsurface=s, base_color=tuple(rng.uniform(0.02, 0.98, 3)), subsurface_color=tuple(rng.uniform(0.02, 0.98, 3)),
                               subsurface_radius=tuple(r), specular=0.0, transmission=(0.0, 0.25, 0.6)[i % 3] if i % 5 == 0 else 0.0,
                               metallic=0.3 if i % 7 == 0 else 0.0))
    return mats


MEDIUM_FIELDS = (("weight", 2), ("albedo", 5), ("radius", 8), ("diffuse_weight", 11), ("sigma_t", 14), ("sigma_s", 17), ("thr0", 20))


def check_medium(got, mats, what):
    """got: (n, 23) float32 in orc_kat_sss_medium's layout, against the model; returns the largest relative error"""
    worst, small_seen = 0.0, set()
    for g, mat in zip(got, mats):
        m = S.medium(mat)
        assert bool(g[0]) == m["enable_diffuse"] and bool(g[1]) == m["enable_subsurface"], (what, mat, g[:2])
        assert m["enable_subsurface"]
        small_seen.add(int((m["radius"] == 0).sum()))
        for name, o in MEDIUM_FIELDS:
            want, have = m[name], g[o:o + 3].astype(np.float64)
            assert np.array_equal(want == 0, have == 0), (what, name, want, have)
            rel = np.abs(have - want) / np.where(want != 0, np.abs(want), 1.0)
            assert rel.max() <= MEDIUM_BOUND, (what, name, want, have, rel.max() / EPS)
            worst = max(worst, rel.max())
    assert small_seen == {0, 1, 2, 3}, small_seen
    return worst


def distance_inputs(n=4096, seed=13):
    """seeded (thr, sigma_s, sigma_t, u0, u1) as float32, (n, 11): media of random materials, throughputs over three decades, a zero
    throughput (the 1 / 3 fallback) every 16th item, one dominant channel every 16th, u0 a hair (3e-5) on either side of each selection
    boundary every fourth; u0 and u1 are draws (multiples of 2^-23)"""
    rng = np.random.RandomState(seed)
    mats = medium_inputs(64, seed + 1)
    med = [S.medium(m) for m in mats if i_ok(m)]
    x = np.zeros((n, 11))
    for i in range(n):
        m = med[i % len(med)]
        thr = 10.0 ** rng.uniform(-2.0, 1.0, 3)
        if i % 16 == 5:
            thr[:] = 0.0
        if i % 16 == 9:
            thr[rng.randint(3)] *= 1e4
        x[i, 0:3], x[i, 3:6], x[i, 6:9] = thr, m["sigma_s"], m["sigma_t"]
        x[i, 9], x[i, 10] = rng.random_sample(), rng.random_sample()
    x = x.astype(np.float32).astype(np.float64)
    b = S.channel_boundaries(S.channel_pdf(x[:, 0:3], x[:, 3:6], x[:, 6:9]))
    k = np.arange(n)
    near = k % 4 == 2
    side = np.where((k // 4) % 2 == 0, -3e-5, 3e-5)
    x[near, 9] = np.clip(b[near, (k[near] // 8) % 2] + side[near], 0.0, 1.0 - 2.0 ** -23)
    x[:, 9:11] = np.floor(x[:, 9:11] * 2.0 ** 23) / 2.0 ** 23
    return x.astype(np.float32)


def i_ok(mat):
    """media whose three channels all scatter (no radius below 1e-8: sigma_t = 1e16 there)"""
    return min(mat["subsurface_radius"]) * mat["subsurface"] > 1e-7


def check_distance(t, pdf, x, what, ch=None):
    """t (n,), channel pdf (n, 3) and, where the back end reports it, the channel picked, against the model on distance_inputs x.
    The channel is otherwise read off t: the one whose sigma_t reproduces it.  Returns (max rel error of t, of the pdf, share of items near a boundary)."""
    xd = x.astype(np.float64)
    want_t, want_pdf, want_ch = S.scatter_distance(xd[:, 0:3], xd[:, 3:6], xd[:, 6:9], xd[:, 9], xd[:, 10])
    b = S.channel_boundaries(want_pdf)
    near = (np.abs(xd[:, 9:10] - b) < BOUNDARY).any(1)
    assert near.mean() <= MAX_NEAR, near.mean()
    t = t.astype(np.float64)
    if ch is None:
        cand = -np.log(1.0 - xd[:, 10:11]) / xd[:, 6:9]
        ch = np.abs(cand / t[:, None] - 1.0).argmin(1)
    assert np.array_equal(ch[~near], want_ch[~near]), (what, np.nonzero(ch != want_ch)[0][:8])
    same = ch == want_ch
    rel_t = np.abs(t[same] / want_t[same] - 1.0)
    rel_p = np.abs(pdf.astype(np.float64) / want_pdf - 1.0)
    assert rel_t.max() <= 3 * EPS and rel_p.max() <= DISTANCE_BOUND, (what, rel_t.max() / EPS, rel_p.max() / EPS)
    third = (xd[:, 0:3] == 0).all(1)
    assert third.sum() >= 100 and (pdf[third] == np.float32(1.0 / 3.0)).all()
    assert sorted(set(want_ch)) == [0, 1, 2] and want_pdf.max() > 0.999
    return rel_t.max(), rel_p.max(), near.mean()


# ------------------------------------------------------------------------------------------------- the oracle's leaves
def test_oracle_medium_matches_the_model():
    L = O.lib()
    mats = medium_inputs()
    got = np.zeros((len(mats), 23), np.float32)
    for g, m in zip(got, mats):
        L.orc_kat_sss_medium(C.byref(O.make_principled(m)), O._ptr(g))
    worst = check_medium(got, mats, "oracle")
    print(f"oracle medium against the model: max relative error {worst:.2e} = {worst / EPS:.1f} eps (bound {MEDIUM_BOUND:.2e} = 67 eps)")


def test_oracle_scatter_distance_matches_the_model():
    L = O.lib()
    x = distance_inputs()
    got = np.zeros((len(x), 5), np.float32)
    for g, xi in zip(got, x):
        L.orc_kat_scatter_distance(O._ptr(np.ascontiguousarray(xi)), O._ptr(g))
    rt, rp, near = check_distance(got[:, 0], got[:, 1:4], x, "oracle", got[:, 4].astype(int))
    print(f"oracle scatter distance against the model: t {rt:.2e} = {rt / EPS:.1f} eps (bound 3 eps), channel pdf {rp:.2e} = {rp / EPS:.1f} eps "
          f"(bound 7 eps); {near:.2%} of the items within {BOUNDARY} of a boundary")


def test_model_reads_the_burley_constants():
    """spot values worked by hand from the text, so that a slip in the model itself cannot hide behind the oracle's: A = 0.8 makes both
    fittings' correction terms vanish"""
    assert abs(S.burley_fitting5(0.8) - 1.05) < 1e-15
    st, ss = S.scattering_coefficients(0.8, 2.0)
    assert abs(st - 1.0 / (2.0 * 1.1)) < 1e-15
    assert abs(ss / st - (1.0 - np.exp(0.8 * (-5.09406 + 0.8 * (2.61188 - 0.8 * 4.31805))))) < 1e-15
    m = S.medium(A.material(subsurface=1.0, subsurface_color=(0.8, 0.8, 0.8), subsurface_radius=(1.0, 2.0, 1e-9), specular=0.0, transmission=0.25))
    assert np.allclose(m["radius"], [0.25 / np.pi / 1.05, 0.5 / np.pi / 1.05, 0.0], rtol=1e-7)
    assert np.allclose(m["weight"], [0.6, 0.6, 0.0], rtol=1e-7) and np.allclose(m["diffuse_weight"], [0, 0, 0.6], rtol=1e-7)
    assert np.allclose(m["thr0"], [0.75, 0.75, 0.0], rtol=1e-7) and m["sigma_t"][2] == 1e16 and m["enable_diffuse"]
    r = S.radius_for_tau0([0.8, 0.5, 0.2], [0.7, 2.5, 8.0], 0.1)
    m = S.medium(A.material(subsurface=1.0, subsurface_color=(0.8, 0.5, 0.2), subsurface_radius=tuple(r), specular=0.0))
    assert np.allclose(m["sigma_t"] * 0.1, [0.7, 2.5, 8.0], rtol=1e-6)
