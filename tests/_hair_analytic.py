"""A float64 model of the reference's hair BSDF and of the single-bounce radiance of a thin strand.  Test infrastructure only.

Written from the text of closure/energy-conserving-hair-bsdf.h and shader/hair-shader.cc:19-151, not from the oracle's restatement.
Local frame (hair-shader.cc:165-168): x = the strand's tangent, so sin(theta) = w.x, and phi = atan2(w.z, w.y).

What the leaf computes (hair_eval), per pair of unit directions and per lobe p = R, TT, TRT (+ the residual lobe 3):
  f cos_i = sum_p Mp(theta_i, theta_o tilted by the scale angle, v_p) Np(phi - Phi_p, s) Ap tint_p     (:295-405)
  pdf     = sum_p Mp Np apPdf_p,   apPdf_p = Y(Ap) / sum Y(Ap)                                          (:367-397)
with the leaf's own approximations restated in float64 (FAST = True): fast_math's polynomial log2 / exp2 / asin / atan2
(pbrlab_math.h:217-341); its sin and cos are good to float32 rounding and stay exact.

Two quirks of the reference, both modelled (Q17, Q18 of DESIGN.md §2):
  Q17  SafeLogI0 (:141-153) returns log(x^2/4 P(x^2/4)) + 1 below x = 7.5 where log I0(x) = log(x^2/4 P(x^2/4) + 1): there Mp is
       e (I0 - 1) / I0 times the normalised longitudinal function -- 0 at x = 0, 0.57 at x = 1, 2.7 at x = 7.4.
  Q18  EnergyConservingHairSample (:499-511) draws theta_i from the NORMALISED longitudinal function (the exact inversion of
       pbrt's Mp), so where Q17 bites the pdf the leaf returns is not the density wi is drawn from.  hair_sample_density is
       that density; the BSDF-sampled path carries f cos_i / pdf, and its expectation gets the factor density / pdf, exactly as
       p_true / q_rep does for the principled closures (tests/_analytic.py, Q15 / Q16)."""
import numpy as np

Y_WEIGHT = np.array([0.212671, 0.715160, 0.072169])     # RgbToY, pbrlab-util.h:48-51
PI = float(np.float32(3.141592653589793))               # kPi is a float (pbrlab_math.h:7)
MODEL_D = 6e-4                                          # tests/test_hair_leaf.py holds the model's deviation from the leaf below this
FAST = True                                             # restate fast_math's approximations (else: exact functions)
LN2 = 0.69314718055994530942
F32_MIN, F32_MAX = float(np.finfo(np.float32).tiny), float(np.finfo(np.float32).max)


# ------------------------------------------------------------------------------------------------- fast_math in float64
def _f32(c):
    return float(np.float32(c))


def fast_log(x):
    """FastLog, pbrlab_math.h:311-341: a polynomial log2 of the mantissa, the input clamped to the finite positive floats"""
    x = np.asarray(x, np.float64)
    if not FAST:
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.log(np.maximum(x, 0.0))
    x = np.clip(np.where(np.isnan(x), F32_MIN, x), F32_MIN, F32_MAX)
    m, e = np.frexp(x)                                   # x = m 2^e, m in [0.5, 1)
    f, ex = 2.0 * m - 1.0, e - 1.0
    f2 = f * f
    f4 = f2 * f2
    hi = f * _f32(-0.00931049621349) + _f32(0.05206469089414)
    lo = f * _f32(0.47868480909345) + _f32(-0.72116591947498)
    hi = f * hi + _f32(-0.13753123777116)
    hi = f * hi + _f32(0.24187369696082)
    hi = f * hi + _f32(-0.34730547155299)
    lo = f * lo + _f32(1.442689881667200)
    return ((f4 * hi) + (f * lo) + ex) * _f32(LN2)


def fast_exp(x):
    """FastExp, :217-246: exp2 of x / ln 2, clamped to [-126, 126], the integer part split off by truncation"""
    x = np.asarray(x, np.float64)
    if not FAST:
        return np.exp(x)
    x = np.clip(x * _f32(1.0 / LN2), -126.0, 126.0)
    m = np.trunc(x)
    x = x - m
    r = _f32(1.33336498402e-3)
    for c in (9.810352697968e-3, 5.551834031939e-2, 0.2401793301105, 0.693144857883, 1.0):
        r = x * r + _f32(c)
    return r * np.exp2(m)


def fast_asin(x):
    """FastAsin, :276-289 (max error 4.5e-5: it moves Phi by up to 2e-4, a visible share of a narrow azimuthal lobe)"""
    x = np.asarray(x, np.float64)
    if not FAST:
        return np.arcsin(np.clip(x, -1.0, 1.0))
    m = np.minimum(np.abs(x), 1.0)
    a = _f32(np.pi / 2) - np.sqrt(1.0 - m) * (_f32(1.5707963267) + m * (_f32(-0.213300989) + m * (_f32(0.077980478) + m * _f32(-0.02164095))))
    return np.copysign(a, x)


def fast_atan2(y, x):
    """FastAtan2, :248-274"""
    y, x = np.asarray(y, np.float64), np.asarray(x, np.float64)
    if not FAST:
        return np.arctan2(y, x)
    a, b = np.abs(x), np.abs(y)
    big, small = np.maximum(a, b), np.minimum(a, b)
    k = np.where(b == 0, 0.0, np.where(a == b, 1.0, small / np.where(big > 0, big, 1.0)))
    t = k * k
    r = k * (_f32(0.430165678) * t + 1.0) / ((_f32(0.0579354987) * t + _f32(0.763007998)) * t + 1.0)
    r = np.where(b > a, _f32(1.570796326794896557998982) - r, r)
    r = np.where(np.signbit(x), PI - r, r)
    return np.copysign(r, y)


def _safe_sqrt(x):
    return np.sqrt(np.maximum(x, 0.0))


# ------------------------------------------------------------------------------------------------- ParamToBsdf
def hair_param_to_bsdf(material, h):
    """hair-shader.cc:19-151 for a material dict (scenes.HAIR_DEFAULTS keys) and the ribbon offset h (any shape): a dict of
    sigma_a (3,), h, v (4,), s, eta, alpha (radians), tints (4,3) = specular, TRANSMISSION, second specular, 1 (:143-146), and
    transparent_scale = 1"""
    bm, bn = float(np.float32(material["roughness"])), float(np.float32(material["azimuthal_roughness"]))
    if int(material["coloring_hair"]) == 0:                                                     # kRGB, :35-46
        c = np.asarray(material["base_color"], np.float32).astype(np.float64)
        den = _f32(5.969) - _f32(0.215) * bn + _f32(2.532) * bn ** 2 - _f32(10.73) * bn ** 3 + _f32(5.574) * bn ** 4 + _f32(0.245) * bn ** 5
        sigma_a = (fast_log(c) / den) ** 2
    else:                                                                                       # kMelanin, :48-64 (random_value = 0.5)
        mel = min(max(float(np.float32(material["melanin"])), 0.0), 1.0) * (1.0 + 2.0 * (0.5 - 0.5))
        red = min(max(float(np.float32(material["melanin_redness"])), 0.0), 1.0)
        mel = -float(fast_log(max(1.0 - mel, _f32(0.0001))))
        eu, pheo = mel * (1.0 - red), mel * red
        sigma_a = np.maximum(0.0, np.array([eu * _f32(0.506) + pheo * _f32(0.343), eu * _f32(0.841) + pheo * _f32(0.733),
                                            eu * _f32(1.653) + pheo * _f32(1.924)]))
    v0 = (_f32(0.726) * bm + _f32(0.812) * bm ** 2 + _f32(3.7) * bm ** 20) ** 2                   # BetamToV, :19-27
    s = np.sqrt(PI / 8.0) * (_f32(0.265) * bn + _f32(1.194) * bn ** 2 + _f32(5.372) * bn ** 22)   # CalcS, :29-33
    tints = np.array([np.asarray(material["specular_tint"], np.float32), np.asarray(material["transmission_tint"], np.float32),
                      np.asarray(material["second_specular_tint"], np.float32), np.ones(3, np.float32)], np.float64)
    return dict(sigma_a=sigma_a, h=np.asarray(h, np.float64), v=np.array([v0, 0.25 * v0, 4.0 * v0, 4.0 * v0]), s=float(s),
                eta=float(np.float32(material["ior"])), alpha=float(np.float32(material["shift"])) * PI / 180.0, tints=tints,
                transparent_scale=1.0)


def bsdf_from_leaf_params(p):
    """the 23 floats of the leaf hooks (tests/test_oracle_vs_reference_leaf._hair_params), (N,23) -> a bsdf dict of arrays"""
    p = np.asarray(p, np.float64)
    return dict(h=p[..., 0], v=p[..., 1:5], s=p[..., 5], sigma_a=p[..., 6:9], eta=p[..., 9], alpha=p[..., 10],
                tints=p[..., 11:23].reshape(p.shape[:-1] + (4, 3)), transparent_scale=p[..., 22])


# ------------------------------------------------------------------------------------------------- the leaf
def _log_i0_leaf(x):
    """SafeLogI0, :141-162, with Q17's misplaced + 1"""
    x = np.abs(x)
    P = (1.00000003928615375e+00, 2.49999576572179639e-01, 2.77785268558399407e-02, 1.73560257755821695e-03, 6.96166518788906424e-05,
         1.89645733877137904e-06, 4.29455004657565361e-08, 3.90565476357034480e-10, 1.48095934745267240e-11)
    x22 = x * x / 4.0
    hp = _f32(P[8])
    for c in P[7::-1]:
        hp = hp * x22 + _f32(c)
    small = fast_log(x22 * hp) + 1.0
    Q = (3.98942651588301770e-01, 4.98327234176892844e-02, 2.91866904423115499e-02, 1.35614940793742178e-02, 1.31409251787866793e-01)
    inv = 1.0 / np.where(x > 0, x, 1.0)
    hq = _f32(Q[4])
    for c in Q[3::-1]:
        hq = hq * inv + _f32(c)
    return np.where(x < 7.5, small, x + 0.5 * fast_log(hq * hq * inv))


def _mp_leaf(si, ci, so, co, v):
    """Mp, :172-202 (the improved-lobe branch)"""
    ccv, ssv = ci * co / v, si * so / v
    v = np.clip(v, 1e-5, 1e4)
    return fast_exp(_log_i0_leaf(ccv) - ssv - 1.0 / v + fast_log(1.0 / v) - fast_log(1.0 - fast_exp(-2.0 / v)))


def _mp_true(si, ci, so, co, v):
    """the normalised longitudinal function EnergyConservingHairSample's theta_i has as its density (per cos theta_i dtheta_i):
    exp(-ssv) I0(ccv) / (2 v sinh(1 / v)), exact float64 (np.i0 scaled: no overflow at small v)"""
    ccv, ssv = ci * co / v, si * so / v
    # log I0: numpy's i0 below 30, the asymptotic expansion above (its next term is 1.4e-7 at 30)
    x = np.abs(ccv)
    small = np.log(np.i0(np.minimum(x, 30.0)))
    ix = 1.0 / np.maximum(x, 30.0)
    big = np.maximum(x, 30.0) - 0.5 * np.log(2.0 * np.pi * np.maximum(x, 30.0)) + np.log1p(ix / 8.0 * (1.0 + 9.0 * ix / 16.0 * (1.0 + 25.0 * ix / 24.0)))
    log_i0 = np.where(x < 30.0, small, big)
    return np.exp(log_i0 - ssv - 1.0 / v + np.log(1.0 / v) - np.log1p(-np.exp(-2.0 / v)))


def fr_dielectric(cos_i, eta_i, eta_t):
    """FrDielectric, :205-229, for cos_i >= 0 (Ap's argument is a product of two square roots)"""
    cos_i = np.clip(cos_i, 0.0, 1.0)
    sin_i = _safe_sqrt(1.0 - cos_i * cos_i)
    sin_t = eta_i / eta_t * sin_i
    cos_t = _safe_sqrt(1.0 - sin_t * sin_t)
    r_parl = (eta_t * cos_i - eta_i * cos_t) / (eta_t * cos_i + eta_i * cos_t)
    r_perp = (eta_i * cos_i - eta_t * cos_t) / (eta_i * cos_i + eta_t * cos_t)
    return np.where(sin_t >= 1.0, 1.0, 0.5 * (r_parl * r_parl + r_perp * r_perp))


def _logistic(x, s):
    n = fast_exp(-np.abs(x) / s)
    return n / (s * (1.0 + n) ** 2)


def _logistic_cdf(x, s):
    return 1.0 / (1.0 + fast_exp(-x / s))


def _np(phi, p, s, gamma_o, gamma_t):
    """Np, :273-289: the logistic trimmed to [-pi, pi] around Phi(p) = 2 p gamma_t - 2 gamma_o + p pi"""
    d = phi - (2.0 * p * gamma_t - 2.0 * gamma_o + p * PI)
    d = d - np.floor(d / (2.0 * PI)) * (2.0 * PI)
    d = np.where(d >= PI, d - 2.0 * PI, d)
    return _logistic(d, s) / (_logistic_cdf(PI, s) - _logistic_cdf(-PI, s))


def _setup(wo, b):
    """everything :301-372 derives from wo and the bsdf alone"""
    so = wo[..., 0]
    co = _safe_sqrt(1.0 - so * so)
    h, eta, alpha = (np.asarray(b[k], np.float64) for k in ("h", "eta", "alpha"))
    s2, c2 = [np.sin(alpha)], [np.cos(alpha)]
    for i in (1, 2):
        s2.append(2.0 * s2[i - 1] * c2[i - 1])
        c2.append(c2[i - 1] ** 2 - s2[i - 1] ** 2)
    # :323-339: R tilts by -2 alpha, TT by +alpha, TRT by +4 alpha, the residual lobe not at all
    so_p = [so * c2[1] - co * s2[1], so * c2[0] + co * s2[0], so * c2[2] + co * s2[2], so]
    co_p = [co * c2[1] + so * s2[1], co * c2[0] - so * s2[0], co * c2[2] - so * s2[2], co]
    phi_o = fast_atan2(wo[..., 2], wo[..., 1])
    sin_t = so / eta
    cos_t = _safe_sqrt(1.0 - sin_t * sin_t)
    with np.errstate(divide="ignore", invalid="ignore"):
        etap = np.sqrt(eta * eta - so * so) / co
        sin_gt = h / etap
    cos_gt = _safe_sqrt(1.0 - sin_gt * sin_gt)
    gamma_t, gamma_o = fast_asin(sin_gt), fast_asin(h)
    with np.errstate(divide="ignore", invalid="ignore"):
        ell = np.asarray(b["transparent_scale"], np.float64) * 2.0 * cos_gt / cos_t
        T = fast_exp(-np.asarray(b["sigma_a"], np.float64) * np.asarray(ell)[..., None])
        f = fr_dielectric(co * _safe_sqrt(1.0 - h * h), 1.0, eta)[..., None]                      # Ap, :231-255
        a1 = (1.0 - f) ** 2 * T
        a2 = a1 * T * f
        a3 = a2 * f * T / (1.0 - T * f)
    a3 = np.where(np.isfinite(a3).all(-1, keepdims=True), a3, 0.0)
    ap = np.stack([np.broadcast_to(f, a1.shape), a1, a2, a3], -2)                                  # (...,4,3)
    y = ap @ Y_WEIGHT
    return so_p, co_p, phi_o, gamma_o, gamma_t, ap, y / y.sum(-1, keepdims=True)


def hair_eval(wi, wo, bsdf, tints=None, density=False):
    """EnergyConservingHairBsdfCosPdf, :295-405: (f cos_i (...,3), pdf (...)) for unit local directions wi, wo (...,3); the
    bsdf's entries broadcast against them.  tints: another (4,3) in place of the bsdf's (the tests' mutations).
    density=True: a third value, the density EnergyConservingHairSample draws wi from (Q18)."""
    wi, wo = np.asarray(wi, np.float64), np.asarray(wo, np.float64)
    so_p, co_p, phi_o, gamma_o, gamma_t, ap, ap_pdf = _setup(wo, bsdf)
    v, s = np.asarray(bsdf["v"], np.float64), np.asarray(bsdf["s"], np.float64)
    tints = np.asarray(bsdf["tints"] if tints is None else tints, np.float64)
    si = wi[..., 0]
    ci = _safe_sqrt(1.0 - si * si)
    phi = fast_atan2(wi[..., 2], wi[..., 1]) - phi_o
    f, pdf, dens = 0.0, 0.0, 0.0
    for p in range(4):
        n_p = _np(phi, p, s, gamma_o, gamma_t) if p < 3 else 1.0 / (2.0 * PI)
        mpnp = _mp_leaf(si, ci, so_p[p], co_p[p], v[..., p]) * n_p
        f = f + mpnp[..., None] * ap[..., p, :] * tints[..., p, :]
        pdf = pdf + mpnp * ap_pdf[..., p]
        if density:
            dens = dens + _mp_true(si, ci, so_p[p], co_p[p], v[..., p]) * n_p * ap_pdf[..., p]
    bad = ~np.isfinite(f).all(-1) | ~np.isfinite(pdf)                                              # :392-402
    f, pdf = np.where(bad[..., None], 0.0, f), np.where(bad, 0.0, pdf)
    return (f, pdf, dens) if density else (f, pdf)


def hair_sample_density(wi, wo, bsdf):
    """the density (per solid angle) of EnergyConservingHairSample's wi: lobe p with probability apPdf_p, theta_i from the normalised
    longitudinal function about the tilted theta_o (:499-511), phi from the trimmed logistic about Phi_p or uniform (:513-519)"""
    return hair_eval(wi, wo, bsdf, density=True)[2]


# ------------------------------------------------------------------------------------------------- a thin strand under one quad
TMIN = 1e-3                                             # Q9: continuation and shadow rays start here


def self_hit_angle(r):
    """psi_min with r (1 + cot psi_min) = TMIN: a ray that leaves a straight strand of radius r at an angle psi >= psi_min to its
    axis has its nearest axis point at a depth <= r (1 + cot psi) <= TMIN in its own frame (at most r off the axis, at most r / sin psi
    along it), and curve_test accepts t > tmin only: the strand cannot be hit again"""
    return float(np.arctan(1.0 / (TMIN / r - 1.0)))


def strand_hits(geo, org, dirs, margin=0.0):
    """the float64 ribbon of tests/test_geometry_f64.py (geo = its Geometry of the scene) along camera rays: per ray (on, x, h, t) --
    whether a piece of the ribbon is hit, the hit point org + t dir, the contract's v (= h, with its sign) and t.  margin < 0: rays
    that pass within -margin radii of the ribbon's edge count as on it (Geometry's own margin already leaves out the last 3e-3 of
    the width, where float32 positions decide)"""
    on = np.zeros(len(dirs), bool)
    t_out, h_out = np.zeros(len(dirs)), np.zeros(len(dirs))
    o = np.broadcast_to(org, dirs.shape)
    for c0 in range(0, len(dirs), 4000):
        sl = slice(c0, c0 + 4000)
        t, m, _, _, v, kind, _, _ = geo.candidates(o[sl], dirs[sl], np.zeros(len(dirs[sl])))
        t = np.where((kind == 1) & (m >= margin), t, np.inf)
        k = np.argmin(t, 1)
        rows = np.arange(len(k))
        on[sl], t_out[sl], h_out[sl] = np.isfinite(t[rows, k]), t[rows, k], v[rows, k]
    return on, org + np.where(on, t_out, 0.0)[:, None] * dirs, h_out, t_out


class StrandExpectation:
    """E(x, wo, h) of a camera path that meets a thin straight strand under one emitting quad (a black material), per RGB channel:

      E = sum over the light's faces of  int F(wi, wo, h) Le |cos_l| / d^2 [w_nee + (p_true / q_bsdf) w_bsdf] dA

    F = the leaf's f cos_i, in the frame ex = the tangent, ey = normalize((wo x ex) x ex), ez = ex x ey (hair-shader.cc:166-168);
    q_bsdf = the pdf the leaf returns, p_true = the density it samples (Q18);
    q_nee  = pA d^2 / |cos_l (wi . ex)|: DirectIllumination is handed the TANGENT as the receiver's normal (hair-shader.cc:189,
             shader-utils.h:188-193, Q3), and the bsdf_f it gets is F / |wi . ex| (hair-shader.cc:197), so NEE adds F Le |cos_l| / (pA d^2) w_nee;
    w_nee  = q_nee^2 / (q_nee^2 + q_bsdf^2), on BOTH sides of the quad: hair-shader.cc:199 passes hemisphere = false;
    w_bsdf = q_bsdf^2 / (q_bsdf^2 + (pA d^2 / |wi . n_s|)^2) where the sampled ray meets the quad's kFront side (render.cc:43-61), else 0.
    Nothing else contributes: see tests/test_hair_radiance.py's conditions (a) and (b).

    alts (three more channels each, in this order): "flip_h" (h -> -h), "swap_tints" (the TT and TRT tints exchanged), "physical_mis"
    (w_nee + w_bsdf := 1), "count_emission" (w_bsdf on the quad's back as well).  The hemisphere rule would give 0 wherever the
    quad faces away."""

    ALTS = ("flip_h", "swap_tints", "physical_mis", "count_emission")

    def __init__(self, material, axis, light_tris, le, order=4, splits=2, alts=()):
        assert all(a in self.ALTS for a in alts)
        self.material, self.axis, self.order, self.alts = material, np.asarray(axis, np.float64), order, tuple(alts)
        self.le = np.asarray(le, np.float64)
        tris = np.asarray(light_tris, np.float64)                                 # (F,3,3) world
        ng = np.cross(tris[:, 1] - tris[:, 0], tris[:, 2] - tris[:, 0])
        area = 0.5 * np.linalg.norm(ng, axis=1)
        self.pA = 1.0 / area.sum()                                                # Q10 with one Le: max(Le) / sum(max(Le) area)
        self.ng = ng / np.linalg.norm(ng, axis=1, keepdims=True)
        self.tris = tris
        self.splits = splits
        self.channels = 3 * (1 + len(self.alts))

    def _points(self, order, splits):
        """quadrature points on the light, shared by every x (the seen part of the strand is a few 1e-3 of the light's distance long):
        (Q,3) points, (Q,) weights = dA, (Q,3) normals"""
        gs, gw = np.polynomial.legendre.leggauss(order)
        gs, gw = 0.5 * (gs + 1), 0.5 * gw
        S_, T_ = (a.ravel() for a in np.meshgrid(gs, gs, indexing="ij"))
        W_ = np.outer(gw, gw).ravel()
        pts, wts, nrm = [], [], []
        for tri, n in zip(self.tris, self.ng):
            sub = tri[None]
            for _ in range(splits):
                a, b, c = sub[:, 0], sub[:, 1], sub[:, 2]
                ab, bc, ca = (a + b) / 2, (b + c) / 2, (c + a) / 2
                sub = np.concatenate([np.stack(q, 1) for q in ((a, ab, ca), (ab, b, bc), (ca, bc, c), (ab, bc, ca))])
            A, B, C = sub[:, 0], sub[:, 1], sub[:, 2]
            area2 = np.linalg.norm(np.cross(B - A, C - A), axis=1)
            # collapsed square -> triangle: y = A + s (B - A) + s t (C - B), dA = area2 s ds dt
            y = A[:, None] + S_[None, :, None] * (B - A)[:, None] + (S_ * T_)[None, :, None] * (C - B)[:, None]
            pts.append(y.reshape(-1, 3)), wts.append((area2[:, None] * (S_ * W_)[None]).ravel())
            nrm.append(np.broadcast_to(n, (y.shape[0] * y.shape[1], 3)))
        return np.concatenate(pts), np.concatenate(wts), np.concatenate(nrm)

    def __call__(self, x, wo, h, order=None, chunk=400):
        x, wo, h = np.asarray(x, np.float64), np.asarray(wo, np.float64), np.asarray(h, np.float64)
        y, wq, ng = self._points(order or self.order, self.splits)
        out = np.zeros((len(x), self.channels))
        ex = self.axis
        for c0 in range(0, len(x), chunk):
            sl = slice(c0, c0 + chunk)
            out[sl] = self._integrate(x[sl], wo[sl], h[sl], ex, y, wq, ng)
        return out

    def _integrate(self, x, wo, h, ex, y, wq, ng):
        ey = np.cross(np.cross(wo, ex), ex)
        ey = ey / np.linalg.norm(ey, axis=-1, keepdims=True)
        ez = np.cross(ex, ey)
        loc = lambda v: np.stack([v @ ex, np.sum(v * ey[:, None], -1), np.sum(v * ez[:, None], -1)], -1) if v.ndim == 3 else \
            np.stack([v @ ex, np.sum(v * ey, -1), np.sum(v * ez, -1)], -1)  # noqa: E731
        dv = y[None] - x[:, None]                                                  # (N,Q,3)
        d2 = np.sum(dv * dv, -1)
        wi = dv / np.sqrt(d2)[..., None]
        cos_l = -np.sum(wi * ng[None], -1)                                         # > 0: the quad's front faces x
        wil, wol = loc(wi), loc(wo)[:, None]
        q_nee = self.pA * d2 / np.abs(cos_l * wil[..., 0])
        q_light = self.pA * d2 / np.abs(cos_l)                                     # n_s = n_g: the quad has no vertex normals
        geom = (np.abs(cos_l) / d2 * wq[None])[..., None] * self.le

        def estimate(hh, alts):
            """E and the mutations in `alts` that share the leaf's values at hh"""
            b = hair_param_to_bsdf(self.material, hh[:, None])
            F, q, p = hair_eval(wil, wol, b, density=True)
            ok = q > 0
            qs = np.where(ok, q, 1.0)
            w_nee = np.where(ok, q_nee ** 2 / (q_nee ** 2 + qs ** 2), 1.0)
            w_hit = np.where(ok, p / qs * qs ** 2 / (qs ** 2 + q_light ** 2), 0.0)
            out = []
            for a in (None,) + tuple(alts):
                Fa = F
                if a == "swap_tints":
                    Fa = hair_eval(wil, wol, b, tints=b["tints"][[0, 2, 1, 3]])[0]
                w = w_nee + np.where((cos_l > 0) | (a == "count_emission"), w_hit, 0.0) if a != "physical_mis" else 1.0
                out.append(np.sum(Fa * geom * np.asarray(w)[..., None], 1))
            return out

        shared = [a for a in self.alts if a != "flip_h"]
        g = dict(zip([None] + shared, estimate(h, shared)))
        if "flip_h" in self.alts:
            g["flip_h"] = estimate(-h, ())[0]
        return np.concatenate([g[a] for a in (None,) + self.alts], -1)
