"""Float64 model of the random-walk subsurface closure, written from the reference's text:
src/shader/random-walk-sss.h:35-405 and ParamToBsdf's subsurface branch (cycles-principled-shader.cc:326-365).

Leaves.  medium() is ParamToBsdf's subsurface branch + BssrdfSetup(true, true, true) + ComputeScatteringCoefficient;
channel_pdf / scatter_distance are SampleChannel / SampleScatterDistance; walk_event is one iteration of the walk's loop
(:322-361) followed by the head of the next one (:288-314), fed by PCG32 draws (the generator of tests/_camera_analytic.py).

Transport.  slab(a, tau0, n) solves the gray plane-parallel slab: cosine-distributed entry at the top face, isotropic scattering,
single-scattering albedo a, optical thickness tau0.  With psi(t) the collision density per entering walk,
    psi(t) = 2 E2(t) + (a / 2) int_0^tau0 E1(|t - t'|) psi(t') dt'
(2 E2: first collisions of a cosine-distributed beam; (1 / 2) E1: the depth distribution of the next collision after an isotropic
scattering).  Nystrom on Gauss-Legendre panels graded towards both faces, the logarithmic singularity of E1 subtracted with
int_0^tau0 (1 / 2) E1(|t - t'|) dt' = 1 - E2(t) / 2 - E2(tau0 - t) / 2.  Then
    R = int psi a E2(t) / 2 dt             (a scattered walk leaves through the top face)
    T = 2 E3(tau0) + int psi a E2(tau0 - t) / 2 dt
    A = (1 - a) int psi dt.
slab_mc is the same problem by analog Monte Carlo in three dimensions (optionally with side walls), chandrasekhar_R the half-space
limit from Chandrasekhar's H function.

Radiance.  Under a constant environment L a one-closure subsurface slab shows L thr0 (R + KAPPA T), not L thr0 (R + T): see
exit_weights()."""
import numpy as np
from scipy.special import expn

from _camera_analytic import _pcg32

BSSRDF_MIN_RADIUS = 1e-8          # random-walk-sss.h:76
CUT_OFF = 1e-3                    # kClosureWeightCutOff = kEps
F32_EPS = float(np.finfo(np.float32).eps)
MAX_BOUNCES = 8192                # :281


def _sat(x):
    return min(max(float(x), 0.0), 1.0)


def _f32(v):
    """the float32 value a parameter is stored as, in float64"""
    return np.asarray(v, np.float32).astype(np.float64)


def safe_divide(a, b):
    """SafeDivideSpectrum, pbrlab-util.h:25-46"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    ok = np.abs(b) >= F32_EPS
    return np.where(ok, a / np.where(ok, b, 1.0), 0.0)


def burley_fitting5(A):
    """:40-43, diffuse surface transmission, equation (5)"""
    return 1.85 - A + 7.0 * np.abs((A - 0.8) ** 3)


def scattering_coefficients(A, d):
    """ComputeScatteringCoefficientFromAlbedo, :111-121 -> sigma_t, sigma_s"""
    A, d = np.asarray(A, np.float64), np.asarray(d, np.float64)
    a = 1.0 - np.exp(A * (-5.09406 + A * (2.61188 - A * 4.31805)))
    s = 1.9 - A + 3.5 * (A - 0.8) ** 2
    sigma_t = 1.0 / np.maximum(d * s, 1e-16)
    return sigma_t, sigma_t * a


def medium(mat):
    """The closure set's subsurface part and the walk's medium for principled parameters `mat` (a dict with scenes.PRINCIPLED_DEFAULTS'
    keys, no textures): enable flags, subsurface weight / albedo / radius, the diffuse weight BssrdfSetup adds, sigma_t, sigma_s, thr0."""
    base, sc, r = _f32(mat["base_color"]), _f32(mat["subsurface_color"]), _f32(mat["subsurface_radius"])
    s = float(_f32(mat["subsurface"]))
    metallic, transmission = float(_f32(mat["metallic"])), float(_f32(mat["transmission"]))
    diffuse_w = (1.0 - _sat(metallic)) * (1.0 - _sat(transmission))                      # :326-327
    mixed = sc * s + base * (1.0 - s)                                                    # :334-335
    out = dict(enable_diffuse=False, enable_subsurface=False, weight=np.zeros(3), albedo=np.zeros(3), radius=np.zeros(3),
               diffuse_weight=np.zeros(3))
    if mixed.mean() > CUT_OFF:
        if s < CUT_OFF and diffuse_w > CUT_OFF:                                          # :339-343
            out["enable_diffuse"], out["diffuse_weight"] = True, base * diffuse_w
        elif s > CUT_OFF:                                                                # :344-363
            weight, albedo, radius = mixed * diffuse_w, mixed.copy(), r * s
            # BssrdfSetup(burley_radius, scale_mfp, use_eq5), :71-104
            small = radius < BSSRDF_MIN_RADIUS
            kd = np.where(small, weight, 0.0)
            weight, radius = np.where(small, 0.0, weight), np.where(small, 0.0, radius)
            add = kd if small.any() else np.zeros(3)
            if not small.all():
                radius = 0.25 * (1.0 / np.pi) * radius / burley_fitting5(albedo)          # :48-69
            out.update(enable_subsurface=True, weight=weight, albedo=albedo, radius=radius)
            if np.abs(add).sum() >= F32_EPS:                                             # !IsBlack, :359-362
                out["enable_diffuse"], out["diffuse_weight"] = True, add
    sigma_t, sigma_s = scattering_coefficients(out["albedo"], out["radius"])           # :123-136
    out.update(sigma_t=sigma_t, sigma_s=sigma_s, thr0=safe_divide(out["weight"], out["albedo"]))
    return out


def channel_pdf(thr, sigma_s, sigma_t):
    """SampleChannel's pdf, :150-163, for (N, 3) arrays"""
    w = np.abs(np.asarray(thr, np.float64) * safe_divide(sigma_s, sigma_t))
    sm = w.sum(-1, keepdims=True)
    return np.where(sm > 0.0, w / np.where(sm > 0.0, sm, 1.0), 1.0 / 3.0)


def channel_boundaries(pdf):
    """the two values of u0 at which the channel changes: pdf_x and pdf_x + pdf_y"""
    return np.stack([pdf[..., 0], pdf[..., 0] + pdf[..., 1]], -1)


def scatter_distance(thr, sigma_s, sigma_t, u0, u1):
    """SampleScatterDistance, :174-187 -> t, channel pdf (N, 3), channel (N,)"""
    sigma_t = np.asarray(sigma_t, np.float64)
    pdf = channel_pdf(thr, sigma_s, sigma_t)
    b = channel_boundaries(pdf)
    u0 = np.asarray(u0, np.float64)
    ch = np.where(u0 < b[..., 0], 0, np.where(u0 < b[..., 1], 1, 2))
    st = np.take_along_axis(np.broadcast_to(sigma_t, pdf.shape), ch[..., None], -1)[..., 0]
    return -np.log(1.0 - np.asarray(u1, np.float64)) / st, pdf, ch


def uniform_sample_sphere(u1, u2):
    """sampler/sampling-utils.h:16-23 (y up)"""
    u = 2.0 * u2 - 1.0
    norm = np.sqrt(np.maximum(0.0, 1.0 - u * u))
    th = 2.0 * np.pi * u1
    return np.stack([norm * np.cos(th), u, norm * np.sin(th)], -1)


def draws_from(state, inc, n):
    """n draws (float32 in [0, 1), as float64) of PCG32 generators at `state` with increment `inc` (uint64 arrays) -> (N, n), new state"""
    state, inc = np.array(state, np.uint64), np.asarray(inc, np.uint64)
    out = np.zeros((len(state), n))
    with np.errstate(over="ignore"):
        for k in range(n):
            state, x = _pcg32(state, inc)
            out[:, k] = ((x >> np.uint32(9)) | np.uint32(0x3F800000)).view(np.float32) - np.float32(1.0)
    return out, state


def walk_event(org, dirn, sigma_t, sigma_s, thr, t_scatter, bounce, rng_state, rng_inc, hit_t=None):
    """One event of the walk's loop (:322-361) on (N, ...) arrays.
    hit_t given: the bounded ray hit a surface at hit_t (:335-341) -> the exit throughput thr T / dot(channel pdf, T).
    Else the ray ended in the medium (:343-361, then :288-314 of the next iteration): throughput thr sigma_s T / dot(channel pdf,
    sigma_t T); roulette with p = saturate(max(thr)) against one draw q (alive when q < p, then thr / p); the origin advances by
    t dir; the step index grows and the walk ends past 8192; the next direction is UniformSampleSphere with the FIRST draw as u2 (g++
    evaluates the two Draw() arguments right to left), normalised; two more draws give the next distance.
    -> dict(alive, org, dir, thr, t_scatter, bounce, rng_state, p, q, channel); the values of a dead walk are those of its last step."""
    org, dirn, sigma_t, sigma_s, thr = (np.asarray(v, np.float64) for v in (org, dirn, sigma_t, sigma_s, thr))
    chpdf = channel_pdf(thr, sigma_s, sigma_t)
    if hit_t is not None:
        trans = np.exp(-sigma_t * np.asarray(hit_t, np.float64)[:, None])
        return dict(thr=thr * trans / (chpdf * trans).sum(-1, keepdims=True))
    t = np.asarray(t_scatter, np.float64)
    trans = np.exp(-sigma_t * t[:, None])
    pdf = (chpdf * sigma_t * trans).sum(-1, keepdims=True)
    thr = thr * (sigma_s * trans) / pdf
    p = np.clip(thr.max(-1), 0.0, 1.0)
    d, state = draws_from(rng_state, rng_inc, 5)
    q = d[:, 0]
    bounce = np.asarray(bounce, np.int64) + 1
    alive = (q < p) & (bounce <= MAX_BOUNCES)
    thr = thr / np.where(p > 0, p, 1.0)[:, None]
    org = org + t[:, None] * dirn
    wi = uniform_sample_sphere(d[:, 2], d[:, 1])
    wi = wi / np.linalg.norm(wi, axis=-1, keepdims=True)
    t_next, _, ch = scatter_distance(thr, sigma_s, sigma_t, d[:, 3], d[:, 4])
    return dict(alive=alive, org=org, dir=wi, thr=thr, t_scatter=t_next, bounce=bounce, rng_state=state, p=p, q=q, channel=ch,
                u0=d[:, 3], next_pdf=channel_pdf(thr, sigma_s, sigma_t))


# ------------------------------------------------------------------------------------------------- the gray slab
def _panels(tau0, n):
    """panel edges on [0, tau0]: from each face n geometrically growing panels (smallest 1e-12 of the half-thickness) up to the middle,
    every panel cut so that none is longer than 4 / n mean free paths"""
    half = 0.5 * tau0
    e = half * np.concatenate([[0.0], np.geomspace(1e-12, 1.0, n)])
    hmax = 4.0 / n
    out = [0.0]
    for lo, hi in zip(e[:-1], e[1:]):
        k = int(np.ceil((hi - lo) / hmax))
        out.extend(lo + (hi - lo) * np.arange(1, k + 1) / k)
    e = np.array(out)
    return np.concatenate([e, tau0 - e[-2::-1]])


def slab_nodes(tau0, n, order=8):
    x, w = np.polynomial.legendre.leggauss(order)
    e = _panels(tau0, n)
    h = np.diff(e)
    t = (e[:-1, None] + 0.5 * h[:, None] * (x[None] + 1.0)).ravel()
    return t, (0.5 * h[:, None] * w[None]).ravel()


def slab(a, tau0, n=24):
    """-> R, T, A of the gray slab (see the module's docstring); n: panels per half of the grading (the resolution)"""
    t, w = slab_nodes(tau0, n)
    d = np.abs(t[:, None] - t[None])
    np.fill_diagonal(d, 1.0)
    k = 0.5 * expn(1, d)
    np.fill_diagonal(k, 0.0)
    kw = k * w[None]
    s = 1.0 - 0.5 * expn(2, t) - 0.5 * expn(2, tau0 - t)
    # psi_i = f_i + a [sum_j kw_ij (psi_j - psi_i) + s_i psi_i]
    m = np.eye(len(t)) - a * (kw - np.diag(kw.sum(1)) + np.diag(s))
    psi = np.linalg.solve(m, 2.0 * expn(2, t))
    R = float((w * psi * a * 0.5 * expn(2, t)).sum())
    T = float(2.0 * expn(3, tau0) + (w * psi * a * 0.5 * expn(2, tau0 - t)).sum())
    A = float((1.0 - a) * (w * psi).sum())
    return R, T, A


def chandrasekhar_R(a, n=256, iters=400):
    """the half space's reflectance for cosine-distributed entry: 1 - 2 sqrt(1 - a) int_0^1 H(mu) mu dmu, H from iterating
    1 / H(mu) = sqrt(1 - a) + (a / 2) int_0^1 mu' H(mu') / (mu + mu') dmu' (Chandrasekhar's equation in its contracting form)"""
    x, w = np.polynomial.legendre.leggauss(n)
    mu, w = 0.5 * (x + 1.0), 0.5 * w
    H = np.ones(n)
    for _ in range(iters):
        Hn = 1.0 / (np.sqrt(1.0 - a) + 0.5 * a * ((w * mu * H)[None] / (mu[:, None] + mu[None])).sum(1))
        if np.abs(Hn - H).max() < 1e-15:
            H = Hn
            break
        H = Hn
    return float(1.0 - 2.0 * np.sqrt(1.0 - a) * (w * H * mu).sum())


def slab_mc(a, tau0, n=1000000, seed=1, half_width=None, batches=100):
    """analog Monte Carlo of the slab in float64, three-dimensional: lengths in units of the thickness (sigma_t = tau0), the slab is
    0 <= depth <= 1, walks enter at the lateral origin.  half_width: side walls at |x|, |y| = half_width, a walk that reaches one
    leaves through it.  -> dict(R, T, se_R, se_T, wall, reach): means, standard errors over `batches` batches, the share of walks that left
    through a wall and the largest lateral excursion of any walk"""
    rng = np.random.RandomState(seed)
    mu = np.sqrt(rng.random_sample(n))
    phi = 2.0 * np.pi * rng.random_sample(n)
    st = np.sqrt(1.0 - mu * mu)
    d = np.stack([st * np.cos(phi), st * np.sin(phi), mu], -1)        # z = depth
    pos = np.zeros((n, 3))
    idx = np.arange(n)
    res = np.zeros(n, np.int8)                                        # 1 R, 2 T, 3 wall
    reach = 0.0
    while len(idx):
        s = -np.log(1.0 - rng.random_sample(len(idx))) / tau0
        new = pos + s[:, None] * d
        # the first boundary the segment crosses
        with np.errstate(divide="ignore", invalid="ignore"):
            tz = np.where(d[:, 2] > 0, (1.0 - pos[:, 2]) / d[:, 2], np.where(d[:, 2] < 0, -pos[:, 2] / d[:, 2], np.inf))
            tw = np.full(len(idx), np.inf)
            if half_width is not None:
                for c in (0, 1):
                    tw = np.minimum(tw, np.where(d[:, c] != 0, (half_width * np.sign(d[:, c]) - pos[:, c]) / d[:, c], np.inf))
        out_z, out_w = (tz <= s) & (tz <= tw), (tw <= s) & (tw < tz)
        res[idx[out_z]] = np.where(d[out_z, 2] > 0, 2, 1)
        res[idx[out_w]] = 3
        inside = ~(out_z | out_w)
        reach = max(reach, float(np.abs(new[inside, :2]).max()) if inside.any() else 0.0)
        keep = inside & (rng.random_sample(len(idx)) < a)
        idx, pos = idx[keep], new[keep]
        u = 2.0 * rng.random_sample(len(idx)) - 1.0
        ph = 2.0 * np.pi * rng.random_sample(len(idx))
        sn = np.sqrt(1.0 - u * u)
        d = np.stack([sn * np.cos(ph), sn * np.sin(ph), u], -1)
    b = res.reshape(batches, -1)
    r, t = (b == 1).mean(1), (b == 2).mean(1)
    return dict(R=r.mean(), T=t.mean(), se_R=r.std(ddof=1) / np.sqrt(batches), se_T=t.std(ddof=1) / np.sqrt(batches),
                wall=(res == 3).mean(), reach=reach)


# ------------------------------------------------------------------------------------------------- radiance under a constant sky
# A walk's exit continues as a Lambert surface of weight thr (cycles-principled-shader.cc:197-214): NEE in the EXIT frame, then a
# cosine-distributed direction in the exit frame -- which CyclesPrincipledShader takes to world space with the ENTRY frame (:468-470,
# SURVEY Q21).  A walk that leaves through the face it entered by has the same frame twice and returns thr L (the furnace property of
# tests/_env_analytic.py: w_nee + w_bsdf = 1).  A walk that leaves a slab through the opposite face sends its BSDF ray back INTO the
# slab, where it meets the entry face from behind and dies (the walk refuses a back face, :236-240); only its NEE part arrives:
#     KAPPA = int over the hemisphere of (cos / pi) w_nee dw,  w_nee = p^2 / (p^2 + q^2),  p = 1 / (4 pi),  q = cos / pi
#           = int_0^1 2 mu / (1 + 16 mu^2) dmu = ln(17) / 16.
KAPPA = float(np.log(17.0) / 16.0)


def exit_weights(quirk=True):
    """(weight of R, weight of T) in a one-closure slab's radiance under a constant sky"""
    return (1.0, KAPPA if quirk else 1.0)


def slab_radiance(mat, thickness, L, n=24, plate_depth=None, quirk=True, gray_mean=False, plate_open=False):
    """what a pixel on a wide slab of principled material `mat` (subsurface the only closure) converges to under the constant
    environment L: L thr0 (R + KAPPA T) per channel, tau0 = sigma_t x thickness and a = sigma_s / sigma_t.
    plate_depth: a black plate of another instance inside the slab at that depth ends every walk that meets it (:371-378), so the
    slab is cut there and nothing is transmitted: L thr0 R(a, sigma_t plate_depth).
    plate_open: R + T of the cut slab instead (a plate that passed the walks on).
    quirk=False: the exit ray taken to world space with the exit frame (R + T).  gray_mean: one gray medium of the mean coefficients."""
    m = medium(mat)
    assert m["enable_subsurface"] and not m["enable_diffuse"], "subsurface must be the only diffuse closure"
    sigma_t, sigma_s = m["sigma_t"].astype(np.float32).astype(np.float64), m["sigma_s"].astype(np.float32).astype(np.float64)
    if gray_mean:
        sigma_t, sigma_s = np.full(3, sigma_t.mean()), np.full(3, sigma_s.mean())
    wr, wt = exit_weights(quirk)
    out = np.zeros(3)
    for c in range(3):
        a = sigma_s[c] / sigma_t[c]
        if plate_depth is None:
            R, T, _ = slab(a, sigma_t[c] * thickness, n)
            out[c] = wr * R + wt * T
        else:
            R, T, _ = slab(a, sigma_t[c] * plate_depth, n)
            out[c] = R + T if plate_open else R
    return np.asarray(L, np.float64) * m["thr0"] * out


def radius_for_tau0(A, tau0, thickness, subsurface=1.0):
    """the subsurface_radius parameter that gives optical thickness tau0 across `thickness` for apparent albedo A"""
    A = np.asarray(A, np.float64)
    s = 1.9 - A + 3.5 * (A - 0.8) ** 2
    d = thickness / (np.asarray(tau0, np.float64) * s)                   # sigma_t = 1 / (d s)
    return d * burley_fitting5(A) * 4.0 * np.pi / subsurface
