"""A float64 numpy model of pbrhip_scene_object_ids, pbrhip_svgf_accumulate and pbrhip_svgf_filter (include/pbrhip.h): the
definitions restated tap by tap, the parameters read as the float32 values the library receives, the rounding bounds the GPU tests
assert, and the conditioning check of the inputs.  It shares no code with the library; the taps of the accumulation are
_temporal_model's (the header defines them as pbrhip_temporal_accumulate's).

The bounds are first order in u = 2^-24, by operation count; where a bound multiplies a weight's error into a difference of colours the
factor 1.01 stands for the second-order terms, which are u times smaller.  What enters:

  accumulation   e = (rgb / count) / max(a, 1e-3): four roundings, d(e) <= 5 u |e| (the albedo carries two of them); the blend is
                 _temporal_model.accumulate's with e for c (a convex combination; the absolute error of q = x + m moves the bilinear
                 weights by D): d(h), d(len), d(al) as there.  lum is three products and two sums of one sign: d(lum x) <= d(x) + 4 u lum|x|.
                 d = l - lum(h): d(d) <= d(l) + d(lum h) + u |d|.  out_var = (1 - al) (v + (al d) d):
                   d(var) <= (d(al) + u) (v + al d^2) + (1 - al) [d(v) + d(al) d^2 + al (2 |d| + d(d)) d(d) + 3 u (v + al d^2)] + u var
                 (the square keeps its second-order term: where d = 0 it is all there is)
                 with d(v) <= D range(hist_var) + 8 u max(hist_var), like d(h).
  filter, per    gv is a convex combination of nine v: d(gv) <= max d(v_q) + 16 u gv; |sqrt a - sqrt b| <= min(|a - b| / 2 sqrt(min), sqrt|a - b|);
  iteration      S = sigma_lum sqrt(gv) + eps: d(S) <= sigma_lum d(sqrt) + 2 u S.  x_l = |l_p - l_q| / S carries the relative error of S -- and
                 so that of v from the iteration before -- and the absolute errors of both l: d(x_l) <= (d(l_p) + d(l_q) + u |l_p - l_q|) / S
                 + x_l d(S) / S + u x_l.  x_z is five roundings of exact inputs: 6 u x_z.  exp(-x) moves by e^-x (d(x) + 2 u) = x e^-x times
                 the relative error of x, plus the library's own 2 u.  N_p . N_q carries 4 u sum|N_p N_q| absolutely; every squaring doubles
                 its relative error: the bound evaluates (dot +- that)^(2^k) directly and adds 2^k u.  A tap weight is those factors
                 times h (exact) with two more roundings.  The convex combination e_p + sum hw (e_q - e_p) / sum hw passes the inputs'
                 errors through with the weights, turns d(hw) into sum d(hw) |e_q - out| / sum hw, and rounds 64 u of the weighted range
                 (25 differences, products and two sums of 25 terms, a division) + 2 u |out|.  v' = sum hw^2 v_q / (sum hw)^2:
                   d(v') <= sum hw^2 d(v_q) / W^2 + [sum 2 hw d(hw) v_q / W^2 + 2 v' sum d(hw) / W] + 96 u v',  W = sum hw.
  variance in    len < 4: the same weights without x_l over 48 taps; m and sigma2 are convex combinations in the difference form:
                 d(m) <= sum g d(l_q) / G + sum d(g) |l_q - m| / G + 110 u sum g |l_q - l_p| / G + 2 u |m|,
                 d(sigma2) <= sum g (2 |l_q - m| + t) t / G with t = d(l_q) + d(m) + sum d(g) |(l_q - m)^2 - sigma2| / G + 110 u sigma2; v0 = sigma2 4 / len: + 2 u v0.
  output         e max(a, 1e-3): d <= d(e) a + 4 u |out|.

Decisions.  The accumulation's thresholds are pbrhip_temporal_accumulate's and are reported in `margins` as there.  The id test
(equality of integers), the background test (guide.w == 0 on an input) and liveness (illum.w > 0 on an input) are exact on both sides and need
no margin.  len >= 4 is exact when the length is a whole number; a length that came out of a float32 blend is only safe away from 4:
the filter reports ("len", the distance of the nearest non-integer length to 4)."""
import numpy as np

import _temporal_model as TM

F = np.float32
EPS = TM.EPS
NONE = TM.NONE
ID_PRIMITIVE, ID_INSTANCE, ID_GEOM = 0, 1, 2
ITERATIONS, NORMAL_SQUARINGS, SIGMA_LUM, SIGMA_DEPTH = 5, 7, 1.0, 0.2  # the header's defaults
LUM_EPS = np.float64(F(1e-4))
ALBEDO_MIN = np.float64(F(1e-3))
LUM = np.array([0.2126, 0.7152, 0.0722], F).astype(np.float64)  # the kernel's float32 constants
B3 = np.array([1.0, 4.0, 6.0, 4.0, 1.0]) / 16.0
ORDER2 = 1.01


def lum(e):
    return e[..., 0] * LUM[0] + e[..., 1] * LUM[1] + e[..., 2] * LUM[2]


def object_ids(shade, ident, what):
    """ids[p] = word 24 + what of the ShadeRec of slot ident[p, 0]; NONE for a miss or a slot the scene does not have"""
    shade, slot = np.asarray(shade, np.uint32), np.asarray(ident, np.uint32)[..., 0]
    ok = slot < len(shade)
    return np.where(ok, shade[np.where(ok, slot, 0), 24 + what], NONE).astype(np.uint32)


def albedo(albedo_hits, feature_count, shape):
    """max(a, 1e-3) (H, W, 3): a = (albedo_hits.rgb + misses) / feature_count, 1 where feature_count == 0 or without the buffers"""
    if albedo_hits is None:
        return np.ones(tuple(shape) + (3,))
    ah, m = np.asarray(albedo_hits, F).astype(np.float64), np.asarray(feature_count).astype(np.float64)
    has = m > 0
    a = np.where(has[..., None], (ah[..., :3] + (m - ah[..., 3])[..., None]) / np.where(has, m, 1)[..., None], 1.0)
    return np.maximum(a, ALBEDO_MIN)


# ------------------------------------------------------------------------------------------------ accumulation
def accumulate(rgba, count, motion, guide, hist_illum, hist_var, hist_guide, alpha_min, sigma_depth, normal_cos_min, max_history,
               albedo_hits=None, feature_count=None, ids=None, hist_ids=None, margins=None, bound=None):
    """-> (out_illum (H, W, 4), out_var (H, W)) float64.  margins: as _temporal_model.accumulate's.  bound: a list that receives
    (bound of out_illum (H, W, 4), bound of out_var (H, W))."""
    rgba, motion, guide = (np.asarray(a, F).astype(np.float64) for a in (rgba, motion, guide))
    count = np.asarray(count, np.uint32)
    H, W = count.shape
    alpha_min, sigma_depth, normal_cos_min = (np.float64(F(a)) for a in (alpha_min, sigma_depth, normal_cos_min))
    some = count > 0
    a = albedo(albedo_hits, feature_count, (H, W))
    c = np.where(some[..., None], rgba[..., :3] / np.maximum(count, 1)[..., None], 0.0)
    e = c / a
    plain = np.concatenate([e, some[..., None].astype(np.float64)], -1)
    b_plain = np.concatenate([5 * EPS * np.abs(e), np.zeros((H, W, 1))], -1)
    if hist_illum is None:
        if bound is not None:
            bound.append((b_plain, np.zeros((H, W))))
        return plain, np.zeros((H, W))
    hi, hv, hg = (np.asarray(x, F).astype(np.float64) for x in (hist_illum, hist_var, hist_guide))
    fx, fy, x0, y0 = TM._taps(motion, W, H)
    valid, curve, z = (motion[..., 3] != 0) & some, motion[..., 3] == 2, motion[..., 2]
    S, acc, accv, dw = np.zeros((H, W)), np.zeros((H, W, 4)), np.zeros((H, W)), np.zeros((H, W))
    yy, xx = np.mgrid[0:H, 0:W]
    dfx, dfy = EPS * np.abs(xx + motion[..., 0]), EPS * np.abs(yy + motion[..., 1])
    for t in range(4):
        i, j = t & 1, t >> 1
        tx, ty = x0 + i, y0 + j
        inside = (tx >= 0) & (ty >= 0) & (tx < W) & (ty < H) & np.isfinite(tx) & np.isfinite(ty)
        ix, iy = np.where(inside, tx, 0).astype(np.int64), np.where(inside, ty, 0).astype(np.int64)
        Hq, Gq, Vq = hi[iy, ix], hg[iy, ix], hv[iy, ix]
        nd = (Gq[..., :3] * guide[..., :3]).sum(-1)
        nd = np.where(curve, np.abs(nd), nd)
        live = inside & valid & (Hq[..., 3] > 0) & (Gq[..., 3] > 0)
        dz, lim = np.abs(Gq[..., 3] - z), sigma_depth * z
        ok = live & (dz <= lim) & (nd >= normal_cos_min)
        if margins is not None:
            margins.append(np.where(live, np.abs(dz - lim) / np.maximum(np.abs(lim), 1e-30), np.inf).min())
            margins.append(np.where(live, np.abs(nd - normal_cos_min), np.inf).min())
        if ids is not None:
            ok &= np.asarray(hist_ids, np.uint32)[iy, ix] == np.asarray(ids, np.uint32)  # integers: exact on both sides
        wx, wy = np.where(i, fx, 1 - fx), np.where(j, fy, 1 - fy)
        w = np.where(ok, wx * wy, 0.0)
        dw += np.where(ok, 3 * EPS * wx * wy + dfx * wy + dfy * wx, 0.0)
        S += w
        acc += w[..., None] * Hq
        accv += w * Vq
    use = S > 0
    Sd = np.where(use, S, 1.0)
    h, n, v = acc[..., :3] / Sd[..., None], acc[..., 3] / Sd, accv / Sd
    ln = np.minimum(n + 1.0, float(max_history))
    al = np.maximum(1.0 / ln, alpha_min)
    l, lh = lum(e), lum(h)
    d = l - lh
    blend = np.concatenate([h + al[..., None] * (e - h), ln[..., None]], -1)
    var = (1.0 - al) * (v + al * d * d)
    if margins is not None:
        frac = np.concatenate([fx[valid], 1 - fx[valid], fy[valid], 1 - fy[valid]]) if valid.any() else np.array([1.0])
        margins.append(("frac", frac.min()))
    if bound is not None:
        D = dw / Sd
        d_h = D * (hi[..., :3].max() - hi[..., :3].min()) + 8 * EPS * np.abs(hi[..., :3]).max()
        d_v = D * (hv.max() - hv.min()) + 8 * EPS * np.abs(hv).max()
        d_len = D * max_history + 8 * EPS * max_history + EPS * ln
        d_al = d_len / (ln * ln) + EPS * al
        d_e = 5 * EPS * np.abs(e)
        d_rgb = d_h[..., None] + d_al[..., None] * np.abs(e - h) + 4 * EPS * (np.abs(h) + np.abs(e)) + d_e
        d_d = (d_e.max(-1) + 4 * EPS * lum(np.abs(e))) + (d_h + 4 * EPS * lum(np.abs(h))) + EPS * np.abs(d)
        inner = v + al * d * d
        d_var = (d_al + EPS) * inner + (1 - al) * (d_v + d_al * d * d + al * (2 * np.abs(d) + d_d) * d_d + 3 * EPS * inner) + EPS * var
        bound.append((np.where(use[..., None], np.concatenate([d_rgb, d_len[..., None]], -1), b_plain), np.where(use, d_var, 0.0)))
    return np.where(use[..., None], blend, plain), np.where(use, var, 0.0)


def conditioned(margins):
    """_temporal_model.conditioned's thresholds (1e-4 of a decision threshold, 1e-3 for a fractional part of q), and no non-integer length
    within 1e-3 of 4"""
    return TM.conditioned(margins)


# ------------------------------------------------------------------------------------------------ filter
def _shift(a, dy, dx, fill=0.0):
    """a at q = p + (dx, dy), `fill` outside; and the mask of the q inside the image"""
    H, W = a.shape[:2]
    ys, xs = np.mgrid[0:H, 0:W]
    qy, qx = ys + dy, xs + dx
    inside = (qy >= 0) & (qy < H) & (qx >= 0) & (qx < W)
    out = a[np.clip(qy, 0, H - 1), np.clip(qx, 0, W - 1)]
    return np.where(inside.reshape(inside.shape + (1,) * (a.ndim - 2)), out, fill), inside


def _pair(live, guide, ids, dy, dx, s, sigma_depth, nsq):
    """the tap q = p + s (dx, dy): exists (live, inside, the same side of the background, the same id), w_n with its error, x_z"""
    N, z = guide[..., :3], guide[..., 3]
    lq, inside = _shift(live, s * dy, s * dx, False)
    gq = _shift(guide, s * dy, s * dx)[0]
    bg_p, bg_q = z == 0, gq[..., 3] == 0
    exists = live & inside & lq & (bg_p == bg_q)
    if ids is not None:
        exists &= _shift(ids, s * dy, s * dx, 0)[0] == ids
    terms = N * gq[..., :3]
    dot, ddot = terms.sum(-1), 4 * EPS * np.abs(terms).sum(-1)
    k = 2.0 ** nsq
    wn, hi, lo = (np.maximum(0.0, x) ** k for x in (dot, dot + ddot, dot - ddot))
    dwn = np.maximum(hi - wn, wn - lo) + k * EPS * hi
    xz = np.zeros_like(z)
    if sigma_depth > 0:
        dz = np.abs(z - gq[..., 3])
        with np.errstate(divide="ignore", invalid="ignore"):
            xz = np.where((dz == 0) | bg_p, 0.0, dz / ((sigma_depth * z * s) * np.sqrt(float(dx * dx + dy * dy))))
    surf = exists & ~bg_p
    return exists, np.where(surf, wn, 1.0), np.where(surf, dwn, 0.0), np.where(surf, xz, 0.0)


def _weight(exists, wn, dwn, xz, xl, dxl):
    """g = w_n exp(-(x_z + x_l)) and its error bound; 0 where the tap does not exist"""
    arg = xz + xl
    E = np.exp(-arg)
    dE = E * (np.expm1(6 * EPS * xz + dxl + EPS * arg) + 2 * EPS)
    g = wn * E
    return np.where(exists, g, 0.0), np.where(exists, dwn * E + wn * dE + 2 * EPS * g, 0.0)


def variance_in(illum, var, guide, ids, sigma_depth, nsq):
    """v(0) and its error bound: var where len >= 4 (a negative one reads as 0), else the 7 x 7 estimate; 0 where not live"""
    live, ln = illum[..., 3] > 0, illum[..., 3]
    l, L = lum(illum[..., :3]), lum(np.abs(illum[..., :3]))
    dl = 4 * EPS * L
    taps = []
    for dy in range(-3, 4):
        for dx in range(-3, 4):
            if dx or dy:
                ex, wn, dwn, xz = _pair(live, guide, ids, dy, dx, 1, sigma_depth, nsq)
                g, dg = _weight(ex, wn, dwn, xz, 0.0, 0.0)
                taps.append((g, dg, _shift(l, dy, dx)[0], _shift(dl, dy, dx)[0]))
    G = 1.0 + sum(t[0] for t in taps)
    m = l + sum(g * (lq - l) for g, _, lq, _ in taps) / G
    dm = ((dl + sum(g * dlq for g, _, _, dlq in taps)) + ORDER2 * sum(dg * np.abs(lq - m) for _, dg, lq, _ in taps)
          + 110 * EPS * sum(g * np.abs(lq - l) for g, _, lq, _ in taps)) / G + 2 * EPS * np.abs(m)
    s2 = ((l - m) ** 2 + sum(g * (lq - m) ** 2 for g, _, lq, _ in taps)) / G
    ds2 = (((2 * np.abs(l - m) + dl + dm) * (dl + dm) + sum(g * (2 * np.abs(lq - m) + dlq + dm) * (dlq + dm) for g, _, lq, dlq in taps))
           + ORDER2 * sum(dg * np.abs((lq - m) ** 2 - s2) for _, dg, lq, _ in taps)) / G + 110 * EPS * s2
    lnd = np.where(live, ln, 1.0)
    young = live & (ln < 4)
    v0 = np.where(young, s2 * 4.0 / lnd, np.maximum(var, 0.0))
    dv0 = np.where(young, ds2 * 4.0 / lnd + 2 * EPS * v0, 0.0)
    return np.where(live, v0, 0.0), np.where(live, dv0, 0.0)


def iterate(e, v, de, dv, live, guide, ids, i, sigma_lum, sigma_depth, nsq):
    """one A-trous iteration with step 2^i -> e', v' and their error bounds (de, dv: (H, W), the inputs' bounds; de over the channels)"""
    s = 1 << i
    l = lum(e)
    dl = de + 4 * EPS * lum(np.abs(e))
    gs, gw, dgv = np.zeros_like(v), np.zeros_like(v), np.zeros_like(v)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            k = (2 - abs(dx)) * (2 - abs(dy))
            ok = live & _shift(live, dy, dx, False)[0]
            gs += np.where(ok, k * _shift(v, dy, dx)[0], 0.0)
            gw += np.where(ok, k, 0.0)
            dgv = np.maximum(dgv, np.where(ok, _shift(dv, dy, dx)[0], 0.0))
    gv = gs / np.where(live, gw, 1.0)
    dgv = dgv + 16 * EPS * gv
    sq = np.sqrt(gv)
    dsq = np.minimum(dgv / (2 * np.sqrt(np.maximum(gv - dgv, 1e-300))), np.sqrt(dgv)) + EPS * sq
    S = sigma_lum * sq + LUM_EPS
    dS = abs(sigma_lum) * dsq + 2 * EPS * S
    h0 = B3[2] * B3[2]
    sw, num, sv = np.full(v.shape, h0), np.zeros_like(e), h0 * h0 * v
    a_in, a_dw, a_rng, v_in, v_dw = h0 * de, np.zeros_like(v), np.zeros_like(v), h0 * h0 * dv, np.zeros_like(v)
    taps = []
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            if not (dx or dy):
                continue
            ex, wn, dwn, xz = _pair(live, guide, ids, dy, dx, s, sigma_depth, nsq)
            eq, vq = _shift(e, s * dy, s * dx)[0], _shift(v, s * dy, s * dx)[0]
            xl = dxl = 0.0
            if sigma_lum > 0:
                adl = np.abs(l - _shift(l, s * dy, s * dx)[0])
                xl = adl / S
                dxl = (dl + _shift(dl, s * dy, s * dx)[0] + EPS * adl) / (S - dS) + xl * dS / (S - dS) + EPS * xl
            g, dg = _weight(ex, wn, dwn, xz, xl, dxl)
            hh = B3[dx + 2] * B3[dy + 2]
            w, dw = g * hh, dg * hh + EPS * g * hh
            sw += w
            num += w[..., None] * (eq - e)
            sv += w * w * vq
            a_in += w * _shift(de, s * dy, s * dx)[0]
            a_rng += w * np.abs(eq - e).max(-1)
            v_in += w * w * _shift(dv, s * dy, s * dx)[0]
            v_dw += 2 * w * dw * vq
            taps.append((dw, eq))
    out = e + num / sw[..., None]
    sdw = sum(dw for dw, _ in taps)
    a_dw = sum(dw * np.abs(eq - out).max(-1) for dw, eq in taps)  # (the centre's weight 1 h is exact)
    de_out = (a_in + ORDER2 * a_dw + 64 * EPS * a_rng) / sw + 2 * EPS * np.abs(out).max(-1)
    v_out = sv / (sw * sw)
    dv_out = v_in / (sw * sw) + ORDER2 * (v_dw / (sw * sw) + 2 * v_out * sdw / sw) + 96 * EPS * v_out
    z = lambda x: np.where(live.reshape(live.shape + (1,) * (x.ndim - 2)), x, 0.0)  # noqa: E731
    return z(out), z(v_out), z(de_out), z(dv_out)


def filter(illum, var, guide, ids=None, albedo_hits=None, feature_count=None, iterations=0, sigma_lum=SIGMA_LUM, sigma_depth=SIGMA_DEPTH,
           normal_squarings=NORMAL_SQUARINGS, margins=None, bound=None):
    """-> (out_rgba, out_feedback) (H, W, 4) float64.  bound: a list that receives the two (H, W, 4) bounds."""
    illum, var, guide = (np.asarray(x, F).astype(np.float64) for x in (illum, var, guide))
    ids = None if ids is None else np.asarray(ids, np.uint32)
    sigma_lum, sigma_depth = np.float64(F(sigma_lum)), np.float64(F(sigma_depth))
    H, W = var.shape
    live, ln = illum[..., 3] > 0, illum[..., 3]
    if margins is not None:
        odd = live & (ln != np.round(ln))
        margins.append(("len", np.where(odd, np.abs(ln - 4.0), np.inf).min()))
    e = np.where(live[..., None], illum[..., :3], 0.0)
    v, dv = variance_in(illum, var, guide, ids, sigma_depth, normal_squarings)
    de = np.zeros((H, W))
    fb = db = None
    for i in range(iterations or ITERATIONS):
        e, v, de, dv = iterate(e, v, de, dv, live, guide, ids, i, sigma_lum, sigma_depth, normal_squarings)
        if i == 0:
            fb = np.concatenate([e, np.where(live, ln, 0.0)[..., None]], -1)
            db = np.concatenate([np.repeat(de[..., None], 3, -1), np.zeros((H, W, 1))], -1)
    a = albedo(albedo_hits, feature_count, (H, W))
    out = np.concatenate([np.where(live[..., None], e * a, 0.0), live[..., None].astype(np.float64)], -1)
    if bound is not None:
        bound.append((np.concatenate([de[..., None] * a + 4 * EPS * np.abs(out[..., :3]), np.zeros((H, W, 1))], -1), db))
    return out, fb
