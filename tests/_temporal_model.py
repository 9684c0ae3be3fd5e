"""A float64 numpy model of pbrhip_render_motion and pbrhip_temporal_accumulate (include/pbrhip.h): the two cameras as
the library derives them (their float32 parameters, bit for bit: the derivation is the host's), the pixel-centre rays in float32 operation
for operation, the inverse projections, X_prev from (slots, ident) and the accumulation in float64, the rounding bounds the GPU tests
assert, and the conditioning check of the accumulation's inputs."""
import numpy as np

F = np.float32
EPS = 2.0 ** -24  # unit roundoff of float32
NONE = 0xFFFFFFFF


# ------------------------------------------------------------------------------------------------ cameras
def user_camera(eye, lookat, up, vfov, W, H):
    """pbrhip.cpp::make_user_camera: the frame in double, rounded once -> dict of float32 values"""
    eye, lookat, up = (np.asarray(v, F).astype(np.float64) for v in (eye, lookat, up))
    f = lookat - eye
    f = f / np.sqrt((f * f).sum())
    r = np.array([f[1] * up[2] - f[2] * up[1], f[2] * up[0] - f[0] * up[2], f[0] * up[1] - f[1] * up[0]])
    r = r / np.sqrt((r * r).sum())
    u = np.array([r[1] * f[2] - r[2] * f[1], r[2] * f[0] - r[0] * f[2], r[0] * f[1] - r[1] * f[0]])
    h = np.tan(np.float64(F(vfov)) * np.pi / 360.0)
    return dict(kind="user", eye=eye.astype(F), f=f.astype(F), r=r.astype(F), u=u.astype(F), h=F(h), ha=F(h * W / H))


def reference_camera(bmin, bmax, W, H):
    """pbrhip.cpp::make_camera: single precision throughout"""
    bmin, bmax = np.asarray(bmin, F), np.asarray(bmax, F)
    if bmax[0] - bmin[0] > bmax[1] - bmin[1]:
        hs = bmax[0] - bmin[0]
        vs = hs * F(H) / F(W)
    else:
        vs = bmax[1] - bmin[1]
        hs = vs * F(W) / F(H)
    half = F(0.5)
    cx, cy = (bmax[0] + bmin[0]) * half, (bmax[1] + bmin[1]) * half
    return dict(kind="reference", org=np.array([cx, cy, bmax[2] + hs * half * np.sqrt(F(3.0))], F), x_corner=F(cx - hs * half),
                y_corner=F(cy + vs * half), z_corner=F(bmax[2]), dx=F(hs / F(W)), dy=F(vs / F(H)))


def _normalize_raw(p):
    inv = F(1.0) / np.sqrt((p[..., 0] * p[..., 0] + p[..., 1] * p[..., 1]) + p[..., 2] * p[..., 2])
    return p * inv[..., None]


def centre_rays(cam, W, H, x=None, y=None):
    """the rays k_motion traces (dcamera_pixel.h with jx = jy = 0.5), float32 operation for operation -> (org, dir) float32 (..., 3)"""
    if x is None:
        y, x = np.mgrid[0:H, 0:W]
    fx, fy = np.asarray(x).astype(F) + F(0.5), np.asarray(y).astype(F) + F(0.5)
    if cam["kind"] == "user":
        sx = (F(2.0) * fx / F(W) - F(1.0)) * cam["ha"]
        sy = (F(1.0) - F(2.0) * fy / F(H)) * cam["h"]
        p = (cam["f"] + sx[..., None] * cam["r"]) + sy[..., None] * cam["u"]
        o = np.broadcast_to(cam["eye"], p.shape)
        return o.astype(F), _normalize_raw(p.astype(F)).astype(F)
    t = np.stack([cam["x_corner"] + cam["dx"] * fx, cam["y_corner"] - cam["dy"] * fy, np.broadcast_to(cam["z_corner"], fx.shape)], -1).astype(F)
    o = np.broadcast_to(cam["org"], t.shape).astype(F)
    return o, _normalize_raw((t - o).astype(F)).astype(F)


def project(cam, X, W, H):
    """the continuous pixel coordinates at which the camera's pinhole sees the points X (..., 3), float64 -> (px, py, dist, front)"""
    X = np.asarray(X, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        if cam["kind"] == "user":
            v = X - cam["eye"].astype(np.float64)
            f, r, u = (cam[k].astype(np.float64) for k in "fru")
            z = v @ f
            px = ((v @ r) / z / np.float64(cam["ha"]) + 1.0) * (0.5 * W)
            py = (1.0 - (v @ u) / z / np.float64(cam["h"])) * (0.5 * H)
            front = z > 0
        else:
            org = cam["org"].astype(np.float64)
            v = X - org
            k = (np.float64(cam["z_corner"]) - org[2]) / v[..., 2]
            px = (org[0] + k * v[..., 0] - np.float64(cam["x_corner"])) / np.float64(cam["dx"])
            py = (np.float64(cam["y_corner"]) - (org[1] + k * v[..., 1])) / np.float64(cam["dy"])
            front = (k > 0) & np.isfinite(k)
    return px, py, np.sqrt((v * v).sum(-1)), front


# ------------------------------------------------------------------------------------------------ motion
def x_prev(slots, shade, ident):
    """the hit's point on the pose `slots` (n, 4, 4) was read at: a triangle's (1 - u - v) v0 + u v1 + v v2, a curve piece's
    a + (4 u - sub) (b - a).  ident (..., 4) uint32 -> (X (..., 3) float64, hit, curve)"""
    ident = np.asarray(ident, np.uint32)
    hit = ident[..., 0] != NONE
    slot = np.where(hit, ident[..., 0], 0)
    u, v = (ident[..., k].view(F).astype(np.float64) for k in (1, 2))
    sl = np.asarray(slots, F)[slot].astype(np.float64)
    curve = (((np.asarray(shade, np.uint32)[slot, 3] >> 24) & 2) != 0) & hit
    tri = (1.0 - u - v)[..., None] * sl[..., 0, :3] + u[..., None] * sl[..., 1, :3] + v[..., None] * sl[..., 2, :3]
    sub = np.asarray(slots, F)[slot][..., 2, 0].view(np.uint32).astype(np.float64)
    cur = sl[..., 0, :3] + (4.0 * u - sub)[..., None] * (sl[..., 1, :3] - sl[..., 0, :3])
    return np.where(curve[..., None], cur, tri), hit, curve


def motion(slots, shade, ident, cam_prev, W, H):
    """pbrhip_render_motion's motion buffer in float64 from the snapshot's slots, the returned ident and the snapshot's camera"""
    X, hit, curve = x_prev(slots, shade, ident)
    px, py, dist, front = project(cam_prev, X, W, H)
    y, x = np.mgrid[0:H, 0:W]
    ok = hit & front
    out = np.stack([px - (x + 0.5), py - (y + 0.5), dist, np.where(curve, 2.0, 1.0)], -1)
    return np.where(ok[..., None], out, 0.0)


def motion_bound(slots, ident, cam_prev, W, H, want):
    """The float32 rounding bounds of (mx, my) in pixels and of z_prev relatively, per pixel, by operation count (u = 2^-24).  With M the
    largest coordinate of the scene and S = M + |eye|: X_prev carries <= 8 u M per component (two roundings in 1 - u - v, three products,
    two sums of terms <= M), v = X_prev - eye <= 9 u S.  A dot product with a unit vector: <= sqrt(3) 9 u S + 3 u |v| =: u T.
    User camera: sx = a / z: u [T (1 + |sx|) / z + |sx|]; px = (sx / ha + 1) W / 2: one division, one sum, one product, two more ulps of
    ha itself (tan may differ in its last bit between two libms), then the subtraction of the pixel centre:
      d(mx) <= u {(W / 2 ha) [T (1 + |sx|) / z + 5 |sx|] + W / 2 + |px| + |mx|}
    Reference camera: k = (z_corner - org.z) / v.z: relative 9 u S / |v.z| + 2 u; t = org + k v, (t - corner) / dx:
      d(mx) <= u {[9 |k| S + |k v.x| (9 S / |v.z| + 3) + |t| + |t - corner|] / dx + |px| + |mx|}
    z_prev = sqrt(v . v): relative u (16 S / |v| + 4)."""
    sl = np.asarray(slots, F).astype(np.float64)
    M = np.abs(sl[:, :3, :3]).max()
    mx, my, R = want[..., 0], want[..., 1], np.maximum(want[..., 2], 1e-30)
    y, x = np.mgrid[0:H, 0:W]
    px, py = mx + x + 0.5, my + y + 0.5
    if cam_prev["kind"] == "user":
        S = M + np.abs(cam_prev["eye"]).max()
        T = 16.0 * S + 3.0 * R
        ha, h = float(cam_prev["ha"]), float(cam_prev["h"])
        sx, sy = (px / (0.5 * W) - 1.0) * ha, (1.0 - py / (0.5 * H)) * h
        z = R / np.sqrt(1.0 + sx * sx + sy * sy)
        bx = EPS * ((0.5 * W / ha) * (T * (1 + np.abs(sx)) / z + 5 * np.abs(sx)) + 0.5 * W + np.abs(px) + np.abs(mx))
        by = EPS * ((0.5 * H / h) * (T * (1 + np.abs(sy)) / z + 5 * np.abs(sy)) + 0.5 * H + np.abs(py) + np.abs(my))
    else:
        org = cam_prev["org"].astype(np.float64)
        S = M + np.abs(org).max()
        dx, dy, xc, yc = (float(cam_prev[k]) for k in ("dx", "dy", "x_corner", "y_corner"))
        tx, ty = xc + dx * px, yc - dy * py
        depth = abs(float(cam_prev["z_corner"]) - org[2])
        k = np.sqrt((tx - org[0]) ** 2 + (ty - org[1]) ** 2 + depth ** 2) / R  # |t - org| / |v|
        vz = depth / k
        bx = EPS * ((9 * k * S + np.abs(tx - org[0]) * (9 * S / vz + 3) + np.abs(tx) + np.abs(tx - xc)) / dx + np.abs(px) + np.abs(mx))
        by = EPS * ((9 * k * S + np.abs(ty - org[1]) * (9 * S / vz + 3) + np.abs(ty) + np.abs(ty - yc)) / dy + np.abs(py) + np.abs(my))
    return bx, by, EPS * (16.0 * S / R + 4.0)


# ------------------------------------------------------------------------------------------------ accumulation
def _taps(motion, W, H):
    y, x = np.mgrid[0:H, 0:W]
    qx, qy = x + motion[..., 0].astype(np.float64), y + motion[..., 1].astype(np.float64)
    x0, y0 = np.floor(qx), np.floor(qy)
    return qx - x0, qy - y0, x0, y0


def accumulate(rgba, count, motion, guide, hist_rgba, hist_guide, alpha_min, sigma_depth, normal_cos_min, max_history, margins=None, bound=None):
    """pbrhip_temporal_accumulate in float64 (the parameters as the float32 values the library receives).  margins: a list that receives
    how close the inputs come to a decision threshold (conditioned() reads it).  bound: a list that receives the (H, W, 4) float32
    rounding bound of the result (u = 2^-24).  The blend is a convex combination, so rounding is not amplified -- but for the one
    place where float32 loses ABSOLUTE accuracy: q = x + m is rounded to u |q|, which moves the fractional part f by that much, a weight
    by d(w) <= 3 u w + u |q.x| w_y + u |q.y| w_x, and the normalised weights by D = sum d(w) / S.  Hence
      d(h) <= D range(hist) + 8 u max|hist|, d(n) <= D max_history + 8 u max_history, d(len) <= d(n) + u len,
      d(a) <= d(len) / len^2 + u a, d(out.rgb) <= d(h) + d(a) |c - h| + 4 u (|h| + |c|)."""
    rgba, motion, guide = (np.asarray(a, F).astype(np.float64) for a in (rgba, motion, guide))
    count = np.asarray(count, np.uint32)
    H, W = count.shape
    alpha_min, sigma_depth, normal_cos_min = (np.float64(F(a)) for a in (alpha_min, sigma_depth, normal_cos_min))
    c = np.where(count[..., None] > 0, rgba[..., :3] / np.maximum(count, 1)[..., None], 0.0)
    out = np.concatenate([c, (count > 0)[..., None].astype(np.float64)], -1)
    if hist_rgba is None:
        return out
    hr, hg = np.asarray(hist_rgba, F).astype(np.float64), np.asarray(hist_guide, F).astype(np.float64)
    fx, fy, x0, y0 = _taps(motion, W, H)
    valid, curve, z = (motion[..., 3] != 0) & (count > 0), motion[..., 3] == 2, motion[..., 2]
    S, acc, dw = np.zeros((H, W)), np.zeros((H, W, 4)), np.zeros((H, W))
    yy, xx = np.mgrid[0:H, 0:W]
    dfx, dfy = EPS * np.abs(xx + motion[..., 0]), EPS * np.abs(yy + motion[..., 1])
    for t in range(4):
        i, j = t & 1, t >> 1
        tx, ty = x0 + i, y0 + j
        inside = (tx >= 0) & (ty >= 0) & (tx < W) & (ty < H) & np.isfinite(tx) & np.isfinite(ty)
        ix, iy = np.where(inside, tx, 0).astype(np.int64), np.where(inside, ty, 0).astype(np.int64)
        Hq, Gq = hr[iy, ix], hg[iy, ix]
        nd = (Gq[..., :3] * guide[..., :3]).sum(-1)
        nd = np.where(curve, np.abs(nd), nd)
        live = inside & valid & (Hq[..., 3] > 0) & (Gq[..., 3] > 0)
        dz, lim = np.abs(Gq[..., 3] - z), sigma_depth * z
        ok = live & (dz <= lim) & (nd >= normal_cos_min)
        if margins is not None:
            margins.append(np.where(live, np.abs(dz - lim) / np.maximum(np.abs(lim), 1e-30), np.inf).min())
            margins.append(np.where(live, np.abs(nd - normal_cos_min), np.inf).min())
        wx, wy = np.where(i, fx, 1 - fx), np.where(j, fy, 1 - fy)
        w = np.where(ok, wx * wy, 0.0)
        dw += np.where(ok, 3 * EPS * wx * wy + dfx * wy + dfy * wx, 0.0)
        S += w
        acc += w[..., None] * Hq
    use = S > 0
    Sd = np.where(use, S, 1.0)
    h, n = acc[..., :3] / Sd[..., None], acc[..., 3] / Sd
    ln = np.minimum(n + 1.0, float(max_history))
    a = np.maximum(1.0 / ln, alpha_min)
    blend = np.concatenate([h + a[..., None] * (c - h), ln[..., None]], -1)
    if margins is not None:
        frac = np.concatenate([fx[valid], 1 - fx[valid], fy[valid], 1 - fy[valid]]) if valid.any() else np.array([1.0])
        margins.append(("frac", frac.min()))
    if bound is not None:
        D = dw / Sd
        hmax = np.abs(hr[..., :3]).max()
        d_h = D * (hr[..., :3].max() - hr[..., :3].min()) + 8 * EPS * hmax
        d_len = D * max_history + 8 * EPS * max_history + EPS * ln
        d_a = d_len / (ln * ln) + EPS * a
        d_rgb = d_h[..., None] + d_a[..., None] * np.abs(c - h) + 4 * EPS * (np.abs(h) + np.abs(c))
        plain = np.concatenate([EPS * np.abs(c), np.zeros((H, W, 1))], -1)  # (c, 1): one division
        bound.append(np.where(use[..., None], np.concatenate([d_rgb, d_len[..., None]], -1), plain))
    return np.where(use[..., None], blend, out)


def conditioned(margins):
    """no tap within 1e-4 (relative for the depth, absolute for the cosine, which is of order 1) of a threshold, no fractional part of q
    within 1e-3 of 0 or 1: float32 and float64 then take the same decisions"""
    fr = [m[1] for m in margins if isinstance(m, tuple)]
    th = [m for m in margins if not isinstance(m, tuple)]
    return min(th, default=np.inf) > 1e-4 and min(fr, default=1.0) > 1e-3
