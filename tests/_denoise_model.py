"""float64 numpy model of pbrhip_denoise (include/pbrhip.h): the edge-avoiding A-trous filter on albedo-demodulated
colour.  It restates the specification, tap by tap, and shares no code with the library."""
import numpy as np

ITERATIONS, NORMAL_SQUARINGS = 5, 7
B3 = np.array([1.0, 4.0, 6.0, 4.0, 1.0]) / 16.0


def prepare(rgba, count, albedo_hits=None, normal_depth=None, feature_count=None, albedo=True):
    """-> e0 (H, W, 3), a (H, W, 3) unclamped albedo, valid (H, W), surface (H, W), N (H, W, 3), z (H, W)"""
    rgba = np.asarray(rgba, np.float64)
    n = np.asarray(count).astype(np.float64)
    H, W = n.shape
    valid = n > 0
    c = np.where(valid[..., None], rgba[..., :3] / np.where(valid, n, 1)[..., None], 0.0)
    a = np.ones((H, W, 3))
    surface = np.zeros((H, W), bool)
    N = np.zeros((H, W, 3))
    z = np.zeros((H, W))
    if albedo_hits is not None:
        ah, nd = np.asarray(albedo_hits, np.float64), np.asarray(normal_depth, np.float64)
        m = np.asarray(feature_count).astype(np.float64)
        k = ah[..., 3]
        if albedo:
            has = m > 0
            a = np.where(has[..., None], (ah[..., :3] + (m - k)[..., None]) / np.where(has, m, 1)[..., None], 1.0)
        ln = np.sqrt((nd[..., :3] ** 2).sum(-1))
        surface = (k > 0) & (ln > 0)
        N = np.where(surface[..., None], nd[..., :3] / np.where(ln > 0, ln, 1)[..., None], 0.0)
        z = np.where(surface, nd[..., 3] / np.where(k > 0, k, 1), 0.0)
    e0 = c / np.maximum(a, 1e-3)
    return e0, a, valid, surface, N, z


def weights(e, valid, surface, N, z, i, dx, dy, sigma_color, sigma_depth, normal_squarings):
    """w(p, q) for the tap q = p + 2^i (dx, dy) of every pixel p, and the mask of the taps that exist: (H, W) each.  (dx, dy) != (0, 0)."""
    H, W = valid.shape
    s = 1 << i
    ys, xs = np.mgrid[0:H, 0:W]
    qy, qx = ys + s * dy, xs + s * dx
    inside = (qy >= 0) & (qy < H) & (qx >= 0) & (qx < W)
    qy, qx = np.clip(qy, 0, H - 1), np.clip(qx, 0, W - 1)
    exists = inside & valid[qy, qx]
    sp, sq = surface, surface[qy, qx]
    wn = np.maximum(0.0, (N * N[qy, qx]).sum(-1))
    for _ in range(normal_squarings):
        wn = wn * wn
    wn = np.where(sp & sq, wn, np.where(sp == sq, 1.0, 0.0))  # both background: 1; exactly one: 0
    wz = np.ones((H, W))
    if sigma_depth > 0:
        dz = np.abs(z - z[qy, qx])
        with np.errstate(divide="ignore", invalid="ignore"):
            x = np.where(dz == 0, 0.0, dz / (sigma_depth * z * (s * np.hypot(dx, dy))))
        wz = np.where(sp & sq, np.exp(-x), 1.0)
    wc = np.ones((H, W))
    if sigma_color > 0:
        d2 = ((e - e[qy, qx]) ** 2).sum(-1)
        with np.errstate(divide="ignore", invalid="ignore"):
            wc = np.exp(-np.where(d2 == 0, 0.0, d2 / (sigma_color * 2.0 ** -i) ** 2))
    return wn * wz * wc, exists, qy, qx


def iterate(e, valid, surface, N, z, i, sigma_color, sigma_depth, normal_squarings):
    num = np.zeros_like(e)
    den = np.zeros(valid.shape)
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            h = B3[dx + 2] * B3[dy + 2]
            if dx == 0 and dy == 0:
                num += h * e
                den += h
                continue
            w, exists, qy, qx = weights(e, valid, surface, N, z, i, dx, dy, sigma_color, sigma_depth, normal_squarings)
            w = np.where(exists, w, 0.0) * h
            num += w[..., None] * e[qy, qx]
            den += w
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(valid[..., None], num / den[..., None], 0.0)


def denoise(rgba, count, albedo_hits=None, normal_depth=None, feature_count=None, iterations=0, sigma_color=0.0, sigma_depth=0.0,
            normal_squarings=NORMAL_SQUARINGS, albedo=True):
    """-> (H, W, 4) float64: the denoised mean colour | 1, (0, 0, 0, 0) where count == 0.  A non-positive sigma switches its weight off."""
    e, a, valid, surface, N, z = prepare(rgba, count, albedo_hits, normal_depth, feature_count, albedo)
    for i in range(iterations or ITERATIONS):
        e = iterate(e, valid, surface, N, z, i, sigma_color, sigma_depth, normal_squarings)
    out = np.zeros(e.shape[:2] + (4,))
    out[..., :3] = np.where(valid[..., None], e * a, 0.0)
    out[..., 3] = valid
    return out
