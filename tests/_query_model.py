"""The nearest-point contract of DESIGN.md §19 in numpy float32, operation for operation as pbrlab_amd/csrc/query.hip evaluates it
(every operation rounded once, no contraction), a brute force over all slots of a committed scene, and a float64 evaluation of the same
distance.  Arrays broadcast: p (..., 3) against primitives (..., 3)."""
import numpy as np

F = np.float32
NONE = 0xFFFFFFFF
SLOT_IS_CURVE = 2  # kSlotIsCurve (dscene.h), in the top byte of ShadeRec word 3


def dot(a, b):
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def vbox_lo(v):
    """dtrace.h::vbox_lo: fma(-|v|, 2^-17, v) - 1e-31f (the product with a power of two is exact, so the float64 sum rounded once is the fma)"""
    v64 = v.astype(np.float64)
    return (v64 - np.abs(v64) * 2.0 ** -17).astype(F) - F(1e-31)


def vbox_hi(v):
    v64 = v.astype(np.float64)
    return (v64 + np.abs(v64) * 2.0 ** -17).astype(F) + F(1e-31)


def box_dist2(lo, hi, p):
    """squared distance from p to [lo, hi]: per axis max(max(lo - p, p - hi), 0), summed as dot sums"""
    m = np.fmax(np.fmax(lo - p, p - hi), F(0))
    return m[..., 0] * m[..., 0] + m[..., 1] * m[..., 1] + m[..., 2] * m[..., 2]


def own_box_dist2(lo, hi, p):
    return box_dist2(vbox_lo(lo), vbox_hi(hi), p)


def seg_dist2(p, x, y):
    """-> (d2, t, q): t = clamp(dot(p - x, e) / dot(e, e), 0, 1), 0 when dot(e, e) is not > 0; q = x + t e"""
    e = y - x
    ee = dot(e, e)
    with np.errstate(all="ignore"):
        t = np.fmin(np.fmax(dot(p - x, e) / ee, F(0)), F(1))
    t = np.where(ee > 0, t, F(0)).astype(F)
    q = x + t[..., None] * e
    d = p - q
    return dot(d, d), t, q


def tri_nearest(p, a, b, c):
    """-> (D2, u, v, q, clamped): the triangle rule; clamped marks the candidates the validation bound L changed"""
    p, a, b, c = np.broadcast_arrays(p, a, b, c)
    one, zero = F(1), F(0)
    d2, t, q = seg_dist2(p, a, b)
    u, v = t, np.zeros_like(t)
    for (x, y), uv in (((b, c), lambda t: (one - t, t)), ((c, a), lambda t: (np.zeros_like(t), one - t))):
        e2, t, qe = seg_dist2(p, x, y)
        rep = e2 < d2
        ue, ve = uv(t)
        d2, u, v, q = np.where(rep, e2, d2), np.where(rep, ue, u), np.where(rep, ve, v), np.where(rep[..., None], qe, q)
    n = cross(b - a, c - a)
    nn = dot(n, n)
    s_ab, s_bc, s_ca = dot(cross(b - a, p - a), n), dot(cross(c - b, p - b), n), dot(cross(a - c, p - c), n)
    inside = (nn > 0) & (s_ab >= 0) & (s_bc >= 0) & (s_ca >= 0)
    h = dot(p - a, n)
    with np.errstate(all="ignore"):
        w = h / nn
        dp = w * h
        qp = p - w[..., None] * n
        up, vp = s_ca / nn, s_ab / nn
    rep = inside & (dp < d2)
    d2, u, v, q = np.where(rep, dp, d2), np.where(rep, up, u), np.where(rep, vp, v), np.where(rep[..., None], qp, q)
    lo, hi = np.fmin(np.fmin(a, b), c), np.fmax(np.fmax(a, b), c)
    L = own_box_dist2(lo, hi, p)
    clamped = d2 < L
    return np.where(clamped, L, d2).astype(F), u.astype(F), v.astype(F), q.astype(F), clamped


def piece_nearest(p, a4, b4, sub):
    """a curve piece: end points a4, b4 (xyz + radius), sub = its index in the cubic -> (D2, u, v, q, clamped)"""
    a, b = a4[..., :3], b4[..., :3]
    p, a, b = np.broadcast_arrays(p, a, b)
    d2, t, q = seg_dist2(p, a, b)
    u = (sub.astype(F) + t) * F(0.25)
    rm = np.fmax(np.abs(a4[..., 3]), np.abs(b4[..., 3]))[..., None]
    L = own_box_dist2(np.fmin(a, b) - rm, np.fmax(a, b) + rm, p)
    clamped = d2 < L
    return np.where(clamped, L, d2).astype(F), u.astype(F), np.zeros_like(u), q.astype(F), clamped


def tri_dist64(p, a, b, c):
    """the same distance (not squared) in float64, without the validation bound"""
    p, a, b, c = (np.asarray(x, np.float64) for x in (p, a, b, c))

    def seg(x, y):
        e = y - x
        ee = dot(e, e)
        with np.errstate(all="ignore"):
            t = np.where(ee > 0, np.clip(dot(p - x, e) / ee, 0.0, 1.0), 0.0)
        d = p - (x + t[..., None] * e)
        return dot(d, d)
    d2 = np.minimum(np.minimum(seg(a, b), seg(b, c)), seg(c, a))
    n = cross(b - a, c - a)
    nn = dot(n, n)
    inside = (nn > 0) & (dot(cross(b - a, p - a), n) >= 0) & (dot(cross(c - b, p - b), n) >= 0) & (dot(cross(a - c, p - c), n) >= 0)
    h = dot(p - a, n)
    with np.errstate(all="ignore"):
        dp = np.where(inside, h * h / nn, np.inf)
    return np.sqrt(np.minimum(d2, dp))


def candidates(points, slots, shade, chunk=256):
    """every (query, slot) candidate of a committed scene (Scene.read_slots()) -> D2, u, v, q, clamped, shapes (Q, N[, 3])"""
    slots, shade = np.asarray(slots, F), np.asarray(shade, np.uint32)
    p = np.ascontiguousarray(points, F).reshape(-1, 4)[:, :3]
    nq, ns = len(p), len(slots)
    curve = ((shade[:, 3] >> 24) & SLOT_IS_CURVE) != 0
    out = [np.zeros((nq, ns), F), np.zeros((nq, ns), F), np.zeros((nq, ns), F), np.zeros((nq, ns, 3), F), np.zeros((nq, ns), bool)]
    ti, ci = np.nonzero(~curve)[0], np.nonzero(curve)[0]
    for at in range(0, nq, chunk):
        pp = p[at:at + chunk, None, :]
        if len(ti):
            r = tri_nearest(pp, slots[None, ti, 0, :3], slots[None, ti, 1, :3], slots[None, ti, 2, :3])
            for o, x in zip(out, r):
                o[at:at + chunk, ti] = x
        if len(ci):
            r = piece_nearest(pp, slots[None, ci, 0, :], slots[None, ci, 1, :], slots[ci, 2, 0].view(np.uint32)[None, :])
            for o, x in zip(out, r):
                o[at:at + chunk, ci] = x
    return out


def brute_force(points, slots, shade, cand=None):
    """The contract's answer per query over all slots: the smallest D2 <= max_dist^2, equal D2 to the smaller gid.  Inactive queries (a
    non-finite coordinate, max_dist NaN or < 0) miss.  cand: candidates(points, slots, shade) where the caller has them already (every
    query active).  -> dict(found, slot, gid, d2, dist, u, v, q, ties (gids sharing the minimum),
    clamped (candidates the bound changed))"""
    pts = np.ascontiguousarray(points, F).reshape(-1, 4)
    shade = np.asarray(shade, np.uint32)
    nq, ns = len(pts), len(shade)
    with np.errstate(all="ignore"):
        md2 = pts[:, 3] * pts[:, 3]
        active = np.isfinite(pts[:, :3]).all(axis=1) & (pts[:, 3] >= 0)
    res = dict(found=np.zeros(nq, bool), slot=np.full(nq, NONE, np.uint32), gid=np.full(nq, NONE, np.uint32), d2=np.zeros(nq, F), dist=np.zeros(nq, F),
               u=np.zeros(nq, F), v=np.zeros(nq, F), q=np.zeros((nq, 3), F), ties=np.zeros(nq, np.int64), clamped=0)
    if ns == 0 or nq == 0:
        return res
    safe = np.where(active[:, None], pts, F(0)).astype(F)
    D2, U, V, Q, clamped = candidates(safe, slots, shade) if cand is None else cand
    gid = shade[:, 24].astype(np.int64)
    valid = (D2 <= md2[:, None]) & active[:, None]
    dm = np.where(valid, D2, np.inf)
    mn = dm.min(axis=1)
    cand = valid & (dm == mn[:, None])
    best = np.where(cand, gid[None, :], 1 << 40).argmin(axis=1)
    found = cand.any(axis=1)
    r = np.arange(nq)
    res["found"], res["ties"], res["clamped"] = found, cand.sum(axis=1), int(clamped[active].sum())
    res["slot"] = np.where(found, best, NONE).astype(np.uint32)
    res["gid"] = np.where(found, gid[best], NONE).astype(np.uint32)
    for k, a in (("d2", D2), ("u", U), ("v", V)):
        res[k] = np.where(found, a[r, best], F(0)).astype(F)
    res["q"] = np.where(found[:, None], Q[r, best], F(0)).astype(F)
    res["dist"] = np.sqrt(res["d2"])
    return res


def expected_buffers(res):
    """-> (ident (n, 4) uint32, closest (n, 4) float32) as pbrhip_nearest_point writes them"""
    n = len(res["found"])
    ident, closest = np.zeros((n, 4), np.uint32), np.zeros((n, 4), F)
    ident[:, 0] = res["slot"]
    ident[:, 1], ident[:, 2], ident[:, 3] = res["u"].view(np.uint32), res["v"].view(np.uint32), res["dist"].view(np.uint32)
    ident[~res["found"], 1:] = 0
    closest[:, :3], closest[:, 3] = res["q"], res["d2"]
    closest[~res["found"]] = 0
    return ident, closest


def soup_points(tris, seed, n=3000):
    """The query set of the tests for a triangle set tris (T, 3, 3): n / 6 points on vertices, n / 6 on centroids, n / 6 within 1e-3 of
    centroids, the rest uniform in the box; a fifth of each of the first three groups is aimed at triangles 60 .. 119 of
    tests/_soups.py's soup (coplanar overlaps and their exact duplicates: equal distances).  Every third query has max_dist = 0.05, the
    others none.  -> (n, 4) float32"""
    rng = np.random.RandomState(4200 + seed)
    tris = np.asarray(tris, F)
    g = n // 6
    t = len(tris)

    def pick():
        k = rng.randint(t, size=g)
        if t >= 120:
            k[:g // 5] = 60 + rng.randint(60, size=g // 5)
        return k
    k = pick()
    on_vertex = tris[k, rng.randint(3, size=g)]
    cen = (tris[:, 0] + tris[:, 1] + tris[:, 2]) / F(3)
    on_centroid = cen[pick()]
    near = cen[pick()] + ((rng.rand(g, 3) * 2 - 1) * 1e-3).astype(F)
    lo, hi = tris.reshape(-1, 3).min(axis=0), tris.reshape(-1, 3).max(axis=0)
    inside = (lo + rng.rand(n - 3 * g, 3).astype(F) * (hi - lo)).astype(F)
    p = np.concatenate([on_vertex, on_centroid, near, inside]).astype(F)
    p = p[rng.permutation(n)]
    md = np.full(n, np.inf, F)
    md[::3] = F(0.05)
    return np.ascontiguousarray(np.concatenate([p, md[:, None]], axis=1), F)


def binary_walk(nodes, point, d2_row):
    """dnearest.h::nearest_traverse over a binary tree, restated for one query: nodes = BvhNode records (tests/_lbvh_model.py::NODE_DT, the
    stored boxes), point = (x, y, z, max_dist), d2_row = the contract's D2 of every slot in leaf order.  Children whose box distance does
    not exceed the best D2 so far, the nearer first, the other pushed.  -> (the largest number of live stack entries, the best D2)"""
    leaf_bit, empty = 0x80000000, 0xFFFFFFFF
    p = np.asarray(point[:3], F)
    best = F(point[3]) * F(point[3])
    stack, peak, cur = [], 0, 0
    while True:
        nd = nodes[cur]
        ref = (int(nd["c0"]), int(nd["c1"]))
        L = [box_dist2(nd["lo"][:, c], nd["hi"][:, c], p) for c in (0, 1)]
        hit = [ref[c] != empty and bool(L[c] <= best) for c in (0, 1)]
        nxt = None
        if hit[0] and hit[1]:
            near, far = (1, 0) if L[1] < L[0] else (0, 1)
            stack.append(ref[far])
            peak = max(peak, len(stack))
            nxt = ref[near]
        elif hit[0] or hit[1]:
            nxt = ref[0] if hit[0] else ref[1]
        while True:
            if nxt is None:
                if not stack:
                    return peak, best
                nxt = stack.pop()
            if not nxt & leaf_bit:
                break
            first, count = (nxt & 0x3FFFFFFF) >> 3, (nxt & 7) + 1
            for s in range(first, first + count):
                if d2_row[s] <= best:
                    best = d2_row[s]
            nxt = None
        cur = nxt
