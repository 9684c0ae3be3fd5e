"""The all-hits contract of DESIGN.md §21 for triangles in numpy float32: dtrace.h::tri_test + hit_inside operation for operation (every
operation rounded once, no contraction; the three fma of the validation as float64 sums rounded once, which they equal because one
factor is a power of two), and a brute force over all triangle slots of a committed scene: per ray the number of accepted hits in
(tmin, tmax] and the K first of the order (t, gid, u) in the identity format."""
import numpy as np

from _query_model import cross, dot, vbox_hi, vbox_lo

F = np.float32
NONE = 0xFFFFFFFF
SLOT_IS_CURVE = 2  # kSlotIsCurve (dscene.h), in the top byte of ShadeRec word 3
RAY_DT = np.dtype([("org", "<f4", 3), ("tmin", "<f4"), ("dir", "<f4", 3), ("tmax", "<f4")])


def as_rays(rays):
    """RAY_DT records or (n, 8) float32 rows -> (n, 8) float32"""
    rays = np.asarray(rays)
    if rays.dtype.names:
        return np.ascontiguousarray(rays, RAY_DT).view(F).reshape(-1, 8)
    return np.ascontiguousarray(rays, F).reshape(-1, 8)


def ray_active(r):
    """dtrace.h::ray_active: no NaN, origin and direction finite, a direction other than zero, 0 <= tmin <= tmax"""
    with np.errstate(all="ignore"):
        return (np.isfinite(r[:, 0:3]).all(axis=1) & np.isfinite(r[:, 4:7]).all(axis=1) & (r[:, 4:7] != 0).any(axis=1) & (r[:, 3] >= 0) & (r[:, 7] >= r[:, 3]))


def _widen(x, sign):
    """fma(sign * |x|, 2^-16, x)"""
    x64 = x.astype(np.float64)
    return (x64 + sign * np.abs(x64) * 2.0 ** -16).astype(F)


def hit_inside(lo, hi, o, inv, t):
    """dtrace.h::hit_inside: t within the ray's interval through the box [vbox_lo(lo), vbox_hi(hi)], widened by 2^-16 relative"""
    a = b = None
    for k in range(3):
        t0, t1 = (vbox_lo(lo[..., k]) - o[..., k]) * inv[..., k], (vbox_hi(hi[..., k]) - o[..., k]) * inv[..., k]
        mn, mx = np.fmin(t0, t1), np.fmax(t0, t1)
        a, b = (mn, mx) if a is None else (np.fmax(a, mn), np.fmin(b, mx))
    a, b = _widen(a, -1.0), _widen(b, 1.0)
    return (a <= t) & (t <= b)


def tri_test(v0, v1, v2, o, d, inv3, tmin):
    """dtrace.h::tri_test -> (ok, t, u, v); arrays broadcast, the last axis holds x, y, z"""
    with np.errstate(all="ignore"):
        e1, e2 = v1 - v0, v2 - v0
        p = cross(d, e2)
        det = dot(e1, p)
        inv = F(1) / det
        s = o - v0
        uu = dot(s, p) * inv
        q = cross(s, e1)
        vv = dot(d, q) * inv
        tt = dot(e2, q) * inv
        ok = (det != 0) & (uu >= 0) & (uu <= 1) & (vv >= 0) & (uu + vv <= 1) & (tt > tmin)
        lo, hi = np.fmin(np.fmin(v0, v1), v2), np.fmax(np.fmax(v0, v1), v2)
        ok &= hit_inside(lo, hi, o, inv3, tt)
    return ok, tt.astype(F), uu.astype(F), vv.astype(F)


def brute_force(rays, slots, shade, K, chunk=512):
    """Every ray against every triangle slot of a committed scene (Scene.read_slots(); curve slots are left out) ->
    dict(count (n,) uint32 = |H|, ident (n, K, 4) uint32 = the K first hits of the order (t, gid, u) as slot, bits of u, v, t, the rest
    (NONE, 0, 0, 0), ties (n,) = the number of pairs of successive hits of a ray with equal t and different gid)"""
    r = as_rays(rays)
    slots, shade = np.asarray(slots, F), np.asarray(shade, np.uint32)
    tri = np.nonzero(((shade[:, 3] >> 24) & SLOT_IS_CURVE) == 0)[0] if len(shade) else np.zeros(0, np.int64)
    n, T = len(r), len(tri)
    count, ident, ties = np.zeros(n, np.uint32), np.zeros((n, K, 4), np.uint32), np.zeros(n, np.int64)
    ident[:, :, 0] = NONE
    if n == 0 or T == 0:
        return dict(count=count, ident=ident, ties=ties)
    active = ray_active(r)
    v0, v1, v2 = (slots[tri, c, :3][None] for c in range(3))
    gid = shade[tri, 24].astype(np.int64)
    for at in range(0, n, chunk):
        rr = r[at:at + chunk]
        o, d = rr[:, None, 0:3], rr[:, None, 4:7]
        with np.errstate(all="ignore"):
            inv3 = F(1) / d
        ok, t, u, v = tri_test(v0, v1, v2, o, d, inv3, rr[:, None, 3])
        with np.errstate(all="ignore"):
            ok &= (t <= rr[:, None, 7]) & active[at:at + chunk, None]
        count[at:at + chunk] = ok.sum(axis=1)
        g = np.broadcast_to(gid[None, :], ok.shape)
        order = np.lexsort((u, g, t, ~ok), axis=-1)  # accepted hits first, by (t, gid, u)
        m = len(rr)
        rows = np.arange(m)[:, None]
        top = order[:, :K]
        okk = ok[rows, top]
        blk = np.zeros((m, top.shape[1], 4), np.uint32)
        blk[..., 0] = np.where(okk, tri[top], NONE)
        for w, a in ((1, u), (2, v), (3, t)):
            blk[..., w] = np.where(okk, a[rows, top].view(np.uint32), 0)
        ident[at:at + chunk, :top.shape[1]] = blk
        if T > 1:
            a, b = order[:, :-1], order[:, 1:]
            tie = ok[rows, a] & ok[rows, b] & (t[rows, a] == t[rows, b]) & (g[rows, a] != g[rows, b])
            ties[at:at + chunk] = tie.sum(axis=1)
    return dict(count=count, ident=ident, ties=ties)


def binary_walk_all(nodes, ray, slots, shade):
    """dallhits.h::all_traverse (dtrace.h::walk_tree with its box tests) with COUNT over a binary tree, restated for one ray: nodes = BvhNode records
    (tests/_lbvh_model.py::NODE_DT, the stored boxes), children whose slab interval -- box_test2's, widened by 2^-16 -- meets [tmin, tmax],
    the nearer first, the other pushed.  -> (the largest number of live stack entries, the number of accepted hits)"""
    leaf_bit, empty = 0x80000000, 0xFFFFFFFF
    r = as_rays(ray)[0]
    o, d, tmin, tmax = r[0:3], r[4:7], r[3], r[7]
    with np.errstate(all="ignore"):
        inv = F(1) / d
    stack, peak, cur, hits = [], 0, 0, 0

    def box(nd, c):
        with np.errstate(all="ignore"):
            p, q = (nd["lo"][:, c] - o) * inv, (nd["hi"][:, c] - o) * inv
            a, b = np.fmin(p, q), np.fmax(p, q)
            a, b = np.fmax(np.fmax(a[0], a[1]), a[2]), np.fmin(np.fmin(b[0], b[1]), b[2])
            a, b = _widen(np.asarray(a, F), -1.0), _widen(np.asarray(b, F), 1.0)
            return bool(a <= b and b >= tmin and a <= tmax), a
    while True:
        nd = nodes[cur]
        ref = (int(nd["c0"]), int(nd["c1"]))
        (h0, t0), (h1, t1) = box(nd, 0), box(nd, 1)
        h0, h1 = h0 and ref[0] != empty, h1 and ref[1] != empty
        nxt = None
        if h0 and h1:
            near, far = (1, 0) if t1 < t0 else (0, 1)
            stack.append(ref[far])
            peak = max(peak, len(stack))
            nxt = ref[near]
        elif h0 or h1:
            nxt = ref[0] if h0 else ref[1]
        while True:
            if nxt is None:
                if not stack:
                    return peak, hits
                nxt = stack.pop()
            if not nxt & leaf_bit:
                break
            first, cnt = (nxt & 0x3FFFFFFF) >> 3, (nxt & 7) + 1
            hits += int(brute_force(r[None], slots[first:first + cnt], shade[first:first + cnt], 0)["count"][0])
            nxt = None
        cur = nxt


def fat_comb_triangles():
    """The depth-64 comb of tests/_lbvh_model.py::comb_triangles(1) with the teeth on the x and y axes grown until each covers the origin
    of its plane z = 0: corners lo, (hi.x, lo.y), (lo.x, hi.y) of the box c -+ (2^b + 1) in x and y, exact in float32.  The box centres
    -- all a Morton key sees -- are the comb's, so the Morton tree is the same chain; but a ray up the z axis now crosses the boxes of
    63 of the 65 leaves, where no straight line crosses more than 22 of the thin comb's.  -> (triangles, lo, hi)"""
    import _lbvh_model as M
    c = M.comb_points(1)
    tri = M.comb_triangles(1)[0].copy()
    for i in range(2, 2 + 42):  # after the origin and the far corner: 21 teeth on x, then 21 on y (then those on z, which stay)
        h = F(2.0 ** ((i - 2) % 21) + 1.0)
        lo, hi = c[i] - np.array([h, h, 0], F), c[i] + np.array([h, h, 0], F)
        tri[i] = [[lo[0], lo[1], 0], [hi[0], lo[1], 0], [lo[0], hi[1], 0]]
    lo, hi = tri.min(axis=1), tri.max(axis=1)
    assert tri.dtype == np.float32 and np.array_equal(F(0.5) * (lo + hi), c)
    return tri, lo, hi
