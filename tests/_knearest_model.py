"""The k-nearest contract of DESIGN.md §22 in numpy float32: a brute force over tests/_query_model.py::candidates -- §19's candidate of
every (query, slot), operation for operation -- ordered by (D2, gid, sub), and dknearest.h's traversal with the K-th-best bound restated
for one query over a binary tree."""
import numpy as np

import _query_model as QM

F = np.float32
NONE = 0xFFFFFFFF


def sub_of(slots, shade):
    """the piece index of every slot: word 8 of a curve slot, 0 for a triangle"""
    slots, shade = np.asarray(slots, F), np.asarray(shade, np.uint32)
    if len(shade) == 0:
        return np.zeros(0, np.int64)
    curve = ((shade[:, 3] >> 24) & QM.SLOT_IS_CURVE) != 0
    return np.where(curve, np.ascontiguousarray(slots[:, 2, 0]).view(np.uint32), 0).astype(np.int64)


def brute_force(points, slots, shade, K, cand=None):
    """Every query against every slot of a committed scene (Scene.read_slots()) -> dict(count (n,) uint32 = the slots with
    D2 <= max_dist^2 (a NaN never, an inactive query none), ident (n, K, 4) uint32 = the K first of the order (D2, gid, sub) as slot,
    bits of u, v, sqrt(D2), the rest (NONE, 0, 0, 0), closest (n, K, 4) float32 = q | D2 of the listed, the rest zeros, ties (n,) bool =
    entries K and K + 1 of the order exist and have equal D2: a tie across the cut (K = 0: none), order (n, N) = every slot in the order,
    the qualifying ones first, d2 (n, N) = D2 along that order, inf where not qualifying).  cand: candidates(points, slots, shade) of
    active queries where the caller has them."""
    pts = np.ascontiguousarray(points, F).reshape(-1, 4)
    slots, shade = np.asarray(slots, F), np.asarray(shade, np.uint32)
    nq, ns = len(pts), len(shade)
    count, ident, closest = np.zeros(nq, np.uint32), np.zeros((nq, K, 4), np.uint32), np.zeros((nq, K, 4), F)
    ident[:, :, 0] = NONE
    res = dict(count=count, ident=ident, closest=closest, ties=np.zeros(nq, bool), order=np.zeros((nq, ns), np.int64), d2=np.zeros((nq, ns), F))
    if nq == 0 or ns == 0:
        return res
    with np.errstate(all="ignore"):
        md2 = pts[:, 3] * pts[:, 3]
        active = np.isfinite(pts[:, :3]).all(axis=1) & (pts[:, 3] >= 0)
        safe = np.where(active[:, None], pts, F(0)).astype(F)
        D2, U, V, Q, _ = QM.candidates(safe, slots, shade) if cand is None else cand
        valid = (D2 <= md2[:, None]) & active[:, None]
    gid = np.broadcast_to(shade[:, 24].astype(np.int64)[None, :], D2.shape)
    sub = np.broadcast_to(sub_of(slots, shade)[None, :], D2.shape)
    order = np.lexsort((sub, gid, np.where(valid, D2, F(0)), ~valid), axis=-1)  # the qualifying first, by (D2, gid, sub)
    rows = np.arange(nq)[:, None]
    count[:] = valid.sum(axis=1)
    res["order"], res["d2"] = order, np.where(valid[rows, order], D2[rows, order], np.inf)
    top = order[:, :K]
    ok = valid[rows, top]
    k = top.shape[1]
    ident[:, :k, 0] = np.where(ok, top, NONE)
    with np.errstate(all="ignore"):
        dist = np.sqrt(D2)
    for w, a in ((1, U), (2, V), (3, dist)):
        ident[:, :k, w] = np.where(ok, a[rows, top].view(np.uint32), 0)
    closest[:, :k, :3] = np.where(ok[..., None], Q[rows, top], F(0))
    closest[:, :k, 3] = np.where(ok, D2[rows, top], F(0))
    if 0 < K < ns:
        a, b = order[:, K - 1], order[:, K]
        r = np.arange(nq)
        res["ties"] = valid[r, a] & valid[r, b] & (D2[r, a] == D2[r, b])
    return res


def binary_walk_k(nodes, point, d2_row, gid_row, K):
    """dknearest.h::knearest_traverse without count over a binary tree, restated for one query: nodes = BvhNode records
    (tests/_lbvh_model.py::NODE_DT, the stored boxes), point = (x, y, z, max_dist), d2_row / gid_row = the contract's D2 and the gid of
    every slot in leaf order.  The bound is max_dist^2 until K candidates are listed, then the K-th entry's D2; children whose box
    distance does not exceed it, the nearer first, the other pushed.  -> (the largest number of live stack entries, the listed (D2,
    gid) in order)"""
    leaf_bit, empty = 0x80000000, 0xFFFFFFFF
    p = np.asarray(point[:3], F)
    md2 = F(point[3]) * F(point[3])
    bound, best = md2, []
    stack, peak, cur = [], 0, 0
    while True:
        nd = nodes[cur]
        ref = (int(nd["c0"]), int(nd["c1"]))
        L = [QM.box_dist2(nd["lo"][:, c], nd["hi"][:, c], p) for c in (0, 1)]
        hit = [ref[c] != empty and bool(L[c] <= bound) for c in (0, 1)]
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
                if d2_row[s] <= md2 and d2_row[s] <= bound:
                    best = sorted(best + [(float(d2_row[s]), int(gid_row[s]))])[:K]
                    if len(best) == K:
                        bound = F(best[-1][0])
            nxt = None
        cur = nxt
