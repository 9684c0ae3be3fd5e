"""The collapse of the GPU-built binary tree into the 4-wide quantised tree (pbrlab_amd/csrc/qtree_gpu.hip, builder BVH_GPU_LBVH_WIDE),
predicted bit for bit from its definition ("The collapse, exactly"), and a structural checker of any
(binary tree, Q tree) pair.  No tolerance anywhere.

  collapse        the model over _lbvh_model.build's tree: np.float32 arithmetic for the areas, the host libm's fmaf through ctypes
                  for the expression the traversal evaluates (never emulated in float64: that rounds twice), Python floats for the
                  steps the quantiser takes in double
  check_qtree     independent of the model and vectorised level by level (also for half a million boxes): every slot under exactly
                  one leaf record, every Q child a subtree of the binary tree whose stored box its rebuilt box contains, records and
                  hit codes equal to the slots, 4-aligned points, references within their bit fields, pair bit == count, stack need
  make_slots      64-byte slot records for bare boxes, as a committed scene lays them out
  mutations       one wrong byte or reference each, all of which check_qtree must reject"""
import ctypes
import ctypes.util
import math

import numpy as np

import _lbvh_model as M

F = np.float32
LEAF_BIT, CURVE_BIT, EMPTY_CHILD, NONE = M.LEAF_BIT, M.CURVE_BIT, M.EMPTY_CHILD, 0xFFFFFFFF
CURVE_PAIR_BIT = 4                                                       # dscene.h::kCurvePairBit
TRI_PAIR_WORDS = 5                                                       # dscene.h::kTriPairWords
HIT_SLOT_MASK = 0x07FFFFFF                                               # dscene.h::kHitSlotMask
ROUTE_BITS = (1 << 27, 1 << 28, 1 << 29, 1 << 30)                        # kHitMore, kHitHair, kHitLight, kHitNoMaterial
STACK_DEPTH = M.STACK_DEPTH
FLT_MIN = F(1.1754944e-38)
# QNode (dscene.h): per axis an origin and a step, 8-bit bounds of four children (byte i of a word = child i), four references
QNODE_DT = np.dtype([("org", "<f4", 3), ("sx", "<f4"), ("sy", "<f4"), ("sz", "<f4"), ("qlo", "<u4", 3), ("qhi", "<u4", 3), ("c", "<u4", 4)])
assert QNODE_DT.itemsize == 64

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.fmaf.restype = ctypes.c_float
_libm.fmaf.argtypes = [ctypes.c_float] * 3


def fmaf(a, b, c):
    """the host libm's fmaf: a * b + c rounded once to float32"""
    return F(_libm.fmaf(float(a), float(b), float(c)))


def fmaf_np(q, s, org):
    """fmaf over arrays, for the checker: q * s is exact in float64 (8 x 24 bits); the sum is rounded to ODD in float64 (two-sum gives
    the exact error), after which the rounding to float32 is the rounding of the exact value (53 >= 24 + 2 bits).  Pinned against libm's
    fmaf in tests/test_qcollapse_model_cpu.py."""
    t = np.asarray(q, np.float64) * np.asarray(s, np.float64)
    o = np.broadcast_to(np.asarray(org, np.float64), t.shape)
    r = t + o
    bb = r - t
    e = (t - (r - bb)) + (o - bb)
    even = (r.view(np.int64) & 1) == 0
    r = np.where((e != 0) & even, np.nextafter(r, np.where(e > 0, np.inf, -np.inf)), r)
    return r.astype(np.float32)


# ------------------------------------------------------------------------------------------------ slots
def make_slots(lo, hi, kinds, seed=0):
    """(n, 4, 4) float32, one 64-byte record per PRIMITIVE as a scene's slots are laid out: a triangle's three corners (inside its
    box), the routing bits in .w of the third word; a curve piece's two end points xyz + radius, its index in the cubic as the bits of
    the third word's .x, routing bits in .w"""
    lo, hi, kinds = M._boxes(lo, hi, kinds)
    n = len(kinds)
    r = np.random.RandomState(1000 + seed)
    s = np.zeros((n, 4, 4), np.float32)
    u = s.view(np.uint32)
    tri = kinds == 0
    s[tri, 0, :3], s[tri, 2, :3] = lo[tri], hi[tri]
    s[tri, 1, 0], s[tri, 1, 1], s[tri, 1, 2] = hi[tri, 0], lo[tri, 1], hi[tri, 2]
    s[~tri, 0, :3], s[~tri, 1, :3] = lo[~tri], hi[~tri]
    s[~tri, 0, 3] = s[~tri, 1, 3] = F(0.001)
    u[~tri, 2, 0] = r.randint(0, 4, size=n).astype(np.uint32)[~tri]
    route = np.zeros(n, np.uint32)
    for b in ROUTE_BITS:
        route |= np.where(r.rand(n) < 0.3, np.uint32(b), np.uint32(0))
    u[:, 2, 3] = route
    return s


# ------------------------------------------------------------------------------------------------ the model
def quantise(boxes):
    """bvh_build.cpp's quantise_node (qquant.h), operation for operation.  boxes: [(lo, hi)] of float32 triples, 1..4 of them.
    -> (org[3], step[3], qlo[3], qhi[3], retries) or None when a node cannot be quantised"""
    n = len(boxes)
    org, step, qlo, qhi, retries = [F(0)] * 3, [F(0)] * 3, [0] * 3, [0] * 3, 0
    with np.errstate(over="ignore", invalid="ignore"):
        for a in range(3):
            lo, hi = F(np.inf), F(-np.inf)
            for blo, bhi in boxes:                                        # std::min / std::max as they evaluate
                lo = blo[a] if blo[a] < lo else lo
                hi = bhi[a] if hi < bhi[a] else hi
            if not (lo <= hi) or not np.isfinite(lo) or not np.isfinite(hi):
                return None
            sc = np.nextafter(F(F(hi - lo) / F(253.0)), F(np.inf))
            sc = FLT_MIN if sc < FLT_MIN else sc
            tries = 0
            while True:
                if tries > 40 or not np.isfinite(sc):
                    return None
                ok, wl, wh = True, 0, 0
                for i in range(4):
                    if i >= n:
                        wl |= 255 << (8 * i)
                        continue
                    blo, bhi = boxes[i][0][a], boxes[i][1][a]
                    ql = int(math.floor((float(blo) - float(lo)) / float(sc)))
                    qh = int(math.ceil((float(bhi) - float(lo)) / float(sc)))
                    ql, qh = max(0, min(255, ql)), max(0, min(255, qh))
                    while ql > 0 and not (fmaf(ql, sc, lo) <= blo):
                        ql -= 1
                    while qh < 255 and not (fmaf(qh, sc, lo) >= bhi):
                        qh += 1
                    if not (fmaf(ql, sc, lo) <= blo and fmaf(qh, sc, lo) >= bhi):
                        ok = False
                        break
                    wl |= ql << (8 * i)
                    wh |= qh << (8 * i)
                if ok:
                    org[a], step[a], qlo[a], qhi[a] = lo, sc, wl, wh
                    break
                sc = F(sc * (F(1.03125) if tries < 8 else F(2.0)))
                tries += 1
                retries += 1
    return org, step, qlo, qhi, retries


def area(lo, hi):
    """A = dx*dy + dy*dz + dz*dx in float32, the products and sums in this order, each rounded"""
    with np.errstate(over="ignore", invalid="ignore"):
        d = hi - lo
        assert d.dtype == np.float32
        return F(F(F(d[0] * d[1]) + F(d[1] * d[2])) + F(d[2] * d[0]))


def frontier(B, v):
    """the frontier of binary node v: [(ref, lo, hi)] with the boxes the parents store"""
    Fr = [(int(B[f][v]), B["lo"][v, :, c].copy(), B["hi"][v, :, c].copy()) for c, f in enumerate(("c0", "c1")) if int(B[f][v]) != EMPTY_CHILD]
    while len(Fr) < 4:
        best, best_a = -1, None
        for i, (r, lo, hi) in enumerate(Fr):
            if r & LEAF_BIT:
                continue
            A = area(lo, hi)
            if best < 0 or A > best_a:                                    # ties: the earliest
                best, best_a = i, A
        if best < 0:
            break
        u = Fr[best][0]
        kids = [(int(B[f][u]), B["lo"][u, :, c].copy(), B["hi"][u, :, c].copy()) for c, f in enumerate(("c0", "c1"))]
        assert all(k[0] != EMPTY_CHILD for k in kids), "an inner node of the binary tree has two children"
        Fr[best:best + 1] = kids
    return Fr


def leaf_fields(ref):
    return (ref & 0x3FFFFFFF) >> 3, (ref & 7) + 1, bool(ref & CURVE_BIT)


def stack_need(qnodes):
    """need(node) = (children - 1) + max over inner children need(child); children need not follow their parent"""
    c = qnodes["c"].astype(np.int64)
    need, state, todo = [0] * len(c), [0] * len(c), [0]
    while todo:
        i = todo[-1]
        inner = [int(r) for r in c[i] if not r & LEAF_BIT]
        if state[i] == 0:
            state[i] = 1
            todo.extend(inner)
            continue
        todo.pop()
        nc = int((c[i] != EMPTY_CHILD).sum())
        need[i] = (nc - 1 if nc else 0) + max([need[k] for k in inner], default=0)
    return need[0]


def collapse(nodes, slots, kinds_in_order):
    """-> dict(qnodes, tri, pts, hit, stack_need, retries, quantised): what pbrhip_qtree_collapse must return for the binary tree `nodes`
    (of _lbvh_model.build) over `slots` ((n, 4, 4) float32 IN LEAF ORDER) of kinds_in_order"""
    B = nodes
    n = len(kinds_in_order)
    tri_pairs = not np.asarray(kinds_in_order).any()
    su = np.ascontiguousarray(slots, np.float32).view(np.uint32)
    fronts, todo = {}, [0]
    while todo:
        v = todo.pop()
        fronts[v] = frontier(B, v)
        todo.extend(r for r, _, _ in fronts[v] if not r & LEAF_BIT)
    heads = sorted(fronts)                                                # ascending binary index: node 0 is Q node 0
    qidx = {v: i for i, v in enumerate(heads)}
    leaves = sorted(leaf_fields(r) for v in heads for r, _, _ in fronts[v] if r & LEAF_BIT)   # by first slot
    tri_rec, curve_rec, nt, nc = {}, {}, 0, 0
    for first, count, curve in leaves:
        if curve:
            curve_rec[first], nc = nc, nc + 1
        else:
            tri_rec[first], nt = nt, nt + (1 if tri_pairs else count)
    tri_words = (nt * (TRI_PAIR_WORDS if tri_pairs else 3) + 3) // 4 * 4
    npts = 4 + 4 * nc + 4
    tri, pts, hit = np.zeros((tri_words, 4), np.uint32), np.zeros((npts, 4), np.uint32), np.full(npts, NONE, np.uint32)
    code = lambda k: int(k) | int(su[k, 2, 3])                           # noqa: E731
    for first, count, curve in leaves:
        if curve:
            P = 4 + 4 * curve_rec[first]
            for i in range(count):
                pts[P + 2 * i], pts[P + 2 * i + 1], hit[P + 2 * i] = su[first + i, 0], su[first + i, 1], code(first + i)
        elif not tri_pairs:
            for i in range(count):
                w = 3 * (tri_rec[first] + i)
                tri[w:w + 3] = su[first + i, :3]
                tri[w + 2, 3] = code(first + i)
        else:
            a, b = su[first], su[first + 1 if count == 2 else first]
            cb = code(first + 1) if count == 2 else NONE
            w = TRI_PAIR_WORDS * tri_rec[first]
            tri[w:w + 5] = [(a[0, 0], b[0, 0], a[0, 1], b[0, 1]), (a[0, 2], b[0, 2], a[1, 0], b[1, 0]), (a[1, 1], b[1, 1], a[1, 2], b[1, 2]),
                            (a[2, 0], b[2, 0], a[2, 1], b[2, 1]), (a[2, 2], b[2, 2], code(first), cb)]
    q = np.zeros(len(heads), QNODE_DT)
    q["c"] = EMPTY_CHILD
    retries, quantised = 0, True
    for v in heads:
        Fr, i = fronts[v], qidx[v]
        res = quantise([(lo, hi) for _, lo, hi in Fr])
        if res is None:
            quantised = False
        else:
            org, step, qlo, qhi, r = res
            q["org"][i], (q["sx"][i], q["sy"][i], q["sz"][i]), q["qlo"][i], q["qhi"][i] = org, step, qlo, qhi
            retries += r
        for k, (r, _, _) in enumerate(Fr):
            if not r & LEAF_BIT:
                q["c"][i, k] = qidx[r]
                continue
            first, count, curve = leaf_fields(r)
            if curve:
                P = 4 + 4 * curve_rec[first]
                sub = [int(su[first + j, 2, 0]) & 3 for j in range(count)]
                q["c"][i, k] = LEAF_BIT | CURVE_BIT | ((P | sub[0]) << 3) | ((CURVE_PAIR_BIT | sub[1]) if count == 2 else 0)
            else:
                q["c"][i, k] = LEAF_BIT | (tri_rec[first] << 3) | (count - 1)
    return dict(qnodes=q, tri=tri.view(np.float32), pts=pts.view(np.float32), hit=hit, stack_need=stack_need(q), retries=retries,
                quantised=quantised, n=n)


def build(lo, hi, kinds, slots):
    """boxes, kinds and per-PRIMITIVE slots -> (binary nodes, order, depth, the model's collapse over them)"""
    nodes, order, depth, _ = M.build(lo, hi, kinds)
    return nodes, order, depth, collapse(nodes, np.asarray(slots)[order], np.asarray(kinds)[order])


def same(a, b):
    """names of the parts of two collapses that differ: bytes, but bounds-free (a Q tree holds no -0 / NaN ambiguity: org is one of
    the binary tree's bounds, compared as float32 values)"""
    bad = []
    qa, qb = a["qnodes"], b["qnodes"]
    if qa.shape != qb.shape:
        return ["qnodes.shape"]
    for f in ("sx", "sy", "sz", "qlo", "qhi", "c"):
        if qa[f].tobytes() != qb[f].tobytes():
            bad.append(f)
    if not np.array_equal(qa["org"], qb["org"]):
        bad.append("org")
    for f in ("tri", "pts", "hit"):
        if a[f].shape != b[f].shape or a[f].tobytes() != b[f].tobytes():
            bad.append(f)
    if a["stack_need"] != b["stack_need"]:
        bad.append("stack_need")
    return bad


# ------------------------------------------------------------------------------------------------ the checker
class QTreeError(AssertionError):
    pass


def _req(cond, what):
    if not cond:
        raise QTreeError(what)


def _binary_refs(B, n):
    """every reference a walk from the root of the binary tree reaches -> (sorted keys first * (n + 1) + last, ref, lo, hi) with the box
    its parent stores; slot ranges bottom-up (an LBVH's leaves tile the slots left to right: _lbvh_model.check_tree)"""
    m = len(B)
    refs = np.stack([B["c0"], B["c1"]], axis=1).astype(np.int64)
    levels, frontier = [], np.zeros(1, np.int64)
    while frontier.size:
        levels.append(frontier)
        r = refs[frontier]
        frontier = r[((r & LEAF_BIT) == 0)]
        _req((frontier < m).all() and len(levels) <= m, "the binary tree is broken")
    first, last = np.zeros(m, np.int64), np.zeros(m, np.int64)
    out = []
    for idx in reversed(levels):
        f2, l2 = [], []
        for c in range(2):
            r = refs[idx, c]
            empty, leaf = r == EMPTY_CHILD, (r & LEAF_BIT) != 0
            ch = np.where(leaf, 0, r)
            f = np.where(leaf, (r >> 3) & 0x7FFFFFF, first[ch])
            l = np.where(leaf, f + (r & 7), last[ch])
            keep = ~empty
            out.append((f[keep] * (n + 1) + l[keep], r[keep], B["lo"][idx, :, c][keep], B["hi"][idx, :, c][keep]))
            f2.append(np.where(empty, np.iinfo(np.int64).max, f))
            l2.append(np.where(empty, -1, l))
        first[idx], last[idx] = np.minimum(f2[0], f2[1]), np.maximum(l2[0], l2[1])
    key, ref = np.concatenate([o[0] for o in out]), np.concatenate([o[1] for o in out])
    lo, hi = np.concatenate([o[2] for o in out]), np.concatenate([o[3] for o in out])
    o = np.argsort(key, kind="stable")
    _req(np.unique(key).size == key.size, "two references of the binary tree cover the same slots")
    return key[o], ref[o], lo[o], hi[o], (first[0], last[0])


def check_qtree(B, slots, q):
    """Raises QTreeError unless q = dict(qnodes, tri, pts, hit, stack_need) is a valid collapse of the binary tree B over `slots`
    ((n, 4, 4) float32 in leaf order).  Which frontier a node took is NOT checked (any valid frontier passes): that is the model's."""
    su = np.ascontiguousarray(slots, np.float32).view(np.uint32).astype(np.int64)
    n = len(su)
    Q, tri, pts, hit = q["qnodes"], np.ascontiguousarray(q["tri"], np.float32).view(np.uint32).astype(np.int64), \
        np.ascontiguousarray(q["pts"], np.float32).view(np.uint32).astype(np.int64), np.asarray(q["hit"]).astype(np.int64)
    nq = len(Q)
    _req(nq >= 1 and Q.dtype == QNODE_DT, "no Q nodes")
    _req(len(tri) % 4 == 0, "the triangle area is not a multiple of 4 words")
    _req(len(pts) >= 8 and len(pts) % 4 == 0 and len(hit) == len(pts), "points / hit codes have the wrong length")
    _req(len(pts) < (1 << 27) and len(tri) < 3 * (1 << 27), "a record index does not fit its reference")
    _req(not pts[:4].any() and not pts[-4:].any(), "the padding points are not zero")
    _req((hit[:4] == NONE).all() and (hit[-4:] == NONE).all(), "a hit code in the padding")
    bkey, bref, blo, bhi, root_range = _binary_refs(B, n)
    code = np.arange(n) | su[:, 2, 3]
    C = Q["c"].astype(np.int64)
    used = C != EMPTY_CHILD
    _req((used[:, :-1] | ~used[:, 1:]).all(), "an empty child before a used one")
    # down
    seen = np.zeros(nq, bool)
    levels, frontier = [], np.zeros(1, np.int64)
    while frontier.size:
        _req(not seen[frontier].any() and np.unique(frontier).size == frontier.size, "a Q node is reachable along two paths")
        seen[frontier] = True
        levels.append(frontier)
        r = C[frontier]
        inner = (r & LEAF_BIT) == 0
        _req((r[inner] < nq).all(), "a child index is out of range")
        frontier = r[inner]
    _req(seen.all(), "a Q node is not reachable")
    # up: slot range and stack need per node; leaf records against the slots; boxes against the binary tree's
    first, last, need = np.zeros(nq, np.int64), np.zeros(nq, np.int64), np.zeros(nq, np.int64)
    covered = np.zeros(n + 1, np.int64)
    pieces = 0
    tri_only = not ((bref & LEAF_BIT != 0) & (bref & CURVE_BIT != 0)).any()
    step = np.stack([Q["sx"], Q["sy"], Q["sz"]], axis=1)
    for idx in reversed(levels):
        prev_last = None
        nc = used[idx].sum(axis=1)
        _req((nc >= 1).all(), "a Q node without children")
        deepest = np.zeros(len(idx), np.int64)
        for k in range(4):
            r, u = C[idx, k], used[idx, k]
            leaf, curve = u & ((r & LEAF_BIT) != 0), (r & CURVE_BIT) != 0
            inner = u & ~leaf
            ch = np.where(inner, r, 0)
            f, l = first[ch].copy(), last[ch].copy()
            deepest = np.maximum(deepest, np.where(inner, need[ch], 0))
            cnt = np.ones(len(idx), np.int64)
            # triangle leaves
            t = leaf & ~curve
            rec = (r >> 3) & 0x7FFFFFF
            cnt = np.where(t, (r & 7) + 1, cnt)
            _req((cnt[t] <= 2).all(), "a triangle leaf of more than two")
            if len(tri) == 0:
                _req(not t.any(), "a triangle leaf without triangle records")
                sa = np.zeros(len(idx), np.int64)
            elif tri_only:
                w = np.where(t, rec * TRI_PAIR_WORDS, 0)
                _req((w[t] + TRI_PAIR_WORDS <= len(tri)).all(), "a triangle record is out of range")
                ca, cb = tri[w + 4, 2], tri[w + 4, 3]
                sa = ca & HIT_SLOT_MASK
                _req((sa[t] + cnt[t] <= n).all(), "a triangle record names a slot out of range")
                sa = np.where(t, sa, 0)
                sb = np.where(t & (cnt == 2), sa + 1, sa)
                _req((ca[t] == code[sa][t]).all() and (cb[t] == np.where(cnt == 2, code[sb], NONE)[t]).all(), "a TriPair's hit codes are not its slots'")
                A, Bs = su[sa], su[sb]
                want = np.stack([A[:, 0, 0], Bs[:, 0, 0], A[:, 0, 1], Bs[:, 0, 1], A[:, 0, 2], Bs[:, 0, 2], A[:, 1, 0], Bs[:, 1, 0], A[:, 1, 1], Bs[:, 1, 1],
                                 A[:, 1, 2], Bs[:, 1, 2], A[:, 2, 0], Bs[:, 2, 0], A[:, 2, 1], Bs[:, 2, 1], A[:, 2, 2], Bs[:, 2, 2]], axis=1)
                got = np.stack([tri[w + j] for j in range(5)], axis=1).reshape(len(idx), 20)[:, :18]
                _req((got[t] == want[t]).all(), "a TriPair's corners are not its slots'")
            else:
                w = np.where(t, rec * 3, 0)
                _req((w[t] + 3 * cnt[t] <= len(tri)).all(), "a triangle record is out of range")
                sa = tri[w + 2, 3] & HIT_SLOT_MASK
                _req((sa[t] + cnt[t] <= n).all(), "a triangle record names a slot out of range")
                sa = np.where(t, sa, 0)
                for j in range(2):
                    tj = t & (cnt > j)
                    sj = np.where(tj, sa + j, 0)
                    wj = np.where(tj, w + 3 * j, 0)
                    _req((tri[wj + 2, 3][tj] == code[sj][tj]).all(), "a triangle's hit code is not its slot's")
                    got = np.stack([tri[wj], tri[wj + 1], tri[wj + 2]], axis=1).reshape(len(idx), 12)[:, :11]
                    _req((got[tj] == su[sj][:, :3].reshape(len(idx), 12)[:, :11][tj]).all(), "a triangle's corners are not its slot's")
            f, l = np.where(t, sa, f), np.where(t, sa + cnt - 1, l)
            # curve leaves
            cv = leaf & curve
            Psub = (r >> 3) & 0x7FFFFFF
            P = np.where(cv, Psub & ~3, 4)
            pair = cv & ((r & CURVE_PAIR_BIT) != 0)
            _req((P[cv] >= 4).all() and (P[cv] + 4 <= len(pts) - 4).all(), "a curve record is out of range")
            _req(((r & 3)[cv & ~pair] == 0).all(), "bits of a second piece without the pair bit")
            s0 = hit[P] & HIT_SLOT_MASK
            _req((hit[P][cv] != NONE).all() and (s0[cv] + np.where(pair, 2, 1)[cv] <= n).all(), "a curve record without its hit code")
            s0 = np.where(cv, s0, 0)
            s1 = np.where(pair, s0 + 1, s0)
            _req((hit[P][cv] == code[s0][cv]).all() and (hit[P + 2][cv] == np.where(pair, code[s1], NONE)[cv]).all(), "a curve record's hit codes are not its slots' (pair bit == count)")
            _req((hit[P + 1][cv] == NONE).all() and (hit[P + 3][cv] == NONE).all(), "a hit code where no piece starts")
            _req(((pts[P] == su[s0, 0]) & (pts[P + 1] == su[s0, 1])).all(axis=1)[cv].all(), "a curve record's first piece is not its slot's")
            _req(((pts[P + 2] == su[s1, 0]) & (pts[P + 3] == su[s1, 1])).all(axis=1)[pair].all(), "a curve record's second piece is not its slot's")
            _req(not pts[P + 2][cv & ~pair].any() and not pts[P + 3][cv & ~pair].any(), "points behind a one-piece record")
            _req(((Psub & 3)[cv] == (su[s0, 2, 0] & 3)[cv]).all() and ((r & 3)[pair] == (su[s1, 2, 0] & 3)[pair]).all(), "a piece's index in its cubic")
            pieces += int(cv.sum() + pair.sum())
            cnt = np.where(cv, np.where(pair, 2, 1), cnt)
            f, l = np.where(cv, s0, f), np.where(cv, s1, l)
            np.add.at(covered, f[leaf], 1)
            np.add.at(covered, l[leaf] + 1, -1)
            # the child is a subtree of the binary tree, in order, and its rebuilt box contains the box the binary tree stores
            if prev_last is not None:
                _req((f[u] == prev_last[u] + 1).all(), "the children of a Q node do not tile its slots in order")
            at = np.searchsorted(bkey, f * (n + 1) + l)
            at = np.minimum(at, len(bkey) - 1)
            _req((bkey[at][u] == (f * (n + 1) + l)[u]).all(), "a Q child is not a subtree of the binary tree")
            br = bref[at]
            _req((((br & LEAF_BIT) != 0) == leaf)[u].all(), "a leaf of one tree is an inner node of the other")
            _req((((br & CURVE_BIT) != 0) == curve)[leaf].all() and (((br & 7) + 1) == cnt)[leaf].all(), "a leaf's kind or count is not the binary tree's")
            qlo = np.stack([(Q["qlo"][idx, a] >> (8 * k)) & 255 for a in range(3)], axis=1).astype(np.float32)
            qhi = np.stack([(Q["qhi"][idx, a] >> (8 * k)) & 255 for a in range(3)], axis=1).astype(np.float32)
            _req((qlo[~u] == 255).all() and (qhi[~u] == 0).all(), "the bounds of an unused child can be hit")
            rlo, rhi = fmaf_np(qlo, step[idx], Q["org"][idx]), fmaf_np(qhi, step[idx], Q["org"][idx])
            _req(((rlo <= blo[at]) & (rhi >= bhi[at])).all(axis=1)[u].all(), "a rebuilt box does not contain the binary tree's")
            prev_last = np.where(u, l, prev_last if prev_last is not None else l)
            if k == 0:
                first[idx] = f
        last[idx] = prev_last
        need[idx] = nc - 1 + deepest
    _req((np.cumsum(covered)[:n] == 1).all(), "a slot is not under exactly one leaf record")
    _req(first[0] == root_range[0] == 0 and last[0] == root_range[1] == n - 1, "the root does not cover every slot")
    _req(int((hit != NONE).sum()) == pieces, "a hit code where no piece starts")
    _req(int(q["stack_need"]) == int(need[0]), "the stack need is wrong")


# ------------------------------------------------------------------------------------------------ doctored trees
def _find(q, want):
    """(node, child) of the first child reference for which want(ref) holds, in node order"""
    for i, row in enumerate(q["qnodes"]["c"]):
        for k, r in enumerate(row):
            if int(r) != EMPTY_CHILD and want(int(r)):
                return i, k
    raise AssertionError("no such child")


def mutations(q):
    """name -> q': edits of a correct collapse (of a mixed set of a few hundred) that check_qtree must reject: one wrong byte or one
    wrong reference each.  How the tests that run on the device's output are shown to be able to fail -- never by breaking a kernel."""
    out = {}

    def edit(name):
        out[name] = dict(q, qnodes=q["qnodes"].copy(), tri=q["tri"].copy(), pts=q["pts"].copy(), hit=q["hit"].copy())
        return out[name]
    is_tri = lambda r: bool(r & LEAF_BIT) and not r & CURVE_BIT            # noqa: E731
    is_curve = lambda r: bool(r & LEAF_BIT) and bool(r & CURVE_BIT)        # noqa: E731
    i, k = _find(q, is_tri)
    N = q["qnodes"]
    # a bound byte moved inwards: find a child whose low byte can rise
    m = edit("qlo_byte_raised")
    lo_b = (int(N["qlo"][i, 0]) >> (8 * k)) & 255
    hi_b = (int(N["qhi"][i, 0]) >> (8 * k)) & 255
    m["qnodes"]["qlo"][i, 0] = (int(N["qlo"][i, 0]) & ~(255 << (8 * k))) | (min(lo_b + 1, 255) << (8 * k))
    m = edit("qhi_byte_lowered")
    m["qnodes"]["qhi"][i, 0] = (int(N["qhi"][i, 0]) & ~(255 << (8 * k))) | (max(hi_b - 1, 0) << (8 * k))
    m = edit("step_one_ulp_smaller")
    m["qnodes"]["sy"][:] = np.nextafter(N["sy"], F(0))                     # every node: some child's upper bound falls inside its box
    edit("triangle_count_raised")["qnodes"]["c"][i, k] ^= 1               # 1 <-> 2 primitives behind a triangle leaf
    edit("triangle_record_moved")["qnodes"]["c"][i, k] += 8
    ci, ck = _find(q, is_curve)
    edit("curve_pair_bit_flipped")["qnodes"]["c"][ci, ck] ^= CURVE_PAIR_BIT
    edit("curve_sub_index_changed")["qnodes"]["c"][ci, ck] ^= 8
    edit("curve_record_moved")["qnodes"]["c"][ci, ck] += 4 << 3
    P = ((int(N["c"][ci, ck]) >> 3) & 0x7FFFFFF) & ~3
    edit("hit_code_wrong_slot")["hit"][P] ^= 1
    edit("hit_code_routing_bit")["hit"][P] ^= 1 << 28
    edit("hit_code_where_no_piece_starts")["hit"][P + 1] = q["hit"][P]
    edit("point_changed").__getitem__("pts").view(np.uint32)[P + 1, 3] ^= 1
    edit("padding_point_not_zero").__getitem__("pts").view(np.uint32)[2, 0] = 1
    edit("triangle_corner_changed").__getitem__("tri").view(np.uint32)[0, 0] ^= 1
    ii, ik = _find(q, lambda r: not r & LEAF_BIT)
    m = edit("child_redirected")
    other = [int(r) for r in N["c"].ravel() if not int(r) & LEAF_BIT and int(r) != int(N["c"][ii, ik])]
    m["qnodes"]["c"][ii, ik] = other[-1]
    edit("child_dropped")["qnodes"]["c"][i, k] = EMPTY_CHILD
    m = edit("children_swapped")
    m["qnodes"]["c"][0, [0, 1]] = m["qnodes"]["c"][0, [1, 0]]
    edit("stack_need_lowered")["stack_need"] = q["stack_need"] - 1
    edit("stack_need_raised")["stack_need"] = q["stack_need"] + 1
    m = edit("unused_child_bounds")
    e = np.argwhere(N["c"] == EMPTY_CHILD)
    assert len(e), "the tree to doctor needs a node with an unused child"
    m["qnodes"]["qlo"][e[0][0], 2] &= ~np.uint32(1 << (8 * int(e[0][1])))
    return out


# ------------------------------------------------------------------------------------------------ primitive sets
def extra_sets():
    """the sets the collapse adds to _lbvh_model.box_sets(): small boxes far from the origin (a step below the resolution of org: the
    quantiser's step-growth retries) and a mixed set of triangles and curve pieces"""
    sets = {}
    r = np.random.RandomState(21)
    c = (r.rand(300, 3) * 0.5).astype(np.float32) + F(1e6)
    h = (r.rand(300, 3) * 0.01 + 0.001).astype(np.float32)
    sets["shifted_1e6_300"] = ((c - h).astype(np.float32), (c + h).astype(np.float32), np.zeros(300, np.uint8))
    r = np.random.RandomState(22)
    c, h = r.rand(500, 3).astype(np.float32), (r.rand(500, 3) * 0.03).astype(np.float32)
    sets["mixed_500"] = (c - h, c + h, (r.rand(500) < 0.4).astype(np.uint8))
    return sets


def all_sets():
    return dict(M.box_sets(), **extra_sets())


def bushy_comb_points(levels):
    """Box centres whose Morton tree keeps the BINARY depth at 2 * levels + 1 while the collapsed tree needs 3 * levels stack entries:
    a comb that takes two key bits per level -- under the prefix 00..0 of level j sit one primitive at 01, one at 10, two at 11 (a
    leaf of two) and, at 00, the next level -- so every head's frontier is [next head, leaf, leaf, leaf of two]: three entries left
    behind per level, where the plain comb (_lbvh_model.comb_points) leaves one per binary level.  Cells are exact: the centres are
    cell + 0.5 except the two corners of the grid (0 and 2097151), like the plain comb's."""
    assert 1 <= levels <= 31

    def cell(bits):                                                      # 63 key bits, x first -> integer cell per axis
        c = [0, 0, 0]
        for t, b in enumerate(bits):
            c[t % 3] |= b << (20 - t // 3)
        return c
    pts = []
    for j in range(levels):
        pre, rest = [0] * (2 * j), 63 - 2 * j - 2
        for two, fill in (((0, 1), 0), ((1, 0), 0), ((1, 1), 0), ((1, 1), 1)):
            pts.append([k + 0.5 for k in cell(pre + list(two) + [fill] * rest)])
    pts[3] = [2097151.0] * 3                                             # (level 0's 11 + all ones: the far corner of the grid)
    pts.append([0.0, 0.0, 0.0])                                          # the deepest 00: the near corner
    return np.array(pts, np.float32)


def bushy_comb_triangles(levels):
    """the bushy comb as triangles, like _lbvh_model.comb_triangles -> (triangles (n, 3, 3), lo, hi)"""
    c = bushy_comb_points(levels)
    off = np.array([[-0.25, -0.25, 0.0], [0.25, -0.25, 0.0], [0.0, 0.25, 0.0]], np.float32)
    tri = c[:, None, :] + off[None]
    assert np.array_equal(tri.astype(np.float64), c.astype(np.float64)[:, None, :] + off[None])
    return tri, tri.min(axis=1), tri.max(axis=1)


# ------------------------------------------------------------------------------------------------ node visits, from the model
def _slab(o, d, lo, hi):
    """rays (m, 3) against boxes (m, 3): the interval [0, inf) meets the box"""
    with np.errstate(divide="ignore", invalid="ignore"):
        t0, t1 = (lo - o) / d, (hi - o) / d
    near, far = np.fmin(t0, t1).max(axis=1), np.fmax(t0, t1).min(axis=1)
    return np.maximum(near, 0) <= far


def node_visits(B, q, org, dirs):
    """-> (binary, wide): node visits of rays that visit EVERY node whose stored (rebuilt) box they meet -- no order, no cut at a hit: what
    the shape of either tree costs, without the primitives"""
    org, dirs = np.asarray(org, np.float64), np.asarray(dirs, np.float64)
    ray, node, binary = np.arange(len(org)), np.zeros(len(org), np.int64), 0
    while ray.size:
        binary += ray.size
        nxt = []
        for c, f in enumerate(("c0", "c1")):
            r = B[f][node].astype(np.int64)
            go = ((r & LEAF_BIT) == 0) & _slab(org[ray], dirs[ray], B["lo"][node, :, c].astype(np.float64), B["hi"][node, :, c].astype(np.float64))
            nxt.append((ray[go], r[go]))
        ray, node = np.concatenate([x[0] for x in nxt]), np.concatenate([x[1] for x in nxt])
    Q_, step = q["qnodes"], np.stack([q["qnodes"]["sx"], q["qnodes"]["sy"], q["qnodes"]["sz"]], axis=1)
    ray, node, wide = np.arange(len(org)), np.zeros(len(org), np.int64), 0
    while ray.size:
        wide += ray.size
        nxt = []
        for k in range(4):
            r = Q_["c"][node, k].astype(np.int64)
            lo = fmaf_np(((Q_["qlo"][node] >> (8 * k)) & 255).astype(np.float32), step[node], Q_["org"][node]).astype(np.float64)
            hi = fmaf_np(((Q_["qhi"][node] >> (8 * k)) & 255).astype(np.float32), step[node], Q_["org"][node]).astype(np.float64)
            go = ((r & LEAF_BIT) == 0) & _slab(org[ray], dirs[ray], lo, hi)
            nxt.append((ray[go], r[go]))
        ray, node = np.concatenate([x[0] for x in nxt]), np.concatenate([x[1] for x in nxt])
    return binary, wide
