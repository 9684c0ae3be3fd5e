"""The refit of a committed tree pair (pbrlab_amd/csrc/refit_gpu.hip, pbrhip_scene_refit / pbrhip_tree_refit), predicted bit for bit from
its definition ("The refit, exactly") over numpy arrays.  No tolerance anywhere.

  tight_boxes     a slot's tight box: a triangle's min / max of its three corners, a curve piece's min(a, b) - r and max(a, b) + r with
                  r = max(|a.w|, |b.w|)
  refit           the model: for EVERY child reference of either tree the union of the tight boxes of all slots below it -- the slots
                  are found by walking the tree (slot ranges, bottom up), never by reusing a child's boxes as the kernels do -- then
                  W() = _lbvh_model.widen_*, and for the Q nodes the quantiser of _qcollapse_model (quantise_np restates it over arrays;
                  the CPU tests pin it to quantise); leaf records from the slots their own codes name
  check           the refitted pair still passes _lbvh_model.check_tree and _qcollapse_model.check_qtree
  case / perturb  the trees and the moved slots the CPU and GPU tests share"""
import numpy as np

import _lbvh_model as M
import _qcollapse_model as Q

F = np.float32
LEAF_BIT, CURVE_BIT, EMPTY_CHILD, NONE = Q.LEAF_BIT, Q.CURVE_BIT, Q.EMPTY_CHILD, Q.NONE
MASK = Q.HIT_SLOT_MASK
PERTURBATIONS = ("jitter", "far", "shift_1e6")


# ------------------------------------------------------------------------------------------------ slots
def tight_boxes(slots, curve):
    """slots (n, 4, 4) float32, curve (n,) bool -> (lo, hi) (n, 3) float32"""
    s = np.ascontiguousarray(slots, np.float32)
    curve = np.asarray(curve, bool)[:, None]
    a, b, c = s[:, 0, :3], s[:, 1, :3], s[:, 2, :3]
    r = np.maximum(np.abs(s[:, 0, 3]), np.abs(s[:, 1, 3]))[:, None]
    with np.errstate(over="ignore"):
        lo = np.where(curve, np.minimum(a, b) - r, np.minimum(np.minimum(a, b), c))
        hi = np.where(curve, np.maximum(a, b) + r, np.maximum(np.maximum(a, b), c))
    assert lo.dtype == np.float32 and hi.dtype == np.float32
    return lo, hi


def case(lo, hi, kinds, seed=0):
    """a primitive set of _qcollapse_model.all_sets() -> (lo, hi, kinds, slots) with per-PRIMITIVE slots and THEIR tight boxes: the tree
    and the slots come from the same numbers, as at a commit (make_slots gives a curve piece a radius its set's box does not have)"""
    slots = Q.make_slots(lo, hi, kinds, seed)
    tlo, thi = tight_boxes(slots, np.asarray(kinds) != 0)
    return tlo, thi, np.asarray(kinds), slots


def perturb(slots, curve, how, seed=0):
    """moved slots (leaf order or not: per slot).  jitter: every corner / end point by up to its box's extent; far: a tenth of the
    primitives translated by three scene extents; shift_1e6: everything translated by 1e6.  Radii, piece indices and routing bits stay."""
    s = np.array(slots, np.float32)
    curve = np.asarray(curve, bool)
    n = len(s)
    r = np.random.RandomState(500 + seed)
    lo, hi = tight_boxes(s, curve)
    words = np.where(curve, 2, 3)
    live = (np.arange(4)[None, :] < words[:, None])[:, :, None]           # the words that hold points
    with np.errstate(over="ignore"):
        if how == "jitter":
            d = ((r.rand(n, 4, 3) * 2 - 1).astype(np.float32) * (hi - lo)[:, None, :]).astype(np.float32)
        elif how == "far":
            ext = (hi.max(axis=0) - lo.min(axis=0)).astype(np.float32)
            pick = r.rand(n) < 0.1
            pick[0] = True
            sign = np.where(r.rand(n, 3) < 0.5, F(-3), F(3)).astype(np.float32)
            d = np.where(pick[:, None], sign * ext[None, :], F(0)).astype(np.float32)[:, None, :].repeat(4, axis=1)
        elif how == "shift_1e6":
            d = np.full((n, 4, 3), 1e6, np.float32)
        else:
            raise ValueError(how)
        s[:, :, :3] = np.where(live, s[:, :, :3] + d, s[:, :, :3])
    assert np.isfinite(s[:, :2]).all()
    return s


# ------------------------------------------------------------------------------------------------ the quantiser over arrays
def quantise_np(blo, bhi, cnt):
    """qquant.h::quantise_node for m nodes at once: blo / bhi (m, 4, 3) float32, cnt (m,) children in use (a prefix)
    -> (org (m, 3), step (m, 3), qlo (m, 3) uint32, qhi (m, 3) uint32, ok (m,))"""
    m = len(cnt)
    used = np.arange(4)[None, :] < np.asarray(cnt)[:, None]
    org, step = np.zeros((m, 3), F), np.zeros((m, 3), F)
    qlo, qhi, ok = np.zeros((m, 3), np.uint32), np.zeros((m, 3), np.uint32), np.ones(m, bool)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        for a in range(3):
            l = np.where(used, blo[:, :, a], F(np.inf)).min(axis=1)
            h = np.where(used, bhi[:, :, a], F(-np.inf)).max(axis=1)
            good = (l <= h) & np.isfinite(l) & np.isfinite(h)
            ok &= good
            sc = np.nextafter(((h - l) / F(253.0)).astype(np.float32), F(np.inf))
            sc = np.where(sc < Q.FLT_MIN, Q.FLT_MIN, sc).astype(np.float32)
            act = np.flatnonzero(good)
            tries = 0
            while act.size:
                fin = np.isfinite(sc[act])
                if tries > 40:
                    fin[:] = False
                ok[act[~fin]] = False
                act = act[fin]
                if not act.size:
                    break
                la, sa = l[act], sc[act]
                node_ok = np.ones(len(act), bool)
                wl, wh = np.zeros(len(act), np.uint32), np.zeros(len(act), np.uint32)
                for i in range(4):
                    u = used[act, i]
                    cl, ch = blo[act, i, a], bhi[act, i, a]
                    ql = np.floor((cl.astype(np.float64) - la.astype(np.float64)) / sa.astype(np.float64))
                    qh = np.ceil((ch.astype(np.float64) - la.astype(np.float64)) / sa.astype(np.float64))
                    ql = np.clip(np.nan_to_num(ql, nan=0.0), 0, 255).astype(np.int64)
                    qh = np.clip(np.nan_to_num(qh, nan=0.0), 0, 255).astype(np.int64)
                    while True:
                        dec = u & (ql > 0) & ~(Q.fmaf_np(ql.astype(np.float32), sa, la) <= cl)
                        if not dec.any():
                            break
                        ql -= dec
                    while True:
                        inc = u & (qh < 255) & ~(Q.fmaf_np(qh.astype(np.float32), sa, la) >= ch)
                        if not inc.any():
                            break
                        qh += inc
                    good_i = (Q.fmaf_np(ql.astype(np.float32), sa, la) <= cl) & (Q.fmaf_np(qh.astype(np.float32), sa, la) >= ch)
                    node_ok &= good_i | ~u
                    wl |= (np.where(u, ql, 255).astype(np.uint32) << np.uint32(8 * i))
                    wh |= (np.where(u, qh, 0).astype(np.uint32) << np.uint32(8 * i))
                done = act[node_ok]
                org[done, a], step[done, a], qlo[done, a], qhi[done, a] = la[node_ok], sa[node_ok], wl[node_ok], wh[node_ok]
                act = act[~node_ok]
                sc[act] = (sc[act] * (F(1.03125) if tries < 8 else F(2.0))).astype(np.float32)
                tries += 1
    return org, step, qlo, qhi, ok


# ------------------------------------------------------------------------------------------------ the model
def _levels(refs, m):
    """the reachable nodes of a tree with child references refs (m, fan), level by level from the root"""
    levels, frontier, total = [], np.zeros(1, np.int64), 0
    while frontier.size:
        levels.append(frontier)
        total += frontier.size
        assert total <= m, "the tree is broken"
        r = refs[frontier]
        frontier = r[(r & LEAF_BIT) == 0]
        assert (frontier < m).all()
    return levels


def _range_boxes(tlo, thi, f, l):
    """W(union of the tight boxes of slots f .. l) for arrays of ranges"""
    n = len(tlo)
    if len(f) == 0:
        return np.zeros((0, 3), F), np.zeros((0, 3), F)
    idx = np.stack([f, l + 1], axis=1).reshape(-1)
    pad_lo, pad_hi = np.concatenate([tlo, tlo[-1:]]), np.concatenate([thi, thi[-1:]])   # (reduceat wants indices < len)
    assert (f <= l).all() and (l < n).all()
    lo = np.minimum.reduceat(pad_lo, idx, axis=0)[0::2]
    hi = np.maximum.reduceat(pad_hi, idx, axis=0)[0::2]
    return M.widen_lo(lo), M.widen_hi(hi)


def refit(nodes, slots, q=None):
    """-> (nodes', q'): what pbrhip_tree_refit must return for the binary tree `nodes` (and the Q tree q = dict(qnodes, tri, pts, hit)
    over it) after the slots became `slots` ((n, 4, 4) float32 in leaf order).  References, pad, the NaN box of an empty child, codes,
    hit codes, padding and zero points stay; unreachable nodes are not touched."""
    B = np.array(nodes, M.NODE_DT)
    s = np.ascontiguousarray(slots, np.float32)
    n, m = len(s), len(B)
    refs = np.stack([B["c0"], B["c1"]], axis=1).astype(np.int64)
    levels = _levels(refs, m)
    # the slots below every child reference, by walking the tree: kinds from the leaf references, ranges bottom up
    curve = np.zeros(n, bool)
    first, last, count = np.zeros(m, np.int64), np.zeros(m, np.int64), np.zeros(m, np.int64)
    cf, cl = np.zeros((m, 2), np.int64), np.zeros((m, 2), np.int64)
    for idx in reversed(levels):
        f2, l2, n2 = [], [], []
        for c in range(2):
            r = refs[idx, c]
            empty, leaf = r == EMPTY_CHILD, (r & LEAF_BIT) != 0
            ch = np.where(leaf, 0, r)
            f = np.where(leaf, (r >> 3) & 0x7FFFFFF, first[ch])
            l = np.where(leaf, f + (r & 7), last[ch])
            k = np.where(leaf, (r & 7) + 1, count[ch])
            real = leaf & ~empty
            assert (l[real] < n).all()
            for j in range(int(((r[real] & 7) + 1).max()) if real.any() else 0):
                sel = real & ((r & 7) >= j)
                curve[f[sel] + j] = (r[sel] & CURVE_BIT) != 0
            cf[idx, c], cl[idx, c] = f, l
            f2.append(np.where(empty, np.iinfo(np.int64).max, f)), l2.append(np.where(empty, -1, l)), n2.append(np.where(empty, 0, k))
        first[idx], last[idx], count[idx] = np.minimum(f2[0], f2[1]), np.maximum(l2[0], l2[1]), n2[0] + n2[1]
        assert (count[idx] == last[idx] - first[idx] + 1).all(), "the slots below a node are not a range"
    tlo, thi = tight_boxes(s, curve)
    reach = np.concatenate(levels)
    for c in range(2):
        live = reach[refs[reach, c] != EMPTY_CHILD]
        lo, hi = _range_boxes(tlo, thi, cf[live, c], cl[live, c])
        B["lo"][live, :, c], B["hi"][live, :, c] = lo, hi
    if q is None:
        return B, None
    # ---- the Q tree
    Qn = np.array(q["qnodes"], Q.QNODE_DT)
    tri, pts = np.array(q["tri"], np.float32).reshape(-1, 4), np.array(q["pts"], np.float32).reshape(-1, 4)
    hit = np.asarray(q["hit"]).astype(np.int64)
    tu, pu, su = tri.view(np.uint32), pts.view(np.uint32), s.view(np.uint32)
    tri_pairs = len(pts) == 8
    nq = len(Qn)
    C = Qn["c"].astype(np.int64)
    qlevels = _levels(C, nq)
    used = C != EMPTY_CHILD
    qfirst, qlast = np.zeros(nq, np.int64), np.zeros(nq, np.int64)
    kf, kl = np.zeros((nq, 4), np.int64), np.zeros((nq, 4), np.int64)
    for idx in reversed(qlevels):
        fs, ls = [], []
        for k in range(4):
            r, u = C[idx, k], used[idx, k]
            leaf = u & ((r & LEAF_BIT) != 0)
            cv = leaf & ((r & CURVE_BIT) != 0)
            t = leaf & ~cv
            rec = (r >> 3) & 0x7FFFFFF
            f, l = qfirst[np.where(u & ~leaf, r, 0)].copy(), qlast[np.where(u & ~leaf, r, 0)].copy()
            # curve records: the slots their hit codes name
            P = np.where(cv, rec & ~3, 4)
            pair = cv & ((r & Q.CURVE_PAIR_BIT) != 0)
            sa = np.where(cv, hit[P] & MASK, 0)
            sb = np.where(pair, hit[P + 2] & MASK, sa)
            f, l = np.where(cv, np.minimum(sa, sb), f), np.where(cv, np.maximum(sa, sb), l)
            if cv.any():
                pu[P[cv]], pu[P[cv] + 1] = su[sa[cv], 0], su[sa[cv], 1]
                pu[P[pair] + 2], pu[P[pair] + 3] = su[sb[pair], 0], su[sb[pair], 1]
            if t.any() and tri_pairs:
                w = np.where(t, rec * Q.TRI_PAIR_WORDS, 0)
                ca, cb = tu[w + 4, 2].astype(np.int64), tu[w + 4, 3].astype(np.int64)
                ta = ca & MASK
                tb = np.where(cb == NONE, ta, cb & MASK)
                f, l = np.where(t, np.minimum(ta, tb), f), np.where(t, np.maximum(ta, tb), l)
                A, Bs, wt = su[ta[t]], su[tb[t]], w[t]
                tu[wt + 0] = np.stack([A[:, 0, 0], Bs[:, 0, 0], A[:, 0, 1], Bs[:, 0, 1]], axis=1)
                tu[wt + 1] = np.stack([A[:, 0, 2], Bs[:, 0, 2], A[:, 1, 0], Bs[:, 1, 0]], axis=1)
                tu[wt + 2] = np.stack([A[:, 1, 1], Bs[:, 1, 1], A[:, 1, 2], Bs[:, 1, 2]], axis=1)
                tu[wt + 3] = np.stack([A[:, 2, 0], Bs[:, 2, 0], A[:, 2, 1], Bs[:, 2, 1]], axis=1)
                tu[wt + 4, 0], tu[wt + 4, 1] = A[:, 2, 2], Bs[:, 2, 2]
            elif t.any():
                cnt = np.where(t, (r & 7) + 1, 0)
                lo_s, hi_s = np.full(len(idx), np.iinfo(np.int64).max), np.full(len(idx), -1)
                for j in range(int(cnt.max())):
                    tj = t & (cnt > j)
                    w = np.where(tj, 3 * (rec + j), 0)
                    code = tu[w + 2, 3].copy()
                    sj = code.astype(np.int64) & MASK
                    tu[w[tj]], tu[w[tj] + 1], tu[w[tj] + 2] = su[sj[tj], 0], su[sj[tj], 1], su[sj[tj], 2]
                    tu[w[tj] + 2, 3] = code[tj]
                    lo_s, hi_s = np.where(tj, np.minimum(lo_s, sj), lo_s), np.where(tj, np.maximum(hi_s, sj), hi_s)
                f, l = np.where(t, lo_s, f), np.where(t, hi_s, l)
            kf[idx, k], kl[idx, k] = f, l
            fs.append(np.where(u, f, np.iinfo(np.int64).max)), ls.append(np.where(u, l, -1))
        qfirst[idx], qlast[idx] = np.min(fs, axis=0), np.max(ls, axis=0)
    qreach = np.concatenate(qlevels)
    blo, bhi = np.zeros((nq, 4, 3), F), np.zeros((nq, 4, 3), F)
    for k in range(4):
        live = qreach[used[qreach, k]]
        blo[live, k], bhi[live, k] = _range_boxes(tlo, thi, kf[live, k], kl[live, k])
    cnt = used.sum(axis=1)
    assert (used[:, :-1] | ~used[:, 1:]).all() and (cnt[qreach] >= 1).all()
    org, step, qlo, qhi, ok = quantise_np(blo[qreach], bhi[qreach], cnt[qreach])
    assert ok.all(), "a node cannot be quantised"
    Qn["org"][qreach], Qn["qlo"][qreach], Qn["qhi"][qreach] = org, qlo, qhi
    Qn["sx"][qreach], Qn["sy"][qreach], Qn["sz"][qreach] = step[:, 0], step[:, 1], step[:, 2]
    return B, dict(q, qnodes=Qn, tri=tri, pts=pts, hit=np.array(q["hit"], np.uint32))


def differences(nodes_a, qa, nodes_b, qb):
    """names of the parts of two refitted pairs that differ, as BYTES (a stored bound is never a zero: W() moves it off)"""
    bad = []
    if nodes_a.tobytes() != nodes_b.tobytes():
        bad.append("nodes")
    if (qa is None) != (qb is None):
        return bad + ["qtree"]
    for f in ("qnodes", "tri", "pts", "hit") if qa is not None else ():
        x, y = np.ascontiguousarray(qa[f]), np.ascontiguousarray(qb[f])
        if x.shape != y.shape or x.tobytes() != y.tobytes():
            bad.append(f)
    return bad


def check(nodes, slots, q, depth):
    """the refitted pair is a valid tree over the moved slots: _lbvh_model.check_tree (every stored box contains the widened boxes of
    the primitives below it, ...) and _qcollapse_model.check_qtree (records equal the slots, rebuilt boxes contain the binary tree's)"""
    s = np.ascontiguousarray(slots, np.float32)
    n = len(s)
    curve = np.zeros(n, bool)
    refs = np.stack([nodes["c0"], nodes["c1"]], axis=1).astype(np.int64)
    for lv in _levels(refs, len(nodes)):
        for r in refs[lv].reshape(-1):
            if r != EMPTY_CHILD and r & LEAF_BIT:
                f, c, _ = Q.leaf_fields(int(r))
                curve[f:f + c] = bool(r & CURVE_BIT)
    tlo, thi = tight_boxes(s, curve)
    M.check_tree(nodes, np.arange(n, dtype=np.uint32), depth, tlo, thi, curve.astype(np.uint8))
    if q is not None:
        Q.check_qtree(nodes, s, dict(q, stack_need=Q.stack_need(q["qnodes"])))
