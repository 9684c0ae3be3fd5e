"""The tree of the GPU BVH builder (pbrlab_amd/csrc/bvh_gpu.hip), predicted bit for bit from its definition (DESIGN.md section 8,
"The tree, exactly"), and a structural checker of any such tree.  numpy and Python integers only; no tolerance anywhere: every
arithmetic step of the builder is IEEE single precision without contraction, the keys are integers and the radix tree over sorted
keys is unique.

  morton_keys / build   the model: keys, stable order, the hierarchy top down from the definition of a radix tree, emission
  check_tree            independent of the model and vectorised level by level: also for half a million boxes
  box_sets / comb_*     the primitive sets the CPU and GPU tests share

Out of scope: boxes that are not finite or whose lo + hi overflows (the centre is then inf or NaN and no order is defined)."""
import numpy as np

F = np.float32
LEAF_BIT, CURVE_BIT, EMPTY_CHILD = 0x80000000, 0x40000000, 0xFFFFFFFF   # dscene.h: child references
MAX_LEAF = 2                                                           # kMaxLeaf
STACK_DEPTH = 64                                                       # kStackDepth
CELLS = F(2097151.0)                                                   # 2^21 - 1 cells per axis
NODE_DT = np.dtype([("lo", "<f4", (3, 2)), ("hi", "<f4", (3, 2)), ("c0", "<u4"), ("c1", "<u4"), ("pad", "<u4", 2)])   # BvhNode


def _boxes(lo, hi, kinds):
    lo, hi, kinds = np.asarray(lo), np.asarray(hi), np.asarray(kinds)
    assert lo.dtype == np.float32 and hi.dtype == np.float32 and kinds.dtype == np.uint8
    assert lo.shape == hi.shape == (len(kinds), 3)
    return lo, hi, kinds


# ------------------------------------------------------------------------------------------------ keys
def cells(lo, hi):
    """(n, 3) integer cell of every box centre on the 2^21 - 1 grid over the centres' bounds; every intermediate is a float32"""
    c = F(0.5) * (lo + hi)
    assert c.dtype == np.float32 and np.isfinite(c).all(), "centres must be finite (lo + hi must not overflow)"
    mn, mx = c.min(axis=0), c.max(axis=0)
    ext = mx - mn
    flat = ~(ext > 0)
    q = (c - mn) / np.where(flat, F(1), ext)
    q = np.where(flat, F(0), np.clip(q, F(0), F(1)))
    scaled = q * CELLS
    assert q.dtype == np.float32 and scaled.dtype == np.float32
    return scaled.astype(np.int64)                                      # truncation; 0 <= scaled <= 2097151


def interleave(cell):
    """63-bit key: bit b of the x, y, z cell is bit 3b + 2, 3b + 1, 3b of the key (x highest in each triple)"""
    cell = np.asarray(cell, np.uint64)
    key = np.zeros(len(cell), np.uint64)
    for b in range(21):
        for a in range(3):
            key |= ((cell[:, a] >> np.uint64(b)) & np.uint64(1)) << np.uint64(3 * b + 2 - a)
    return key


def interleave_int(x, y, z):
    """the same for one key, spelled from the most significant bit down with Python integers"""
    key = 0
    for b in range(20, -1, -1):
        for v in (x, y, z):
            key = key * 2 + ((int(v) >> b) & 1)
    return key


def morton_keys(lo, hi):
    return interleave(cells(lo, hi))


# ------------------------------------------------------------------------------------------------ hierarchy
def prefix(k, i, j):
    """length of the common prefix of sorted positions i and j: over the 64-bit keys; equal keys continue over the 32-bit positions"""
    if k[i] != k[j]:
        return 64 - (k[i] ^ k[j]).bit_length()
    return 64 + 32 - (i ^ j).bit_length()


def hierarchy(sorted_keys):
    """The radix tree over the sorted keys, top down.  The node over [f, l] splits after the largest g in [f, l - 1] whose common prefix
    with f is longer than that of (f, l); the root is node 0, the child over [f, g] is inner node g, the one over [g + 1, l] inner node
    g + 1, a one-element range a leaf.  -> dict of lists over the n - 1 inner nodes: left / right (a child c >= 0 is inner node c,
    c < 0 the leaf at sorted position ~c), first, last, height (a leaf has height 0)."""
    k = [int(x) for x in sorted_keys]
    n = len(k)
    m = n - 1
    left, right, first, last, height = ([None] * m for _ in range(5))
    todo, found = [(0, 0, n - 1)], []
    while todo:
        i, f, l = todo.pop()
        assert left[i] is None, "two ranges map to one node index"
        d = prefix(k, f, l)
        g = max(j for j in range(f, l) if j == f or prefix(k, f, j) > d)
        first[i], last[i] = f, l
        left[i] = ~f if f == g else g
        right[i] = ~l if g + 1 == l else g + 1
        if left[i] >= 0:
            todo.append((g, f, g))
        if right[i] >= 0:
            todo.append((g + 1, g + 1, l))
        found.append(i)
    assert len(found) == m
    for i in reversed(found):                                           # children were found after their parents
        height[i] = 1 + max(0 if c < 0 else height[c] for c in (left[i], right[i]))
    return dict(left=left, right=right, first=first, last=last, height=height)


# ------------------------------------------------------------------------------------------------ emission
def widen_lo(v):
    return v - (np.abs(v) * F(2.0 ** -16) + F(1e-30))


def widen_hi(v):
    return v + (np.abs(v) * F(2.0 ** -16) + F(1e-30))


def leaf_ref(kind, first, count):
    return LEAF_BIT | (int(kind) << 30) | (int(first) << 3) | (int(count) - 1)


def build(lo, hi, kinds):
    """-> (nodes, order, depth, tree): what pbrhip_lbvh_build must return for these boxes, and the hierarchy (None for n == 1)"""
    lo, hi, kinds = _boxes(lo, hi, kinds)
    n = len(kinds)
    assert n >= 1
    nodes = np.zeros(max(n - 1, 1), NODE_DT)
    if n == 1:                                                          # a single leaf under the root, the other child empty
        nodes["lo"][0, :, 0], nodes["hi"][0, :, 0] = widen_lo(lo[0]), widen_hi(hi[0])
        nodes["lo"][0, :, 1] = nodes["hi"][0, :, 1] = np.nan
        nodes["c0"][0], nodes["c1"][0] = leaf_ref(kinds[0], 0, 1), EMPTY_CHILD
        return nodes, np.zeros(1, np.uint32), 1, None
    keys = morton_keys(lo, hi)
    order = np.argsort(keys, kind="stable")
    tree = hierarchy(keys[order])
    slo, shi, sk = lo[order], hi[order], kinds[order]
    for i in range(n - 1):
        for c, child in enumerate((tree["left"][i], tree["right"][i])):
            f, l = (~child, ~child) if child < 0 else (tree["first"][child], tree["last"][child])
            nodes["lo"][i, :, c] = widen_lo(slo[f:l + 1].min(axis=0))
            nodes["hi"][i, :, c] = widen_hi(shi[f:l + 1].max(axis=0))
            one_kind = (sk[f:l + 1] == sk[f]).all()
            ref = leaf_ref(sk[f], f, l - f + 1) if l - f + 1 <= MAX_LEAF and one_kind else child
            nodes["c0" if c == 0 else "c1"][i] = ref
    return nodes, order.astype(np.uint32), tree["height"][0] + 1, tree


def nodes_mismatch(a, b):
    """indices of the nodes that differ: references and pad bitwise, bounds as float32 values (-0 == +0: fminf may return either
    zero; NaN == NaN for the empty child of a one-box tree), anything else exactly"""
    assert a.dtype == NODE_DT and b.dtype == NODE_DT and a.shape == b.shape
    bad = (a["c0"] != b["c0"]) | (a["c1"] != b["c1"]) | (a["pad"] != b["pad"]).any(axis=1)
    for f in ("lo", "hi"):
        same = (a[f] == b[f]) | (np.isnan(a[f]) & np.isnan(b[f]))
        bad |= ~same.reshape(len(a), -1).all(axis=1)
    return np.flatnonzero(bad)


# ------------------------------------------------------------------------------------------------ the checker
class TreeError(AssertionError):
    pass


def _req(cond, what):
    if not cond:
        raise TreeError(what)


def check_tree(nodes, order, depth, lo, hi, kinds):
    """Raises TreeError unless (nodes, order, depth) is a valid tree over the boxes: `order` is a permutation; every slot lies in
    exactly one reachable leaf; a leaf holds at most MAX_LEAF primitives, all of its kind; the leaves' slot ranges, left to right,
    tile 0 .. n - 1; every reachable child box contains the widened boxes of all primitives below it; and `depth` is the true
    maximum number of inner nodes on a path from the root to a primitive, plus one -- a two-primitive leaf stands for the inner
    node that was collapsed into it, which the builder's depth counts (so depth also bounds the inner nodes of every stored path).
    Walks down from the root level by level and back up, vectorised per level."""
    lo, hi, kinds = _boxes(lo, hi, kinds)
    n = len(kinds)
    m = max(n - 1, 1)
    nodes, order = np.asarray(nodes), np.asarray(order)
    _req(n >= 1 and nodes.dtype == NODE_DT and nodes.shape == (m,), "node array has the wrong shape")
    _req(order.shape == (n,) and np.array_equal(np.sort(order.astype(np.int64)), np.arange(n)), "order is not a permutation")
    order = order.astype(np.int64)
    wlo, whi, sk = widen_lo(lo[order]), widen_hi(hi[order]), kinds[order].astype(np.int64)
    refs = np.stack([nodes["c0"], nodes["c1"]], axis=1).astype(np.int64)
    if n == 1:
        _req(refs[0, 0] == leaf_ref(kinds[0], 0, 1) and refs[0, 1] == EMPTY_CHILD, "one box: a leaf and an empty child")
        _req((nodes["lo"][0, :, 0] <= wlo[0]).all() and (nodes["hi"][0, :, 0] >= whi[0]).all(), "a box does not contain its primitives")
        _req(not (nodes["lo"][0, :, 1] <= nodes["hi"][0, :, 1]).any(), "the empty child's box can be hit")
        _req(depth == 1, "depth")
        return
    # down: the reachable nodes, level by level
    seen = np.zeros(m, bool)
    levels, frontier = [], np.zeros(1, np.int64)
    while frontier.size:
        _req(not seen[frontier].any() and np.unique(frontier).size == frontier.size, "a node is reachable along two paths")
        seen[frontier] = True
        levels.append(frontier)
        r = refs[frontier]
        _req(not (r == EMPTY_CHILD).any(), "an empty child in a tree of more than one box")
        inner = (r & LEAF_BIT) == 0
        _req((r[inner] < m).all(), "a child index is out of range")
        frontier = r[inner]
    # up: per reachable node the tight (widened) box of its primitives, its slot range and the inner nodes below it
    sub_lo, sub_hi = np.zeros((m, 3), F), np.zeros((m, 3), F)
    sub_first, sub_last, sub_h = (np.zeros(m, np.int64) for _ in range(3))
    covered = np.zeros(n + 1, np.int64)
    for idx in reversed(levels):
        side = []
        for c in range(2):
            r = refs[idx, c]
            leaf = (r & LEAF_BIT) != 0
            ch = np.where(leaf, 0, r)
            f, cnt, kd = np.where(leaf, (r >> 3) & 0x7FFFFFF, 0), np.where(leaf, (r & 7) + 1, 1), (r >> 30) & 1
            _req((cnt <= MAX_LEAF).all(), "a leaf holds more than MAX_LEAF primitives")
            _req((f + cnt <= n).all(), "a leaf's slots are out of range")
            e = f + cnt - 1
            _req((~leaf | ((sk[f] == kd) & (sk[e] == kd))).all(), "a leaf holds a primitive of another kind")
            np.add.at(covered, f[leaf], 1)
            np.add.at(covered, e[leaf] + 1, -1)
            L = leaf[:, None]
            clo = np.where(L, np.minimum(wlo[f], wlo[e]), sub_lo[ch])
            chi = np.where(L, np.maximum(whi[f], whi[e]), sub_hi[ch])
            ok = (nodes["lo"][idx, :, c] <= clo).all(axis=1) & (nodes["hi"][idx, :, c] >= chi).all(axis=1)
            _req(ok.all(), "a box does not contain its primitives")
            side.append((clo, chi, np.where(leaf, f, sub_first[ch]), np.where(leaf, e, sub_last[ch]), np.where(leaf, cnt - 1, sub_h[ch])))
        (llo, lhi, lf, ll, lh), (rlo, rhi, rf, rl, rh) = side
        _req((ll + 1 == rf).all(), "the leaves' slot ranges are not in left-to-right order")
        sub_lo[idx], sub_hi[idx] = np.minimum(llo, rlo), np.maximum(lhi, rhi)
        sub_first[idx], sub_last[idx], sub_h[idx] = lf, rl, 1 + np.maximum(lh, rh)
    _req((np.cumsum(covered)[:n] == 1).all(), "a slot is not in exactly one leaf")
    _req(sub_first[0] == 0 and sub_last[0] == n - 1, "the leaves do not tile 0 .. n - 1")
    _req(depth >= sub_h[0] + 1, "depth is smaller than the deepest path")
    _req(depth == sub_h[0] + 1, "depth is larger than the deepest path")


def reachable_leaf(nodes, want_count):
    """(node, field, child) of a leaf reference with that many primitives that a walk from the root reaches"""
    todo = [0]
    while todo:
        i = todo.pop()
        for c, f in enumerate(("c0", "c1")):
            r = int(nodes[f][i])
            if not r & LEAF_BIT:
                todo.append(r)
            elif (r & 7) + 1 == want_count:
                return i, f, c
    raise AssertionError("no such leaf")


def mutations(nodes, order, depth):
    """name -> (nodes, order, depth): edits of a correct output (of more than a few boxes) that check_tree must reject, one each.  How
    the tests that run on the device's output are shown to be able to fail: on the output, in numpy -- never by breaking a kernel."""
    out = {}

    def edit(name):
        out[name] = [nodes.copy(), order.copy(), depth]
        return out[name]
    i, f, c = reachable_leaf(nodes, 2)
    m = edit("bound_one_ulp_inwards")                                   # every stored bound is the widened bound of a primitive below it
    m[0]["hi"][i, 1, c] = np.nextafter(m[0]["hi"][i, 1, c], F(-np.inf))
    m = edit("root_bound_one_ulp_inwards")
    m[0]["lo"][0, 2, 1] = np.nextafter(m[0]["lo"][0, 2, 1], F(np.inf))
    m = edit("order_swapped")
    m[1][[3, len(order) - 4]] = m[1][[len(order) - 4, 3]]
    j, g, _ = reachable_leaf(nodes, 1)
    edit("leaf_count_raised")[0][g][j] += 1                             # 1 -> 2: a slot in two leaves (or past the end)
    edit("leaf_count_raised_to_3")[0][f][i] += 1                        # 2 -> 3: more than MAX_LEAF
    edit("leaf_kind_flipped")[0][f][i] ^= CURVE_BIT
    edit("depth_lowered")[2] -= 1
    m = edit("child_redirected_to_sibling")
    m[0]["c0"][0] = m[0]["c1"][0]
    return out


# ------------------------------------------------------------------------------------------------ primitive sets
def comb_points(origin_copies=1):
    """Box centres whose Morton tree is a chain: the origin (origin_copies times), (2097151,) * 3 and 2^b + 0.5 on every axis for
    every bit b < 21 -- each point's cell is exactly its integer part, so each has its own highest key bit.  65 points give depth
    64, a second origin 65."""
    pts = [(0.0, 0.0, 0.0)] * origin_copies + [(2097151.0, 2097151.0, 2097151.0)]
    for a in range(3):
        for b in range(21):
            p = [0.0, 0.0, 0.0]
            p[a] = 2.0 ** b + 0.5
            pts.append(tuple(p))
    return np.array(pts, np.float32)


def comb_boxes(origin_copies=1):
    c = comb_points(origin_copies)
    return c - F(0.25), c + F(0.25), np.zeros(len(c), np.uint8)


def comb_triangles(origin_copies=1):
    """the comb as triangles (n, 3, 3) whose box centres are the points: corners c + (-+0.25, -0.25, 0) and c + (0, 0.25, 0), exact in
    float32 -> (triangles, lo, hi) with their boxes"""
    c = comb_points(origin_copies)
    off = np.array([[-0.25, -0.25, 0.0], [0.25, -0.25, 0.0], [0.0, 0.25, 0.0]], np.float32)
    tri = c[:, None, :] + off[None]
    assert tri.dtype == np.float32 and np.array_equal(tri.astype(np.float64), c.astype(np.float64)[:, None, :] + off[None])
    return tri, tri.min(axis=1), tri.max(axis=1)


def _around(c, half):
    c, half = np.asarray(c, np.float32), np.asarray(half, np.float32)
    return (c - half).astype(np.float32), (c + half).astype(np.float32)


def box_sets():
    """name -> (lo, hi, kinds): every small set of the LBVH tests.  Seeded; all coordinates finite."""
    sets = {}
    one = lambda n: np.zeros(n, np.uint8)                                                        # noqa: E731
    for n in (1, 2, 3, 4, 5, 255, 256, 257, 1000):                                                # block edges of the kernels (256 threads)
        r = np.random.RandomState(100 + n)
        sets[f"random_{n}"] = _around(r.rand(n, 3), r.rand(n, 3) * 0.05) + ((r.rand(n) < 0.25).astype(np.uint8),)
    r = np.random.RandomState(1)                                                                  # all keys equal: the pure tie-break tree
    e = r.randint(1, 1025, size=(1000, 3)).astype(np.float32) / F(1024)
    c = np.array([1.0, -2.0, 3.0], np.float32)
    sets["one_centre_1000"] = (c - e, c + e, one(1000))
    r = np.random.RandomState(2)                                                                  # long runs of equal keys among others
    a, b = _around(r.rand(1, 3), r.rand(1, 3) * 0.1), _around(r.rand(1, 3), r.rand(1, 3) * 0.1)
    x = _around(r.rand(100, 3), r.rand(100, 3) * 0.05)
    p = r.permutation(700)
    sets["duplicates_700"] = (np.concatenate([np.repeat(a[0], 300, 0), np.repeat(b[0], 300, 0), x[0]])[p],
                              np.concatenate([np.repeat(a[1], 300, 0), np.repeat(b[1], 300, 0), x[1]])[p], (r.rand(700) < 0.1).astype(np.uint8)[p])
    r = np.random.RandomState(3)
    c, h = r.rand(400, 3), r.rand(400, 3) * 0.05
    c[:, 2], h[:, 2] = 0.5, 0.25
    sets["flat_z_400"] = _around(c, h) + (one(400),)
    c, h = r.rand(400, 3), r.rand(400, 3) * 0.05
    c[:, 0], h[:, 0], c[:, 2], h[:, 2] = -1.5, 0.125, 0.0, 0.0                                    # (z: boxes of no thickness, centre +0)
    sets["flat_xz_400"] = _around(c, h) + (one(400),)
    t = np.round(r.rand(400, 1) * 256) / 256                                                      # on the diagonal, with repeated points
    sets["diagonal_400"] = _around(np.repeat(t, 3, 1), np.full((400, 3), 1.0 / 512)) + ((r.rand(400) < 0.5).astype(np.uint8),)
    r = np.random.RandomState(4)
    sets["negative_300"] = _around(-1 - 2 * r.rand(300, 3), r.rand(300, 3) * 0.1) + (one(300),)
    c = np.round((r.rand(300, 3) * 2 - 1) * 16) / 16                                              # grid points around the origin, zeros among them
    lo, hi = _around(c, np.full((300, 3), 1.0 / 64))
    lo[:10], hi[:10] = -hi[:10], -lo[:10]
    lo[10:20, 1], hi[10:20, 1] = F(-0.0), F(0.0)
    lo[20:25, 1] = hi[20:25, 1] = F(-0.0)                                                         # centre -0
    sets["mixed_sign_300"] = (lo, hi, (r.rand(300) < 0.25).astype(np.uint8))
    r = np.random.RandomState(5)                                                                  # 60 decades in one set
    c = 10.0 ** r.uniform(-30, 30, size=(600, 3))
    c[0], c[1] = 1e-30, 1e30
    sets["span_1e-30_1e30_600"] = _around(c, c * 0.125) + (one(600),)
    r = np.random.RandomState(6)
    sets["overlapping_500"] = _around(0.5 + 1e-6 * r.rand(500, 3), 10 + 90 * r.rand(500, 3)) + ((r.rand(500) < 0.25).astype(np.uint8),)
    r = np.random.RandomState(7)                                                                  # kinds by sorted position
    lo, hi = _around(r.rand(333, 3), r.rand(333, 3) * 0.05)
    rank = np.empty(333, np.int64)
    rank[np.argsort(morton_keys(lo, hi), kind="stable")] = np.arange(333)
    sets["kinds_alternate_333"] = (lo, hi, (rank & 1).astype(np.uint8))                            # no two-primitive leaf may form
    sets["kinds_halves_333"] = (lo, hi, (rank >= 167).astype(np.uint8))
    k = one(333)
    k[77] = 1
    sets["one_curve_333"] = (lo, hi, k)
    sets["comb_65"] = comb_boxes(1)                                                               # depth 64 = the traversal stack
    sets["comb_66"] = comb_boxes(2)                                                               # depth 65
    return sets


LARGE_N = 524288 + 257   # k_lbvh_bounds' grid is capped at 2048 x 256 threads: only more boxes than that reach its stride loop


def large_set():
    r = np.random.RandomState(8)
    c = r.rand(LARGE_N, 3).astype(np.float32)
    h = (r.rand(LARGE_N, 3) * 0.01).astype(np.float32)
    return c - h, c + h, (r.rand(LARGE_N) < 0.25).astype(np.uint8)
