"""CPU: the model of the GPU-built BVH (tests/_lbvh_model.py) and its checker, made trustworthy before any GPU visit.  On every small
primitive set of tests/test_lbvh_gpu.py the model's own tree passes check_tree, its leaves in order are the stable sorted order and
every inner node is a node of the radix tree; the comb sets have the depths the traversal-stack tests need; and check_tree rejects
each of eight edits of a correct output -- the proof that the GPU tests, which run check_tree and compare with the model on what the
device returns, can fail (shown on the output in numpy: a builder kernel with a wrong split may never terminate)."""
import numpy as np
import pytest

import _lbvh_model as M

SETS = M.box_sets()


@pytest.fixture(scope="module")
def built():
    return {name: M.build(*boxes) for name, boxes in SETS.items()}


def test_node_layout_matches_the_binding():
    from pbrlab_amd import api
    assert api.BVHNODE_DT == M.NODE_DT and M.NODE_DT.itemsize == 64


def test_interleave_two_spellings():
    r = np.random.RandomState(0)
    cell = np.concatenate([r.randint(0, 1 << 21, size=(500, 3)), [[0, 0, 0], [2097151] * 3, [1, 0, 0], [0, 1, 0], [0, 0, 1], [1 << 20, 0, 0]]])
    keys = M.interleave(cell)
    assert [int(k) for k in keys] == [M.interleave_int(*c) for c in cell]
    assert int(keys[501]) == (1 << 63) - 1 and [int(k) for k in keys[502:506]] == [4, 2, 1, 1 << 62]
    # the order of keys is the order of (x, y, z) bit triples from the top: x decides before y before z
    assert M.interleave_int(1, 0, 0) > M.interleave_int(0, 1, 1) and M.interleave_int(2, 0, 0) > M.interleave_int(1, 1, 1)


def test_cells_are_float32_arithmetic():
    """the cell of a centre is the float32 expression step by step, truncated"""
    f = np.float32
    lo = np.array([[0, 0, 0], [3, 3, 3], [1, 1.5, 2]], np.float32)
    c = M.cells(lo, lo)
    assert c.tolist() == [[0, 0, 0], [2097151] * 3, [699050, 1048575, 1398100]]
    assert [int(f(f(v) / f(3)) * f(2097151.0)) for v in (1, 1.5, 2)] == c[2].tolist()
    r = np.random.RandomState(9)
    lo, hi = r.rand(200, 3).astype(f), (1 + r.rand(200, 3)).astype(f)
    got = M.cells(lo, hi)
    ctr = [[f(0.5) * f(lo[i, a] + hi[i, a]) for a in range(3)] for i in range(200)]
    mn, mx = [min(row[a] for row in ctr) for a in range(3)], [max(row[a] for row in ctr) for a in range(3)]
    want = [[int(f(f(f(row[a] - mn[a]) / f(mx[a] - mn[a])) * f(2097151.0))) for a in range(3)] for row in ctr]
    assert got.tolist() == want
    flat = M.cells(np.zeros((4, 3), f), np.ones((4, 3), f))                 # all centres equal: extent 0 -> cell 0
    assert (flat == 0).all()


@pytest.mark.parametrize("name", sorted(SETS))
def test_model_tree_is_valid(built, name):
    lo, hi, kinds = SETS[name]
    nodes, order, depth, tree = built[name]
    M.check_tree(nodes, order, depth, lo, hi, kinds)
    assert (nodes["pad"] == 0).all()


@pytest.mark.parametrize("name", sorted(n for n in SETS if n != "random_1"))
def test_model_tree_is_the_radix_tree(built, name):
    lo, hi, kinds = SETS[name]
    nodes, order, depth, tree = built[name]
    n = len(kinds)
    keys = M.morton_keys(lo, hi)
    assert np.array_equal(order, np.argsort(keys, kind="stable")) and (np.diff(keys[order].astype(object)) >= 0).all()
    k = [int(x) for x in keys[order]]
    # in-order leaves = sorted positions 0 .. n - 1
    leaves, todo = [], [0]
    while todo:
        c = todo.pop()
        if c < 0:
            leaves.append(~c)
        else:
            todo += [tree["right"][c], tree["left"][c]]
    assert leaves == list(range(n))
    # every inner node's keys share a strictly longer prefix with each other than with either neighbour outside its range
    for i in range(n - 1):
        f, l = tree["first"][i], tree["last"][i]
        assert f < l
        own = min(M.prefix(k, f, j) for j in range(f + 1, l + 1))
        assert own == M.prefix(k, f, l)
        assert f == 0 or M.prefix(k, f - 1, f) < own
        assert l == n - 1 or M.prefix(k, l, l + 1) < own
    assert (tree["first"][0], tree["last"][0]) == (0, n - 1)


def test_expected_shapes(built):
    """what the sets are meant to exercise, from the model alone"""
    assert len(set(M.morton_keys(*SETS["one_centre_1000"][:2]).tolist())) == 1
    assert built["one_centre_1000"][2] == 11                                # 1000 positions: the tie-break tree has height 10
    keys = M.morton_keys(*SETS["duplicates_700"][:2])
    assert sorted(np.unique(keys, return_counts=True)[1])[-2:] == [300, 300]
    assert (M.cells(*SETS["flat_z_400"][:2])[:, 2] == 0).all() and (M.cells(*SETS["flat_xz_400"][:2])[:, [0, 2]] == 0).all()
    d = M.cells(*SETS["diagonal_400"][:2])
    assert (d[:, 0] == d[:, 1]).all() and (d[:, 0] == d[:, 2]).all() and len(np.unique(d[:, 0])) < 400
    nodes = built["kinds_alternate_333"][0]
    for c in ("c0", "c1"):
        leaf = (nodes[c] & M.LEAF_BIT) != 0
        assert ((nodes[c][leaf] & 7) == 0).all()                            # alternating kinds: only one-primitive leaves
    nodes = built["random_1000"][0]
    assert (((nodes["c0"] & M.LEAF_BIT) != 0) & ((nodes["c0"] & 7) == 1)).any()   # ... and two-primitive leaves elsewhere


def test_comb_depths():
    """the comb reaches exactly the traversal stack's depth, one more origin box exceeds it (commit then builds on the host)"""
    for copies, n, depth in ((1, 65, 64), (2, 66, 65), (3, 67, 66)):
        lo, hi, kinds = M.comb_boxes(copies)
        keys = M.morton_keys(lo, hi)
        assert len(kinds) == n and len(np.unique(keys)) == 65
        assert M.build(lo, hi, kinds)[2] == depth
        tri, tlo, thi = M.comb_triangles(copies)                           # the same boxes in x and y, flat in z, the same centres
        assert np.array_equal(np.float32(0.5) * (tlo + thi), M.comb_points(copies))
        assert np.array_equal(M.morton_keys(tlo, thi), keys) and M.build(tlo, thi, kinds)[2] == depth
    assert M.STACK_DEPTH == 64


def _correct():
    lo, hi, kinds = SETS["random_257"]
    nodes, order, depth, _ = M.build(lo, hi, kinds)
    M.check_tree(nodes, order, depth, lo, hi, kinds)
    return lo, hi, kinds, nodes.copy(), order.copy(), depth


# edit -> what check_tree says about it (two of them can be noticed in more than one way)
MUTATIONS = {"bound_one_ulp_inwards": "does not contain", "root_bound_one_ulp_inwards": "does not contain", "order_swapped": "does not contain|another kind",
             "leaf_count_raised": None, "leaf_count_raised_to_3": "more than MAX_LEAF", "leaf_kind_flipped": "another kind",
             "depth_lowered": "smaller than the deepest path", "child_redirected_to_sibling": None}


@pytest.mark.parametrize("what", sorted(MUTATIONS))
def test_check_tree_rejects(what):
    lo, hi, kinds, nodes, order, depth = _correct()
    muts = M.mutations(nodes, order, depth)
    assert sorted(muts) == sorted(MUTATIONS)
    with pytest.raises(M.TreeError, match=MUTATIONS[what]):
        M.check_tree(*muts[what], lo, hi, kinds)
    M.check_tree(nodes, order, depth, lo, hi, kinds)                        # (the edits were made on copies)


def test_every_bound_of_the_root_is_tight():
    """a stored bound of a reachable child is the widened bound of one of its primitives: one ulp inwards, on any side, is rejected"""
    lo, hi, kinds, nodes, order, depth = _correct()
    for field, towards in (("lo", np.inf), ("hi", -np.inf)):
        for a in range(3):
            for c in range(2):
                mutated = nodes.copy()
                mutated[field][0, a, c] = np.nextafter(mutated[field][0, a, c], np.float32(towards))
                with pytest.raises(M.TreeError, match="does not contain"):
                    M.check_tree(mutated, order, depth, lo, hi, kinds)


def test_comparison_with_the_model_rejects_what_check_tree_cannot_see():
    """edits that leave a valid tree -- a wider box, a node below a collapsed leaf, pad -- fail the bitwise comparison; -0 for +0 does not"""
    lo, hi, kinds, nodes, order, depth = _correct()
    assert len(M.nodes_mismatch(nodes, nodes.copy())) == 0
    wider = nodes.copy()
    wider["lo"][5, 0, 1] = np.nextafter(wider["lo"][5, 0, 1], np.float32(-np.inf))
    M.check_tree(wider, order, depth, lo, hi, kinds)
    assert M.nodes_mismatch(nodes, wider).tolist() == [5]
    i, f, _ = M.reachable_leaf(nodes, 2)
    hidden = (int(nodes[f][i]) >> 3 & 0x7FFFFFF) + (1 if f == "c0" else 0)    # the inner node over that pair (left child: its last slot)
    below = nodes.copy()
    below["c1"][hidden] ^= 8
    M.check_tree(below, order, depth, lo, hi, kinds)
    assert M.nodes_mismatch(nodes, below).tolist() == [hidden]
    padded = nodes.copy()
    padded["pad"][7, 1] = 1
    assert M.nodes_mismatch(nodes, padded).tolist() == [7]
    z = np.zeros(2, M.NODE_DT)
    mz = z.copy()
    mz["lo"][0, 0, 0], mz["hi"][1, 2, 1] = np.float32(-0.0), np.float32(-0.0)
    assert len(M.nodes_mismatch(z, mz)) == 0


def test_check_tree_on_degenerate_sizes():
    for name in ("random_1", "random_2", "random_3"):
        lo, hi, kinds = SETS[name]
        nodes, order, depth, _ = M.build(lo, hi, kinds)
        M.check_tree(nodes, order, depth, lo, hi, kinds)
        with pytest.raises(M.TreeError):
            M.check_tree(nodes, order, depth + 1, lo, hi, kinds)
    lo, hi, kinds = SETS["random_1"]
    nodes, order, depth, _ = M.build(lo, hi, kinds)
    assert nodes["c1"][0] == M.EMPTY_CHILD and np.isnan(nodes["lo"][0, :, 1]).all() and depth == 1


def test_large_set_reaches_the_stride_loop():
    """more boxes than k_lbvh_bounds has threads; its keys and stable order are what the GPU test compares exactly"""
    lo, hi, kinds = M.large_set()
    assert len(kinds) == M.LARGE_N > 2048 * 256
    keys = M.morton_keys(lo, hi)
    order = np.argsort(keys, kind="stable")
    assert (np.diff(keys[order].astype(np.int64)) >= 0).all()
