"""CPU: the exact model of the device collapse (tests/_qcollapse_model.py; DESIGN.md section 8, "The collapse, exactly") and its
structural checker, before either is pointed at the device (tests/test_qcollapse_gpu.py): the model's trees pass the checker on every
primitive set, the checker rejects doctored trees (one wrong byte or reference each), the smallest trees have the shapes the
definition gives, and the quantiser both builders now share (pbrlab_amd/csrc/qquant.h) left the HOST builder's output unchanged: a
stand-alone program over bvh_build.cpp prints hashes of build_qlayout's output for a few soups, recorded before the move."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import _lbvh_model as M
import _qcollapse_model as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
SETS = Q.all_sets()
F = np.float32


def _built(name, all_triangles=False):
    lo, hi, kinds = SETS[name]
    if all_triangles:
        kinds = np.zeros(len(kinds), np.uint8)
    slots = Q.make_slots(lo, hi, kinds)
    nodes, order, depth, q = Q.build(lo, hi, kinds, slots)
    return nodes, slots[order], q


def test_array_fmaf_equals_libm():
    """the checker's vectorised fmaf is libm's: random operands, exact ties of the float64 sum, huge and tiny magnitudes"""
    r = np.random.RandomState(5)
    q = r.randint(0, 256, 40000).astype(np.float32)
    s = (r.rand(40000) * 10.0 ** r.uniform(-35, 30, 40000)).astype(np.float32)
    org = ((r.rand(40000) - 0.5) * 10.0 ** r.uniform(-35, 30, 40000)).astype(np.float32)
    # ties: org + q * s exactly half way between two float32 (s = half an ulp of org, q odd), and one float64 ulp beside them
    base = (1 + r.randint(0, 1 << 23, 2000)).astype(np.float32) * F(2.0) ** -23 + F(1)
    q[:2000], org[:2000] = (2 * r.randint(0, 128, 2000) + 1), base
    s[:1000] = F(2.0) ** -24
    s[1000:2000] = np.nextafter(F(2.0) ** -24, F(1))
    got = Q.fmaf_np(q, s, org)
    want = np.array([Q.fmaf(a, b, c) for a, b, c in zip(q, s, org)], np.float32)
    assert got.tobytes() == want.tobytes()


@pytest.mark.parametrize("name", sorted(SETS))
def test_model_tree_passes_the_checker(name):
    nodes, slots, q = _built(name)
    assert q["quantised"]
    Q.check_qtree(nodes, slots, q)
    assert Q.stack_need(q["qnodes"]) == q["stack_need"]
    n = len(slots)
    assert len(q["qnodes"]) <= max(n - 1, 1) and len(q["pts"]) % 4 == 0 and len(q["tri"]) % 4 == 0


def test_checker_rejects_doctored_trees():
    nodes, slots, q = _built("mixed_500")
    Q.check_qtree(nodes, slots, q)
    muts = Q.mutations(q)
    assert len(muts) == 20
    for what, edited in muts.items():
        try:
            Q.check_qtree(nodes, slots, edited)
        except Q.QTreeError:
            continue
        pytest.fail(f"the checker accepted the doctored tree '{what}'")
    # ... and on a triangle-only set (TriPair records)
    nodes, slots, q = _built("random_257", all_triangles=True)
    Q.check_qtree(nodes, slots, q)
    for word, lane in ((0, 1), (4, 2), (4, 3), (2, 0)):
        e = dict(q, tri=q["tri"].copy())
        e["tri"].view(np.uint32)[word, lane] ^= 1
        with pytest.raises(Q.QTreeError):
            Q.check_qtree(nodes, slots, e)


def test_smallest_trees():
    """n = 1: one node holding the leaf; n = 2, 3: one node, two leaves (a subtree of two triangles is a leaf); n = 5: one node whose
    frontier took the root's inner child apart -- three leaves, stack need 2"""
    E = Q.EMPTY_CHILD
    want = {1: ([0x80000000, E, E, E], 0), 2: ([0x80000000, 0x80000008, E, E], 1), 3: ([0x80000000, 0x80000009, E, E], 1),
            5: ([0x80000001, 0x80000009, 0x80000010, E], 2)}
    for n, (children, need) in want.items():
        nodes, slots, q = _built(f"random_{n}", all_triangles=True)
        assert len(q["qnodes"]) == 1 and q["qnodes"]["c"][0].tolist() == children and q["stack_need"] == need, n
        used = sum(c != E for c in children)
        for a in range(3):                                               # unused children: qlo byte 255, qhi byte 0
            assert all((int(q["qnodes"]["qlo"][0, a]) >> (8 * k)) & 255 == 255 for k in range(used, 4))
            assert all((int(q["qnodes"]["qhi"][0, a]) >> (8 * k)) & 255 == 0 for k in range(used, 4))
        assert len(q["pts"]) == 8 and not q["pts"].any() and (q["hit"] == Q.NONE).all()
        Q.check_qtree(nodes, slots, q)
    # one curve piece: the record at point 4, its reference P | sub, no pair bit
    lo, hi, _ = SETS["random_1"]
    slots = Q.make_slots(lo, hi, np.ones(1, np.uint8))
    nodes, order, depth, q = Q.build(lo, hi, np.ones(1, np.uint8), slots)
    sub = int(slots.view(np.uint32)[0, 2, 0]) & 3
    assert q["qnodes"]["c"][0].tolist() == [Q.LEAF_BIT | Q.CURVE_BIT | ((4 | sub) << 3), E, E, E]
    assert len(q["pts"]) == 12 and len(q["tri"]) == 0 and q["hit"].tolist()[4] == int(slots.view(np.uint32)[0, 2, 3])
    Q.check_qtree(nodes, slots, q)


def test_frontier_rule():
    """the greedy rule on a hand-made tree: the member with the largest area is taken apart first, ties go to the earliest, the two
    children replace it in place"""
    B = np.zeros(4, M.NODE_DT)
    leaf = lambda k: M.leaf_ref(0, k, 1)                                 # noqa: E731

    def box(i, c, lo, hi):
        B["lo"][i, :, c], B["hi"][i, :, c] = lo, hi
    B["c0"][0], B["c1"][0] = 1, 2                                        # two inner children of equal area: the earliest goes first
    box(0, 0, 0, 1), box(0, 1, 2, 3)
    B["c0"][1], B["c1"][1] = leaf(0), leaf(1)
    box(1, 0, 0, 0.5), box(1, 1, 0.5, 1)
    B["c0"][2], B["c1"][2] = 3, leaf(4)
    box(2, 0, 2, 2.5), box(2, 1, 2.5, 3)
    B["c0"][3], B["c1"][3] = leaf(2), leaf(3)
    box(3, 0, 2, 2.25), box(3, 1, 2.25, 2.5)
    assert [r for r, _, _ in Q.frontier(B, 0)] == [leaf(0), leaf(1), 3, leaf(4)]
    box(0, 0, 0, 0.25)                                                   # the first is the smallest now: node 2 goes first, then node 3
    assert [r for r, _, _ in Q.frontier(B, 0)] == [1, leaf(2), leaf(3), leaf(4)]
    assert Q.area(np.array([0, 0, 0], F), np.array([1, 2, 3], F)) == F(11)


def test_quantiser_edges():
    """a box of no extent: the FLT_MIN step; bounds are moved outwards until fmaf(q, s, org) encloses the child; a box that is not finite
    cannot be quantised"""
    z = np.zeros(3, F)
    org, step, qlo, qhi, retries = Q.quantise([(z, z)])
    assert step == [Q.FLT_MIN] * 3 and [w & 255 for w in qlo] == [0, 0, 0] and [w & 255 for w in qhi] == [0, 0, 0] and retries == 0
    lo, hi = np.array([1e6, -3, 0.1], F), np.array([1e6 + 0.25, 5, 0.7], F)
    inner = (lo + F(0.3) * (hi - lo), lo + F(0.6) * (hi - lo))
    org, step, qlo, qhi, _ = Q.quantise([(lo, hi), inner])
    for a in range(3):
        for k, (blo, bhi) in enumerate([(lo, hi), inner]):
            assert Q.fmaf((qlo[a] >> (8 * k)) & 255, step[a], org[a]) <= blo[a] and Q.fmaf((qhi[a] >> (8 * k)) & 255, step[a], org[a]) >= bhi[a]
        assert (qlo[a] >> 16) == 0xFFFF and (qhi[a] >> 16) == 0
    assert Q.quantise([(z, np.array([np.inf, 0, 0], F))]) is None and Q.quantise([(np.array([np.nan, 0, 0], F), z)]) is None


def test_host_built_trees_are_unchanged(tmp_path):
    """build_qlayout over bvh_build.cpp of the working tree == the hashes recorded from the file before the quantiser became a shared
    header (tests/golden/qlayout_hashes.txt).  The translation unit includes the HIP headers (vector types), hence hipcc, host only.
    (shifted_1e6_800 -- boxes that float32 collapses to points of a 1/16 grid around 1e6 -- was recorded again when the builder began
    to halve ranges whose box has no area instead of peeling one primitive off per level: 175 nodes where there were 221.)"""
    assert os.path.exists(HIPCC), "hipcc builds the library: without it nothing here can be tested"
    cs = os.path.join(ROOT, "pbrlab_amd", "csrc")
    exe = str(tmp_path / "qlayout_hash")
    subprocess.check_call([HIPCC, "--offload-host-only", "-std=c++17", "-O1", "-ffp-contract=off", "-I" + cs, "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "qlayout_hash.cc"), os.path.join(cs, "bvh_build.cpp"), "-o", exe, "-lpthread"])
    got = subprocess.run([exe], capture_output=True, text=True, timeout=300, check=True).stdout
    want = open(os.path.join(ROOT, "tests", "golden", "qlayout_hashes.txt")).read()
    assert got.splitlines() == want.splitlines() and len(want.splitlines()) == 8
