"""CPU: the exact model of the refit (tests/_refit_model.py; DESIGN.md section 8, "The refit, exactly") before it is pointed at the device
(tests/test_refit_gpu.py).

The identity property: on every primitive set, a refit with UNCHANGED slots gives back the bytes of the tree the builder's model made --
binary nodes, Q nodes, records (the 1e6-shifted set and the sixty-decade set included).  The model forms every child's box from all slots
below it and widens once, as both builders do; the kernels keep unwidened unions in working arrays for the same reason -- uniting
widened boxes would be cheaper, but widening is not monotone everywhere, which is stated here.  Then: moved slots give valid trees, doctored
outputs are rejected, the array quantiser is the scalar one, the kernels exist by name without scratch, and the entry points fail loudly
without a device."""
import numpy as np
import pytest

import _codeobj as CO
import _lbvh_model as M
import _qcollapse_model as Q
import _refit_model as R

SETS = Q.all_sets()
F = np.float32
EINVAL, ENODEVICE = -1, -3
KERNELS = ["k_rf_bin", "k_rf_pack", "k_rf_plan", "k_rf_q", "k_rf_scatter"]


def _built(name):
    lo, hi, kinds, slots = R.case(*SETS[name])
    nodes, order, depth, q = Q.build(lo, hi, kinds, slots)
    return nodes, slots[order], kinds[order] != 0, q, depth


@pytest.mark.parametrize("name", sorted(SETS))
def test_unchanged_slots_give_back_the_built_tree(name):
    nodes, slots, curve, q, depth = _built(name)
    assert q["quantised"]
    n2, q2 = R.refit(nodes, slots, q)
    assert R.differences(n2, q2, nodes, q) == []
    n3, none = R.refit(nodes, slots)
    assert none is None and n3.tobytes() == nodes.tobytes()
    R.check(n2, slots, q2, depth)


def test_widening_is_not_monotone_everywhere():
    """Why the kernels keep UNWIDENED unions in their working arrays instead of uniting the widened boxes a child node stores: W(min(a, b))
    == min(W(a), W(b)) needs W to be non-decreasing, and v -+ (|v| * 2^-16 + 1e-30) is that only where the relative term carries the
    rounding: from 4e-30 upwards over neighbouring floats of random values and of every binade boundary -- but not below, where the sum
    in brackets steps by one ulp of 1e-30 (9.4e-38) between two neighbours that are 2.8e-40 apart."""
    r = np.random.RandomState(9)
    v = np.concatenate([(r.rand(200000).astype(np.float32) - F(0.5)) * (F(10.0) ** r.uniform(-38, 31, 200000)).astype(np.float32),
                        np.ldexp(F(1), np.arange(-126, 104)).astype(np.float32), -np.ldexp(F(1), np.arange(-126, 104)).astype(np.float32),
                        np.array([0.0, -0.0, 1e-30, -1e-30, 1e6, 1e6 + 0.0625], np.float32)])
    v = np.sort(np.concatenate([v, np.nextafter(v, F(np.inf)), np.nextafter(v, F(-np.inf))]))
    assert (M.widen_lo(v) < v).all() and (M.widen_hi(v) > v).all()        # strictly outside: a stored bound is never +-0
    for side in (v[v >= F(4e-30)], v[v <= F(-4e-30)]):
        assert len(side) > 100000
        for w in (M.widen_lo, M.widen_hi):
            assert (np.diff(w(side)) >= 0).all()
    a = F(3.081488e-33)
    b = np.nextafter(a, F(1))
    assert a < b and M.widen_lo(a) > M.widen_lo(b)                        # the counter-example
    assert M.widen_lo(min(a, b)) != min(M.widen_lo(a), M.widen_lo(b))     # the union of widened boxes is not the widened union


@pytest.mark.parametrize("name", ["random_5", "random_257", "mixed_500", "shifted_1e6_300", "span_1e-30_1e30_600", "comb_65", "flat_xz_400"])
def test_array_quantiser_is_the_scalar_one(name):
    nodes, slots, curve, q, depth = _built(name)
    Qn = q["qnodes"]
    todo, fronts = [0], {}
    while todo:
        v = todo.pop()
        fronts[v] = Q.frontier(nodes, v)
        todo.extend(r for r, _, _ in fronts[v] if not r & Q.LEAF_BIT)
    heads = sorted(fronts)
    blo, bhi, cnt = np.zeros((len(heads), 4, 3), F), np.zeros((len(heads), 4, 3), F), np.zeros(len(heads), np.int64)
    for i, v in enumerate(heads):
        cnt[i] = len(fronts[v])
        for k, (_, lo, hi) in enumerate(fronts[v]):
            blo[i, k], bhi[i, k] = lo, hi
    org, step, qlo, qhi, ok = R.quantise_np(blo, bhi, cnt)
    assert ok.all()
    assert org.tobytes() == Qn["org"].tobytes() and qlo.tobytes() == Qn["qlo"].tobytes() and qhi.tobytes() == Qn["qhi"].tobytes()
    assert np.stack([Qn["sx"], Qn["sy"], Qn["sz"]], axis=1).tobytes() == step.tobytes()


def test_array_quantiser_on_nodes_a_few_ulps_wide():
    """nodes a few ulps wide far from the origin, where the grid is finer than org's resolution: the scalar quantiser's words"""
    r = np.random.RandomState(12)
    m = 300
    base = (F(1e6) + r.randint(0, 64, (m, 1, 3)).astype(np.float32) * F(0.0625)).astype(np.float32)
    blo = (base + r.randint(0, 4, (m, 4, 3)).astype(np.float32) * F(0.0625)).astype(np.float32)
    bhi = (blo + r.randint(0, 6, (m, 4, 3)).astype(np.float32) * F(0.0625)).astype(np.float32)
    cnt = r.randint(1, 5, m)
    org, step, qlo, qhi, ok = R.quantise_np(blo, bhi, cnt)
    for i in range(m):
        want = Q.quantise([(blo[i, k], bhi[i, k]) for k in range(cnt[i])])
        assert ok[i] and want is not None
        assert [org[i].tolist(), step[i].tolist(), qlo[i].tolist(), qhi[i].tolist()] == [[float(x) for x in want[0]], [float(x) for x in want[1]], want[2], want[3]], i


def test_array_quantiser_refuses_what_the_scalar_one_refuses():
    z = np.zeros((1, 4, 3), F)
    inf = z.copy()
    inf[0, 0, 0] = np.inf
    assert not R.quantise_np(z, inf, np.ones(1, np.int64))[4][0]
    nan = z.copy()
    nan[0, 0, 1] = np.nan
    assert not R.quantise_np(nan, z, np.ones(1, np.int64))[4][0]
    org, step, qlo, qhi, ok = R.quantise_np(z, z, np.ones(1, np.int64))
    assert ok[0] and (step == Q.FLT_MIN).all() and (qlo == 0xFFFFFF00).all() and (qhi == 0).all()


@pytest.mark.parametrize("how", R.PERTURBATIONS)
@pytest.mark.parametrize("name", ["random_1", "random_2", "random_3", "random_257", "mixed_500", "kinds_alternate_333", "shifted_1e6_300",
                                  "span_1e-30_1e30_600", "comb_66", "one_centre_1000"])
def test_moved_slots_give_a_valid_pair(name, how):
    nodes, slots, curve, q, depth = _built(name)
    moved = R.perturb(slots, curve, how)
    n2, q2 = R.refit(nodes, moved, q)
    R.check(n2, moved, q2, depth)
    # topology, codes and padding stayed
    for f in ("c0", "c1", "pad"):
        assert n2[f].tobytes() == nodes[f].tobytes()
    assert q2["qnodes"]["c"].tobytes() == q["qnodes"]["c"].tobytes() and q2["hit"].tobytes() == q["hit"].tobytes()
    assert not q2["pts"][:4].any() and not q2["pts"][-4:].any()
    if (name, how) not in (("span_1e-30_1e30_600", "shift_1e6"), ("shifted_1e6_300", "jitter")):   # (moves below the resolution of the coordinates)
        assert "nodes" in R.differences(n2, q2, nodes, q)


def test_doctored_refits_are_rejected():
    """one stale box, one stale record word, one changed reference: each differs from the model, and the checkers reject the pair"""
    nodes, slots, curve, q, depth = _built("mixed_500")
    moved = R.perturb(slots, curve, "far")
    n2, q2 = R.refit(nodes, moved, q)
    R.check(n2, moved, q2, depth)
    first_moved = int(np.flatnonzero((moved != slots).any(axis=(1, 2)))[0])
    # the parent of that slot's leaf, in either tree
    bi, bc = next((i, c) for i in range(len(nodes)) for c, f in enumerate(("c0", "c1"))
                  if nodes[f][i] & Q.LEAF_BIT and nodes[f][i] != Q.EMPTY_CHILD and Q.leaf_fields(int(nodes[f][i]))[0] <= first_moved
                  < sum(Q.leaf_fields(int(nodes[f][i]))[:2]))
    stale = n2.copy()
    stale["lo"][bi, :, bc], stale["hi"][bi, :, bc] = nodes["lo"][bi, :, bc], nodes["hi"][bi, :, bc]
    assert R.differences(stale, q2, n2, q2) == ["nodes"]
    with pytest.raises(M.TreeError):
        R.check(stale, moved, q2, depth)
    # a Q node left as it was
    changed = np.flatnonzero((q2["qnodes"]["org"] != q["qnodes"]["org"]).any(axis=1))
    assert len(changed)
    qs = dict(q2, qnodes=q2["qnodes"].copy())
    leafy = next(int(i) for i in changed[::-1] if (q["qnodes"]["c"][i] & Q.LEAF_BIT).all())
    qs["qnodes"][leafy] = q["qnodes"][leafy]
    assert R.differences(n2, qs, n2, q2) == ["qnodes"]
    with pytest.raises(Q.QTreeError):
        R.check(n2, moved, qs, depth)
    # a record word left as it was: a point of a curve record, a corner of a triangle slot
    for part in ("pts", "tri"):
        w = int(np.flatnonzero((q2[part] != q[part]).any(axis=1))[0])
        qs = dict(q2, **{part: q2[part].copy()})
        qs[part][w] = q[part][w]
        assert R.differences(n2, qs, n2, q2) == [part]
        with pytest.raises(Q.QTreeError):
            R.check(n2, moved, qs, depth)
    # a changed reference
    i, k = Q._find(q2, lambda r: bool(r & Q.LEAF_BIT) and not r & Q.CURVE_BIT)
    qs = dict(q2, qnodes=q2["qnodes"].copy())
    qs["qnodes"]["c"][i, k] += 8
    assert R.differences(n2, qs, n2, q2) == ["qnodes"]
    with pytest.raises(Q.QTreeError):
        R.check(n2, moved, qs, depth)
    swapped = n2.copy()
    swapped["c0"][0], swapped["c1"][0] = n2["c1"][0], n2["c0"][0]
    assert R.differences(swapped, q2, n2, q2) == ["nodes"]
    with pytest.raises(AssertionError):
        R.check(swapped, moved, q2, depth)


def test_every_refit_kernel_is_listed_and_uses_no_scratch():
    assert CO.available(), "libpbrhip.so or the LLVM tools are missing"
    import _codeobj_tus as T
    table = T.kernel_table()
    mine = {k.split("::")[-1].split("(")[0]: v for k, v in table.items() if "k_rf_" in k}
    print({k: (v["vgpr_count"], v["private_segment_fixed_size"]) for k, v in mine.items()})
    assert sorted(mine) == KERNELS
    for k, v in mine.items():
        assert v["private_segment_fixed_size"] == 0, (k, v)


def test_symbols_and_names_exist():
    import pbrlab_amd as pa
    from pbrlab_amd import _lib, api
    L = _lib.lib()
    for name in ("pbrhip_scene_update_triangle_mesh", "pbrhip_scene_update_curve_mesh", "pbrhip_scene_update_instance_transform",
                 "pbrhip_scene_refit", "pbrhip_tree_refit"):
        assert name in _lib.EXPORTS and hasattr(L, name), name
    for name in ("UpdateTriangleMesh", "UpdateCurveMesh", "UpdateInstanceTransform", "RefitScene"):
        assert hasattr(pa.Scene, name), name
    assert hasattr(api, "tree_refit") and L.pbrhip_abi_version() == 6


def test_entry_points_fail_loudly():
    """a NULL scene is refused by every new entry point; without a device there is no scene to edit and the hook says so"""
    import pbrlab_amd as pa
    from pbrlab_amd import _lib
    L = _lib.lib()
    v = np.zeros((3, 4), np.float32)
    assert L.pbrhip_scene_update_triangle_mesh(None, 0, v.ctypes.data, 3, None, 0) == EINVAL
    assert L.pbrhip_scene_update_curve_mesh(None, 0, v.ctypes.data, 3) == EINVAL
    assert L.pbrhip_scene_update_instance_transform(None, 0, None) == EINVAL
    assert L.pbrhip_scene_refit(None) == EINVAL and b"NULL" in L.pbrhip_last_error()
    nodes, slots, curve, q, depth = _built("random_3")
    assert L.pbrhip_tree_refit(0, 3, None, nodes.ctypes.data, None, 0, None, 0, 0, None, None, 0) == EINVAL
    assert L.pbrhip_tree_refit(0, 1 << 27, slots.ctypes.data, nodes.ctypes.data, None, 0, None, 0, 0, None, None, 0) == EINVAL
    assert L.pbrhip_tree_refit(0, 0, None, None, None, 0, None, 0, 0, None, None, 0) == 0            # n == 0: nothing to do
    if pa.device_count() == 0:
        with pytest.raises(pa.PbrHipError) as e:
            pa.api.tree_refit(slots, nodes, q)
        assert e.value.code == ENODEVICE
        with pytest.raises(pa.PbrHipError) as e:
            pa.Scene()                                                    # ... and no scene whose geometry could be edited
        assert e.value.code == ENODEVICE


def test_shim_has_the_edit_calls(tmp_path):
    """include/pbrlab_hip.hpp: the four names compile against the header with the argument types a caller holds"""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / "shim_refit.cc"
    src.write_text('#include "pbrlab_hip.hpp"\n'
                   "void edit(pbrlab::Scene& s, const pbrlab::MeshPtr& tri, const pbrlab::MeshPtr& hair, const std::vector<float>& v, const float m[4][4]) {\n"
                   "  s.UpdateTriangleMesh(tri, v);\n  s.UpdateTriangleMesh(tri, v, v);\n  s.UpdateCurveMesh(hair, v);\n"
                   "  s.UpdateInstanceTransform(0u, m);\n  s.RefitScene();\n}\n")
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I" + os.path.join(root, "include"), str(src)])
