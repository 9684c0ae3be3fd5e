"""K-nearest queries without a GPU: the symbols and names exist and the ABI version stands; the numpy model of the
contract (tests/_knearest_model.py) is pinned to the nearest-point model -- its first entry is tests/_query_model.py's brute force byte
for byte, shorter lists are prefixes of longer ones --; the soup's query set meets the cases the GPU comparison
(tests/test_knearest_gpu.py) needs, so that it cannot pass vacuously; the order (D2, gid, sub) on hand-made cases; and the entry points
refuse bad arguments before any device work."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import _knearest_model as KM
import _query_model as QM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("pbrhip_k_nearest", "pbrhip_k_nearest_device")
NAMES = ("KNearest", "KNearestDevice")
EINVAL = -1
F = np.float32
NONE = 0xFFFFFFFF
CUTS = (1, 4, 32)


def test_symbols_and_names_exist():
    from pbrlab_amd import _lib, api
    L = _lib.lib()
    hdr = open(os.path.join(ROOT, "include", "pbrhip.h")).read()
    shim = open(os.path.join(ROOT, "include", "pbrlab_hip.hpp")).read()
    for name in SYMBOLS:
        assert name in _lib.EXPORTS and hasattr(L, name) and re.search(r"\b" + name + r"\s*\(", hdr), name
    for name in NAMES:
        assert hasattr(api.Scene, name) and re.search(r"\b" + name + r"\b", shim), name
    assert re.search(r"#define PBRHIP_K_NEAREST_MAX 32u\b", hdr) and api.K_NEAREST_MAX == 32
    assert L.pbrhip_abi_version() == 6 and re.search(r"#define PBRHIP_ABI_VERSION 6u\b", hdr)  # functions only: the layouts stand
    # k-nearest left the "Not provided" lists
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for text in (hdr, design):
        for m in re.finditer(r"Not provided", text):
            end = re.search(r"\*/|\n\n", text[m.start():])
            assert "k-nearest" not in text[m.start():m.start() + (end.start() if end else 2000)], text[m.start():m.start() + 300]
    assert "## 22." in design


def soup_points(tris, seed):
    """tests/_query_model.py::soup_points with the unbounded queries 1, 4, 7, ... given the radius 0.25: a third at 0.05, a third at
    0.25, a third unbounded"""
    pts = QM.soup_points(tris, seed, 3000)
    pts[1::3, 3] = F(0.25)
    return pts


@functools.lru_cache(maxsize=None)
def soup_case(seed):
    """-> (points, slots, shade, the model with 33 listed) of the soup with 30 extra slivers; slot = gid = the triangle's index"""
    import _soups
    desc = _soups.triangle_soup(seed, 30)[0]
    tris = np.ascontiguousarray(desc.vertices[:, :3].reshape(-1, 3, 3), F)
    n = len(tris)
    slots, shade = np.zeros((n, 4, 4), F), np.zeros((n, 32), np.uint32)
    slots[:, :3, :3], shade[:, 24] = tris, np.arange(n)
    pts = soup_points(tris, seed)
    cand = QM.candidates(pts, slots, shade)
    return pts, slots, shade, KM.brute_force(pts, slots, shade, 33, cand=cand), cand


@pytest.mark.parametrize("seed", (0, 1, 3))
def test_model_entry_0_is_the_nearest_point_models_answer(seed):
    pts, slots, shade, res, cand = soup_case(seed)
    want_ident, want_closest = QM.expected_buffers(QM.brute_force(pts, slots, shade, cand=cand))
    one = KM.brute_force(pts, slots, shade, 1, cand=cand)
    assert one["ident"][:, 0].tobytes() == want_ident.tobytes() and one["closest"][:, 0].tobytes() == want_closest.tobytes()
    assert np.array_equal(one["count"] > 0, want_ident[:, 0] != NONE)
    # shorter lists are prefixes of longer ones, and count does not depend on K
    for k in (0, 1, 4, 32):
        part = KM.brute_force(pts, slots, shade, k, cand=cand)
        assert part["ident"].tobytes() == np.ascontiguousarray(res["ident"][:, :k]).tobytes(), k
        assert part["closest"].tobytes() == np.ascontiguousarray(res["closest"][:, :k]).tobytes(), k
        assert np.array_equal(part["count"], res["count"]), k
    # the listed D2 ascend, and the distance is their square root
    d2 = res["closest"][:, :, 3]
    listed = np.arange(33)[None, :] < res["count"][:, None]
    assert (np.where(listed, d2, np.inf)[:, 1:] >= np.where(listed, d2, np.inf)[:, :-1]).all()
    assert np.array_equal(res["ident"][:, :, 3][listed], np.sqrt(d2[listed]).view(np.uint32))


@pytest.mark.parametrize("seed", (0, 1, 3))
def test_soup_meets_the_cases_the_gpu_comparison_needs(seed):
    """seed 3 is the soup tests/test_knearest_gpu.py runs"""
    pts, slots, shade, res, cand = soup_case(seed)
    count, ident, closest, d2 = res["count"], res["ident"], res["closest"], res["d2"]
    n = len(slots)
    assert n == 430 and len(pts) == 3000
    cuts = {k: int(((count > k) & (d2[:, k - 1] == d2[:, k])).sum()) for k in CUTS}
    print(f"seed {seed}: count == 0: {int((count == 0).sum())}, 4 < count <= 32: {int(((count > 4) & (count <= 32)).sum())}, "
          f"32 < count < {n}: {int(((count > 32) & (count < n)).sum())}, count == {n}: {int((count == n).sum())}, ties across the cuts: {cuts}")
    assert (count == 0).sum() >= 100 and (count > 4).sum() >= 100
    assert ((count > 32) & (count < n)).sum() >= 10
    assert (count == n).sum() == 1000  # the unbounded third: no D2 of this soup is a NaN
    for k in CUTS:
        assert cuts[k] >= 40, (k, cuts)
        assert np.array_equal(KM.brute_force(pts, slots, shade, k, cand=cand)["ties"], (count > k) & (d2[:, k - 1] == d2[:, k]))
    # triangles 100 .. 119 are exact duplicates of 60 .. 79: a list that holds one holds its twin before it, with equal candidate bytes
    rows, cols = np.nonzero((ident[:, :32, 0] >= 100) & (ident[:, :32, 0] < 120))
    assert len(rows) >= 50
    twin = ((ident[rows, :32, 0] == (ident[rows, cols, 0] - 40)[:, None]) & (ident[rows, :32, 1:] == ident[rows, cols, None, 1:]).all(axis=-1)
            & (closest[rows, :32].view(np.uint32) == closest[rows, cols, None].view(np.uint32)).all(axis=-1))
    assert (twin & (np.arange(32)[None, :] < cols[:, None])).any(axis=1).all()


def test_the_order_is_d2s_not_the_distances():
    """sqrtf merges distinct D2: queries whose list holds two successive entries with different D2 and equal distance words.  The model
    -- and the kernel -- order them by D2, which closest's w shows."""
    pts, slots, shade, res, cand = soup_case(3)
    d2, dist = res["closest"][:, :, 3], res["ident"][:, :, 3]
    listed = np.arange(33)[None, :] < res["count"][:, None]
    merged = listed[:, 1:] & (d2[:, 1:] != d2[:, :-1]) & (dist[:, 1:] == dist[:, :-1])
    rows = np.nonzero(merged.any(axis=1))[0]
    print(f"{len(rows)} of {len(pts)} queries with two of their first 33 entries at different D2 and equal sqrt(D2)")
    assert len(rows) >= 1
    q, j = rows[0], int(np.argmax(merged[rows[0]]))
    assert d2[q, j] < d2[q, j + 1] and dist[q, j] == dist[q, j + 1] and res["ident"][q, j, 0] != res["ident"][q, j + 1, 0]


def test_model_orders_ties_by_gid_and_drops_inactive_queries():
    tri = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], F)
    slots, shade = np.zeros((4, 4, 4), F), np.zeros((4, 32), np.uint32)
    slots[:, :3, :3] = tri
    slots[2, :3, 2], slots[3, :3, 2] = -1.0, 0.5
    shade[:, 24] = (7, 3, 1, 9)  # slots 0 and 1 coincide: gid 3 before gid 7; slot 3 is nearer, slot 2 farther
    pts = np.zeros((5, 4), F)
    pts[:, :3], pts[:, 3] = (0.25, 0.25, 2.0), np.inf  # distances 1.5 (slot 3), 2 (slots 1, 0), 3 (slot 2)
    pts[1, 3] = 2.0    # max_dist exactly ON the coinciding pair: D2 <= max_dist^2 accepts
    pts[2, 3] = 1.75   # the nearest alone
    pts[3, 0] = np.nan  # inactive
    pts[4, 3] = -1.0   # inactive
    res = KM.brute_force(pts, slots, shade, 3)
    assert res["count"].tolist() == [4, 3, 1, 0, 0] and res["ties"].tolist() == [False] * 5
    assert res["ident"][0, :, 0].tolist() == [3, 1, 0] and res["ident"][0, :, 3].view(F).tolist() == [1.5, 2.0, 2.0]
    assert res["ident"][1, :, 0].tolist() == [3, 1, 0] and res["ident"][2, :, 0].tolist() == [3, NONE, NONE]
    assert (res["ident"][3:] == (NONE, 0, 0, 0)).all() and not res["closest"][3:].any() and not res["closest"][2, 1:].any()
    assert res["ident"][0, 0].tolist() == [3] + np.array([0.25, 0.25, 1.5], F).view(np.uint32).tolist()
    assert res["closest"][0].tolist() == [[0.25, 0.25, 0.5, 2.25], [0.25, 0.25, 0.0, 4.0], [0.25, 0.25, 0.0, 4.0]]
    assert KM.brute_force(pts, slots, shade, 2)["ties"].tolist() == [True, True, False, False, False]  # the pair straddles the cut at K = 2
    assert KM.brute_force(pts, slots, shade, 0)["count"].tolist() == [4, 3, 1, 0, 0]


def cubic_pieces(order):
    """one cubic as four pieces along the x axis, joints at x = 0 .. 4 (exactly representable), radius 1/8, in the slot order `order`"""
    slots, shade = np.zeros((4, 4, 4), F), np.zeros((4, 32), np.uint32)
    for s, sub in enumerate(order):
        slots[s, 0], slots[s, 1] = (sub, 0, 0, 0.125), (sub + 1, 0, 0, 0.125)
        slots[s, 2, 0] = np.array([sub], np.uint32).view(F)[0]
    shade[:, 3], shade[:, 24] = QM.SLOT_IS_CURVE << 24, 5
    return slots, shade


@pytest.mark.parametrize("order", [(0, 1, 2, 3), (3, 2, 1, 0), (2, 0, 3, 1)])
def test_two_pieces_of_a_cubic_at_one_joint_are_ordered_by_sub(order):
    """a query on the normal through the joint x = 2: pieces 1 and 2 at equal D2, gid and u = 0.5 -- the smaller sub first, under every
    slot order"""
    slots, shade = cubic_pieces(order)
    pts = np.array([[2.0, 1.0, 0.0, np.inf], [2.0, 1.0, 0.0, 1.0]], F)
    res = KM.brute_force(pts, slots, shade, 4)
    sub = KM.sub_of(slots, shade)
    assert sub.tolist() == list(order) and res["count"].tolist() == [4, 2]
    assert sub[res["ident"][0, :, 0]].tolist() == [1, 2, 0, 3] and sub[res["ident"][1, :2, 0]].tolist() == [1, 2]
    a, b = res["ident"][0, 0], res["ident"][0, 1]
    assert a[0] != b[0] and a[1:].tolist() == b[1:].tolist() == np.array([0.5, 0.0, 1.0], F).view(np.uint32).tolist()
    assert res["closest"][0, :2].tolist() == [[2.0, 0.0, 0.0, 1.0]] * 2 and res["closest"][0, 2:, 3].tolist() == [2.0, 2.0]
    assert KM.brute_force(pts, slots, shade, 1)["ties"].tolist() == [True, True]


def test_entry_points_refuse_bad_arguments_before_any_device_work():
    from pbrlab_amd import _lib
    L = _lib.lib()
    fake = C.c_void_p(16)  # never dereferenced: the checks below come before the scene is touched
    a, b, c, d = 4096, 8192, 12288, 16384
    big = C.c_size_t(1 << 31)

    def refused(rc, word):
        assert rc == EINVAL and word in L.pbrhip_last_error(), (rc, L.pbrhip_last_error())

    host, dev = L.pbrhip_k_nearest, (lambda s, p, n, k, cnt, idt, cl: L.pbrhip_k_nearest_device(s, p, n, k, None, cnt, idt, cl))
    for f in (host, dev):
        refused(f(None, a, 4, 4, b, c, d), b"NULL")
        refused(f(fake, None, 4, 4, b, c, d), b"NULL")
        refused(f(fake, a, 4, 4, None, None, None), b"NULL")   # no output
        refused(f(fake, a, 4, 4, None, None, d), b"NULL")      # closest alone is no usable output
        refused(f(fake, a, 4, 4, b, None, d), b"NULL")         # closest requires ident
        refused(f(fake, a, 4, 0, None, c, None), b"NULL")      # max_k == 0 requires count
        refused(f(fake, a, 4, 33, b, c, d), b"max_k")
        refused(f(fake, a, 4, 0xFFFFFFFF, b, c, None), b"max_k")
        refused(f(fake, a, big, 4, b, c, d), b"too many")
        refused(f(fake, a, 1 << 26, 32, b, c, d), b"too many")  # n * max_k == 2^31
        refused(f(fake, a, (1 << 31) - 1, 2, b, None, None), b"too many")
    for off in (4, 8, 12):
        refused(dev(fake, a + off, 4, 4, b, c, d), b"aligned")
        refused(dev(fake, a, 4, 4, b, c + off, d), b"aligned")
        refused(dev(fake, a, 4, 4, b, c, d + off), b"aligned")
    refused(dev(fake, a, 4, 4, b + 2, c, d), b"aligned")


def test_python_refuses_bad_arguments_before_any_c_call():
    from pbrlab_amd import api
    from test_query_cpu import FakeTensor

    class Stub:  # the checks never reach the library: no scene is needed
        device = 0
        h = None
    s = Stub()
    f = api.Scene.KNearestDevice
    with pytest.raises(TypeError):
        f(s, np.zeros((4, 4), F), 4)                          # host memory is not a device array
    for bad in (FakeTensor((4, 4), device=("cpu", None)), FakeTensor((4, 4), device=("cuda", 1)), FakeTensor((4, 5)), FakeTensor((16,)), FakeTensor((4, 4), contiguous=False)):
        with pytest.raises(ValueError):
            f(s, bad, 4)
    with pytest.raises(TypeError):
        f(s, FakeTensor((4, 4), dtype="torch.float64"), 4)
    with pytest.raises(TypeError):
        f(s, (1, 2, 3), 4)
    for k in (-1, 33, 2.5, True):
        with pytest.raises(ValueError):
            f(s, FakeTensor((4, 4)), k)
        with pytest.raises(ValueError):
            api.Scene.KNearest(s, np.zeros((4, 4), F), k)
    with pytest.raises(ValueError):
        f(s, (4096, 4), 4, count=False, ident=False)
    with pytest.raises(ValueError):
        f(s, (4096, 4), 0, count=None)                         # max_k == 0 leaves the count alone
    with pytest.raises(ValueError):
        f(s, (4096, 4), 4, count=8192, ident=False, closest=12288)  # closest needs ident
    with pytest.raises(TypeError):
        f(s, (4096, 4), 4)                                     # outputs are allocated only beside tensor points
    with pytest.raises(TypeError):
        f(s, (4096, 4), 4, count=8192, ident=12288, closest=True)
    for bad in (np.zeros((4, 3), F), np.zeros(8, F), np.zeros((2, 2, 4), F), np.zeros((3, 5), F)):
        with pytest.raises(ValueError):
            api.Scene.KNearest(s, bad, 4)


def test_model_walk_of_the_comb_with_k_32_needs_more_stack_than_lds_holds():
    """What tests/test_knearest_gpu.py::test_comb_reaches_the_spill_part_of_the_stack relies on, without a GPU: over the Morton tree of the
    depth-64 comb (tests/_lbvh_model.py) a query near the origin end without a bound and with K = 32 holds more than the 40 live stack
    entries of kSimpleLdsStack, one with a tight bound none; and the walk's list is the brute force's."""
    import _lbvh_model as M
    tri, lo, hi = M.comb_triangles(1)
    nodes, order, depth, _ = M.build(lo, hi, np.zeros(len(lo), np.uint8))
    assert depth == M.STACK_DEPTH == 64
    slots, shade = np.zeros((len(tri), 4, 4), F), np.zeros((len(tri), 32), np.uint32)
    slots[:, :3, :3], shade[:, 24] = tri[order], order
    near = comb_queries()
    d2 = QM.candidates(near, slots, shade)[0]
    res = KM.brute_force(near, slots, shade, 32)
    walks = [KM.binary_walk_k(nodes, near[i], d2[i], shade[:, 24], 32) for i in range(len(near))]
    peaks = sorted(set(w[0] for w in walks))
    print("live stack entries of the model's walk with K = 32:", peaks)
    assert max(peaks) > 40 and min(peaks) == 0
    for i, (peak, best) in enumerate(walks):
        k = min(int(res["count"][i]), 32)
        assert len(best) == k and [b[0] for b in best] == res["closest"][i, :k, 3].tolist(), i
        assert [b[1] for b in best] == shade[res["ident"][i, :k, 0], 24].tolist(), i
    assert (res["count"][0::4] == 65).all() and (res["count"][1::4] < 32).all()


def comb_queries():
    """64 queries near the origin end of the comb, unbounded; every fourth (1, 5, ...) with a bound that prunes the chain at once"""
    rng = np.random.RandomState(3)
    near = np.concatenate([rng.rand(64, 3) * 0.6 - 0.3, np.full((64, 1), np.inf)], axis=1).astype(F)
    near[1::4, 3] = 0.4
    return near
