"""All-hits ray queries without a GPU: the symbols and names exist and the ABI version stands; the numpy model of the
contract (tests/_allhits_model.py) is pinned to the oracle on the adversarial soup of tests/_soups.py -- its first hit is the oracle's
brute-force closest hit bit for bit, and peeling the oracle visits exactly the model's distinct distances --; the soup meets the cases the
GPU comparison (tests/test_allhits_gpu.py) needs, so that it cannot pass vacuously; and the entry points refuse bad arguments before any
device work."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import _allhits_model as AM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("pbrhip_trace_all", "pbrhip_trace_all_device")
NAMES = ("TraceAll", "TraceAllDevice")
EINVAL = -1
F = np.float32
NONE = 0xFFFFFFFF


def test_symbols_and_names_exist():
    from pbrlab_amd import _lib, api
    L = _lib.lib()
    hdr = open(os.path.join(ROOT, "include", "pbrhip.h")).read()
    shim = open(os.path.join(ROOT, "include", "pbrlab_hip.hpp")).read()
    for name in SYMBOLS:
        assert name in _lib.EXPORTS and hasattr(L, name) and re.search(r"\b" + name + r"\s*\(", hdr), name
    for name in NAMES:
        assert hasattr(api.Scene, name) and re.search(r"\b" + name + r"\b", shim), name
    assert re.search(r"#define PBRHIP_ALL_HITS_MAX 32u\b", hdr) and api.ALL_HITS_MAX == 32
    assert L.pbrhip_abi_version() == 6 and re.search(r"#define PBRHIP_ABI_VERSION 6u\b", hdr)  # functions only: the layouts stand
    # all-hits left the "Not provided" lists
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "all-hits queries" not in hdr and "all-hits queries" not in design and "## 21." in design


@functools.lru_cache(maxsize=None)
def soup_case(seed):
    """-> (oracle scene, rays, slots, shade, brute force with every hit listed) of the soup with 30 extra slivers; slot = gid = the
    triangle's index in the description"""
    import _soups
    desc, so, rays = _soups.triangle_soup(seed, 30)
    tris = np.ascontiguousarray(desc.vertices[:, :3].reshape(-1, 3, 3), F)
    n = len(tris)
    slots, shade = np.zeros((n, 4, 4), F), np.zeros((n, 32), np.uint32)
    slots[:, :3, :3], shade[:, 24] = tris, np.arange(n)
    k = int(AM.brute_force(rays, slots, shade, 0)["count"].max())
    return so, rays, slots, shade, AM.brute_force(rays, slots, shade, k)


@pytest.mark.parametrize("seed", range(2))
def test_model_first_hit_is_the_oracles_brute_force_closest_hit(seed):
    so, rays, slots, shade, res = soup_case(seed)
    want = so.trace_closest(rays, brute_force=True)
    first = res["ident"][:, 0]
    hit = want["instance_id"] != NONE
    assert np.array_equal(hit, first[:, 0] != NONE) and np.array_equal(hit, res["count"] > 0) and hit.sum() > 5000
    for word, f in ((1, "u"), (2, "v"), (3, "t")):
        assert np.array_equal(first[hit, word], want[f][hit].view(np.uint32)), f
    assert (first[~hit] == (NONE, 0, 0, 0)).all()
    # the soup's two meshes hold triangles 0 .. 249 and 250 ..: one instance each
    assert np.array_equal(first[hit, 0], want["instance_id"][hit] * 250 + want["prim_id"][hit])
    # K = 1 and a truncated list are prefixes of the full one, and count does not depend on K
    for k in (1, 4):
        part = AM.brute_force(rays[:2000], slots, shade, k)
        assert np.array_equal(part["ident"], res["ident"][:2000, :k]) and np.array_equal(part["count"], res["count"][:2000])


@pytest.mark.parametrize("seed", range(2))
def test_peeling_the_oracle_visits_the_models_distinct_distances(seed):
    """tmin advanced to the last t: the oracle's next closest hit is the model's next distinct t, until the oracle misses exactly where
    the model's list ends.  (What peeling loses -- every hit but one of a tie -- is the difference between count and the steps.)"""
    so, rays, slots, shade, res = soup_case(seed)
    ident, count = res["ident"], res["count"]
    n, k = ident.shape[:2]
    t = ident[:, :, 3].view(F)
    listed = np.arange(k)[None, :] < count[:, None]
    new = listed & np.concatenate([np.ones((n, 1), bool), t[:, 1:] != t[:, :-1]], axis=1)  # the first entry of every distinct t
    steps = new.sum(axis=1)
    padded = np.where(listed, t, np.inf)
    assert (steps < count).any() and (padded[:, 1:] >= padded[:, :-1]).all()
    peel = rays.copy()
    alive = np.ones(n, bool)
    for j in range(int(steps.max()) + 1):
        got = so.trace_closest(peel, brute_force=True)
        hit = (got["instance_id"] != NONE) & alive
        assert np.array_equal(hit, steps > j), j
        rows = np.nonzero(hit)[0]
        col = np.argmax(np.cumsum(new[rows], axis=1) == j + 1, axis=1)  # the j-th distinct t of each of these rays
        assert np.array_equal(got["t"][rows].view(np.uint32), ident[rows, col, 3]), j
        assert np.array_equal(got["u"][rows].view(np.uint32), ident[rows, col, 1]) and np.array_equal(got["instance_id"][rows] * 250 + got["prim_id"][rows], ident[rows, col, 0])
        alive = hit
        peel["tmin"][rows] = got["t"][rows]  # (a ray that has missed keeps its interval and misses again)
    assert not alive.any()


@pytest.mark.parametrize("seed", (0, 1, 3))
def test_soup_meets_the_cases_the_gpu_comparison_needs(seed):
    """seed 3 is the soup tests/test_allhits_gpu.py runs"""
    so, rays, slots, shade, res = soup_case(seed)
    count, ident = res["count"], res["ident"]
    print(f"seed {seed}: {len(rays)} rays, |H| up to {count.max()}, {int((count > 4).sum())} rays with |H| > 4, {int((res['ties'] > 0).sum())} with a tie, {int((count == 0).sum())} without a hit")
    assert (count > 4).sum() >= 100, "truncation at K = 4 must happen"
    assert (count == 0).sum() >= 100 and count.max() <= 32
    assert (res["ties"] > 0).sum() >= 100
    # triangles 100 .. 119 are exact duplicates of 60 .. 79: a ray that hits one has both, at equal t, the smaller id first
    rows, cols = np.nonzero((ident[:, :, 0] >= 100) & (ident[:, :, 0] < 120))
    assert len(rows) >= 50
    twin = (ident[rows, :, 0] == (ident[rows, cols, 0] - 40)[:, None]) & (ident[rows, :, 1:] == ident[rows, cols, None, 1:]).all(axis=-1)
    assert (twin & (np.arange(ident.shape[1])[None, :] < cols[:, None])).any(axis=1).all()


def test_model_orders_ties_by_gid_and_drops_inactive_rays():
    tri = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], F)
    slots, shade = np.zeros((4, 4, 4), F), np.zeros((4, 32), np.uint32)
    slots[:, :3, :3] = tri
    slots[2, :3, 2], slots[3, :3, 2] = -1.0, 0.5
    shade[:, 24] = (7, 3, 1, 9)  # slots 0 and 1 coincide: gid 3 before gid 7; slot 3 is nearer, slot 2 farther
    rays = np.zeros(4, AM.RAY_DT)
    rays["org"], rays["dir"], rays["tmax"] = (0.25, 0.25, 2.0), (0, 0, -1), np.inf
    rays["tmax"][1] = 2.0   # ends ON the coinciding pair: t <= tmax is accepted
    rays["tmin"][2] = 1.5   # starts ON the nearest: tmin < t is not
    rays["dir"][3] = 0      # inactive
    res = AM.brute_force(rays, slots, shade, 3)
    assert res["count"].tolist() == [4, 3, 3, 0] and res["ties"].tolist() == [1, 1, 1, 0]
    assert res["ident"][0, :, 0].tolist() == [3, 1, 0] and res["ident"][0, :, 3].view(F).tolist() == [1.5, 2.0, 2.0]
    assert res["ident"][1, :, 0].tolist() == [3, 1, 0] and res["ident"][2, :, 0].tolist() == [1, 0, 2]
    assert (res["ident"][3] == (NONE, 0, 0, 0)).all()
    assert res["ident"][0, 0].tolist() == [3] + np.array([0.25, 0.25, 1.5], F).view(np.uint32).tolist()


def test_entry_points_refuse_bad_arguments_before_any_device_work():
    from pbrlab_amd import _lib
    L = _lib.lib()
    fake = C.c_void_p(16)  # never dereferenced: the checks below come before the scene is touched
    a, b, c = 4096, 8192, 12288
    big = C.c_size_t(1 << 31)

    def refused(rc, word):
        assert rc == EINVAL and word in L.pbrhip_last_error(), (rc, L.pbrhip_last_error())

    host, dev = L.pbrhip_trace_all, (lambda s, r, n, k, cnt, idt: L.pbrhip_trace_all_device(s, r, n, k, None, cnt, idt))
    for f in (host, dev):
        refused(f(None, a, 4, 4, b, c), b"NULL")
        refused(f(fake, None, 4, 4, b, c), b"NULL")
        refused(f(fake, a, 4, 4, None, None), b"NULL")     # both outputs
        refused(f(fake, a, 4, 0, None, c), b"NULL")        # max_hits == 0 requires count
        refused(f(fake, a, 4, 33, b, c), b"max_hits")
        refused(f(fake, a, 4, 0xFFFFFFFF, b, c), b"max_hits")
        refused(f(fake, a, big, 4, b, c), b"too many")
        refused(f(fake, a, 1 << 26, 32, b, c), b"too many")  # n * max_hits == 2^31
        refused(f(fake, a, (1 << 31) - 1, 2, b, None), b"too many")
    for off in (4, 8, 12):
        refused(dev(fake, a + off, 4, 4, b, c), b"aligned")
        refused(dev(fake, a, 4, 4, b, c + off), b"aligned")
    refused(dev(fake, a, 4, 4, b + 2, c), b"aligned")


def test_python_refuses_bad_arguments_before_any_c_call():
    from pbrlab_amd import api
    from test_query_cpu import FakeTensor

    class Stub:  # the checks never reach the library: no scene is needed
        device = 0
        h = None
    s = Stub()
    f = api.Scene.TraceAllDevice
    with pytest.raises(TypeError):
        f(s, np.zeros((4, 8), F), 4)                          # host memory is not a device array
    for bad in (FakeTensor((4, 8), device=("cpu", None)), FakeTensor((4, 8), device=("cuda", 1)), FakeTensor((4, 9)), FakeTensor((32,)), FakeTensor((4, 8), contiguous=False)):
        with pytest.raises(ValueError):
            f(s, bad, 4)
    with pytest.raises(TypeError):
        f(s, FakeTensor((4, 8), dtype="torch.float64"), 4)
    with pytest.raises(TypeError):
        f(s, (1, 2, 3), 4)
    for k in (-1, 33, 2.5, True):
        with pytest.raises(ValueError):
            f(s, FakeTensor((4, 8)), k)
        with pytest.raises(ValueError):
            api.Scene.TraceAll(s, np.zeros((4, 8), F), k)
    with pytest.raises(ValueError):
        f(s, (4096, 4), 4, count=False, ident=False)
    with pytest.raises(ValueError):
        f(s, (4096, 4), 0, count=None)                         # max_hits == 0 leaves the count alone
    with pytest.raises(TypeError):
        f(s, (4096, 4), 4)                                     # outputs are allocated only beside tensor rays
    for bad in (np.zeros((4, 7), F), np.zeros(8, F), np.zeros((2, 2, 8), F)):
        with pytest.raises(ValueError):
            api.Scene.TraceAll(s, bad, 4)


def test_model_walk_of_the_fat_comb_needs_more_stack_than_lds_holds():
    """What tests/test_allhits_gpu.py::test_combs_reach_the_spill_part_of_the_stack relies on, without a GPU.  Over the Morton tree of
    the depth-64 comb a ray up the z axis crosses the boxes of the 22 leaves on that axis and holds 20 live stack entries: the teeth on
    the other two axes are thin and lie off the ray, and no straight line meets more, so a ray cannot fill the kSimpleLdsStack = 40
    entries that live in LDS there.  On the fat comb -- the same box centres, hence the same chain -- the same ray crosses 63 leaf boxes
    on its way down the chain and holds 62.  The walk's hit count is the brute force's on both."""
    import _lbvh_model as M
    ray = np.array([[0, 0, -10, 0, 0, 0, 1, np.inf]], F)
    for (tri, lo, hi), want_peak, want_hits in ((M.comb_triangles(1), 20, 22), (AM.fat_comb_triangles(), 62, 64)):
        nodes, order, depth, _ = M.build(lo, hi, np.zeros(len(lo), np.uint8))
        assert depth == M.STACK_DEPTH == 64
        slots, shade = np.zeros((len(tri), 4, 4), F), np.zeros((len(tri), 32), np.uint32)
        slots[:, :3, :3], shade[:, 24] = tri[order], order
        peak, hits = AM.binary_walk_all(nodes, ray, slots, shade)
        res = AM.brute_force(ray, slots, shade, 32)
        assert (peak, hits) == (want_peak, want_hits) and res["count"][0] == hits
    assert want_peak > 40 and res["ties"][0] >= 40  # the fat teeth share the plane z = 0: one t, ordered by gid
    assert (np.diff(shade[res["ident"][0, :, 0], 24].astype(np.int64)) > 0).all()
