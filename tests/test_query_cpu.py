"""Ray and nearest-point queries from device memory without a GPU: the symbols and names exist and the ABI version stands,
the entry points refuse bad arguments before any device work, the Python wrappers refuse bad arrays before any C call, and the float32
model of the nearest-point contract (tests/_query_model.py) is held to a float64 evaluation on the adversarial soups of tests/_soups.py.

The model's error, measured on seeds 0-3 with 30 extra slivers and 3000 points each (1.29 M candidates per seed): the largest
|sqrt(D2) - d64| is 4.54 units of 2^-24 (largest |coordinate| of the point and the triangle + d64) -- 4.16, 4.54, 4.06, 4.05 per seed --
with no NaN; the validation bound changed 9 candidates, all on seed 3.  (tests/test_placements_cpu.py holds the same bar away from the
unit box.)  The bound asserted below is twice the measured figure: it is a
property of the definition, checked against float64, not of the code under test."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import _query_model as QM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("pbrhip_trace_closest_device", "pbrhip_trace_any_device", "pbrhip_nearest_point", "pbrhip_nearest_point_device")
NAMES = ("TraceClosestDevice", "TraceAnyDevice", "NearestPoint", "NearestPointDevice")
EINVAL = -1
F = np.float32
MODEL_ERR_UNITS = 2 * 4.54  # twice the measured worst case (module docstring)


def test_symbols_and_names_exist():
    import pbrlab_amd as pa
    from pbrlab_amd import _lib, api
    L = _lib.lib()
    hdr = open(os.path.join(ROOT, "include", "pbrhip.h")).read()
    for name in SYMBOLS:
        assert name in _lib.EXPORTS and hasattr(L, name) and re.search(r"\b" + name + r"\s*\(", hdr), name
    for name in NAMES:
        assert hasattr(api.Scene, name), name
    assert hasattr(api, "POINT_DT") and pa.POINT_DT is api.POINT_DT and api.POINT_DT.itemsize == 16
    assert re.search(r"\}\s*pbrhip_point;", hdr)
    assert L.pbrhip_abi_version() == 6 and re.search(r"#define PBRHIP_ABI_VERSION 6u\b", hdr)  # functions only: the layouts stand
    shim = open(os.path.join(ROOT, "include", "pbrlab_hip.hpp")).read()
    for name in NAMES:
        assert re.search(r"\b" + name + r"\b", shim), name


def test_entry_points_refuse_bad_arguments_before_any_device_work():
    from pbrlab_amd import _lib
    L = _lib.lib()
    fake = C.c_void_p(16)  # never dereferenced: the checks below come before the scene is touched
    buf = np.zeros((4, 9), np.float32)
    a, b, c = buf.ctypes.data, buf.ctypes.data + 64, buf.ctypes.data + 96
    big = C.c_size_t(1 << 31)

    def refused(rc, word):
        assert rc == EINVAL and word in L.pbrhip_last_error(), (rc, L.pbrhip_last_error())

    for f in (L.pbrhip_trace_closest_device, L.pbrhip_nearest_point_device):
        refused(f(None, a, 4, None, b, c), b"NULL")
        refused(f(fake, None, 4, None, b, c), b"NULL")
        refused(f(fake, a, 4, None, None, None), b"NULL")  # both outputs
        refused(f(fake, a, big, None, b, c), b"too many")
        refused(f(fake, a, big, None, None, c), b"too many")
    refused(L.pbrhip_trace_any_device(None, a, 4, None, b), b"NULL")
    refused(L.pbrhip_trace_any_device(fake, None, 4, None, b), b"NULL")
    refused(L.pbrhip_trace_any_device(fake, a, 4, None, None), b"NULL")
    refused(L.pbrhip_trace_any_device(fake, a, big, None, b), b"too many")
    refused(L.pbrhip_nearest_point(None, a, 4, b, c), b"NULL")
    refused(L.pbrhip_nearest_point(fake, None, 4, b, c), b"NULL")
    refused(L.pbrhip_nearest_point(fake, a, 4, None, None), b"NULL")
    refused(L.pbrhip_nearest_point(fake, a, big, b, c), b"too many")


class FakeTensor:
    """what the binding looks at of a tensor, and nothing else: no torch is needed to be refused"""

    class Dev:
        def __init__(self, type_, index):
            self.type, self.index = type_, index

    def __init__(self, shape, dtype="torch.float32", device=("cuda", 0), contiguous=True):
        self.shape, self.dtype, self.device, self._c = shape, dtype, FakeTensor.Dev(*device), contiguous

    def data_ptr(self):
        raise AssertionError("a refused array is never dereferenced")

    def is_contiguous(self):
        return self._c


def test_python_refuses_bad_arrays_before_any_c_call():
    from pbrlab_amd import api

    class Stub:  # the checks never reach the library: no scene is needed
        device = 0
        h = None
    s = Stub()
    for f, words in ((api.Scene.TraceClosestDevice, 8), (api.Scene.TraceAnyDevice, 8), (api.Scene.NearestPointDevice, 4)):
        with pytest.raises(TypeError):
            f(s, np.zeros((4, words), np.float32))                    # host memory is not a device array
        with pytest.raises(ValueError):
            f(s, FakeTensor((4, words), device=("cpu", None)))        # ... nor is a CPU tensor
        with pytest.raises(ValueError):
            f(s, FakeTensor((4, words), device=("cuda", 1)))          # another GPU than the scene's
        with pytest.raises(TypeError):
            f(s, FakeTensor((4, words), dtype="torch.float64"))
        with pytest.raises(ValueError):
            f(s, FakeTensor((4, words + 1)))
        with pytest.raises(ValueError):
            f(s, FakeTensor((4 * words,)))
        with pytest.raises(ValueError):
            f(s, FakeTensor((4, words), contiguous=False))
        with pytest.raises(TypeError):
            f(s, (1, 2, 3))


@functools.lru_cache(maxsize=None)
def soup_case(seed):
    """-> (tris, slots, shade, points, candidates, brute force) of the soup with 30 extra slivers; slot = gid = the triangle's index"""
    import _soups
    desc = _soups.triangle_soup(seed, 30)[0]
    tris = np.ascontiguousarray(desc.vertices[:, :3].reshape(-1, 3, 3), F)
    n = len(tris)
    slots, shade = np.zeros((n, 4, 4), F), np.zeros((n, 32), np.uint32)
    slots[:, :3, :3], shade[:, 24] = tris, np.arange(n)
    pts = QM.soup_points(tris, seed)
    return tris, slots, shade, pts, QM.candidates(pts, slots, shade), QM.brute_force(pts, slots, shade)


@pytest.mark.parametrize("seed", range(4))
def test_model_is_finite_and_close_to_float64(seed):
    tris, slots, shade, pts, (D2, U, V, Q, clamped), res = soup_case(seed)
    assert len(pts) == 3000 and D2.shape == (3000, len(tris))
    for a in (D2, U, V, Q):
        assert not np.isnan(a).any()
    p = pts[:, None, :3]
    d64 = QM.tri_dist64(p, tris[None, :, 0], tris[None, :, 1], tris[None, :, 2])
    big = np.maximum(np.abs(p).max(axis=-1), np.abs(tris).reshape(len(tris), 9).max(axis=1)[None, :])
    err = np.abs(np.sqrt(D2.astype(np.float64)) - d64) / (2.0 ** -24 * (big + d64))
    print(f"seed {seed}: largest |sqrt(D2) - d64| = {err.max():.3f} units, {int(clamped.sum())} clamped candidates")
    assert err.max() <= MODEL_ERR_UNITS
    # the closest point is where the distance says: |p - q| of the winners against sqrt(D2), in the same units (coordinates below 4).
    # (Barycentrics are exact only on well-shaped triangles: test_model_tie_rule_and_inactive_queries checks them there.)
    f = res["found"]
    d = (pts[f, :3] - res["q"][f]).astype(np.float64)
    assert np.abs(np.sqrt((d * d).sum(axis=1)) - np.sqrt(res["d2"][f].astype(np.float64))).max() <= MODEL_ERR_UNITS * 2.0 ** -24 * 4.0


def test_model_meets_the_cases_the_gpu_comparison_needs():
    clamped = ties = 0
    for seed in range(4):
        res = soup_case(seed)[5]
        clamped += res["clamped"]
        ties += int((res["ties"] >= 2).sum())
        third = np.arange(3000) % 3 == 0
        assert res["found"][~third].all()                            # no bound: every query finds something
        assert res["found"][third].sum() >= 200 and (~res["found"][third]).sum() >= 200, seed
    print(f"{clamped} clamped candidates, {ties} queries whose minimum two gids share")
    assert clamped >= 1 and ties >= 100


def test_model_tie_rule_and_inactive_queries():
    tri = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], F)
    slots, shade = np.zeros((3, 4, 4), F), np.zeros((3, 32), np.uint32)
    slots[:, :3, :3] = tri
    slots[2, :3, 2] = 5.0
    shade[:, 24] = (7, 3, 1)  # two copies: gid 3 wins over 7; the far one has the smallest gid and loses
    pts = np.array([[0.25, 0.25, 1.0, np.inf], [0.25, 0.25, 1.0, 0.5], [0.25, 0.25, 1.0, 1.0], [np.nan, 0, 0, 1], [0, np.inf, 0, 1],
                    [0, 0, 0, -1.0], [0, 0, 0, np.nan], [2.0, 0.0, 0.0, np.inf]], F)
    res = QM.brute_force(pts, slots, shade)
    assert res["found"].tolist() == [True, False, True, False, False, False, False, True]
    assert res["slot"][[0, 2, 7]].tolist() == [1, 1, 1] and res["ties"][[0, 2]].tolist() == [2, 2]
    assert res["d2"][0] == 1.0 and res["u"][0] == 0.25 and res["v"][0] == 0.25 and res["q"][0].tolist() == [0.25, 0.25, 0.0]
    assert res["d2"][7] == 1.0 and res["u"][7] == 1.0 and res["v"][7] == 0.0 and res["q"][7].tolist() == [1.0, 0.0, 0.0]
    ident, closest = QM.expected_buffers(res)
    assert ident[1].tolist() == [QM.NONE, 0, 0, 0] and closest[1].tolist() == [0, 0, 0, 0]
    assert ident[0].tolist() == [1] + np.array([0.25, 0.25, 1.0], F).view(np.uint32).tolist()
    # a curve piece: the distance to its axis, u = (sub + t) / 4
    cs, ch = np.zeros((1, 4, 4), F), np.zeros((1, 32), np.uint32)
    cs[0, 0], cs[0, 1] = (0, 0, 0, 0.1), (2, 0, 0, 0.1)
    cs[0, 2, 0] = np.array([2], np.uint32).view(F)[0]
    ch[0, 3] = QM.SLOT_IS_CURVE << 24
    r = QM.brute_force(np.array([[0.5, 1.0, 0.0, np.inf]], F), cs, ch)
    assert r["d2"][0] == 1.0 and r["u"][0] == F(2.25) * F(0.25) and r["v"][0] == 0 and r["q"][0].tolist() == [0.5, 0.0, 0.0]


def test_misaligned_device_pointers_are_refused_before_the_scene_is_touched():
    """the kernels move 16 bytes at a time (include/pbrhip.h): rays, points, ident and closest that are not 16-byte aligned are
    PBRHIP_EINVAL, d_hits needs 4 bytes, the occlusion bytes nothing"""
    from pbrlab_amd import _lib
    L = _lib.lib()
    fake = C.c_void_p(16)
    a, b, c = 4096, 8192, 12288  # (never dereferenced)

    def refused(rc):
        assert rc == EINVAL and b"aligned" in L.pbrhip_last_error(), (rc, L.pbrhip_last_error())
    for off in (4, 8, 12):
        refused(L.pbrhip_trace_closest_device(fake, a + off, 4, None, b, c))
        refused(L.pbrhip_trace_closest_device(fake, a, 4, None, b + off, c))
        refused(L.pbrhip_trace_any_device(fake, a + off, 4, None, b))
        refused(L.pbrhip_nearest_point_device(fake, a + off, 4, None, b, c))
        refused(L.pbrhip_nearest_point_device(fake, a, 4, None, b + off, c))
        refused(L.pbrhip_nearest_point_device(fake, a, 4, None, b, c + off))
    refused(L.pbrhip_trace_closest_device(fake, a, 4, None, b, c + 2))


def test_nearest_point_refuses_wrong_shapes_before_any_c_call():
    from pbrlab_amd import api

    class Stub:
        h = None
    for bad in (np.zeros((4, 3), np.float32), np.zeros(8, np.float32), np.zeros((2, 2, 4), np.float32), np.zeros((3, 5), np.float32)):
        with pytest.raises(ValueError):
            api.Scene.NearestPoint(Stub(), bad)


def test_model_walk_of_the_comb_needs_more_stack_than_lds_holds():
    """What tests/test_query_gpu.py::test_comb_reaches_the_spill_part_of_the_stack relies on, without a GPU: over the Morton tree of the
    depth-64 comb (tests/_lbvh_model.py) a query near the origin end without a bound holds 62 live stack entries -- more than the 40 of
    kSimpleLdsStack --, one with a tight bound none; and the walk's answer is the brute force's."""
    import _lbvh_model as M
    tri, lo, hi = M.comb_triangles(1)
    nodes, order, depth, _ = M.build(lo, hi, np.zeros(len(lo), np.uint8))
    assert depth == M.STACK_DEPTH == 64
    slots, shade = np.zeros((len(tri), 4, 4), F), np.zeros((len(tri), 32), np.uint32)
    slots[:, :3, :3], shade[:, 24] = tri[order], order
    rng = np.random.RandomState(3)
    near = np.concatenate([rng.rand(64, 3) * 0.6 - 0.3, np.full((64, 1), np.inf)], axis=1).astype(F)
    near[1::4, 3] = 0.4
    res, d2 = QM.brute_force(near, slots, shade), QM.candidates(near, slots, shade)[0]
    walks = [QM.binary_walk(nodes, near[i], d2[i]) for i in range(len(near))]
    assert sorted(set(w[0] for w in walks)) == [0, 62]
    assert all(w[1] == res["d2"][i] for i, w in enumerate(walks) if res["found"][i]) and res["found"][0::4].all()
