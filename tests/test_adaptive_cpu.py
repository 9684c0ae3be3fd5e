"""Adaptive sampling without a GPU: the symbols and Python names exist and fail loudly, the decision kernels keep their
budgets and stay out of the render kernels' code object, and the numpy model of tests/_adaptive_model.py agrees with hand-made cases."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import _adaptive_model as AM
import _codeobj as CO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "shim_adaptive")
SYMBOLS = ("pbrhip_render_adaptive", "pbrhip_render_adaptive_device", "pbrhip_adaptive_step")
EINVAL, ENODEVICE = -1, -3
AS_KERNELS = ("k_as_error", "k_as_scan", "k_as_scatter")


def test_symbols_and_names_exist():
    import pbrlab_amd as pa
    from pbrlab_amd import _lib, api
    L = _lib.lib()
    hdr = open(os.path.join(ROOT, "include", "pbrhip.h")).read()
    for name in SYMBOLS:
        assert name in _lib.EXPORTS and hasattr(L, name) and re.search(r"\b" + name + r"\s*\(", hdr), name
    assert L.pbrhip_abi_version() == 6
    assert hasattr(pa, "RenderAdaptive") and hasattr(api, "RenderAdaptive") and hasattr(api, "adaptive_step")
    # the header's defaults are the binding's
    assert int(re.search(r"#define PBRHIP_ADAPTIVE_FIRST_LEVEL (\d+)u", hdr).group(1)) == api.ADAPTIVE_FIRST_LEVEL
    assert float(re.search(r"#define PBRHIP_ADAPTIVE_THRESHOLD ([0-9.eE+-]+)f", hdr).group(1)) == api.ADAPTIVE_THRESHOLD


def test_null_scene_is_refused():
    from pbrlab_amd import _lib, api
    L = _lib.lib()
    desc = api._desc(8, 8, 4)
    rgba, count = np.zeros((8, 8, 4), np.float32), np.zeros((8, 8), np.uint32)
    for fn in (L.pbrhip_render_adaptive, L.pbrhip_render_adaptive_device):
        rc = fn(None, C.byref(desc), 0.1, 0, None, rgba.ctypes.data, count.ctypes.data, None, None, None, None)
        assert rc == EINVAL and b"NULL" in L.pbrhip_last_error()
    with pytest.raises(api.PbrHipError) as e:
        api.RenderAdaptive(None, 8, 8, 4)
    assert e.value.code == EINVAL and "NULL" in str(e.value)


def test_adaptive_step_fails_loudly_without_device():
    import pbrlab_amd as pa
    from pbrlab_amd import api
    if pa.device_count() > 0:
        pytest.skip("a GPU is present")
    z = np.zeros((8, 8, 4), np.float32)
    with pytest.raises(pa.PbrHipError) as e:
        api.adaptive_step(z, z, 2, 4, 0.1, [0])
    assert e.value.code == ENODEVICE
    # the argument checks come first
    for bad in (dict(tiles_in=[1]), dict(tiles_in=[0, 0]), dict(threshold=-1.0), dict(threshold=float("nan")), dict(n_now=2)):
        kw = dict(n_prev=2, n_now=4, threshold=0.1, tiles_in=[0])
        kw.update(bad)
        with pytest.raises(pa.PbrHipError) as e:
            api.adaptive_step(z, z, **kw)
        assert e.value.code == EINVAL, bad


def test_decision_kernels_stay_within_their_budgets():
    if not CO.available():
        pytest.skip("libpbrhip.so or the LLVM tools are missing")
    import _codeobj_tus as T
    table = T.kernel_table()
    assert sorted(k for k in table if "k_as_" in k) == sorted(AS_KERNELS)
    for name in AS_KERNELS:
        got = table[name]
        assert got["private_segment_fixed_size"] == 0, (name, got)
        assert not any(p in name for p in ("k_rf_", "k_qc_", "k_dg_", "k_features", "k_denoise"))
    err = table["k_as_error"]
    assert CO.waves_per_simd(err["vgpr_count"]) >= 8 and err["group_segment_fixed_size"] == 0, err  # no LDS: the butterfly is cross-lane
    assert table["k_as_scatter"]["group_segment_fixed_size"] == 0
    assert table["k_as_scan"]["group_segment_fixed_size"] == 2 * 16 * 4  # the one hand-over: two words per wave of the block
    # the render kernels' translation unit is still the library's first code object, without any of these
    first = CO.kernel_table()
    assert not any("k_as_" in k for k in first) and all(k in table for k in first)
    assert any(k.startswith("k_trace") for k in first) and "k_accumulate" in first


# ---------------------------------------------------------------------------------------------------- the model
def _layers(h, w, seed, n_prev=4, n_now=8):
    rng = np.random.RandomState(seed)
    A = np.zeros((h, w, 4), np.float32)
    A[..., :3] = rng.uniform(0, 3, (h, w, 3)) * n_prev
    A[..., 3] = n_prev
    I = A.copy()
    I[..., :3] += (rng.uniform(0, 3, (h, w, 3)) * (n_now - n_prev)).astype(np.float32)
    I[..., 3] = n_now
    return I, A


def test_model_equal_halves_give_zero():
    _, A = _layers(16, 24, 1)
    I = A.copy()
    I[..., :3] = A[..., :3] * np.float32(2)  # the second half's sum equals the first's, exactly
    tiles = np.arange(6, dtype=np.uint32)
    out, pix, err, snap = AM.step(I, A, 4, 8, 0.0, tiles)
    assert (err == 0).all() and len(out) == 0 and len(pix) == 0  # E == 0 <= 0: every tile stops, even at threshold 0
    assert snap.tobytes() == I.tobytes()
    # and unequal halves do not
    I[3, 5, 1] += np.float32(1)
    out, _, err, _ = AM.step(I, A, 4, 8, 0.0, tiles)
    assert list(out) == [0] and err[0, 0] > 0 and (err.reshape(-1)[1:] == 0).all()


def test_model_clipped_tile_divides_by_its_own_pixels():
    h, w = 5, 3  # one tile of 15 pixels
    I, A = _layers(h, w, 2)
    e = AM.pixel_error(I, A, 4, 8)
    E = AM.tile_error(e, 0, w, h)
    want = e.astype(np.float64).sum() / 15
    assert abs(E - want) <= 1e-15 * want and abs(E - e.astype(np.float64).sum() / 64) > 0.1 * want
    assert AM.tile_box(0, w, h) == (0, 0, 3, 5) and list(AM.tile_pixels(0, w, h)) == list(range(15))
    # a one-pixel-wide tile column: 57 = 7 x 8 + 1
    assert AM.tile_box(7, 57, 20) == (56, 0, 1, 8) and list(AM.tile_pixels(15, 57, 20)) == [8 * 57 + 56 + 57 * r for r in range(8)]
    assert AM.tile_box(23, 57, 20) == (56, 16, 1, 4)


def test_model_butterfly_order():
    """the sum is the butterfly's, not a running sum: values whose float64 sum depends on the order"""
    e = np.zeros((8, 8), np.float32)
    e[0, 0], e[0, 1], e[0, 2] = 1e30, -1e30, 1.0  # lanes 0, 1, 2: (lane 0 + lane 1) + (lane 2 + lane 3) = 0 + 1
    assert AM.tile_error(e, 0, 8, 8) == 1.0 / 64
    e[0, 1], e[0, 2] = 1.0, -1e30  # (1e30 + 1) + (-1e30 + 0) = 0 in float64, where 1e30 - 1e30 + 1 = 1
    assert AM.tile_error(e, 0, 8, 8) == 0.0


def test_model_nan_tile_stays_active_and_compaction_is_stable():
    h, w = 24, 32  # 4 x 3 tiles
    I, A = _layers(h, w, 3)
    I[9, 17, 0] = np.nan  # tile 1 * 4 + 2 = 6
    I[:8, 8:16] = A[:8, 8:16]
    I[:8, 8:16, :3] *= np.float32(2)  # tile 1 converged exactly
    order = np.array([11, 6, 1, 0, 9, 4], np.uint32)
    huge = 1e30
    out, pix, err, snap = AM.step(I, A, 4, 8, huge, order)
    assert list(out) == [6]  # every finite tile stops at a huge threshold, the NaN tile does not
    assert err.view(np.uint32)[1, 2] == 0x7FC00000 and list(pix) == list(AM.tile_pixels(6, w, h))
    e = AM.pixel_error(I, A, 4, 8)
    thr = np.float32(np.median([AM.tile_error(e, t, w, h) for t in (11, 0, 9, 4)]))
    out, pix, err, snap = AM.step(I, A, 4, 8, thr, order)
    kept = [t for t in order if t == 6 or (t != 1 and AM.tile_error(e, t, w, h) > np.float64(thr))]
    assert list(out) == kept and 2 <= len(kept) <= 4  # the order they had, not image order
    assert list(pix) == [p for t in kept for p in AM.tile_pixels(t, w, h)]
    assert err[0, 1] == 0 and err[2, 2] == 0 and err[1, 1] == 0  # tile 1: E == 0; tiles 10 and 5 were not listed
    # the snapshot follows the listed tiles only
    mask = np.zeros((h, w), bool)
    for t in order:
        x0, y0, cw, ch = AM.tile_box(t, w, h)
        mask[y0:y0 + ch, x0:x0 + cw] = True
    assert snap[mask].tobytes() == I[mask].tobytes() and snap[~mask].tobytes() == A[~mask].tobytes()


def test_model_levels():
    assert AM.levels(4, 24) == [4, 8, 16, 24]
    assert AM.levels(8, 64) == [8, 16, 32, 64]
    assert AM.levels(2, 3) == [2, 3]
    assert AM.levels(8, 8) == [8] and AM.levels(100, 7) == [7]
    assert AM.levels(3, 100) == [3, 6, 12, 24, 48, 96, 100]


def test_model_run_is_made_of_plain_frames():
    """frames whose value is n x (a per-pixel constant) never differ between halves: everything stops at the first decision; a noisy
    region keeps going to the maximum"""
    h, w = 20, 28
    rng = np.random.RandomState(7)
    base = rng.uniform(0.1, 1.0, (h, w, 3)).astype(np.float32)
    noise = {n: rng.uniform(0.0, 2.0, (8, 8, 3)).astype(np.float32) for n in (4, 8, 16, 24)}

    def frame_at(n):
        f = np.zeros((h, w, 4), np.float32)
        f[..., :3] = base * np.float32(n)
        f[8:16, 16:24, :3] = noise[n] * np.float32(n)  # tile 1 * 4 + 2: a different mean at every level
        f[..., 3] = n
        return f, np.full((h, w), n, np.uint32)

    r = AM.run(frame_at, w, h, 24, 1e-4, first_level=4)
    assert r["levels"] == [4, 8, 16, 24] and r["rounds"] == 4
    want = np.full((h, w), 8, np.uint32)
    want[8:16, 16:24] = 24
    assert np.array_equal(r["count"], want) and r["samples"] == int(want.sum())
    for n in (8, 24):
        assert r["rgba"][want == n].tobytes() == frame_at(n)[0][want == n].tobytes()
    assert r["tile_error"][1, 2] > 1e-4 and (np.delete(r["tile_error"].reshape(-1), 6) <= 1e-4).all()
    # a rank without tiles, and a maximum at the first level
    assert AM.run(frame_at, w, h, 24, 0.1, 4, tiles=[])["rounds"] == 0
    r = AM.run(frame_at, w, h, 4, 0.1, first_level=4)
    assert r["rounds"] == 1 and (r["count"] == 4).all() and not r["tile_error"].any()
    # shards: the ranks' tiles partition the image's
    parts = [AM.rank_tiles(60, 44, k, 3, 8) for k in range(3)]
    assert sorted(np.concatenate(parts)) == list(range(8 * 6)) and len(AM.rank_tiles(60, 44, 50, 64, 8)) == 0


# ---------------------------------------------------------------------------------------------------- CLI and C++ shim
def test_cli_rejects_bad_adaptive_flags():
    cli = os.path.join(ROOT, "pbrlab_amd", "pbrlab-hip-cli")
    if not os.path.exists(cli):
        pytest.skip("pbrlab-hip-cli not built")
    for args, msg in ((["--adaptive"], "missing value for --adaptive"), (["--adaptive", "-1"], "--adaptive needs a finite threshold >= 0"),
                      (["--adaptive", "nan"], "--adaptive needs a finite threshold >= 0"), (["--min-spp", "4"], "--min-spp needs --adaptive"),
                      (["--adaptive", "0.1", "--min-spp", "0"], "--min-spp needs an integer in 1.."),
                      (["--adaptive", "0.1", "--gpus", "2"], "--adaptive renders on one GPU")):
        r = subprocess.run([cli, "scene.obj"] + args, capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and msg in r.stderr, (args, r.returncode, r.stderr)


def test_adaptive_shim_caller_compiles():
    import pbrlab_amd as pa
    lib = os.path.join(ROOT, "pbrlab_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "shim_adaptive.cc"),
                           "-L" + lib, "-lpbrhip", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib", "-lpthread", "-o", EXE])
    if pa.device_count() == 0:
        r = subprocess.run([EXE], capture_output=True, text=True)
        assert r.returncode == 3, r.stderr
