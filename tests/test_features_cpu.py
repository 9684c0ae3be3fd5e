"""Feature buffers and denoiser without a GPU: the symbols and Python names exist and fail loudly without a device,
the new kernels keep their register / scratch budgets, and the float64 filter model of tests/_denoise_model.py agrees with closed forms."""
import os
import subprocess

import numpy as np
import pytest

import _codeobj as CO
import _denoise_model as DM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "pbrlab_amd", "pbrlab-hip-cli")
EXE = os.path.join(ROOT, "tests", "cpp", "shim_features")
SYMBOLS = ("pbrhip_render_features", "pbrhip_render_features_device", "pbrhip_denoise", "pbrhip_denoise_device")
ENODEVICE = -3

# DESIGN.md §12.  k_features: 40 KB of LDS stack per block admit four blocks per CU = four waves per SIMD, so 128 VGPRs are free;
# the filter kernels: at least four waves per SIMD (at 46-48 registers they reach eight).
FEATURE_KERNELS = ("k_features<true, false>", "k_features<true, true>", "k_features<false, true>")
DENOISE_KERNELS = ("k_denoise_prepare", "k_denoise_iteration<false>", "k_denoise_iteration<true>")


def test_symbols_and_names_exist():
    import pbrlab_amd as pa
    from pbrlab_amd import _lib, api
    L = _lib.lib()
    for name in SYMBOLS:
        assert name in _lib.EXPORTS and hasattr(L, name), name
    for name in ("FeatureLayer", "RenderFeatures", "Denoise"):
        assert hasattr(api, name) and hasattr(pa, name), name
    f = pa.FeatureLayer(5, 3)
    assert f.albedo.shape == (3, 5, 4) and f.normal_depth.shape == (3, 5, 4) and f.count.shape == (3, 5)
    f.albedo[...] = (0.5, 0.25, 1.0, 2.0)
    f.normal_depth[...] = (0.0, 0.0, 8.0, 6.0)
    f.count[...] = 4
    assert np.allclose(f.mean_albedo(), ((0.5 + 2) / 4, (0.25 + 2) / 4, (1.0 + 2) / 4))  # two misses count as white
    assert np.allclose(f.mean_normal(), (0, 0, 1)) and np.allclose(f.mean_depth(), 3.0)
    f.Clear()
    assert not f.albedo.any() and not f.count.any() and np.isinf(f.mean_depth()).all() and np.allclose(f.mean_albedo(), 1.0)


def test_denoise_fails_loudly_without_device():
    import pbrlab_amd as pa
    if pa.device_count() > 0:
        pytest.skip("a GPU is present")
    layer = pa.RenderLayer(8, 6)
    layer.count[...] = 1
    with pytest.raises(pa.PbrHipError) as e:
        pa.Denoise(layer)
    assert e.value.code == ENODEVICE
    with pytest.raises(pa.PbrHipError) as e:
        pa.Denoise(layer, pa.FeatureLayer(8, 6))
    assert e.value.code == ENODEVICE


def test_new_kernels_stay_within_their_budgets():
    if not CO.available():
        pytest.skip("libpbrhip.so or the LLVM tools are missing")
    import _codeobj_tus as T
    table = T.kernel_table()
    for name in FEATURE_KERNELS:
        assert name in table, (name, sorted(k for k in table if "feature" in k))
        got = table[name]
        assert got["private_segment_fixed_size"] == 0, (name, got)
        assert got["vgpr_count"] <= 128 and CO.waves_per_simd(got["vgpr_count"]) >= 4, (name, got)
        assert got["group_segment_fixed_size"] == 40 * 256 * 4, (name, got)  # the LDS part of the traversal stack: four blocks per CU
    for name in DENOISE_KERNELS:
        assert name in table, (name, sorted(k for k in table if "denoise" in k))
        got = table[name]
        assert got["private_segment_fixed_size"] == 0 and CO.waves_per_simd(got["vgpr_count"]) >= 4, (name, got)
        assert got["group_segment_fixed_size"] == 0, (name, got)
    # the render kernels' translation unit is still the library's first code object, with every kernel the budget tests name
    first = CO.kernel_table()
    assert not any("k_features" in k or "k_denoise" in k for k in first) and all(k in table for k in first)


# ---------------------------------------------------------------------------------------------------- the float64 model
def _plane(H, W, normal=(0.0, 0.0, 1.0), depth=3.0, hits=4):
    ah = np.zeros((H, W, 4))
    ah[..., :3] = 0.5 * hits
    ah[..., 3] = hits
    nd = np.zeros((H, W, 4))
    nd[..., :3] = np.asarray(normal) * hits
    nd[..., 3] = depth * hits
    return ah, nd, np.full((H, W), hits, np.uint32)


def test_model_constant_image_is_a_fixed_point():
    H, W = 23, 31
    rng = np.random.RandomState(3)
    ah, nd, fc = _plane(H, W)
    nd[..., :3] = rng.normal(size=(H, W, 3))  # any features
    nd[..., 3] = rng.uniform(1, 9, (H, W)) * 4
    ah[5:9, 4:20] = 0  # a background region
    count = np.full((H, W), 8, np.uint32)
    rgba = np.zeros((H, W, 4))
    rgba[..., :3] = np.array([0.3, 0.6, 0.9]) * 8
    out = DM.denoise(rgba, count, None, None, None, sigma_color=1.0, sigma_depth=1.0)
    assert np.abs(out[..., :3] - (0.3, 0.6, 0.9)).max() < 1e-14 and (out[..., 3] == 1).all()
    # with features the demodulated colour is what stays constant
    rgba[..., :3] = 8 * 0.7 * DM.prepare(rgba, count, ah, nd, fc)[1]
    out = DM.denoise(rgba, count, ah, nd, fc, sigma_color=1.0, sigma_depth=1.0)
    assert np.abs(out[..., :3] - rgba[..., :3] / 8).max() < 1e-14


def _separable_b3(img, iterations):
    """the plain B3 A-trous convolution with renormalised borders: rows, then columns, by explicit shifts (an independent code path)"""
    out = img.copy()
    H, W = img.shape[:2]
    for i in range(iterations):
        s = 1 << i
        for axis, n in ((1, W), (0, H)):
            num, den = np.zeros_like(out), np.zeros(out.shape[:2] + (1,))
            for k, h in zip(range(-2, 3), DM.B3):
                lo, hi = max(0, -k * s), min(n, n - k * s)
                if lo >= hi:
                    continue
                dst = [slice(None)] * 3
                src = [slice(None)] * 3
                dst[axis], src[axis] = slice(lo, hi), slice(lo + k * s, hi + k * s)
                num[tuple(dst)] += h * out[tuple(src)]
                den[tuple(dst)] += h
            out = num / den
    return out


def test_model_without_edge_stopping_is_the_b3_atrous_transform():
    H, W = 37, 45
    rng = np.random.RandomState(5)
    ah, nd, fc = _plane(H, W)
    count = np.full((H, W), 2, np.uint32)
    rgba = np.zeros((H, W, 4))
    rgba[..., :3] = rng.uniform(0, 2, (H, W, 3))
    want = _separable_b3(rgba[..., :3] / 2 / 0.5, 4) * 0.5
    got = DM.denoise(rgba, count, ah, nd, fc, iterations=4, sigma_color=0.0, sigma_depth=0.0)
    assert np.abs(got[..., :3] - want).max() < 1e-13


def test_model_weights_of_a_hand_computed_example():
    """5 x 5, iteration 0, the tap one to the right and one down of the centre: N_p = (0, 0, 1), N_q = (0, 0.6, 0.8), two squarings ->
    0.8^4; z_p = 2, z_q = 2.5, sigma_depth = 0.5 -> exp(-0.5 / (0.5 x 2 x sqrt 2)); e_p - e_q = (0.3, 0, 0.4), sigma_color = 0.5 -> exp(-1)"""
    H = W = 5
    ah, nd, fc = _plane(H, W, depth=2.0, hits=1)
    ah[..., :3] = 1.0
    nd[3, 3] = (0.0, 0.6, 0.8, 2.5)
    count = np.ones((H, W), np.uint32)
    rgba = np.zeros((H, W, 4))
    rgba[..., :3] = (0.5, 0.2, 0.6)
    rgba[3, 3, :3] = (0.2, 0.2, 0.2)
    e, a, valid, surface, N, z = DM.prepare(rgba, count, ah, nd, fc)
    w, exists, qy, qx = DM.weights(e, valid, surface, N, z, 0, 1, 1, 0.5, 0.5, 2)
    assert exists[2, 2] and (qy[2, 2], qx[2, 2]) == (3, 3)
    want = 0.8 ** 4 * np.exp(-0.5 / (0.5 * 2.0 * np.sqrt(2.0))) * np.exp(-(0.09 + 0.16) / 0.25)
    assert abs(w[2, 2] - want) < 1e-15
    # a step of 2: sigma_color halves, the distance doubles
    w, exists, qy, qx = DM.weights(e, valid, surface, N, z, 1, 1, 1, 0.5, 0.5, 2)
    assert exists[1, 1] and (qy[1, 1], qx[1, 1]) == (3, 3)
    want = 0.8 ** 4 * np.exp(-0.5 / (0.5 * 2.0 * 2 * np.sqrt(2.0))) * np.exp(-(0.09 + 0.16) / 0.0625)
    assert abs(w[1, 1] - want) < 1e-15
    # a background tap and a hole
    ah[3, 3, 3] = 0
    e, a, valid, surface, N, z = DM.prepare(rgba, count, ah, nd, fc)
    assert DM.weights(e, valid, surface, N, z, 0, 1, 1, 0.5, 0.5, 2)[0][2, 2] == 0
    count[3, 3] = 0
    e, a, valid, surface, N, z = DM.prepare(rgba, count, ah, nd, fc)
    assert not DM.weights(e, valid, surface, N, z, 0, 1, 1, 0.5, 0.5, 2)[1][2, 2]


# ---------------------------------------------------------------------------------------------------- CLI and C++ shim
def test_cli_rejects_bad_feature_flags():
    if not os.path.exists(CLI):
        pytest.skip("pbrlab-hip-cli not built")
    for args, msg in ((["--aov"], "missing value for --aov"), (["--feature-spp", "0"], "--feature-spp needs an integer in 1.."),
                      (["--feature-spp", "many"], "--feature-spp needs an integer in 1.."), (["--denoise", "--feature-spp", "-3"], "--feature-spp needs an integer in 1.."),
                      (["--feature-spp", "4"], "--feature-spp needs --aov or --denoise")):
        r = subprocess.run([CLI, "scene.obj"] + args, capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and msg in r.stderr, (args, r.returncode, r.stderr)


def test_features_shim_caller_compiles():
    import pbrlab_amd as pa
    lib = os.path.join(ROOT, "pbrlab_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "shim_features.cc"),
                           "-L" + lib, "-lpbrhip", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib", "-lpthread", "-o", EXE])
    if pa.device_count() == 0:
        r = subprocess.run([EXE], capture_output=True, text=True)
        assert r.returncode == 3, r.stderr
