"""The look-at camera without a GPU: the float64 model's draws against the oracle's generator, the CLI's flag checks,
the C++ caller of Scene::SetCamera compiling, and the register / scratch budgets of the camera kernels."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import _camera_analytic as CA
from _codeobj import waves_per_simd
from test_kernel_budgets import kernel_table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "pbrlab_amd", "pbrlab-hip-cli")
EXE = os.path.join(ROOT, "tests", "cpp", "shim_camera")

# kernel -> max VGPRs (8 waves per SIMD: both are one pass over memory)
CAMERA_BUDGETS = {"k_generate_camera": 64, "k_camera_rays": 64}


def test_model_draws_match_the_oracle_generator():
    import _oracle as O
    L = O.OracleScene().L
    for init in (0, 7, (5 << 32) + 1234, (1 << 63) + 99):
        for seq in (1234567890, 2718281828, 1):
            a = np.zeros(6, np.float32)
            L.orc_kat_rng(C.c_uint64(init), C.c_uint64(seq), 6, a.ctypes.data_as(C.POINTER(C.c_float)))
            assert np.array_equal(CA.draws([init], seq, 6)[0].astype(np.float32), a), (init, seq)


def test_model_frame_is_orthonormal_and_keeps_the_reference_orientation():
    cam = CA.LookAt((0, 0, 5), (0, 0, 0), (0, 1, 0), 60.0, 64, 48)
    assert np.allclose(cam.f, (0, 0, -1)) and np.allclose(cam.r, (1, 0, 0)) and np.allclose(cam.u, (0, 1, 0))
    d = cam.dirs(np.array([0.0, 63.0]), np.array([0.0, 47.0]), 0.5, 0.5)
    assert d[0, 0] < 0 < d[0, 1] and d[1, 0] > 0 > d[1, 1]  # row 0 is the top, column 0 the left


def test_cli_rejects_bad_camera_flags():
    if not os.path.exists(CLI):
        pytest.skip("pbrlab-hip-cli not built")
    for args, msg in ((["--lookat", "0,0,0"], "--lookat needs --eye"), (["--eye", "0,0,1"], "--eye needs --lookat"),
                      (["--eye", "1,2", "--lookat", "0,0,0"], "--eye needs three finite numbers"),
                      (["--eye", "1,2,x", "--lookat", "0,0,0"], "--eye needs three finite numbers"),
                      (["--eye", "1,2,3", "--lookat", "0,0,nan"], "--lookat needs three finite numbers"),
                      (["--eye", "1,2,3", "--lookat", "0,0,0", "--fov", "wide"], "--fov needs a finite number")):
        r = subprocess.run([CLI, "scene.obj"] + args, capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and msg in r.stderr, (args, r.returncode, r.stderr)


def test_camera_shim_caller_compiles():
    import pbrlab_amd as pa
    lib = os.path.join(ROOT, "pbrlab_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "shim_camera.cc"),
                           "-L" + lib, "-lpbrhip", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib", "-lpthread", "-o", EXE])
    if pa.device_count() == 0:
        r = subprocess.run([EXE], capture_output=True, text=True)
        assert r.returncode == 3, r.stderr


def test_camera_kernels_stay_within_their_budgets():
    table = kernel_table()
    for name, vgprs in CAMERA_BUDGETS.items():
        assert name in table, name
        got = table[name]
        assert got["vgpr_count"] <= vgprs and waves_per_simd(got["vgpr_count"]) == 8, (name, got)
        assert got["private_segment_fixed_size"] == 0, (name, got)
