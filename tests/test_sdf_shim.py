"""tests/cpp/shim_sdf.cc: pbrlab::Scene::SignedDistance, SignedDistanceDevice, SignedDistanceGridDevice and SignedDistanceInfo through the
C++ shim (include/pbrlab_hip.hpp).  Without a device the caller compiles and fails loudly, like shim_query; on the GPU its answers,
printed as words, equal the Python binding's on the same scene and queries."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "shim_sdf")
F = np.float32
INF = np.inf
POINTS = [(0.25, 0.125, 1.25, INF), (0.0, 0.0, 0.0, INF), (2.0, 0.0, 1.25, INF), (2.0, 1.5, 1.25, INF), (0.5, 0.375, 0.0, INF), (0.25, 0.125, 1.25, 0.5),
          (np.nan, 0, 0, INF)]
FACES = [0, 2, 1, 0, 3, 2, 5, 6, 7, 5, 7, 4, 1, 5, 4, 1, 4, 0, 3, 6, 2, 3, 7, 6, 2, 6, 5, 2, 5, 1, 0, 7, 3, 0, 4, 7]


def test_sdf_shim_caller_compiles():
    import pbrlab_amd as pa
    lib = os.path.join(ROOT, "pbrlab_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "shim_sdf.cc"),
                           "-L" + lib, "-lpbrhip", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib", "-lpthread", "-o", EXE])
    if pa.device_count() == 0:
        r = subprocess.run([EXE], capture_output=True, text=True)
        assert r.returncode == 3 and "shim:" in r.stderr, (r.returncode, r.stderr)


def _python_lines():
    """the shim's scene and queries through the Python binding, formatted as the shim prints them"""
    import torch
    import pbrlab_amd as pa
    from pbrlab_amd import scenes
    x, y, z = 1.0, 0.5, 0.25
    verts = np.array([[-x, -y, -z, 1], [x, -y, -z, 1], [x, y, -z, 1], [-x, y, -z, 1], [-x, -y, z, 1], [x, -y, z, 1], [x, y, z, 1], [-x, y, z, 1]], F)
    mat = dict(scenes.PRINCIPLED_DEFAULTS, kind="principled", name="grey", base_color=(0.25, 0.25, 0.25))
    desc = scenes.SceneDesc(verts, np.zeros((0, 4), F), [mat], [scenes.Shape("box", np.array(FACES, np.uint32).reshape(-1, 3), None, np.zeros(12, np.uint32))])
    s = pa.scene_from_desc(desc)
    pts = np.array(POINTS, F)
    ident, closest, sd = (t.cpu().numpy().view(np.uint32) for t in s.SignedDistanceDevice(torch.from_numpy(pts).to("cuda:0")))
    hi, hc, hs = s.SignedDistance(pts)
    assert np.array_equal(hi, ident) and np.array_equal(hc.view(np.uint32), closest) and np.array_equal(hs.view(np.uint32), sd)
    grid = s.SignedDistanceGridDevice((-1.5, -0.75, 0.0), (1.5, 0.75, 0.5), (3, 2, 2))
    assert tuple(grid.shape) == (2, 2, 3)
    info = s.SignedDistanceInfo()
    word = lambda a: " ".join(f"{int(v):08x}" for v in a)
    lines = [f"S {i} {word(ident[i])} | {word(closest[i])} | {word(sd[i])}" for i in range(len(pts))]
    lines.append("G " + word(grid.cpu().numpy().view(np.uint32).reshape(-1)))
    lines.append("T " + " ".join(str(info[k]) for k in ("triangles", "vertices", "edges_manifold", "edges_boundary", "edges_nonmanifold", "edges_inconsistent")))
    return lines


@pytest.mark.gpu
def test_sdf_shim_caller_runs_and_matches_python():
    import pbrlab_amd as pa
    if pa.device_count() < 1:
        pytest.fail("no HIP device: the GPU tests must run on an MI355X (there is no CPU fallback)")
    pa.set_device(0)
    test_sdf_shim_caller_compiles()
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "shim ok" in r.stdout, (r.returncode, r.stdout + r.stderr)
    got = [ln for ln in r.stdout.splitlines() if ln[:2] in ("S ", "G ", "T ")]
    assert got == _python_lines()
