"""tests/cpp/shim_emission.cc: pbrlab::RenderFeaturesEmission, SplitEmission and MergeEmission through the C++ shim
(include/pbrlab_hip.hpp).  Without a device the caller compiles and fails loudly, like shim_smoke; on the GPU it runs
render -> features + emission -> motion -> ids -> split -> accumulate -> filter -> merge and split -> denoise -> merge."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "shim_emission")


def test_emission_shim_caller_compiles():
    import pbrlab_amd as pa
    lib = os.path.join(ROOT, "pbrlab_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "shim_emission.cc"),
                           "-L" + lib, "-lpbrhip", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib", "-lpthread", "-o", EXE])
    if pa.device_count() == 0:
        r = subprocess.run([EXE], capture_output=True, text=True)
        assert r.returncode == 3 and "shim:" in r.stderr, (r.returncode, r.stderr)


@pytest.mark.gpu
def test_emission_shim_caller_runs():
    import pbrlab_amd as pa
    if pa.device_count() < 1:
        pytest.fail("no HIP device: the GPU tests must run on an MI355X (there is no CPU fallback)")
    test_emission_shim_caller_compiles()
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "shim ok" in r.stdout, (r.returncode, r.stdout + r.stderr)
