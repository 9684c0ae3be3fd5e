"""CPU: the environment light's host tables (pbrlab_amd/csrc/env_tables.cpp) and direction <-> texel mapping (denv.h) --
scripts/fuzz/env_check.cpp compiled for the host only, on random and degenerate maps (1x1, one bright texel, black rows,
all black, 4096 x 2048 with a sun).  Checked there: the alias table reproduces every texel's probability to 1e-6 relative,
black texels are never chosen, the device's selection (64-bit texel, 32-bit coin against the keep threshold) is within its stated
bound of the table, the normaliser matches an independent long-double sum to 1e-12, sum pdf_env * omega = 1 to 1e-7 (float pdfs),
texel centres and quarter points map back to their texel (also through a rotation) with the functions the kernels run, an
all-black map is no environment, bad input is refused."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"


def test_env_tables_on_random_and_degenerate_maps(tmp_path):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    cs = os.path.join(ROOT, "pbrlab_amd", "csrc")
    exe = str(tmp_path / "env_check")
    subprocess.check_call([HIPCC, "--offload-host-only", "-std=c++17", "-O2", "-ffp-contract=off", "-I" + cs, "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "scripts", "fuzz", "env_check.cpp"), os.path.join(cs, "env_tables.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "cases ok" in r.stdout, r.stdout + r.stderr
