#!/usr/bin/env python3
"""Writes the stored answers of the reference library for the tests that compare against it, so that those tests run on any
checkout (where oracle/_ref/ is built they still call the live library).  Run where the reference tree exists, after build():

  ref_leaf_outputs.npz    what the REFERENCE's own leaf functions (oracle/_ref/libref_leaf.so) return for the seeded inputs of
                          tests/test_oracle_vs_reference_leaf.py: "<case>/<array>", made by that module's REF_CASES[case].
  io/ref_io_outputs.npz   what the reference's own loaders and JPEG writer (oracle/_ref/libref_io.so) returned, or wrote, for
                          every input of tests/test_io_cpu.py, keyed by the input's bytes (tests/_refio.py): recorded by running
                          that module against the live library.  Loader results are kept as digests, the writer's files whole.
                          The two EXR fuzz tests are left out: their inputs come from the reference's EXR writer, whose files
                          (random float planes) are too large to store, so those tests need the live library.
                          A few mutated files of the mutation fuzz tests make stb read past their end: those digests change
                          from run to run, and the tests count such files as disagreements, live or stored, within their margin.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _oracle as O  # noqa: E402


def make_leaf():
    import test_oracle_vs_reference_leaf as T
    R = O.ref()
    out = {}
    for case, compute in sorted(T.REF_CASES.items()):
        for name, a in compute(R).items():
            out[f"{case}/{name}"] = np.asarray(a)
    np.savez_compressed(O.REF_OUTPUTS, **out)
    print(f"{O.REF_OUTPUTS}: {len(out)} arrays, {os.path.getsize(O.REF_OUTPUTS)} bytes")


def make_io():
    import pytest
    import _refio
    _refio.RECORD = _refio.STORED
    rc = pytest.main(["-q", "-p", "no:cacheprovider", os.path.join(ROOT, "tests", "test_io_cpu.py"),
                      "-k", "not test_exr_decode_fuzz_vs_reference and not test_exr_piz_vs_reference"])
    if rc != 0:
        raise SystemExit(f"tests/test_io_cpu.py failed against the live library (rc {rc}): nothing written")
    n = _refio.save_recorded()
    print(f"{_refio.STORED}: {n} answers, {os.path.getsize(_refio.STORED)} bytes")


if __name__ == "__main__":
    import _refio
    if not (O.have_ref() and _refio.available()):
        raise SystemExit("oracle/_ref/ is not built (build(), where the reference tree exists)")
    make_leaf()
    make_io()
