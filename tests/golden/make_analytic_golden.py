#!/usr/bin/env python3
"""Records tests/golden/analytic_expectations.npz: the float64 values tests/_analytic.py::Expectation returns on 300 receiver points of
each untextured case of tests/test_analytic_radiance.py (the points, the directions to the camera, E and the case's alternatives).
It was recorded at the commit before Expectation learned to resolve a base colour per point, and test_untextured_expectations_are_
unchanged holds every later model to those values bit for bit.  Re-record only when a change of the model is meant to move them."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_analytic_radiance as T  # noqa: E402


def main():
    out = {}
    for case in T.CASES:
        e = T.expected(case)
        i = np.random.RandomState(5).choice(len(e["pts"]), min(300, len(e["pts"])), replace=False)
        out[case + "/pts"], out[case + "/wo"] = e["pts"][i], e["wo"][i]
        out[case + "/E"] = e["ex"](e["pts"][i], e["wo"][i])
        print(case, out[case + "/E"].shape, float(np.abs(out[case + "/E"]).max()))
    np.savez_compressed(os.path.join(HERE, "analytic_expectations.npz"), **out)


if __name__ == "__main__":
    main()
