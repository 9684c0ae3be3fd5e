"""Registers and scratch of the shaft grid's kernels, read from the gfx950 code object inside the built libpbrhip.so (no GPU needed).

`k_shaft_grid` (kernels.hip; shaft_grid.h) is new.  It runs once per commit or refit, one thread per (light, cell), and walks the Q tree
with a private stack: kShaftStack = kStackDepth + 4 = 68 words = 272 bytes of scratch are its design, the cell's list and record (15
words) may join them; 512 bytes bound the two with room for the compiler's own temporaries, and 128 registers keep four waves per SIMD
while the walk waits on memory.  `k_shade_principled<0>`, which now carries the grid's lookup and leaf tests, keeps the budget
tests/test_kernel_budgets.py gives it (128 registers, no scratch); it is asserted there and, for the reader of this file, here."""
import pytest

import _codeobj as CO
from _codeobj import waves_per_simd


def kernel_table():
    if not CO.available():
        pytest.skip("built library or LLVM tools not available")
    return CO.kernel_table()


def test_the_build_kernel():
    table = kernel_table()
    assert "k_shaft_grid" in table, sorted(table)
    got = table["k_shaft_grid"]
    print("k_shaft_grid", got)
    assert got["vgpr_count"] <= 128 and waves_per_simd(got["vgpr_count"]) >= 4, got
    assert 272 <= got["private_segment_fixed_size"] <= 512, got
    assert got["group_segment_fixed_size"] == 0, got


def test_the_shading_kernel_that_uses_the_grid():
    got = kernel_table()["k_shade_principled<0>"]
    print("k_shade_principled<0>", got)
    assert got["vgpr_count"] <= 128 and got["private_segment_fixed_size"] == 0, got
