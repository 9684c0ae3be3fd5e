"""Register / scratch / LDS budgets of knearest.hip's kernel, read from the built libpbrhip.so in
test_allhits_budgets.py's way (no GPU needed; register and scratch metadata only).

k_knearest<COUNT, CURVES, WIDE> is in k_all_hits' launch class: kSimpleLdsStack = 40 stack entries per lane in LDS -- 40 * 256 * 4
bytes per block --, __launch_bounds__(256, 4), so four blocks per CU need at most 128 VGPRs.  No instance may use scratch: the list of
the K best lives in the query's output rows, not in an indexed register array.  The VGPR ceilings are the counts of the code object
built on 2026-10-21, rounded up to the next allocation granule of eight: <COUNT, CURVES, WIDE> without count 76 / 82 / 76 / 80 for
<false, false>, <false, true>, <true, false>, <true, true>, with count 79 / 84 / 79 / 83."""
import pytest

import _codeobj as CO
import _codeobj_tus as TUS

K_SIMPLE_LDS_STACK = 40  # dscene.h
LDS = K_SIMPLE_LDS_STACK * 256 * 4
# kernel -> max VGPRs (2026-10-21); measured in the comments
BUDGETS = {
    "k_knearest<false, false, false>": 80,   # 76
    "k_knearest<false, false, true>": 88,    # 82
    "k_knearest<false, true, false>": 80,    # 76
    "k_knearest<false, true, true>": 80,     # 80
    "k_knearest<true, false, false>": 80,    # 79
    "k_knearest<true, false, true>": 88,     # 84
    "k_knearest<true, true, false>": 80,     # 79
    "k_knearest<true, true, true>": 88,      # 83
}


def _table():
    if not CO.available():
        pytest.skip("built library or LLVM tools not available")
    return TUS.kernel_table()


def test_k_nearest_kernels_use_no_scratch_and_stay_within_their_registers():
    table = _table()
    for name, vgprs in BUDGETS.items():
        assert name in table, (name, sorted(k for k in table if "k_knearest" in k))
        got = table[name]
        print(name, got)
        assert got["private_segment_fixed_size"] == 0, (name, got)
        assert got["vgpr_count"] <= vgprs, (name, got)
        assert got["group_segment_fixed_size"] == LDS == 40960, (name, got)
    # and nothing in knearest.hip escaped the table above
    assert sorted(k for k in table if "k_knearest" in k) == sorted(BUDGETS)


def test_k_nearest_kernels_are_in_the_all_hits_kernels_occupancy_class():
    table = _table()
    for name in BUDGETS:
        assert CO.waves_per_simd(table[name]["vgpr_count"]) >= 4, (name, table[name])
    for name in ("k_all_hits<false, false, false>", "k_all_hits<true, true, true>"):
        assert table[name]["group_segment_fixed_size"] == LDS
