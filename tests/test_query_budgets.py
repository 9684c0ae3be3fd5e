"""Register / scratch / LDS budgets of the query.hip kernels, read from the built libpbrhip.so in
test_emission_budgets.py's way (no GPU needed): query.hip is a translation unit of its own, so every code object of the library is read.

No kernel may use scratch.  LDS is what the kernels declare: k_query_nearest holds kSimpleLdsStack = 40 stack entries per lane (40 KB
per block of 256, four blocks per CU: k_features' class, __launch_bounds__(256, 4), at most 128 VGPRs); k_query_pv holds trace_pv's
part of the stack -- 16 entries per lane, 20 for the Q tree of a scene with curves -- and with curves the 10 words of the ray frame:
k_hook_pv's figures.  The VGPR ceilings are the measured counts rounded up to the next allocation granule of eight.  Measured:
k_query_nearest<CURVES, WIDE> <false, false> / <false, true> / <true, false> / <true, true> 76 / 74 / 76 / 75 (k_features 112 / 113 / 109
for its three instances); k_query_pv<ANY, CURVES, WIDE> closest 73 / 80 / 78 / 94, any 73 / 90 / 78 / 94 in the same order
(k_hook_pv<false, ...> 79 / 85 / 93 and <true, ...> 82 / 85 / 93 for <false, true>, <true, false>, <true, true>)."""
import pytest

import _codeobj as CO
import _codeobj_tus as TUS

# kernel -> (max VGPRs, max scratch bytes, LDS bytes); measured VGPRs in the comments
BUDGETS = {
    "k_query_nearest<false, false>": (80, 0, 40960),     # 76
    "k_query_nearest<false, true>": (80, 0, 40960),      # 74
    "k_query_nearest<true, false>": (80, 0, 40960),      # 76
    "k_query_nearest<true, true>": (80, 0, 40960),       # 75
    "k_query_pv<false, false, false>": (80, 0, 16384),   # 73
    "k_query_pv<false, false, true>": (80, 0, 16384),    # 80
    "k_query_pv<false, true, false>": (80, 0, 26624),    # 78
    "k_query_pv<false, true, true>": (96, 0, 30720),     # 94
    "k_query_pv<true, false, false>": (80, 0, 16384),    # 73
    "k_query_pv<true, false, true>": (96, 0, 16384),     # 90
    "k_query_pv<true, true, false>": (80, 0, 26624),     # 78
    "k_query_pv<true, true, true>": (96, 0, 30720),      # 94
}
BESIDE = ("k_features<true, false>", "k_features<true, true>", "k_features<false, true>", "k_hook_pv<false, false, true>", "k_hook_pv<false, true, false>",
          "k_hook_pv<false, true, true>", "k_hook_pv<true, false, true>", "k_hook_pv<true, true, false>", "k_hook_pv<true, true, true>")


def _table():
    if not CO.available():
        pytest.skip("built library or LLVM tools not available")
    return TUS.kernel_table()


def test_query_kernels_use_no_scratch_and_stay_within_their_registers():
    table = _table()
    for name, (vgprs, scratch, lds) in BUDGETS.items():
        assert name in table, (name, sorted(k for k in table if "k_query" in k))
        got = table[name]
        print(name, got)
        assert got["private_segment_fixed_size"] <= scratch, (name, got)
        assert got["vgpr_count"] <= vgprs, (name, got)
        assert got["group_segment_fixed_size"] == lds, (name, got)
    for name in BESIDE:
        print(name, table[name])
    # and nothing in query.hip escaped the table above
    assert sorted(k for k in table if "k_query" in k) == sorted(BUDGETS)


def test_nearest_kernel_is_in_k_features_occupancy_class():
    table = _table()
    for name in BUDGETS:
        if "nearest" in name:
            got = table[name]
            assert got["group_segment_fixed_size"] == 40960 and CO.waves_per_simd(got["vgpr_count"]) >= 4 and got["private_segment_fixed_size"] == 0
    for name in ("k_features<true, false>", "k_features<true, true>", "k_features<false, true>"):
        assert table[name]["group_segment_fixed_size"] == 40960
