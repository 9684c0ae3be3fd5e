"""Register / scratch / LDS budgets of the sdf.hip kernels, read from the built libpbrhip.so in test_query_budgets.py's way
(no GPU needed), and k_query_nearest's counts, which sharing dnearest.h with sdf.hip must not have changed.

No kernel may use scratch.  k_signed_query is k_query_nearest's launch class: kSimpleLdsStack = 40 stack entries per lane in LDS (40 KB per
block of 256), four blocks per CU, so at most 128 VGPRs.  The VGPR counts are pinned at what was measured: k_signed_query<CURVES, WIDE,
GRID> 76 / 74 for <false, true, *>, 79 / 75 for <true, false, *>, 78 / 73 for <true, true, *> (points / grid); the table kernels
k_sdf_faces 30 and k_sdf_rows 17; k_query_nearest 76 / 74 / 76 / 75 as before this unit existed."""
import pytest

import _codeobj as CO
import _codeobj_tus as TUS

# kernel -> (VGPRs, LDS bytes)
SIGNED = {
    "k_signed_query<false, true, false>": (76, 40960),
    "k_signed_query<false, true, true>": (74, 40960),
    "k_signed_query<true, false, false>": (79, 40960),
    "k_signed_query<true, false, true>": (75, 40960),
    "k_signed_query<true, true, false>": (78, 40960),
    "k_signed_query<true, true, true>": (73, 40960),
    "k_sdf_faces": (30, 0),
    "k_sdf_rows": (17, 0),
}
NEAREST = {"k_query_nearest<false, false>": 76, "k_query_nearest<false, true>": 74, "k_query_nearest<true, false>": 76, "k_query_nearest<true, true>": 75}


def _table():
    if not CO.available():
        pytest.skip("built library or LLVM tools not available")
    return TUS.kernel_table()


def test_signed_kernels_use_no_scratch_and_keep_their_registers():
    table = _table()
    for name, (vgprs, lds) in SIGNED.items():
        assert name in table, (name, sorted(k for k in table if "k_signed" in k or "k_sdf" in k))
        got = table[name]
        print(name, got)
        assert got["private_segment_fixed_size"] == 0, (name, got)
        assert got["vgpr_count"] == vgprs, (name, got)
        assert got["group_segment_fixed_size"] == lds, (name, got)
    # nothing in sdf.hip escaped the table above
    assert sorted(k for k in table if "k_signed" in k or "k_sdf" in k) == sorted(SIGNED)


def test_signed_query_is_in_k_query_nearest_occupancy_class():
    table = _table()
    for name in SIGNED:
        if "k_signed_query" in name:
            assert CO.waves_per_simd(table[name]["vgpr_count"]) >= 4


def test_k_query_nearest_is_unchanged():
    table = _table()
    for name, vgprs in NEAREST.items():
        got = table[name]
        print(name, got)
        assert got["vgpr_count"] == vgprs and got["private_segment_fixed_size"] == 0 and got["group_segment_fixed_size"] == 40960, (name, got)
