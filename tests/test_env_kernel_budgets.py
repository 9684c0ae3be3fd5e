"""Register / scratch budgets of the environment light's kernels, read from the gfx950 code object like
test_kernel_budgets.py does.

No environment kernel reads or writes scratch: the disassembly of every one of them holds no scratch or buffer instruction, and
its private segment is 0 bytes -- except k_shade_principled<6> (textured materials), whose code object reserves 8 bytes that no
instruction touches, exactly like its twin k_shade_principled<2> of the parent.  Occupancy classes are the twins', except
k_shade_principled<5> (media + environment): three waves per SIMD, where four spilled 12 bytes; its measured cost is in
profiles/README.md."""
import re

import _codeobj as CO
from _codeobj import waves_per_simd
from test_kernel_budgets import kernel_table

# kernel -> (max VGPRs, min waves per SIMD)
ENV_BUDGETS = {
    "k_classify<true>": (64, 8),
    "k_shade_hair<true>": (128, 4),
    "k_sss_step<true>": (128, 4),
    "k_shade_principled<4>": (128, 4),
    "k_shade_principled<5>": (168, 3),
    "k_shade_principled<6>": (168, 3),
    "k_tail<4, false, false, true>": (168, 3),
    "k_tail<4, false, true, true>": (168, 3),
    "k_tail<5, false, false, true>": (168, 3),
    "k_tail<5, false, true, true>": (168, 3),
    "k_tail<6, false, false, true>": (168, 3),
}
RESERVED_UNUSED = {"k_shade_principled<6>": 8}  # private bytes the compiler reserves and no instruction uses (its twin <2> too)


def _env_kernels(table):
    return [k for k in table if re.match(r"k_(classify|shade_hair|sss_step)<true>$", k) or re.match(r"k_(shade_principled|tail)<[456][,>]", k)]


def test_env_kernels_stay_within_their_budgets():
    table = kernel_table()
    for name, (vgprs, waves) in ENV_BUDGETS.items():
        assert name in table, (name, sorted(_env_kernels(table)))
        got = table[name]
        assert got["vgpr_count"] <= vgprs, (name, got)
        assert waves_per_simd(got["vgpr_count"]) >= waves, (name, got)


def test_every_env_kernel_has_no_scratch():
    table = kernel_table()
    env = _env_kernels(table)
    assert len(env) >= 3 + 3 + 16
    for k in env:
        assert table[k]["private_segment_fixed_size"] <= RESERVED_UNUSED.get(k, 0), (k, table[k])
    # and no instruction of any of them touches scratch
    by_name = CO.disassembly()
    for k in env:
        assert k in by_name, k
        bad = [l for l in by_name[k] if re.search(r"\b(scratch_|buffer_)", l)]
        assert not bad, (k, bad[:4])
