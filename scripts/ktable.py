#!/usr/bin/env python3
"""The kernels of a built library, read from its gfx950 code object (tests/_codeobj.py):

  scripts/ktable.py [libpbrhip.so] [name prefix ...]          registers / scratch / LDS of each kernel
  scripts/ktable.py [libpbrhip.so] --diff OTHER.so [old=new ...]
      OTHER's kernels against this library's, instruction by instruction (position-independent text) and by their metadata;
      old=new renames a kernel of OTHER first.  Exit status 1 when a kernel differs or exists on one side only.
  scripts/ktable.py [libpbrhip.so] --diff OTHER.so --histogram [--ignore a,b,...] [name prefix ...]
      the same comparison by what a kernel is made of instead of where it stands: per kernel the metadata that differs and the
      mnemonics whose counts differ (register numbers and instruction order do not count).  Mnemonics of the --ignore list (default:
      s_nop,s_waitcnt,v_mov_b32,s_mov_b32,s_mov_b64 -- waits and copies, which follow register allocation; named without the
      disassembler's encoding suffix: v_mov_b32 covers v_mov_b32_e32 and _e64) are shown in brackets and do not fail the comparison.  Exit status 1 when anything else differs or a kernel exists on one side only."""
import collections
import os
import re
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import _codeobj as CO


def show(lib, prefixes):
    for n, v in sorted(CO.kernel_table(lib).items()):
        if not prefixes or n.startswith(prefixes):
            print(f"{n:50s} vgpr {v['vgpr_count']:4d} sgpr {v['sgpr_count']:4d} scratch {v['private_segment_fixed_size']:4d} lds {v['group_segment_fixed_size']:6d}")


def diff(lib, other, renames):
    ren = dict(r.split("=", 1) for r in renames)
    new_t, new_d = CO.kernel_table(lib), CO.disassembly(lib)
    old_t = {ren.get(k, k): v for k, v in CO.kernel_table(other).items()}
    old_d = {ren.get(k, k): v for k, v in CO.disassembly(other).items()}
    only_old, only_new = sorted(set(old_t) - set(new_t)), sorted(set(new_t) - set(old_t))
    lib, other = os.path.relpath(lib), os.path.relpath(other)
    print(f"kernels: {len(old_t)} in {other}, {len(new_t)} in {lib}")
    for side, names in ((other, only_old), (lib, only_new)):
        for n in names:
            print(f"only in {side}: {n}")
    same = different = 0
    for n in sorted(set(old_t) & set(new_t)):
        meta = [f"{f} {old_t[n][f]} -> {new_t[n][f]}" for f in CO.FIELDS if old_t[n][f] != new_t[n][f]]
        if old_d[n] == new_d[n] and not meta:
            same += 1
            continue
        different += 1
        moved = sum(1 for a, b in zip(old_d[n], new_d[n]) if a != b)
        print(f"DIFF {n}: {len(old_d[n])} -> {len(new_d[n])} instructions, {moved} lines differ in place" + "".join("; " + m for m in meta))
    print(f"identical: {same} different: {different}")
    return 1 if different or only_old or only_new else 0


IGNORE = "s_nop,s_waitcnt,v_mov_b32,s_mov_b32,s_mov_b64"


def ignored(mnemonic, ignore):
    """the ignore list names instructions without the encoding suffix the disassembler appends (v_mov_b32_e32, _e64, _sdwa, _dpp)"""
    return re.sub(r"_(e32|e64|sdwa|dpp)$", "", mnemonic) in ignore


def histogram_diff(lib, other, ignore, prefixes):
    new_t, new_d, old_t, old_d = CO.kernel_table(lib), CO.disassembly(lib), CO.kernel_table(other), CO.disassembly(other)
    pick = lambda t: {n for n in t if not prefixes or n.startswith(prefixes)}
    only = [(os.path.relpath(other), sorted(pick(old_t) - set(new_t))), (os.path.relpath(lib), sorted(pick(new_t) - set(old_t)))]
    for side, names in only:
        for n in names:
            print(f"only in {side}: {n}")
    same = tolerated = different = 0
    for n in sorted(pick(old_t) & set(new_t)):
        meta = [f"{f} {old_t[n][f]} -> {new_t[n][f]}" for f in CO.FIELDS if old_t[n][f] != new_t[n][f]]
        old_h, new_h = (collections.Counter(line.split()[0] for line in d[n]) for d in (old_d, new_d))
        changed = {m: (old_h[m], new_h[m]) for m in sorted(set(old_h) | set(new_h)) if old_h[m] != new_h[m]}
        hard = [f"{m} {a} -> {b}" for m, (a, b) in changed.items() if not ignored(m, ignore)]
        soft = [f"[{m} {a} -> {b}]" for m, (a, b) in changed.items() if ignored(m, ignore)]
        if not meta and not changed:
            same += 1
            continue
        tolerated, different = tolerated + (not (meta or hard)), different + bool(meta or hard)
        print(f"{'DIFF' if meta or hard else 'same'} {n}: {len(old_d[n])} -> {len(new_d[n])} instructions; " + "; ".join(meta + hard + soft))
    print(f"equal histograms: {same}, equal up to {','.join(sorted(ignore))}: {tolerated}, different: {different}")
    return 1 if different or only[0][1] or only[1][1] else 0


if __name__ == "__main__":
    args = sys.argv[1:]
    lib = args.pop(0) if args and args[0] != "--diff" else CO.LIB
    if args and args[0] == "--diff":
        if len(args) < 2:
            sys.exit(__doc__)
        if "--histogram" in args:
            rest, ignore = [a for a in args[2:] if a != "--histogram"], IGNORE
            if "--ignore" in rest:
                i = rest.index("--ignore")
                if i + 1 == len(rest):
                    sys.exit(__doc__)
                ignore = rest[i + 1]
                del rest[i:i + 2]
            sys.exit(histogram_diff(lib, args[1], set(filter(None, ignore.split(","))), tuple(rest)))
        sys.exit(diff(lib, args[1], args[2:]))
    show(lib, tuple(args))
