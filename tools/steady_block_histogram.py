#!/usr/bin/env python3
"""Instruction histogram of the attention kernel's steady tile iteration, from a device-only assembly listing.

    hipcc -O3 -std=c++17 --offload-arch=gfx950 -ffp-contract=off -fno-slp-vectorize -Ipointdsc_amd/csrc \
          --cuda-device-only -S pointdsc_amd/csrc/attention_split.hip -o attention_split.s
    python tools/steady_block_histogram.py attention_split.s [kernel-name substring ...] [--list]

The steady iteration (KIND == 0 of tile_iteration, attention_split_kernel.h) is the basic block of a kernel that holds the most
v_mfma instructions among the blocks inside a loop, ties going to the innermost loop: the block that branches back to its own
header (36 MFMAs in the 64-wide forms, 48 in the 128-wide ones; a block = the instructions between two labels).  For
every kernel whose mangled name contains all the substrings (default: every sc_attention_split_kernel instantiation) the tool
prints the block's size, its v_mfma / ds_read / LDS-DMA counts, the vector instructions that are not MFMAs, the scalar bookkeeping
(s_waitcnt, s_nop, s_add) and any scratch access, then the non-MFMA vector instructions by mnemonic.  --list prints the block.
What profiles/rowmax_forms_ab.txt records before and after a change to the loop.
"""
import collections
import re
import sys


def kernels(text):
    """{mangled name: [lines]} of the functions of a listing"""
    out, name, cur = {}, None, []
    for line in text.splitlines():
        m = re.match(r"^(_Z\w+):", line)
        if m:
            name, cur = m.group(1), []
            continue
        if name and line.startswith(".Lfunc_end"):
            out[name] = cur
            name = None
            continue
        if name:
            cur.append(line)
    return out


def blocks(lines):
    """[(label, [instructions])]: a block starts at a label and ends before the next one"""
    out, label, cur = [], "entry", []
    for line in lines:
        m = re.match(r"^(\.LBB\w+):", line)
        if m:
            out.append((label, cur))
            label, cur = m.group(1), []
            continue
        s = line.split(";")[0].strip()
        if s and not s.startswith(".") and not s.endswith(":"):
            cur.append(s)
    out.append((label, cur))
    return out


def steady_block(lines):
    """the block with the most v_mfma among those inside a loop (a backward branch spans them); ties go to the innermost loop"""
    bl = blocks(lines)
    order = {label: k for k, (label, _) in enumerate(bl)}
    span = {}                                     # block index -> size of the smallest loop around it
    for k, (label, ins) in enumerate(bl):
        for i in ins:
            m = re.match(r"s_c?branch\w*\s+(\.LBB\w+)$", i)
            if m and order.get(m.group(1), len(bl)) <= k:
                for b in range(order[m.group(1)], k + 1):
                    span[b] = min(span.get(b, len(bl)), k + 1 - order[m.group(1)])
    best = None
    for b, size in span.items():
        label, ins = bl[b]
        key = (sum(i.startswith("v_mfma") for i in ins), -size)
        if best is None or key > best[0]:
            best = (key, label, ins)
    return None if best is None else (best[0][0], best[1], best[2])


def classify(ins):
    op = ins.split()[0]
    if op.startswith("v_mfma"):
        return "mfma"
    if op.startswith("ds_"):
        return "lds"
    if op.startswith("buffer_load") and ins.rstrip().endswith("lds"):
        return "lds_dma"
    if op.startswith("scratch_") or (op.startswith("buffer_") and "offen" in ins and "s32" in ins):
        return "scratch"
    if op.startswith(("buffer_", "global_", "flat_")):
        return "vmem"
    if op.startswith("v_"):
        return "valu"
    return "scalar"


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    listing = "--list" in sys.argv
    text = open(args[0]).read()
    want = args[1:] or ["sc_attention_split_kernel"]
    for name, lines in kernels(text).items():
        if not all(w in name for w in want):
            continue
        sb = steady_block(lines)
        if sb is None:
            print(f"{name}: no self-loop block")
            continue
        n_mfma, label, ins = sb
        cls = collections.Counter(classify(i) for i in ins)
        ops = collections.Counter(i.split()[0] for i in ins)
        sc = {k: sum(v for o, v in ops.items() if o.startswith(k)) for k in ("s_waitcnt", "s_nop", "s_add")}
        print(f"{name}\n  block {label}: {len(ins)} instructions | v_mfma {n_mfma} | ds_read_b128 {ops.get('ds_read_b128', 0)} | LDS-DMA {cls['lds_dma']} | "
              f"VALU not MFMA {cls['valu']} | s_waitcnt {sc['s_waitcnt']} s_nop {sc['s_nop']} s_add* {sc['s_add']} | other scalar "
              f"{cls['scalar'] - sum(sc.values())} | scratch {cls['scratch']} | other vmem {cls['vmem']}")
        valu = collections.Counter(i.split()[0] for i in ins if classify(i) == "valu")
        print("  " + "  ".join(f"{o} {c}" for o, c in sorted(valu.items(), key=lambda kv: (-kv[1], kv[0]))))
        if listing:
            for i in ins:
                print("      " + i)


if __name__ == "__main__":
    main()
