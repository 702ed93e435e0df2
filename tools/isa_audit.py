#!/usr/bin/env python3
"""Instruction audit of one kernel in a gfx950 assembly listing (hipcc -save-temps of a unit):
per basic block the count of MFMA (f64 / other), VALU (f64 / other), DS, VMEM and SALU
instructions, every s_waitcnt, the barriers, and what sits between consecutive MFMAs (the
histogram of gap contents).  Blocks are listed in program order with their branch targets, so
the producer's and the consumer's tile loops can be read off (the blocks holding the MFMAs /
the buffer loads that branch back).

  tools/isa_audit.py LISTING.s KERNEL_SUBSTRING [--gaps] > isa_audit.md
"""
from __future__ import annotations

import collections
import re
import sys


def kind(op: str) -> str:
    if op.startswith("v_mfma"):
        return "mfma_f64" if "f64" in op else "mfma_other"
    if op.startswith("v_"):
        return "valu_f64" if op.endswith("_f64") or "_f64_" in op else "valu_other"
    if op.startswith("ds_"):
        return "ds"
    if op.startswith(("buffer_", "global_", "flat_", "scratch_")):
        return "vmem"
    if op == "s_waitcnt":
        return "waitcnt"
    if op == "s_barrier":
        return "barrier"
    if op.startswith(("s_cbranch", "s_branch")):
        return "branch"
    if op.startswith("s_"):
        return "salu"
    return "other"


KINDS = ["mfma_f64", "mfma_other", "valu_f64", "valu_other", "ds", "vmem", "salu", "waitcnt",
         "barrier", "branch"]


def main():
    path, name = sys.argv[1], sys.argv[2]
    gaps = "--gaps" in sys.argv
    lines = open(path).read().split("\n")
    start = next(i for i, l in enumerate(lines) if re.match(r"^_Z\w*:", l) and name in l)
    end = next(i for i in range(start, len(lines)) if lines[i].strip().startswith("s_endpgm"))
    # the metadata of the kernel (registers, scratch, LDS)
    meta = {}
    for l in lines[end:]:
        m = re.match(r"\s*\.amdhsa_(next_free_vgpr|next_free_sgpr|accum_offset|"
                     r"private_segment_fixed_size|group_segment_fixed_size)\s+(\d+)", l)
        if m:
            meta.setdefault(m.group(1), m.group(2))
        if l.strip().startswith(".end_amdhsa_kernel"):
            break
    print(f"# {lines[start].rstrip(':')}\n")
    print("kernel descriptor: " + ", ".join(f"{k} {v}" for k, v in meta.items()) + "\n")
    blocks, cur = [], None
    for l in lines[start + 1:end + 1]:
        s = l.split(";")[0].strip()
        if not s or s.startswith("."):
            if re.match(r"^\.LBB\d+_\d+:", s):
                cur = dict(label=s.rstrip(":"), ops=[])
                blocks.append(cur)
            continue
        if cur is None:
            cur = dict(label="entry", ops=[])
            blocks.append(cur)
        parts = s.split(None, 1)
        cur["ops"].append((parts[0], parts[1] if len(parts) > 1 else ""))
    print("| block | " + " | ".join(KINDS) + " | branches to | s_waitcnt operands |")
    print("|---|" + "---|" * (len(KINDS) + 2))
    for b in blocks:
        c = collections.Counter(kind(op) for op, _ in b["ops"])
        if not b["ops"]:
            continue
        tg = [a for op, a in b["ops"] if kind(op) == "branch"]
        wc = collections.Counter(a for op, a in b["ops"] if op == "s_waitcnt")
        print(f"| {b['label']} | " + " | ".join(str(c.get(k, 0)) for k in KINDS) + " | "
              + " ".join(tg) + " | " + "; ".join(f"{k} ×{v}" for k, v in wc.items()) + " |")
    if gaps:
        print("\n## Between consecutive MFMAs (blocks holding MFMAs)\n")
        for b in blocks:
            ks = [kind(op) for op, _ in b["ops"]]
            if not any(k.startswith("mfma") for k in ks):
                continue
            hist, gap, seq = collections.Counter(), [], []
            seen = False
            for k in ks:
                if k.startswith("mfma"):
                    if seen:
                        g = collections.Counter(gap)
                        key = " ".join(f"{n}{v}" for n, v in sorted(g.items())) or "-"
                        hist[key] += 1
                        seq.append(key)
                    seen, gap = True, []
                else:
                    gap.append(k)
            print(f"### {b['label']}: {sum(k.startswith('mfma') for k in ks)} MFMAs\n")
            for k, v in hist.most_common():
                print(f"- {v} × [{k}]")
            print("\nin order: " + " | ".join(seq) + "\n")


if __name__ == "__main__":
    main()
