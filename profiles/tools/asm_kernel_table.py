#!/usr/bin/env python3
"""Per-kernel table of two device-assembly dumps (NS_ASM_DIR=<dir> nspeech_amd/csrc/build.sh): for every kernel the
instruction count, VGPRs, SGPRs, scratch and static LDS bytes of both, and whether the whole body is byte-identical.
Compares whole bodies and counts only.

    asm_kernel_table.py <parent dir> <change dir> [touched.s ...]

Exit status 1 when a kernel of a file that is not listed as touched differs, or when a kernel of the change needs more scratch
or more VGPRs than in the parent."""
import hashlib
import os
import re
import sys

FIELDS = (("vgpr", ".amdhsa_next_free_vgpr"), ("sgpr", ".amdhsa_next_free_sgpr"),
          ("scratch", ".amdhsa_private_segment_fixed_size"), ("lds", ".amdhsa_group_segment_fixed_size"))


def kernels(path):
    lines = open(path).read().split("\n")
    start = {m.group(1): i for i, l in enumerate(lines) for m in [re.match(r"^(\w+):", l)] if m}
    out = {}
    for i, l in enumerate(lines):
        m = re.match(r"\s*\.amdhsa_kernel (\w+)", l)
        if not m:
            continue
        name = m.group(1)
        rec = {}
        for l2 in lines[i:]:
            if ".end_amdhsa_kernel" in l2:
                break
            for key, word in FIELDS:
                m2 = re.match(r"\s*%s (\d+)" % re.escape(word), l2)
                if m2:
                    rec[key] = int(m2.group(1))
        if name not in start:
            sys.exit("%s: no label line for kernel %s" % (path, name))
        body = []
        for l2 in lines[start[name] + 1:]:
            if l2.startswith(".Lfunc_end"):
                break
            body.append(l2)
        rec["insts"] = sum(1 for b in body if re.match(r"\t[a-z]\w+", b))
        rec["hash"] = hashlib.sha1("\n".join(body).encode()).hexdigest()
        out[name] = rec
    return out


def main():
    parent, change, touched = sys.argv[1], sys.argv[2], set(sys.argv[3:])
    bad = 0
    print("%-12s %-7s %15s %11s %11s %9s %13s  kernel" % ("file", "body", "insts", "vgpr", "sgpr", "scratch", "lds"))
    for f in sorted(os.listdir(change)):
        if not f.endswith(".s"):
            continue
        a, b = kernels(os.path.join(parent, f)), kernels(os.path.join(change, f))
        same = sum(1 for k in b if k in a and a[k]["hash"] == b[k]["hash"])
        for k in sorted(set(a) | set(b)):
            x, y = a.get(k), b.get(k)
            if x is None or y is None:
                print("%-12s %s only in the %s" % (f, k, "change" if x is None else "parent"))
                bad |= f not in touched
                continue
            ident = x["hash"] == y["hash"]
            stray = not ident and f not in touched
            more_scratch, more_vgprs = y["scratch"] > x["scratch"], y["vgpr"] > x["vgpr"]
            bad |= stray or more_scratch or more_vgprs
            flags = " UNTOUCHED-DIFFERS" * stray + " MORE-SCRATCH" * more_scratch + " MORE-VGPRS" * more_vgprs
            if y["scratch"] and not more_scratch:
                flags += " (scratch as in the parent)"
            if ident and not flags:
                continue
            print("%-12s %-7s %7d %7d %5d %5d %5d %5d %4d %4d %6d %6d  %s%s" % (
                f, "same" if ident else "differs", x["insts"], y["insts"], x["vgpr"], y["vgpr"], x["sgpr"], y["sgpr"],
                x["scratch"], y["scratch"], x["lds"], y["lds"], k, flags))
        print("%-12s %d of %d kernels byte-identical to the parent" % (f, same, len(b)))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
