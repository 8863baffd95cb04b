#!/usr/bin/env python3
"""Compare the device code of two builds, kernel by kernel.  No GPU.

    hipcc --offload-arch=gfx950 -O3 -std=c++17 --cuda-device-only -S bonsai_amd/csrc/bns_api.hip -o parent.s    (parent commit)
    hipcc ... -o change.s                                                                                       (working tree)
    tools/codegen_diff.py parent.s change.s > profiles/<tag>_codegen.txt

Per kernel: VGPRs, SGPRs, spilled SGPRs / VGPRs, scratch bytes and LDS bytes from the `amdhsa.kernels` metadata, the static
instruction count, and whether the multiset of instruction mnemonics is the same.  Only kernels that differ are listed; the
last line counts them.  Exit status 1 when a kernel's resources grew (VGPRs, spills, scratch) or its LDS bytes changed.
"""
import collections
import re
import sys

FIELDS = (("vgpr", ".vgpr_count"), ("sgpr", ".sgpr_count"), ("sspill", ".sgpr_spill_count"), ("vspill", ".vgpr_spill_count"),
          ("scratch", ".private_segment_fixed_size"), ("lds", ".group_segment_fixed_size"))


def parse(path):
    """-> {kernel: (resources dict, instruction count, Counter of mnemonics)}"""
    text = open(path).read().splitlines()
    meta, cur = {}, None
    start = next(i for i, l in enumerate(text) if l.startswith("amdhsa.kernels:"))
    for l in text[start + 1:]:
        if l.startswith("  - "):                         # a new kernel's record
            cur = {}
        m = re.match(r"[ -]{4}(\.\w+):\s+(\S+)$", l)
        if m and cur is not None:
            cur[m.group(1)] = m.group(2)
            if m.group(1) == ".name":
                meta[m.group(2)] = cur
        if l.startswith("amdhsa.target"):
            break
    code, name = {}, None
    for l in text[:start]:
        m = re.match(r"(\w+):", l)
        if m and m.group(1) in meta:
            name = m.group(1)
            code[name] = collections.Counter()
        elif l.startswith(".Lfunc_end"):
            name = None
        elif name and re.match(r"\s+[a-z]\w*(\s|$)", l):
            code[name][l.split()[0]] += 1
    out = {}
    for k, rec in meta.items():
        mn = code.get(k, collections.Counter())
        out[k] = ({f: int(rec.get(key, 0)) for f, key in FIELDS}, sum(mn.values()), mn)
    return out


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    a, b = parse(sys.argv[1]), parse(sys.argv[2])
    n_diff, worse = 0, 0
    for k in sorted(set(a) | set(b)):
        if k not in a or k not in b:
            print(f"{k}\n    only in {'parent' if k in a else 'change'}")
            n_diff += 1
            worse += 1
            continue
        (ra, na, ma), (rb, nb, mb) = a[k], b[k]
        if ra == rb and ma == mb:
            continue
        n_diff += 1
        res = "  ".join(f"{f} {ra[f]}" + (f" -> {rb[f]}" if ra[f] != rb[f] else "") for f, _ in FIELDS)
        delta = {m: mb[m] - ma[m] for m in set(ma) | set(mb) if ma[m] != mb[m]}
        mix = "mnemonics equal" if not delta else "mnemonics differ: " + " ".join(f"{m}{d:+d}" for m, d in sorted(delta.items()))
        print(f"{k}\n    {res}\n    instructions {na}" + (f" -> {nb}" if na != nb else "") + f"  {mix}")
        if any(rb[f] > ra[f] for f in ("vgpr", "sspill", "vspill", "scratch")) or ra["lds"] != rb["lds"]:
            worse += 1
    n_order = sum(1 for k in a if k in b and a[k][0] == b[k][0] and a[k][2] == b[k][2])
    print(f"{n_diff} of {len(set(a) | set(b))} kernels differ in resources or instruction mix ({n_order} equal); "
          f"{worse} with more VGPRs, spills or scratch, or other LDS bytes")
    sys.exit(1 if worse else 0)


if __name__ == "__main__":
    main()
