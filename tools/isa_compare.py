#!/usr/bin/env python3
"""Development tool: two ISA listings of csrc/ntt.hip side by side (hipcc -O3 --offload-arch=gfx950 --cuda-device-only -S), per
kernel: static instruction counts (every instruction of the listing once: setup, loop bodies, prefetch blocks) and the
resources of the code object's metadata.  Every kernel that gained a spill or scratch, or lost a workgroup per CU, is listed at the end.

    python3 tools/isa_compare.py parent.s this.s ['ntt_pass' [more name filters]]
"""
import re
import sys
from collections import Counter

ADDR = ("v_add_lshl_u32", "v_lshl_add_u32", "v_lshlrev_b32", "v_lshl_or_b32", "v_lshl_add_u64", "v_lshlrev_b64")
META = (".max_flat_workgroup_size", ".vgpr_count", ".agpr_count", ".sgpr_count", ".vgpr_spill_count", ".sgpr_spill_count", ".private_segment_fixed_size",
        ".group_segment_fixed_size")


def demangle_short(name):
    """ntt_pass_cols_kernelILi8ELi5ELi1ELi8ELb1EE -> ntt_pass_cols_kernel<8,5,1,8,1>"""
    m = re.match(r"_Z\d+(\w+?)I((?:L[ib]\d+E)+)Ev", name)
    if not m:
        return name
    return "%s<%s>" % (m.group(1), ",".join(re.findall(r"L[ib](\d+)E", m.group(2))))


def kernels(path):
    text = open(path).read()
    out = {}
    for m in re.finditer(r"^(_Z\w+):[^\n]*\n(.*?)s_endpgm", text, flags=re.S | re.M):
        ops = Counter()
        for l in m.group(2).splitlines():
            mm = re.match(r"\s+((?:v|s|ds|global|buffer|scratch)_\w+)", l)
            if mm:
                ops[re.sub(r"_e32$|_e64$|_sdwa$|_dpp$", "", mm.group(1))] += 1
        out[m.group(1)] = {"ops": ops}
    for m in re.finditer(r"^  - (?:\.\w+:.*\n    )*?\.name:\s+(\w+)\n((?:    .*\n)*)", text, flags=re.M):
        pass
    # metadata: blocks of "    .key: value" lines between "  - .agpr_count" style list heads; keyed by .name
    for block in re.split(r"^  - ", text[text.find("amdhsa.kernels:"):], flags=re.M)[1:]:
        name = re.search(r"\.name:\s+(\w+)", block)
        if name and name.group(1) in out:
            for k in META:
                v = re.search(r"^\s*" + re.escape(k) + r":\s+(\d+)", block, flags=re.M)
                out[name.group(1)][k] = int(v.group(1)) if v else 0
    return out


def wgs_per_cu(k):
    """workgroups a CU holds: 512 VGPRs per SIMD lane in blocks of 8, at most 8 waves per SIMD, 160 KiB of LDS"""
    waves = max(1, k.get(".max_flat_workgroup_size", 64) // 64)
    per_simd = (waves + 3) // 4
    by_vgpr = min(8, 512 // (8 * ((max(k.get(".vgpr_count", 1), 1) + 7) // 8))) // per_simd
    lds = k.get(".group_segment_fixed_size", 0)
    return min(by_vgpr, (160 * 1024) // lds if lds else 32)


def row(k):
    o = k["ops"]
    valu = sum(v for n, v in o.items() if n.startswith("v_"))
    addr = sum(o[n] for n in ADDR)
    salu = sum(v for n, v in o.items() if re.match(r"s_(add|addc|lshl|lshl\d_add)_", n))
    mul = sum(v for n, v in o.items() if n.startswith("v_mul_") or n.startswith("v_mad_"))
    return valu, mul, addr, salu, k.get(".vgpr_count", 0), k.get(".sgpr_count", 0), k.get(".vgpr_spill_count", 0) + k.get(".sgpr_spill_count", 0), \
        k.get(".private_segment_fixed_size", 0), wgs_per_cu(k)


def main():
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    pats = sys.argv[3:] or ["ntt_pass"]
    print("%-44s %s" % ("kernel", "VALU  mul  vaddr  salu  VGPR SGPR spill scratch WGs/CU   (parent -> this)"))
    worse = []
    for name in sorted(a):
        if name not in b:
            continue
        ra, rb = row(a[name]), row(b[name])
        if rb[6] > ra[6] or rb[7] > ra[7] or rb[8] < ra[8]:
            worse.append((demangle_short(name), (ra[4],) + ra[6:], (rb[4],) + rb[6:]))
        if not any(p in name for p in pats):
            continue
        print("%-44s %s" % (demangle_short(name), "  ".join("%d->%d" % (x, y) for x, y in zip(ra, rb))))
    print("kernels with more spills, more scratch or fewer workgroups per CU (VGPR, spills, scratch, WGs/CU):")
    for w in worse:
        print("  %-44s %s -> %s" % w)
    if not worse:
        print("  none")


if __name__ == "__main__":
    main()
