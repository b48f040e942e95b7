"""Per-kernel comparison of two device assembly files of one translation unit (dev tool for refactors that must not move code generation):
   hipcc <the Makefile's FLAGS> -S --cuda-device-only csrc/<unit>.hip -o new.s      (and the same from the parent commit -> old.s)
   python tools/asm_compare.py old.s new.s
A kernel is IDENTICAL when its instruction text matches line for line after dropping comments, .file / .ident / .loc / .p2align noise and the
per-build __hip_cuid symbol.  For each kernel that differs: old -> new of SGPRs, VGPRs, AGPRs, LDS, scratch bytes, spills (from the .amdhsa
metadata) and the instruction count.  Exit status 1 if a kernel gained scratch, a spill or VGPRs, or if the two files hold different kernels."""
import re, sys

KEYS = ("sgpr_count", "vgpr_count", "agpr_count", "group_segment_fixed_size", "private_segment_fixed_size", "sgpr_spill_count", "vgpr_spill_count")


def kernels(path):
    src = open(path).read()
    meta = {}
    for blk in re.split(r"^  - \.agpr_count:", src, flags=re.M)[1:]:
        blk = "    .agpr_count:" + blk
        name = re.search(r"^\s+\.name:\s+(\S+)", blk, flags=re.M).group(1)
        meta[name] = {k: int(re.search(r"^\s+\.%s:\s+(\d+)" % k, blk, flags=re.M).group(1)) for k in KEYS}
    body = {}
    parts = re.split(r"^(_Z\w+):.*$", src, flags=re.M)
    for name, text in zip(parts[1::2], parts[2::2]):
        if name not in meta:
            continue
        lines = []
        for l in text.split(".Lfunc_end")[0].split("\n"):
            t = l.split(";")[0].strip()
            if not t or t.startswith(("//", ".file", ".ident", ".loc", ".p2align")) or "__hip_cuid" in t:
                continue
            lines.append(t)
        body[name] = lines
    return meta, body


def main():
    om, ob = kernels(sys.argv[1])
    nm, nb = kernels(sys.argv[2])
    bad = set(om) != set(nm)
    for n in sorted(set(om) ^ set(nm)):
        print("ONLY IN", "old" if n in om else "new", n)
    same = [n for n in om if n in nm and ob[n] == nb[n] and om[n] == nm[n]]
    print("%d kernels, %d identical" % (len(om), len(same)))
    for n in sorted(om):
        if n in same or n not in nm:
            continue
        ins = lambda b: sum(not (t.endswith(":") or t.startswith(".")) for t in b)
        print(n)
        print("   " + "  ".join("%s %d -> %d" % (k.replace("_count", "").replace("_fixed_size", ""), om[n][k], nm[n][k]) for k in KEYS) + "  instructions %d -> %d" % (ins(ob[n]), ins(nb[n])))
        if any(nm[n][k] > om[n][k] for k in ("vgpr_count", "private_segment_fixed_size", "sgpr_spill_count", "vgpr_spill_count")):
            print("   REGRESSION")
            bad = True
    sys.exit(1 if bad else 0)


main()
