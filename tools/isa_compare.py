"""Kernel-by-kernel comparison of two ISA listings of the library (make asm: csrc/lbm_hip-gfx950.s): which kernels exist
in one only, and whether every kernel of the first has the same descriptor (.amdhsa_kernel block) and the same
instructions in the second.  Local labels and the basic-block numbers in the assembler's comments carry the function's
ordinal in the file, which moves when kernels are added before it: they are compared without their numbers, and runs of
blanks as one.
python tools/isa_compare.py <parent .s> <this .s> [show]      show: the first lines that differ in the first differing kernel"""
import re, sys, hashlib
def parse(path):
    text = open(path).read()
    kernels = re.findall(r"^\s*\.amdhsa_kernel (\S+)\n(.*?)^\s*\.end_amdhsa_kernel", text, flags=re.S | re.M)
    desc = {k: v for k, v in kernels}
    body = {}
    for k in desc:
        m = re.search(r"^%s:.*?\n(.*?)^\.Lfunc_end\d+:" % re.escape(k), text, flags=re.S | re.M)
        b = m.group(1)
        b = re.sub(r"BB\d+_", "BB_", b)
        b = re.sub(r"\.Ltmp\d+", ".Ltmp", b)
        b = re.sub(r"\.Lfunc_(begin|end)\d+", r".Lfunc_\1", b)
        b = re.sub(r"\.L__unnamed_\d+", ".L__unnamed", b)
        body[k] = re.sub(r"[ \t]+", " ", b)
    return text, desc, body
pa, th = sys.argv[1], sys.argv[2]
t0, d0, b0 = parse(pa)
t1, d1, b1 = parse(th)
print("lines:   parent %d, this %d" % (t0.count("\n"), t1.count("\n")))
print(".amdhsa_kernel symbols: parent %d, this %d" % (len(d0), len(d1)))
print("only in parent:", sorted(set(d0) - set(d1)))
print("only in this:")
for k in sorted(set(d1) - set(d0)):
    print("   ", k)
same = [k for k in d0 if k in d1 and d0[k] == d1[k] and b0[k] == b1[k]]
diff = [k for k in d0 if k in d1 and k not in same]
print("pre-existing kernels with identical instructions and descriptors: %d/%d" % (len(same), len(d0)))
print("different: %d %s" % (len(diff), diff))
h = hashlib.sha256("".join(k + d0[k] + b0[k] for k in sorted(d0)).encode()).hexdigest()
h1 = hashlib.sha256("".join(k + d1[k] + b1[k] for k in sorted(d0) if k in d1).encode()).hexdigest()
print("sha256 over the pre-existing kernels' descriptors and bodies (local labels unnumbered):\n  parent %s\n  this   %s" % (h, h1))
if diff and len(sys.argv) > 3:
    import difflib
    k = diff[0]
    for name, a, b in (("desc", d0[k], d1[k]), ("body", b0[k], b1[k])):
        dl = [l for l in difflib.unified_diff(a.splitlines(), b.splitlines(), lineterm="", n=0)][:14]
        print(name, len(dl)); print("\n".join(dl))
