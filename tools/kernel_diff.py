#!/usr/bin/env python3
"""Do two trees compile to the same GPU code?  No GPU needed.

    python tools/kernel_diff.py PARENT_TREE CHANGE_TREE unit...        (units of unicorn_amd/csrc without the suffix: gemm gemm_h2 norm)

Each unit of each tree is compiled device-only with the flags of unicorn_amd/csrc/build.sh plus -Rpass-analysis=kernel-resource-usage
--save-temps.  Per kernel: the resource remarks and a hash of the normalised listing of its body in the .s file -- comments, .loc / .cfi /
alignment directives dropped; the kernel's own mangled name, the function number in the local labels and the name of the GEMM units' zero
page replaced by placeholders (profiles/mlp_ablation_retired.txt, section 1).  Prints `identical` or the first differing lines per kernel
and exits non-zero on any difference, a kernel on one side only included."""
import hashlib
import os
import re
import shutil
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

FLAGS = "--offload-arch=gfx950 -O3 -std=c++17 -fPIC -munsafe-fp-atomics -Wno-unused-result".split()      # build.sh
EXTRA = "--cuda-device-only -Rpass-analysis=kernel-resource-usage --save-temps".split()
RES = (("VGPRs", "VGPR"), ("AGPRs", "AGPR"), ("TotalSGPRs", "SGPR"), ("ScratchSize [bytes/lane]", "scratch"), ("SGPRs Spill", "sspill"),
       ("VGPRs Spill", "vspill"), ("Occupancy [waves/SIMD]", "occ"), ("LDS Size [bytes/block]", "lds"), ("Dynamic Stack", "dynstack"))
DROP = re.compile(r"^\s*(\.loc|\.cfi_|\.p2align|\.file|\.section|\.text)\b")


def compile_unit(tree, unit, work):
    """-> {mangled kernel name: (resources dict, [listing lines])}"""
    d = os.path.join(work, unit)
    os.makedirs(d)
    src = os.path.join(os.path.abspath(tree), "unicorn_amd", "csrc", unit + ".hip")
    r = subprocess.run(["hipcc"] + FLAGS + EXTRA + ["-c", src, "-o", "unit.o"], cwd=d, capture_output=True, text=True)
    if r.returncode:
        sys.exit("%s: hipcc failed\n%s" % (src, r.stderr[-4000:]))
    res, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"remark:.*?(?:Function Name: (\S+)|\s{3,}([^:]+): (\S+))\s+\[-Rpass", line)
        if not m:
            continue
        if m.group(1):
            cur = res.setdefault(m.group(1), {})
        elif cur is not None:
            cur[m.group(2).strip()] = m.group(3)
    asm = [f for f in os.listdir(d) if f.endswith(".s") and "amdgcn" in f]
    assert len(asm) == 1, asm
    text = open(os.path.join(d, asm[0])).read()
    kernels = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M))
    out = {}
    for m in re.finditer(r"^(\S+):[^\n]*\n(.*?)^\.Lfunc_end\d+:", text, re.M | re.S):
        name = m.group(1)
        if name not in kernels:
            continue
        body = []
        for line in m.group(2).splitlines():
            line = line.split(";")[0].rstrip()
            if not line.strip() or DROP.match(line):
                continue
            line = line.replace(name, "KERNEL")
            line = re.sub(r"\.L(BB|JTI|tmp|func_begin|func_end)\d+", r".L\1", line)
            line = re.sub(r"\b(_ZL\d+)?g_zero_page\w*", "ZERO_PAGE", line)
            body.append(line)
        out[name] = ({short: res.get(name, {}).get(long, "?") for long, short in RES}, body)
    assert kernels == set(out), sorted(kernels - set(out))
    return out


def demangle(names):
    filt = shutil.which("c++filt") or shutil.which("llvm-cxxfilt")
    if not names or not filt:
        return {n: n for n in names}
    r = subprocess.run([filt] + names, capture_output=True, text=True)
    plain = r.stdout.splitlines() if r.returncode == 0 else names
    return {n: re.sub(r"^void |\(GemmArgs\)$", "", p) for n, p in zip(names, plain)}


def main():
    if len(sys.argv) < 4:
        sys.exit(__doc__)
    parent, change, units = sys.argv[1], sys.argv[2], sys.argv[3:]
    differ = 0
    with tempfile.TemporaryDirectory() as work, ThreadPoolExecutor(max(1, min(8, (os.cpu_count() or 2) // 2))) as pool:
        jobs = {(side, u): pool.submit(compile_unit, tree, u, os.path.join(work, side)) for u in units for side, tree in (("parent", parent), ("change", change))}
        for u in units:
            P, C = jobs["parent", u].result(), jobs["change", u].result()
            nice = demangle(sorted(set(P) | set(C)))
            only_p, only_c = sorted(set(P) - set(C)), sorted(set(C) - set(P))
            print("-- %s.hip: kernels parent %d, change %d; only in the parent: %d, only in the change: %d" % (u, len(P), len(C), len(only_p), len(only_c)))
            for n in only_p:
                print("  only in the parent: " + nice[n])
            for n in only_c:
                print("  only in the change: " + nice[n])
            print("%-64s %s instrs  vs parent" % ("kernel", " ".join(short for _, short in RES)))
            bad = len(only_p) + len(only_c)
            for n in sorted(set(P) & set(C), key=lambda k: nice[k]):
                (rp, bp), (rc, bc) = P[n], C[n]
                sha = hashlib.sha256("\n".join(bc).encode()).hexdigest()[:12]
                line = "%-64s %s %6d  " % (nice[n], " ".join("%*s" % (len(short), rc[short]) for _, short in RES), len(bc))
                if rp == rc and bp == bc:
                    print(line + "identical (resources + listing, sha %s)" % sha)
                    continue
                bad += 1
                what = ["%s %s -> %s" % (k, rp[k], rc[k]) for k in rp if rp[k] != rc[k]]
                print(line + "DIFFERS: " + (", ".join(what) if what else "resources identical") + "; listing %d -> %d instructions" % (len(bp), len(bc)))
                first = next((i for i, (a, b) in enumerate(zip(bp, bc)) if a != b), min(len(bp), len(bc)))
                for i in range(first, min(first + 6, max(len(bp), len(bc)))):
                    print("    line %d: parent %-56s | change %s" % (i + 1, bp[i].strip() if i < len(bp) else "-", bc[i].strip() if i < len(bc) else "-"))
            print("kernels of %s.hip that differ: %d" % (u, bad))
            differ += bad
    print("identical" if not differ else "DIFFERENT: %d kernels" % differ)
    sys.exit(1 if differ else 0)


if __name__ == "__main__":
    main()
