#!/usr/bin/env python3
"""Do two trees compile to the same GPU code?  No GPU needed.

    python tools/kernel_diff.py PARENT_TREE CHANGE_TREE unit...        (units of unicorn_amd/csrc without the suffix: gemm gemm_h2 norm)

Each unit of each tree is compiled device-only with the flags of unicorn_amd/csrc/build.sh plus -Rpass-analysis=kernel-resource-usage
--save-temps.  Per kernel: the resource remarks and a hash of the normalised listing of its body in the .s file -- comments, .loc / .cfi /
alignment directives dropped; the kernel's own mangled name, the function number in the local labels and the name of the GEMM units' zero
page replaced by placeholders (profiles/mlp_ablation_retired.txt, section 1).  Prints `identical` or the first differing lines per kernel
and exits non-zero on any difference, a kernel on one side only included.

    --pair OLD=NEW    (repeatable) the parent's kernel template OLD is the change's NEW, whose template arguments begin with OLD's: the
                      listings cannot be compared, so each pair is held to its resources -- no scratch or spill where the parent has none,
                      occupancy not below the parent's, VGPR + AGPR not above the parent's at equal occupancy.

Kernel names are printed demangled, every unit's: _Float16 and __bf16 template arguments read f16 and bf16 (an older c++filt does not know
their codes, so two builtin types stand in for them on the way through it)."""
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
    # an older c++filt gives up on _Float16 (DF16_) and __bf16 (DF16b): two builtin types it knows stand in for them
    r = subprocess.run([filt] + [n.replace("DF16_", "Dh").replace("DF16b", "Ds") for n in names], capture_output=True, text=True)
    plain = [re.sub(r"\bchar16_t\b", "bf16", re.sub(r"\bhalf\b", "f16", p)) for p in r.stdout.splitlines()] if r.returncode == 0 else names
    return {n: re.sub(r"^void |\(GemmArgs\)$", "", p) for n, p in zip(names, plain)}


def pair_renamed(old, new, P, C, nice):
    """the table of --pair OLD=NEW: a parent kernel OLD<a, b, ...> against the change's NEW<a, b, ..., more> -> the number of pairs that break
    a condition, a kernel without a partner included"""
    def by_args(side, name):
        out = {}
        for n in side:
            m = re.match(r"%s<(.*)>\(" % re.escape(name), nice[n])
            if m:
                out[tuple(a.strip() for a in m.group(1).split(","))] = n
        return out
    olds, news = by_args(P, old), by_args(C, new)
    width = max((len(a) for a in olds), default=0)
    news = {a[:width]: n for a, n in news.items()}
    bad = 0
    print("%-30s %-34s %-34s" % ("%s -> %s" % (old, new), "parent VGPR AGPR SGPR scratch occ", "change VGPR AGPR SGPR scratch occ"))
    for a in sorted(set(olds) | set(news)):
        if a not in olds or a not in news:
            bad += 1
            print("%-30s %s" % ("<%s>" % ",".join(a), "only in the parent" if a in olds else "only in the change"))
            continue
        rp, rc = P[olds[a]][0], C[news[a]][0]
        regs = lambda r: int(r["VGPR"]) + int(r["AGPR"])                                                                  # noqa: E731
        spill = lambda r: (r["scratch"], r["sspill"], r["vspill"], r["dynstack"])                                          # noqa: E731
        why = []
        if spill(rp) == ("0", "0", "0", "False") and spill(rc) != spill(rp):
            why.append("scratch or spills")
        if int(rc["occ"]) < int(rp["occ"]):
            why.append("occupancy")
        if int(rc["occ"]) == int(rp["occ"]) and regs(rc) > regs(rp):
            why.append("registers")
        bad += bool(why)
        row = lambda r: "%11s %4s %4s %7s %3s" % (r["VGPR"], r["AGPR"], r["SGPR"], r["scratch"], r["occ"])                 # noqa: E731
        print("%-30s %-34s %-34s %s" % ("<%s>" % ",".join(a), row(rp), row(rc), "WORSE: " + ", ".join(why) if why else "ok"))
    print("pairs of %s -> %s that break a condition: %d of %d" % (old, new, bad, len(set(olds) | set(news))))
    return bad


def main():
    pairs = []
    while "--pair" in sys.argv:
        i = sys.argv.index("--pair")
        pair = sys.argv[i + 1].split("=") if i + 1 < len(sys.argv) else []
        if len(pair) != 2 or not all(pair):
            sys.exit(__doc__)
        pairs.append(pair)
        del sys.argv[i:i + 2]
    if len(sys.argv) < 4:
        sys.exit(__doc__)
    parent, change, units = sys.argv[1], sys.argv[2], sys.argv[3:]
    differ = 0
    with tempfile.TemporaryDirectory() as work, ThreadPoolExecutor(max(1, min(8, (os.cpu_count() or 2) // 2))) as pool:
        jobs = {(side, u): pool.submit(compile_unit, tree, u, os.path.join(work, side)) for u in units for side, tree in (("parent", parent), ("change", change))}
        for u in units:
            P, C = jobs["parent", u].result(), jobs["change", u].result()
            nice = demangle(sorted(set(P) | set(C)))
            renamed = lambda n, side: any(nice[n].startswith(pr[side] + "<") for pr in pairs)                              # noqa: E731
            only_p = sorted(n for n in set(P) - set(C) if not renamed(n, 0))
            only_c = sorted(n for n in set(C) - set(P) if not renamed(n, 1))
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
            for old, new in pairs:
                if any(nice[n].startswith(old + "<") for n in P):
                    bad += pair_renamed(old, new, P, C, nice)
            print("kernels of %s.hip that differ: %d" % (u, bad))
            differ += bad
    print("identical" if not differ else "DIFFERENT: %d kernels" % differ)
    sys.exit(1 if differ else 0)


if __name__ == "__main__":
    main()
