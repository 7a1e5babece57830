#!/usr/bin/env python3
"""Static issue-cost model of the GEMM epilogues.  No GPU needed.

    python tools/epi_cost.py [--tree DIR] [--unit gemm_h2q] [--kernel gemm_h2q_kernel] [--fmt 2] [--blocks N]

Compiles unicorn_amd/csrc/<unit>.hip of the tree (default: the one this file is in) to assembly with the flags of csrc/build.sh plus
--cuda-device-only -S, and splits the listing of every instantiation of <kernel> (--fmt N: only those whose last template argument is N)
into three regions.  The split follows the compiler's own loop annotations of the basic blocks (`in Loop: Header=BB0_19 Depth=2`), not the
order of the listing: hipcc is free to place a block of the epilogue in front of the K loop.

    outside    the code before and behind the loop over the block's tiles
    K loop     the innermost loop that holds the MFMAs
    tile       the rest of the tile loop, i.e. what runs behind the last MFMA of a tile: the epilogue, the statistics, the hand-over
               to the block's next tile

Per region: instruction counts by class and the vector-issue cycles of one wave, 4 x plain VALU + 8 x transcendental (the measured
per-instruction issue costs on the MI355X; lane reads / writes are VALU instructions and counted at 4 in a column of their own).  The count
is STATIC: a block that a launch never enters (an ablation switch, the path of a launch mode, the other side of a tile-uniform branch)
is counted like one that runs for every tile, so the figure bounds the executed cost from above; --blocks N lists the basic blocks of the
tile region that hold at least N instructions, largest first, to tell the two apart.  The K loop's normalised listing is
hashed twice (comments and directives dropped, local label numbers replaced; the second hash also replaces the register numbers): a
change to the epilogue that leaves the first hash alone has not touched the loop body, one that leaves only the second alone has
renumbered its registers and changed no instruction.  Registers, scratch, static LDS and occupancy are the compiler's own figures from the same file.

Mnemonics are classified by prefix only; nothing is assumed about operands."""
import argparse
import hashlib
import os
import re
import subprocess
import sys
import tempfile

FLAGS = "--offload-arch=gfx950 -O3 -std=c++17 -fPIC -munsafe-fp-atomics -Wno-unused-result".split()      # csrc/build.sh
TRANS = ("v_exp_", "v_log_", "v_rcp_", "v_rsq_", "v_sqrt_", "v_sin_", "v_cos_")
LANE = ("v_readlane", "v_writelane", "v_readfirstlane", "v_permlane", "v_mov_b32_dpp", "ds_bpermute", "ds_permute", "ds_swizzle")
VMEM = ("global_", "buffer_", "flat_", "scratch_")
CLASSES = ("valu", "trans", "lane", "mfma", "lds", "vmem", "salu", "smem", "branch", "wait", "other")
INFO = (("NumVgprs", "VGPR"), ("NumAgprs", "AGPR"), ("TotalNumSgprs", "SGPR"), ("ScratchSize", "scratch"), ("LDSByteSize", "LDS(static)"),
        ("Occupancy", "occ"))


def classify(mn):
    if mn.startswith(("v_mfma", "v_smfmac")):
        return "mfma"
    if mn.startswith(LANE):
        return "lane"
    if mn.startswith(TRANS):
        return "trans"
    if mn.startswith("v_"):
        return "valu"
    if mn.startswith("ds_"):
        return "lds"
    if mn.startswith(VMEM):
        return "vmem"
    if mn.startswith(("s_load", "s_buffer_load")):
        return "smem"
    if mn.startswith(("s_cbranch", "s_branch", "s_endpgm", "s_trap", "s_setpc", "s_swappc")):
        return "branch"
    if mn.startswith(("s_waitcnt", "s_barrier", "s_nop", "s_sleep")):
        return "wait"
    if mn.startswith("s_"):
        return "salu"
    return "other"


def compile_asm(tree, unit, work):
    src = os.path.join(os.path.abspath(tree), "unicorn_amd", "csrc", unit + ".hip")
    out = os.path.join(work, unit + ".s")
    r = subprocess.run(["hipcc"] + FLAGS + ["--cuda-device-only", "-S", src, "-o", out], capture_output=True, text=True)
    if r.returncode:
        sys.exit("%s: hipcc failed\n%s" % (src, r.stderr[-4000:]))
    return open(out).read()


BLOCK = re.compile(r"^(?:(\.LBB\d+_\d+):|; %bb\.(\d+):)")


def kernels_of(text, kernel):
    """-> [(mangled name, blocks, {info})] of the instantiations of `kernel`, in file order; a block is (label, loop id or None, depth,
    [instructions]) with the loop the compiler's own annotation names (`in Loop: Header=BB0_19 Depth=2`, `This Inner Loop Header`)"""
    names = [n for n in re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M) if kernel in n]
    out = []
    for name in names:
        m = re.search(r"^%s:[^\n]*\n(.*?)^\.Lfunc_end\d+:(.*?); -- End function(.*?)(?=^\s*\.text|^\s*\.section\s+\.text|\Z)"
                      % re.escape(name), text, re.M | re.S)
        assert m, name
        blocks, note = [["(entry)", None, 0, []]], ""
        for raw in m.group(1).splitlines():
            b = BLOCK.match(raw)
            code = raw.split(";")[0].strip()
            if b:
                blocks.append([b.group(1) or "%bb." + b.group(2), None, 0, []])
                note = raw
            elif not code and not blocks[-1][3]:
                note += raw                      # the annotation of a loop header runs over several comment lines
            elif code and not code.startswith("."):
                blocks[-1][3].append(code)
            if b or (not code and not blocks[-1][3]):
                own = re.search(r"This (?:Inner )?Loop Header: Depth=(\d+)", note)
                mem = re.search(r"in Loop: Header=(\S+) Depth=(\d+)", note)
                if own:
                    blocks[-1][1], blocks[-1][2] = blocks[-1][0].replace(".L", ""), int(own.group(1))
                elif mem:
                    blocks[-1][1], blocks[-1][2] = mem.group(1), int(mem.group(2))
        info = {}
        for key, short in INFO:
            mm = re.search(r"^; %s: (\d+)" % re.escape(key), m.group(3), re.M)
            info[short] = mm.group(1) if mm else "?"
        out.append((name, blocks, info))
    return out


def regions(blocks):
    """-> {"outside": [...], "K loop": [...], "tile": [...]}: lists of blocks.  The K loop is the innermost loop that holds the MFMAs;
    `tile` is the rest of the loop over the block's tiles (epilogue, statistics, hand-over to the next tile); `outside` is the code before
    and behind that loop."""
    mf = {}
    for lab, loop, depth, ins in blocks:
        n = sum(1 for i in ins if classify(i.split()[0]) == "mfma")
        if n and loop:
            mf[(loop, depth)] = mf.get((loop, depth), 0) + n
    if not mf:
        return None
    kid = max(mf, key=lambda k: (k[1], mf[k]))[0]
    reg = {"outside": [], "K loop": [], "tile": []}
    for b in blocks:
        reg["K loop" if b[1] == kid else "tile" if b[2] >= 1 else "outside"].append(b)
    return reg


def count(lines):
    c = dict.fromkeys(CLASSES, 0)
    by = {}
    for l in lines:
        if l.endswith(":"):
            continue
        mn = l.split()[0]
        c[classify(mn)] += 1
        by[mn] = by.get(mn, 0) + 1
    c["cycles"] = 4 * (c["valu"] + c["lane"]) + 8 * c["trans"]
    return c, by


def loop_hash(lines, registers=True):
    """hash of a listing with the local label numbers replaced; registers=False also replaces the register numbers (the allocation is made
    for the whole kernel, so an edit outside the loop can renumber the loop's registers without changing an instruction of it)"""
    norm = [re.sub(r"(\.L|%)(BB|JTI|tmp|bb\.)\d+(_\d+)?", "L", l) for l in lines]
    if not registers:
        norm = [re.sub(r"\b([vsa])(\d+|\[\d+:\d+\])", r"\1#", l) for l in norm]
    return hashlib.sha256("\n".join(norm).encode()).hexdigest()[:16]


def demangle(names):
    try:
        r = subprocess.run(["c++filt"] + names, capture_output=True, text=True)
        plain = r.stdout.splitlines() if r.returncode == 0 and r.stdout else names
    except OSError:
        plain = names
    return {n: re.sub(r"^void |\(GemmArgs\)$", "", p) for n, p in zip(names, plain)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--tree", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    ap.add_argument("--unit", default="gemm_h2q")
    ap.add_argument("--kernel", default="gemm_h2q_kernel")
    ap.add_argument("--fmt", default=None, help="only the instantiations whose last template argument is this (2 = f16x2)")
    ap.add_argument("--blocks", type=int, default=0, help="list the basic blocks behind the K loop with at least this many instructions")
    ap.add_argument("--mnemonics", action="store_true", help="per instantiation, the mnemonic histogram of the region behind the K loop")
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as work:
        text = compile_asm(a.tree, a.unit, work)
    ks = kernels_of(text, a.kernel)
    nice = demangle([k[0] for k in ks])
    print("unit %s.hip, kernel %s: %d instantiations; cycles = 4 x (valu + lane) + 8 x trans, per wave and tile, static" % (a.unit, a.kernel, len(ks)))
    hdr = "%-10s " % "region" + " ".join("%6s" % c for c in CLASSES) + " %8s" % "cycles"
    for name, body, info in sorted(ks, key=lambda k: nice[k[0]]):
        if a.fmt is not None and not re.search(r",\s*%s>" % re.escape(a.fmt), nice[name]):
            continue
        print("\n== %s" % nice[name])
        print("   " + "  ".join("%s %s" % (short, info[short]) for _, short in INFO))
        reg = regions(body)
        if reg is None:
            print("   no MFMA loop found")
            continue
        print("   " + hdr)
        for tag in ("outside", "K loop", "tile"):
            c, by = count([i for b in reg[tag] for i in b[3]])
            print("   %-10s " % tag + " ".join("%6d" % c[k] for k in CLASSES) + " %8d" % c["cycles"])
        kl = [l for b in reg["K loop"] for l in [b[0] + ":"] + b[3]]
        print("   K loop listing sha256[:16] %s, register numbers replaced %s (%d instructions)"
              % (loop_hash(kl), loop_hash(kl, registers=False), sum(1 for l in kl if not l.endswith(":"))))
        if a.mnemonics:
            c, by = count([i for b in reg["tile"] for i in b[3]])
            print("   tile, by mnemonic: " + ", ".join("%s %d" % kv for kv in sorted(by.items(), key=lambda kv: -kv[1]) if kv[1] >= 8))
        if a.blocks:
            for lab, loop, depth, lines in sorted(reg["tile"], key=lambda b: -len(b[3])):
                if len(lines) < a.blocks:
                    break
                c, _ = count(lines)
                print("   block %-12s " % lab + " ".join("%6d" % c[k] for k in CLASSES) + " %8d" % c["cycles"])


if __name__ == "__main__":
    main()
