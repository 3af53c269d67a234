#!/usr/bin/env python3
"""Instruction mix of the timing recovery's pair loops in the gfx950 code of k_msk<false, false, LPW>:

    python tools/msk_loop_isa.py [--asm FILE.s] [--lpw 8] [--core] [--json OUT]

Without --asm, compiles gr-ais_amd/csrc/aisx_msk.hip to assembly with the Makefile's flags (-S --cuda-device-only).
The loops are found by the compiler's loop comments: every innermost loop of the kernel that swaps rows
(v_permlane16/32_swap) is a pair loop; the one of a single basic block is the plain lock-step loop, the one of several
blocks (the tag tests branch) the tagged-run loop.  Reported per loop: VALU (packed counted apart), LDS, SALU, s_nop,
v_mov, s_waitcnt, the total, and for the plain loop the pairs written out per trip (k_msk.h: msk_run_trips), the counts per
pair and the longest chain of register dependences within one trip (each instruction one step; s_nop and s_waitcnt not counted).  --core: the build with the hand-scheduled pair, k_msk_core (its
inline assembly is part of the loop's block like any other instruction)."""
import argparse
import collections
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-Wno-unused-function"]


def compile_asm(out):
    cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950"] + FLAGS + [
        "-S", "--cuda-device-only", "-o", out, os.path.join(ROOT, "gr-ais_amd", "csrc", "aisx_msk.hip")]
    subprocess.run(cmd, check=True, stderr=subprocess.DEVNULL)


def kernel_body(txt, lpw, core=False):
    name = "_Z10k_msk_coreN4aisx9MskParamsE" if core else "_Z5k_mskILb0ELb0ELi%dEEvN4aisx9MskParamsE" % lpw
    m = re.search(r"^%s:[^\n]*\n(.*?)^\.Lfunc_end\d+:" % name, txt, flags=re.S | re.M)
    if not m:
        sys.exit("no %s in the assembly" % name)
    return m.group(1).split("\n")


def blocks(lines):
    """[(label, loop header or None, depth, is_header, [instructions])] in program order"""
    out = []
    cur = None
    for line in lines:
        s = line.strip()
        lab = re.match(r"^(\.LBB\w+|; %bb\.\d+):?(.*)$", s)
        if lab and (s.startswith(".LBB") or s.startswith("; %bb.")):
            rest = lab.group(2)
            hdr = re.search(r"Loop Header: Depth=(\d+)", rest)
            inl = re.search(r"in Loop: Header=(\w+) Depth=(\d+)", rest)
            name = lab.group(1).lstrip(".").replace("; %bb.", "BB_")
            if hdr:
                cur = [name, name.replace("LBB", "BB"), int(hdr.group(1)), True, []]
            elif inl:
                cur = [name, inl.group(1), int(inl.group(2)), False, []]
            else:
                cur = [name, None, 0, False, []]
            out.append(cur)
            continue
        if s.startswith(";") and cur is not None and not cur[4]:
            hdr = re.search(r"Loop Header: Depth=(\d+)", s)
            if hdr:  # (the loop comment on a line of its own after the label)
                cur[1], cur[2], cur[3] = cur[0].replace("LBB", "BB"), int(hdr.group(1)), True
            inl = re.search(r"in Loop: Header=(\w+) Depth=(\d+)", s)
            if inl and not cur[3]:
                cur[1], cur[2] = inl.group(1), int(inl.group(2))
            continue
        if not s or s[0] in ";." or s.endswith(":"):
            continue
        if cur is None:
            cur = ["entry", None, 0, False, []]
            out.append(cur)
        cur[4].append(s.split(";")[0].strip())
    return out


def classify(op):
    if op.startswith("v_pk_"):
        return "valu_pk"
    if op.startswith("v_"):
        return "valu"
    if op.startswith("ds_"):
        return "lds"
    if op.startswith(("global_", "buffer_", "flat_", "scratch_")):
        return "vmem"
    if op.startswith("s_waitcnt"):
        return "waitcnt"
    if op.startswith("s_nop"):
        return "nop"
    if op.startswith(("s_cbranch", "s_branch")):
        return "branch"
    if op.startswith("s_"):
        return "salu"
    return "other"


def regs(tok):
    """the 32-bit registers an operand names"""
    m = re.match(r"^\|?-?([vs])\[(\d+):(\d+)\]", tok)
    if m:
        return ["%s%d" % (m.group(1), i) for i in range(int(m.group(2)), int(m.group(3)) + 1)]
    m = re.match(r"^\|?-?([vs])(\d+)\|?$", tok)
    if m:
        return [m.group(1) + m.group(2)]
    if tok in ("vcc", "scc", "exec"):
        return [tok]
    return []


def chain(instrs):
    """longest path of register dependences in one trip (program order, each instruction 1)"""
    ready = {}
    best = 0
    for ins in instrs:
        op = ins.split()[0]
        if op.startswith(("s_waitcnt", "s_nop", "s_cbranch", "s_branch")):
            continue
        ops = [t.strip() for t in ins[len(op):].split(",") if t.strip()]
        ops = [t.split()[0] for t in ops]
        if op.startswith("ds_write") or op.startswith("s_cmp"):
            dst, src = [], ops
        elif "permlane" in op and "swap" in op:
            dst, src = ops, ops
        else:
            dst, src = ops[:1], ops[1:]
            if op.startswith(("v_cmp", "v_add_co", "v_sub_co", "v_mad_u64", "v_mad_i64")) and len(ops) > 1:
                dst, src = ops[:2], ops[2:]
            if op.startswith(("v_cndmask", "v_addc", "v_subb")):
                src = ops[1:] + ["vcc"]
        d = 1 + max([ready.get(r, 0) for t in src for r in regs(t)] + [0])
        if op.startswith("s_cmp") or op.startswith("v_cmp_") and not dst:
            ready["scc"] = d
        for t in dst:
            for r in regs(t):
                ready[r] = d
        best = max(best, d)
    return best


def mix(instrs):
    c = collections.Counter(classify(i.split()[0]) for i in instrs)
    r = {k: c.get(k, 0) for k in ("valu", "valu_pk", "lds", "salu", "nop", "waitcnt", "branch", "vmem")}
    r["v_mov"] = sum(1 for i in instrs if i.split()[0].startswith(("v_mov_b32", "v_mov_b64", "v_pk_mov")))
    r["v_mad_u64_u32"] = sum(1 for i in instrs if i.split()[0].startswith("v_mad_u64_u32"))
    r["total"] = len(instrs)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--asm", help="an assembly file of aisx_msk.hip (default: compile one)")
    ap.add_argument("--lpw", type=int, default=8)
    ap.add_argument("--core", action="store_true", help="k_msk_core instead of k_msk<false, false, LPW>")
    ap.add_argument("--json", help="write the result here as well")
    a = ap.parse_args()
    path = a.asm
    if not path:
        fd, path = tempfile.mkstemp(suffix=".s")
        os.close(fd)
        compile_asm(path)
    lines = kernel_body(open(path).read(), a.lpw, a.core)
    bl = blocks(lines)
    loops = collections.OrderedDict()
    for b in bl:
        if b[1] is not None:
            loops.setdefault(b[1], []).append(b)
    # innermost loops only: a loop whose header is no other loop's parent; keep those that swap rows
    found = []
    for hdr, bs in loops.items():
        ins = [i for b in bs for i in b[4]]
        if any("permlane16_swap" in i or "permlane32_swap" in i for i in ins):
            found.append((hdr, bs, ins))
    plain = [f for f in found if len(f[1]) == 1]
    tagged = [f for f in found if len(f[1]) > 1]
    res = {"kernel": "k_msk_core" if a.core else "k_msk<false,false,%d>" % a.lpw}
    if plain:
        hdr, bs, ins = min(plain, key=lambda f: len(f[2]))
        # (a trip of the loop is several pairs written out one behind the other, k_msk.h: msk_run_trips; a pair swaps rows twice)
        pairs = max(1, sum(1 for i in ins if "permlane16_swap" in i or "permlane32_swap" in i) // 2)
        m = mix(ins)
        res["plain_pair_loop"] = dict(m, label=hdr, chain=chain(ins), pairs_per_trip=pairs,
                                      per_pair={k: round(m[k] / pairs, 3) for k in ("total", "salu", "branch", "lds")})
    if tagged:
        hdr, bs, ins = min(tagged, key=lambda f: len(f[2]))
        res["tagged_pair_loop"] = dict(mix(ins), label=hdr, blocks=len(bs))
    print(json.dumps(res, indent=1))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    if not a.asm:
        os.unlink(path)


if __name__ == "__main__":
    main()
