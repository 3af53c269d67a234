#!/usr/bin/env python3
"""Resources and static instruction mix of the freq_xlating FIR kernels (gr-ais_amd/csrc/aisx_xlate.hip, k_xlate.h),
compiled for gfx950 with the Makefile's flags: per kernel the registers, LDS and workgroups per CU; the inner loop
(the basic block with the most v_pk_fma_f32 that branches back to itself) by mnemonic; and the staging loop's global
loads (the block that loads from global memory and writes z into LDS).  No GPU needed.
    python tools/xlate_fmt_isa.py [repository root] > profiles/xlate_fmt_isa_after.json"""
import collections
import json
import os
import re
import subprocess
import sys
import tempfile

FLAGS = "-O3 -std=c++17 -fPIC -ffp-contract=off -fno-fast-math -Xclang -target-feature -Xclang -load-store-opt".split()
LDS_PER_CU, VGPR_PER_SIMD = 160 * 1024, 512


def demangle(names):
    try:
        out = subprocess.run(["c++filt"] + names, capture_output=True, text=True).stdout.split("\n")
    except OSError:
        out = names
    return dict(zip(names, out))


def blocks(body):
    """[(label, [instructions])] of a function body"""
    cur, out = "entry", []
    ins = []
    for line in body.split("\n"):
        t = line.strip()
        if not t or t[0] == ";":
            continue
        m = re.match(r"^(\.LBB\d+_\d+):", t)
        if m:
            out.append((cur, ins))
            cur, ins = m.group(1), []
        elif t[0] != ".":
            ins.append(t.split(";")[0].strip())
    out.append((cur, ins))
    return out


def mix(ins):
    c = collections.Counter(i.split()[0] for i in ins)
    return dict(sorted(c.items()))


def main(root):
    src = os.path.join(root, "gr-ais_amd", "csrc", "aisx_xlate.hip")
    with tempfile.TemporaryDirectory() as tmp:
        asm = os.path.join(tmp, "x.s")
        subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950"] + FLAGS + ["-S", "--cuda-device-only", "-o", asm, src],
                       check=True, stderr=subprocess.DEVNULL)
        txt = open(asm).read()
    funcs = re.findall(r"^(_Z\w+):[^\n]*\n(.*?)^\.Lfunc_end\d+:", txt, flags=re.S | re.M)
    names = demangle([f[0] for f in funcs])
    meta_txt = txt[txt.find("amdhsa.kernels"):]
    res = {}
    for name, body in funcs:
        entry = ""
        for e in re.split(r"\n  - \.a", meta_txt):
            if re.search(r"\.name:\s+%s\n" % re.escape(name), e):
                entry = e
                break
        r = {}
        for key in ("vgpr_count", "agpr_count", "sgpr_count", "group_segment_fixed_size", "vgpr_spill_count",
                    "private_segment_fixed_size"):
            mm = re.search(r"\.%s:\s*(\d+)" % key, entry)
            if mm:
                r[key] = int(mm.group(1))
        by_vgpr = VGPR_PER_SIMD // (-(-max(r.get("vgpr_count", 1), 1) // 8) * 8)  # waves per SIMD
        r["workgroups_per_cu"] = min(LDS_PER_CU // max(r.get("group_segment_fixed_size", 1), 1), by_vgpr * 4 // 4)
        bl = blocks(body)
        inner = max(bl, key=lambda b: sum(i.startswith("v_pk_fma_f32") for i in b[1]))
        r["inner_loop"] = dict(label=inner[0], instructions=len(inner[1]), mix=mix(inner[1]))
        stage = [b for b in bl if any(i.startswith("global_load") for i in b[1]) and any(i.startswith("ds_write") for i in b[1])]
        stage += [b for b in bl if any(re.match(r"global_load_(u|s)(byte|short)|global_load_dword\b|global_load_dwordx2", i) for i in b[1])
                  and b not in stage]
        r["staging_loads"] = {b[0]: {k: v for k, v in mix(b[1]).items() if k.startswith(("global_load", "ds_write", "v_cvt", "v_sub_f32",
                                                                                          "v_mul_f32", "v_pk_mul_f32", "v_pk_add_f32"))}
                              for b in stage}
        res[names[name].split("(")[0]] = r
    print(json.dumps(dict(flags=" ".join(FLAGS), kernels=res), indent=1))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
