"""False accepts of the HDLC deframer's single-bit repair on pure noise, on the CPU: the host form
(ais_amd.hdlc_deframer_bp, aisx_hdlc_work_repair) over random bits without rules, with ais_amd.AIS_REPAIR_RULES and with
the same lengths and any message type, beside a count of the candidate frames (a delimiter behind at least length_min
octets) and of those a repair without any rule would accept, from a restatement of the deframer in this file.

Usage: python tools/hdlc_repair_noise.py [--bits 4000000] [--seed 1] --out profiles/hdlc_repair_noise.json"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "gr-ais_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import numpy as np  # noqa: E402

import ais_amd  # noqa: E402


def candidates(bits, lmin, lmax):
    """(candidate frames, plain CRC passes, frames a single-bit repair of any length and type accepts, their lengths)"""
    table = []
    for v in range(256):
        r = v
        for _ in range(8):
            r = (r >> 1) ^ (0x8408 if r & 1 else 0)
        table.append(r)
    inv, s = {}, 0x8000
    for d in range(32767):
        inv.setdefault(s, d)
        s = (s >> 1) ^ (0x8408 if s & 1 else 0)
    ones, frame, shift, nshift = 0, [], 0, 0
    ncand = nplain = nfix = 0
    lengths = {}
    for bit in bits.tolist():
        if ones < 5:
            if len(frame) > lmax:
                frame, shift, nshift = [], 0, 0
            else:
                shift = (shift >> 1) | (0x80 if bit else 0)
                nshift += 1
                if nshift == 8:
                    frame.append(shift)
                    shift, nshift = 0, 0
        elif bit:
            got = len(frame)
            if got >= lmin:
                ncand += 1
                reg = 0xFFFF
                for o in frame[:-2]:
                    reg = (reg >> 8) ^ table[(reg ^ o) & 0xFF]
                syn = (~reg & 0xFFFF) ^ (frame[-2] | (frame[-1] << 8))
                if syn == 0:
                    nplain += 1
                elif inv.get(syn, 1 << 30) < 8 * got:
                    nfix += 1
                    lengths[got - 2] = lengths.get(got - 2, 0) + 1
            frame, shift, nshift = [], 0, 0
        ones = ones + 1 if bit else 0
    return ncand, nplain, nfix, lengths


def host(bits, lmin, lmax, rules):
    d = ais_amd.hdlc_deframer_bp(lmin, lmax, repair=rules)
    pdus, fix = [], []
    for k in range(0, bits.size, 1 << 20):
        p, f = d.work(bits[k:k + (1 << 20)], with_repairs=True)
        pdus += p
        fix += f
    return dict(pdus=len(pdus), repaired=sum(v >= 0 for v in fix), plain=sum(v < 0 for v in fix),
                payload_octets=sorted(len(p) for p, v in zip(pdus, fix) if v >= 0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bits", type=int, default=4000000)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    lmin, lmax = 11, 64
    bits = np.random.default_rng(a.seed).integers(0, 2, a.bits).astype(np.uint8)
    ncand, nplain, nfix, lengths = candidates(bits, lmin, lmax)
    typed = ais_amd.AIS_REPAIR_RULES
    res = dict(bits=a.bits, seed=a.seed, generator="numpy default_rng(seed).integers(0, 2, bits)", deframer=[lmin, lmax],
               candidates=ncand, plain_crc_passes=nplain, unrestricted_repair_accepts=nfix,
               unrestricted_by_payload_octets={str(k): v for k, v in sorted(lengths.items())},
               host_no_rules=host(bits, lmin, lmax, None),
               host_length_only_rules=host(bits, lmin, lmax, {k: None for k in typed}),
               host_ais_repair_rules=host(bits, lmin, lmax, typed),
               rules={str(k): list(v) for k, v in typed.items()})
    assert res["host_no_rules"]["pdus"] == nplain
    assert res["host_length_only_rules"]["repaired"] == sum(v for k, v in lengths.items() if k in typed)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
