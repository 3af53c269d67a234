"""False accepts of the HDLC deframers' error-event repair on pure noise, on the CPU: random bits through a restatement
of the deframer in this file, which collects the candidate frames (a delimiter behind at least length_min octets); each
failed candidate's syndrome is looked up in the tables of aisx_hdlc_event_table for the three event sets -- single,
single + pair, single + pair + skip -- without any rule, with the five AIS lengths and any message type, and with
ais_amd.AIS_REPAIR_RULES; the last two are also run through the host form (ais_amd.hdlc_deframer_bp), which must agree.
Beside them, the frames the plain CRC accepts.

Usage: python tools/hdlc_events_noise.py [--bits 4000000 40000000] [--seed 1] --out profiles/hdlc_events_noise.json"""
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
from ais_amd import framing  # noqa: E402

SETS = (("single", 1), ("single+pair", 3), ("single+pair+skip", 7))


def candidates(bits, lmin, lmax):
    """[(octets, syndrome, type)] of the candidate frames"""
    table = []
    for v in range(256):
        r = v
        for _ in range(8):
            r = (r >> 1) ^ (0x8408 if r & 1 else 0)
        table.append(r)
    ones, frame, shift, nshift = 0, [], 0, 0
    out = []
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
                reg = 0xFFFF
                for o in frame[:-2]:
                    reg = (reg >> 8) ^ table[(reg ^ o) & 0xFF]
                out.append((got, (~reg & 0xFFFF) ^ (frame[-2] | (frame[-1] << 8)), frame[0]))
            frame, shift, nshift = [], 0, 0
        ones = ones + 1 if bit else 0
    return out


def lookup(cands, events, rules):
    """accepted repairs by event id: rules None = any length and type, else {payload octets: type mask}"""
    tab = framing.event_table(events)
    by = [0, 0, 0]
    for got, syn, first_octet in cands:
        if syn == 0 or (rules is not None and got - 2 not in rules):
            continue
        v = int(tab[syn])
        eid, d1 = v >> 14, v & 0x3FFF
        if d1 == 0 or d1 - 1 + eid >= 8 * got:
            continue
        last = 8 * got - d1
        for j in {last, last - eid}:
            if j < 8:
                first_octet ^= 1 << j
        if rules is None or (rules[got - 2] >> (first_octet >> 2)) & 1:
            by[eid] += 1
    return by


def host(bits, lmin, lmax, rules, events):
    d = ais_amd.hdlc_deframer_bp(lmin, lmax, repair=rules, events=events)
    fix = []
    for k in range(0, bits.size, 1 << 20):
        fix += d.work(bits[k:k + (1 << 20)], with_repairs=True)[1]
    return [sum(f >= 0 and f >> 16 == e for f in fix) for e in range(3)], sum(f < 0 for f in fix)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bits", type=int, nargs="+", default=[4000000, 40000000])
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    lmin, lmax = 11, 64
    typed = ais_amd.AIS_REPAIR_RULES
    tmask = {int(r["payload_octets"]): int(r["type_mask"]) for r in framing.repair_rules(typed)}
    anymask = {k: framing.ANY_TYPE for k in tmask}
    res = dict(seed=a.seed, generator="numpy default_rng(seed).integers(0, 2, bits)", deframer=[lmin, lmax],
               rules={str(k): list(v) for k, v in typed.items()},
               note="accepted repairs by event [single, pair, skip]; lengths_only and typed are the host form's counts, "
                    "which equal the table lookup's", runs=[])
    for nbits in a.bits:
        bits = np.random.default_rng(a.seed).integers(0, 2, nbits).astype(np.uint8)
        cands = candidates(bits, lmin, lmax)
        run = dict(bits=nbits, candidates=len(cands), plain_crc_passes=sum(s == 0 for _, s, _ in cands), sets={})
        for name, events in SETS:
            row = dict(events=events, no_rule=lookup(cands, events, None))
            for key, rules, masks in (("lengths_only", {k: None for k in typed}, anymask), ("typed", typed, tmask)):
                by, plain = host(bits, lmin, lmax, rules, events)
                assert by == lookup(cands, events, masks) and plain == run["plain_crc_passes"]
                row[key] = by
            row["totals"] = {k: sum(row[k]) for k in ("no_rule", "lengths_only", "typed")}
            run["sets"][name] = row
        res["runs"].append(run)
        print(json.dumps(run), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
