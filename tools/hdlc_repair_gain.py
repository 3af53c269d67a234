"""What the HDLC deframer's single-bit repair recovers near the decoding threshold, on the CPU: tests/synth.py's bursts
(family S, random 168-bit payloads whose message type is forced to 1, so that ais_amd.AIS_REPAIR_RULES admits them) in
white Gaussian noise at a few Eb/N0, demodulated by the CPU restatement of the stock chain (tests/oracle_py.py) and
deframed by the host form (ais_amd.hdlc_deframer_bp) without and with the rules.  Counts the PDUs that equal a sent
payload, and the repaired PDUs that equal none (miscorrections and false accepts).

Noise model: synth.make_channel's -- complex AWGN of variance N0 per sample on a burst of amplitude `amp`, with
Eb = amp^2 * samples_per_symbol; carrier offsets up to +-500 Hz, random timing and phase.  Seeds: --seed + channel.

Usage: python tools/hdlc_repair_gain.py [--ebn0 12 14 16 18 20 24] [--nchan 12] [--T 131072] [--seed 5000] --out F"""
import argparse
import concurrent.futures as cf
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "gr-ais_amd"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import numpy as np  # noqa: E402

import ais_amd  # noqa: E402
import oracle_py as orc  # noqa: E402
import synth  # noqa: E402

SPS = 4


class TypedPayloads:
    """a numpy Generator whose 168-bit draws (make_burst's payloads) carry message type 1: bits 2..7 of the first octet,
    LSB first"""

    def __init__(self, rng):
        self._rng = rng

    def __getattr__(self, name):
        return getattr(self._rng, name)

    def integers(self, low, high=None, size=None):
        v = self._rng.integers(low, high, size)
        if size == 168:
            v[2:8] = [1, 0, 0, 0, 0, 0]
        return v


def typed_channel(seed, T, ebn0):
    """synth.make_channel with every payload's message type set to 1"""
    real = synth.make_burst
    synth.make_burst = lambda rng, family, sps, **kw: real(TypedPayloads(rng), family, sps, **kw)
    try:
        return synth.make_channel(seed, T, "S", SPS, amp=1.0, ebn0_db=ebn0, cfo_max=500.0)
    finally:
        synth.make_burst = real


def one(args):
    seed, T, ebn0, tmpl = args
    x, infos = typed_channel(seed, T, ebn0)
    bits = orc.Demod(SPS, tmpl, stages=3).step(x)[0]
    bits = np.asarray(bits if bits is not None else [], np.uint8)
    sent = {np.packbits(np.array(i["payload"], np.uint8), bitorder="little").tobytes() for i in infos}
    plain = ais_amd.hdlc_deframer_bp(11, 64).work(bits)
    pdus, fix = ais_amd.hdlc_deframer_bp(11, 64, repair=ais_amd.AIS_REPAIR_RULES).work(bits, with_repairs=True)
    return dict(sent=len(sent), plain=len(set(plain) & sent), plain_wrong=len([p for p in plain if p not in sent]),
                with_repair=len(set(pdus) & sent), repaired=sum(f >= 0 for f in fix),
                repaired_wrong=len([p for p, f in zip(pdus, fix) if f >= 0 and p not in sent]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ebn0", type=float, nargs="+", default=[12, 14, 16, 18, 20, 24])
    ap.add_argument("--nchan", type=int, default=12)
    ap.add_argument("--T", type=int, default=131072)
    ap.add_argument("--seed", type=int, default=5000)
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    tmpl = ais_amd.modulate_vector_bc(ais_amd.gmsk_mod(SPS, 0.4), [1, 1, 0, 0] * 7, [1])
    res = dict(chain="tests/oracle_py.py Demod(4 samples per symbol, stock template, stages=3), hdlc_deframer_bp(11, 64)",
               noise="complex AWGN, Eb = amp^2 * samples_per_symbol (synth.make_channel), cfo within +-500 Hz",
               rules={str(k): list(v) for k, v in ais_amd.AIS_REPAIR_RULES.items()}, nchan=a.nchan, T=a.T, seed=a.seed, levels=[])
    for e in a.ebn0:
        with cf.ProcessPoolExecutor(min(a.nchan, 12)) as ex:
            rows = list(ex.map(one, [(a.seed + c, a.T, e, tmpl) for c in range(a.nchan)]))
        tot = {k: sum(r[k] for r in rows) for k in rows[0]}
        tot["ebn0_db"] = e
        res["levels"].append(tot)
        print(json.dumps(tot), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
