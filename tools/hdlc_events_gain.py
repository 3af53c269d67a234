"""What the HDLC deframers' error-event repair recovers near the decoding threshold, on the CPU: tools/mlse_gain.py's
setup -- tests/synth.py's bursts (family S, 168-bit payloads of message type 1) in white Gaussian noise at a few Eb/N0,
demodulated by the CPU restatement of the stock chain (tests/oracle_py.py) -- with the chain's bits (the plain bit tail)
and with the host form of the sequence detector (ais_amd.mlse_detector) on the chain's symbols, each deframed by the
host form (ais_amd.hdlc_deframer_bp) without repair and with ais_amd.AIS_REPAIR_RULES for the event sets single,
single + pair and single + pair + skip.  Counts the sent payloads recovered and the PDUs that equal none.

Usage: python tools/hdlc_events_gain.py [--ebn0 12 14 16 18 20] [--nchan 12] [--T 131072] [--seed 5000] --out F"""
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
import mlse_cases as mc  # noqa: E402

SETS = (("none", 0), ("single", 1), ("single_pair", 3), ("all", 7))


def one(args):
    seed, T, ebn0, tmpl = args
    bits, syms, sent = mc.noisy_channel(seed, T, ebn0, tmpl)
    det = ais_amd.mlse_detector(0.4)
    mbits = np.concatenate([det.work(syms), det.flush()])
    row = dict(sent=len(sent))
    for name, b in (("tail", bits), ("mlse", mbits)):
        for tag, events in SETS:
            d = ais_amd.hdlc_deframer_bp(11, 64)
            if events:
                d.set_repair(ais_amd.AIS_REPAIR_RULES, events)
            pdus, fix = d.work(b, with_repairs=True)
            row["%s_%s" % (name, tag)] = len(set(pdus) & sent)
            row["%s_%s_unsent" % (name, tag)] = len([p for p in pdus if p not in sent])
            if events == 7:
                row["%s_all_by_event" % name] = [sum(f >= 0 and f >> 16 == e and p in sent for p, f in zip(pdus, fix)) for e in range(3)]
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ebn0", type=float, nargs="+", default=[12, 14, 16, 18, 20])
    ap.add_argument("--nchan", type=int, default=12)
    ap.add_argument("--T", type=int, default=131072)
    ap.add_argument("--seed", type=int, default=5000)
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    tmpl = mc.stock_template()
    res = dict(chain="tests/oracle_py.py Demod(4 samples per symbol, stock template, stages=3); tail: its bits; mlse: "
                     "ais_amd.mlse_detector(0.4) on its symbols; hdlc_deframer_bp(11, 64)",
               noise="complex AWGN, Eb = amp^2 * samples_per_symbol (synth.make_channel), cfo within +-500 Hz",
               rules={str(k): list(v) for k, v in ais_amd.AIS_REPAIR_RULES.items()},
               sets={k: v for k, v in SETS}, nchan=a.nchan, T=a.T, seed=a.seed, levels=[])
    for e in a.ebn0:
        with cf.ProcessPoolExecutor(min(a.nchan, 12)) as ex:
            rows = list(ex.map(one, [(a.seed + c, a.T, e, tmpl) for c in range(a.nchan)]))
        tot = {k: ([sum(v) for v in zip(*(r[k] for r in rows))] if isinstance(rows[0][k], list) else sum(r[k] for r in rows))
               for k in rows[0]}
        tot["ebn0_db"] = e
        res["levels"].append(tot)
        print(json.dumps(tot), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
