"""What the 4-state sequence detector recovers near the decoding threshold, on the CPU: tools/hdlc_repair_gain.py's
setup -- tests/synth.py's bursts (family S, 168-bit payloads of message type 1) in white Gaussian noise at a few Eb/N0,
demodulated by the CPU restatement of the stock chain (tests/oracle_py.py) -- with the chain's bits (the plain bit tail)
and with the host form of the detector (ais_amd.mlse_detector) on the chain's symbols, each deframed by the host form
(ais_amd.hdlc_deframer_bp) without and with ais_amd.AIS_REPAIR_RULES.  Counts the PDUs that equal a sent payload and
those that equal none.

Usage: python tools/mlse_gain.py [--ebn0 10 12 14 16 18 20] [--nchan 12] [--T 131072] [--seed 5000] --out F"""
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


def one(args):
    seed, T, ebn0, tmpl = args
    bits, syms, sent = mc.noisy_channel(seed, T, ebn0, tmpl)
    det = ais_amd.mlse_detector(0.4)
    mbits = np.concatenate([det.work(syms), det.flush()])
    row = dict(sent=len(sent))
    for name, b in (("plain", bits), ("mlse", mbits)):
        for tag, rules in (("", None), ("_repair", ais_amd.AIS_REPAIR_RULES)):
            pdus = ais_amd.hdlc_deframer_bp(11, 64, repair=rules).work(b)
            row[name + tag] = len(set(pdus) & sent)
            row[name + tag + "_wrong"] = len([p for p in pdus if p not in sent])
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ebn0", type=float, nargs="+", default=[10, 12, 14, 16, 18, 20])
    ap.add_argument("--nchan", type=int, default=12)
    ap.add_argument("--T", type=int, default=131072)
    ap.add_argument("--seed", type=int, default=5000)
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    tmpl = mc.stock_template()
    res = dict(chain="tests/oracle_py.py Demod(4 samples per symbol, stock template, stages=3); plain: its bits; mlse: "
                     "ais_amd.mlse_detector(0.4) on its symbols; hdlc_deframer_bp(11, 64)",
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
