"""Cost of the batched message-field decoder (aisx_msg_batch_*) at the benchmark's shape, 4096 channels x 65536 samples
per step, behind the batched HDLC deframer, on one MI355X, beside the NMEA stage in the same run:

  msg_alone    the decoder's kernel over one step's PDUs, hipEvents around each call, after a warm-up
  nmea_alone   the NMEA stage's two kernels over the same PDUs, measured the same way
  step         the pipelined stock chain (ais_demod.work_pipelined) per step with the deframer and its PDU read-back
               behind every step, against the deframer + the decoder + the table read-back; the two variants
               alternate in one process
  host         aisx_msg_decode over the same PDUs through ais_amd.msg_decode, one thread

--hw-queues N sets GPU_MAX_HW_QUEUES for this process (read by the HIP runtime at its first call); the pipelined chain
wants 8 or more.  Writes one JSON file (--out).
Usage: python tools/msg_bench.py [--nchan 4096] [--calls 50] [--steps 20] [--hw-queues 8] --out F"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "gr-ais_amd"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)


def _hw_queues():
    for k, v in enumerate(sys.argv):
        if v == "--hw-queues" and k + 1 < len(sys.argv):
            return sys.argv[k + 1]
        if v.startswith("--hw-queues="):
            return v.split("=", 1)[1]
    return "8"


_q = _hw_queues()
if not _q.isdigit() or not 1 <= int(_q) <= 32:
    sys.exit("msg_bench: --hw-queues must be an integer in 1..32")
os.environ["GPU_MAX_HW_QUEUES"] = _q  # (before torch makes the first HIP call)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import ais_amd  # noqa: E402
import bench  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nchan", type=int, default=4096)
    ap.add_argument("--T", type=int, default=65536)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--hw-queues", type=int, default=8)
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    nchan, T, sps = a.nchan, a.T, 4
    dev = torch.device("cuda", 0)
    opts = dict(samples_per_symbol=sps, bits_per_sec=9600.0, clockrec_gain=0.04, omega_relative_limit=0.01, fftlen=1024)
    tmpl = ais_amd.modulate_vector_bc(ais_amd.gmsk_mod(sps, 0.4), [1, 1, 0, 0] * 7, [1])
    xs = [bench.make_input(nchan, T, "S", sps, dev, r, True) for r in range(2)]
    dem = ais_amd.ais_demod(opts, nchan=nchan, max_items=T, stages="stock", preamble_symbols=tmpl)
    cap = dem.clockrec.out_capacity
    max_pdus = 1 << 17
    des = ["A", "B"] * (nchan // 2) + ["A"] * (nchan % 2)
    hd = ais_amd.hdlc_deframer_batch(11, 64, nchan, cap, max_pdus)
    nm = ais_amd.pdu_to_nmea_batch(des, nchan, max_pdus, 64)
    md = ais_amd.pdu_decode_batch(nchan, max_pdus, 64)
    s = torch.cuda.Stream()
    res = {"shape": dict(nchan=nchan, T=T, length_min=11, length_max=64, max_pdus=max_pdus),
           "device": torch.cuda.get_device_name(0), "gpu_max_hw_queues": int(os.environ["GPU_MAX_HW_QUEUES"])}

    def steps(n, decode):
        n += n % 2  # (x_next alternates between the two inputs: every run ends where the next one starts)
        prev = False
        pdus = 0

        def read():
            return len(md.messages(stream=s)) if decode else len(hd.pdus(stream=s)[0])

        for k in range(n):
            r = dem.work_pipelined(xs[k % 2], x_next=xs[(k + 1) % 2])
            if prev:
                pdus += read()
            dem.wait(r["step"], stream=s)
            hd.work(r["bits"], r["produced"], stream=s)
            if decode:
                md.work(hd, stream=s)
            prev = True
        pdus += read()
        dem.synchronize()
        return r, pdus

    # chain-like PDUs: one step's output deframed (the chain warmed up on the way)
    steps(a.warmup + 2, False)
    torch.cuda.synchronize()
    recs, data = hd.pdus(stream=s)

    def alone(stage):
        for _ in range(a.warmup):
            stage.work(hd, stream=s)
        s.synchronize()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.calls)]
        for e0, e1 in ev:
            e0.record(s)
            stage.work(hd, stream=s)
            e1.record(s)
        s.synchronize()
        ms = sorted(e0.elapsed_time(e1) for e0, e1 in ev)
        return dict(median=ms[len(ms) // 2], min=ms[0], max=ms[-1], calls=a.calls)

    # the two stages alone over the deframer's last results, alternating so that neither has the quieter half of the run
    m1, n1 = alone(md), alone(nm)
    m2, n2 = alone(md), alone(nm)
    table = md.messages(stream=s)
    nrec, text = nm.sentences(stream=s)
    assert len(table) == len(nrec) == len(recs)
    res["msg_alone_ms"] = dict(m1 if m1["median"] <= m2["median"] else m2, runs=[m1["median"], m2["median"]], pdus_per_call=int(len(table)),
                               table_bytes_per_call=int(len(table)) * (4 * len(ais_amd.MSG_COLUMNS) + 48))
    res["nmea_alone_ms"] = dict(n1 if n1["median"] <= n2["median"] else n2, runs=[n1["median"], n2["median"]], pdus_per_call=int(len(nrec)),
                                text_bytes_per_call=len(text))
    res["msg_over_nmea"] = res["msg_alone_ms"]["median"] / res["nmea_alone_ms"]["median"]
    types, counts = np.unique(table["type"], return_counts=True)
    res["types_in_table"] = {int(t): int(c) for t, c in zip(types, counts)}

    # the pipelined step: deframer + PDU read-back against deframer + decoder + table read-back (alternating runs)
    per = {False: [], True: []}
    npdus = {False: 0, True: 0}
    for rep in range(3):
        for decode in (False, True):
            steps(a.warmup, decode)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            _, p = steps(a.steps, decode)
            per[decode].append((time.perf_counter() - t0) * 1e3 / a.steps)
            npdus[decode] = max(npdus[decode], p)
    res["step_ms"] = dict(deframer_pdus=sorted(per[False]), deframer_decoder_table=sorted(per[True]), steps=a.steps,
                          pdus_in_run=npdus[True])
    res["step_cost_ms"] = float(np.median(per[True]) - np.median(per[False]))

    # the host path over the same PDUs: ais_amd.msg_decode per PDU (aisx_msg_decode through ctypes), one thread;
    # every row is compared with the device's on the way
    pdus = [bytes(data[r["offset"]:r["offset"] + r["len"]]) for r in recs]
    t0 = time.perf_counter()
    host = [ais_amd.msg_decode(p) for p in pdus]
    one = time.perf_counter() - t0
    for k in range(0, len(host), 97):
        assert all(host[k][c] == int(table[c.lower()][k]) for c in ais_amd.MSG_COLUMNS), k
    res["host"] = dict(one_thread_ms=one * 1e3, pdus=len(pdus),
                       note="ais_amd.msg_decode per PDU (one ctypes call and one dict each)")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
