"""Cost of the batched NMEA armouring (aisx_nmea_batch_*) at the benchmark's shape, 4096 channels x 65536 samples
per step, behind the batched HDLC deframer, on one MI355X:

  nmea_alone   the NMEA stage's two kernels over one step's PDUs, hipEvents around each call, after a warm-up
  step         the pipelined stock chain (ais_demod.work_pipelined) per step with the deframer and its PDU read-back
               behind every step, against the deframer + the NMEA stage + the text read-back (the pattern
               ais_amd.pdu_to_nmea_batch documents); the two variants alternate in one process
  host         aisx_pdu_to_nmea over the same PDUs through ais_amd.pdu_to_nmea: one thread, a pool of 16

--hw-queues N sets GPU_MAX_HW_QUEUES for this process (read by the HIP runtime at its first call); the pipelined chain
wants 8 or more.  Writes one JSON file (--out).
Usage: python tools/nmea_bench.py [--nchan 4096] [--calls 50] [--steps 20] [--hw-queues 8] --out F"""
import argparse
import concurrent.futures as cf
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
    sys.exit("nmea_bench: --hw-queues must be an integer in 1..32")
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
    s = torch.cuda.Stream()
    res = {"shape": dict(nchan=nchan, T=T, length_min=11, length_max=64, max_pdus=max_pdus, designators="A / B"),
           "device": torch.cuda.get_device_name(0), "gpu_max_hw_queues": int(os.environ["GPU_MAX_HW_QUEUES"])}

    def steps(n, nmea):
        n += n % 2  # (x_next alternates between the two inputs: every run ends where the next one starts)
        prev = False
        pdus = 0

        def read():
            return len(nm.sentences(stream=s)[0]) if nmea else len(hd.pdus(stream=s)[0])

        for k in range(n):
            r = dem.work_pipelined(xs[k % 2], x_next=xs[(k + 1) % 2])
            if prev:
                pdus += read()
            dem.wait(r["step"], stream=s)
            hd.work(r["bits"], r["produced"], stream=s)
            if nmea:
                nm.work(hd, stream=s)
            prev = True
        pdus += read()
        dem.synchronize()
        return r, pdus

    # chain-like PDUs: one step's output deframed (the chain warmed up on the way)
    steps(a.warmup + 2, False)
    torch.cuda.synchronize()
    recs, data = hd.pdus(stream=s)

    # the NMEA stage alone over the deframer's last results
    for _ in range(a.warmup):
        nm.work(hd, stream=s)
    s.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.calls)]
    for e0, e1 in ev:
        e0.record(s)
        nm.work(hd, stream=s)
        e1.record(s)
    s.synchronize()
    ms = sorted(e0.elapsed_time(e1) for e0, e1 in ev)
    nrec, text = nm.sentences(stream=s)
    res["nmea_alone_ms"] = dict(median=ms[len(ms) // 2], min=ms[0], max=ms[-1], calls=a.calls, pdus_per_call=int(len(nrec)),
                                text_bytes_per_call=len(text))

    # the pipelined step: deframer + PDU read-back against deframer + NMEA + text read-back (alternating runs)
    per = {False: [], True: []}
    npdus = {False: 0, True: 0}
    for rep in range(3):
        for nmea in (False, True):
            steps(a.warmup, nmea)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            _, p = steps(a.steps, nmea)
            per[nmea].append((time.perf_counter() - t0) * 1e3 / a.steps)
            npdus[nmea] = max(npdus[nmea], p)
    res["step_ms"] = dict(deframer_pdus=sorted(per[False]), deframer_nmea_text=sorted(per[True]), steps=a.steps,
                          pdus_in_run=npdus[True])
    res["step_cost_ms"] = float(np.median(per[True]) - np.median(per[False]))

    # the host path over the same PDUs: ais_amd.pdu_to_nmea(...).msg_to_sentence (aisx_pdu_to_nmea through ctypes,
    # which lets go of the interpreter lock for the call), one thread and a pool of 16
    pdus = [(int(r["chan"]), bytes(data[r["offset"]:r["offset"] + r["len"]])) for r in recs]
    conv = {d: ais_amd.pdu_to_nmea(d) for d in set(des)}

    def host(part):
        return sum(len(conv[des[c]].msg_to_sentence(p)) + 1 for c, p in part)

    t0 = time.perf_counter()
    n1 = host(pdus)
    one = time.perf_counter() - t0
    with cf.ThreadPoolExecutor(max_workers=16) as ex:
        t0 = time.perf_counter()
        n16 = sum(ex.map(host, [pdus[k::16] for k in range(16)]))
        pool = time.perf_counter() - t0
    assert n1 == n16 == len(text), (n1, n16, len(text))
    res["host"] = dict(one_thread_ms=one * 1e3, pool16_ms=pool * 1e3, pdus=len(pdus), text_bytes=n1,
                       note="ais_amd.pdu_to_nmea(designator).msg_to_sentence per PDU (one ctypes call each)")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
