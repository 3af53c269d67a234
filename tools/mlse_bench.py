"""Cost of the batched sequence detector (aisx_mlse_batch_*) at the benchmark's shape, 4096 channels x 65536 samples
per step (about 16 400 symbols per channel per step), on one MI355X:

  detector_alone   the detector's kernel over one step's symbols, hipEvents around each call, after a warm-up, beside
                   its traffic: 8 bytes read and 1 byte written per symbol (and, where tools/ubench/hbm_ceiling has
                   been built, the copy ceiling it measures in the same run to hold that against)
  step             the pipelined stock chain (ais_demod.work_pipelined) per step with the deframer queued behind every
                   step as ais_amd.hdlc_deframer_batch documents -- and the same with the chain's symbols going through
                   the detector first (ais_amd.mlse_detector_batch's wiring); alternating runs, each after a warm-up

--hw-queues N sets GPU_MAX_HW_QUEUES for this process (read by the HIP runtime at its first call); the pipelined chain
wants 8 or more.  Writes one JSON file (--out).
Usage: python tools/mlse_bench.py [--nchan 4096] [--calls 50] [--steps 20] [--hw-queues 8] --out F"""
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
    sys.exit("mlse_bench: --hw-queues must be an integer in 1..32")
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
    det = ais_amd.mlse_detector_batch(nchan, cap)
    hd = {False: ais_amd.hdlc_deframer_batch(11, 64, nchan, cap, 1 << 17), True: ais_amd.hdlc_deframer_batch(11, 64, nchan, cap + 79, 1 << 17)}
    s = torch.cuda.Stream()
    res = {"shape": dict(nchan=nchan, T=T, max_syms=cap), "device": torch.cuda.get_device_name(0),
           "gpu_max_hw_queues": int(os.environ["GPU_MAX_HW_QUEUES"])}

    def steps(n, mlse):
        n += n % 2  # (x_next alternates between the two inputs: every run ends where the next one starts)
        prev, pdus, h = False, 0, hd[mlse]
        for k in range(n):
            r = dem.work_pipelined(xs[k % 2], x_next=xs[(k + 1) % 2], want_syms=mlse)
            if prev:
                pdus += len(h.pdus(stream=s)[0])
            dem.wait(r["step"], stream=s)
            if mlse:
                bits, nbits = det.process(r["syms"], r["produced"], stream=s)
                h.work(bits, nbits, stream=s)
            else:
                h.work(r["bits"], r["produced"], stream=s)
            prev = True
        pdus += len(h.pdus(stream=s)[0])
        dem.synchronize()
        return r, pdus

    # chain-like symbols: one step's output (the chain warmed up on the way)
    r, _ = steps(a.warmup + 2, True)
    syms, prod = r["syms"].clone(), r["produced"].clone()
    torch.cuda.synchronize()
    ns = prod.cpu().numpy()
    res["symbols_per_step"] = dict(total=int(ns.sum()), per_channel_mean=float(ns.mean()))

    # the detector alone
    for _ in range(a.warmup):
        det.process(syms, prod, stream=s)
    s.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.calls)]
    for e0, e1 in ev:
        e0.record(s)
        det.process(syms, prod, stream=s)
        e1.record(s)
    s.synchronize()
    ms = sorted(e0.elapsed_time(e1) for e0, e1 in ev)
    med = ms[len(ms) // 2]
    res["detector_alone_ms"] = dict(median=med, min=ms[0], max=ms[-1], p10=ms[len(ms) // 10], p90=ms[(9 * len(ms)) // 10], calls=a.calls)
    nbytes = 9 * int(ns.sum())
    res["traffic"] = dict(bytes_per_call=nbytes, achieved_GBs=nbytes / (med * 1e-3) / 1e9)
    ceil = bench.hbm_ceilings() if hasattr(bench, "hbm_ceilings") else None
    if ceil:
        res["traffic"]["hbm_ceilings"] = ceil
    det.reset()

    # the pipelined step with the deframer alone behind it / with detector + deframer
    per = {False: [], True: []}
    npdus = {False: 0, True: 0}
    for rep in range(3):
        for mlse in (False, True):
            steps(a.warmup, mlse)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            _, p = steps(a.steps, mlse)
            per[mlse].append((time.perf_counter() - t0) * 1e3 / a.steps)
            npdus[mlse] = max(npdus[mlse], p)
    res["step_ms"] = dict(deframer=sorted(per[False]), detector_and_deframer=sorted(per[True]), steps=a.steps,
                          pdus_in_run=dict(deframer=npdus[False], detector_and_deframer=npdus[True]))
    res["step_cost_ms"] = float(np.median(per[True]) - np.median(per[False]))
    assert det.status() == 0
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
