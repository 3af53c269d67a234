"""Cost of the batched HDLC deframer (aisx_hdlc_batch_*) at the benchmark's shape, 4096 channels x 65536 samples
per step (about 16 400 bits per channel per step), on one MI355X:

  deframer_alone     the deframer's three kernels over one step's bits, hipEvents around each call, after a warm-up
  step               the pipelined stock chain (ais_demod.work_pipelined) per step, without and with the deframer
                     queued behind every step as ais_amd.hdlc_deframer_batch documents (its PDU read-back included)
  host               aisx_hdlc_work over the same bits, called directly: one thread, a pool of 16

--hw-queues N sets GPU_MAX_HW_QUEUES for this process (read by the HIP runtime at its first call); the pipelined chain
wants 8 or more.  --repair turns the deframer's single-bit repair on with ais_amd.AIS_REPAIR_RULES (the host
comparison then runs the host form with the same rules); --events MASK makes it the repair of the error events of that
mask (ais_amd.AIS_REPAIR_EVENTS = 7: all; 1, the default, is the single-bit repair and its kernel).  Writes one JSON file
(--out).
Usage: python tools/hdlc_bench.py [--nchan 4096] [--calls 50] [--steps 20] [--hw-queues 8] [--repair [--events 7]] --out F"""
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
    sys.exit("hdlc_bench: --hw-queues must be an integer in 1..32")
os.environ["GPU_MAX_HW_QUEUES"] = _q  # (before torch makes the first HIP call)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import ctypes as C  # noqa: E402

import ais_amd  # noqa: E402
import bench  # noqa: E402
from ais_amd import _lib  # noqa: E402
from ais_amd._lib import check  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nchan", type=int, default=4096)
    ap.add_argument("--T", type=int, default=65536)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--hw-queues", type=int, default=8)
    ap.add_argument("--repair", action="store_true")
    ap.add_argument("--events", type=int, default=1)
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    if a.events != 1 and not a.repair:
        sys.exit("hdlc_bench: --events needs --repair")
    nchan, T, sps = a.nchan, a.T, 4
    dev = torch.device("cuda", 0)
    opts = dict(samples_per_symbol=sps, bits_per_sec=9600.0, clockrec_gain=0.04, omega_relative_limit=0.01, fftlen=1024)
    tmpl = ais_amd.modulate_vector_bc(ais_amd.gmsk_mod(sps, 0.4), [1, 1, 0, 0] * 7, [1])
    xs = [bench.make_input(nchan, T, "S", sps, dev, r, True) for r in range(2)]
    dem = ais_amd.ais_demod(opts, nchan=nchan, max_items=T, stages="stock", preamble_symbols=tmpl)
    cap = dem.clockrec.out_capacity
    hd = ais_amd.hdlc_deframer_batch(11, 64, nchan, cap, 1 << 17)
    if a.repair:
        hd.set_repair(ais_amd.AIS_REPAIR_RULES, *([a.events] if a.events != 1 else []))
    rules = ais_amd.framing.repair_rules(ais_amd.AIS_REPAIR_RULES if a.repair else None)
    s = torch.cuda.Stream()
    res = {"shape": dict(nchan=nchan, T=T, length_min=11, length_max=64, max_bits=cap), "device": torch.cuda.get_device_name(0),
           "gpu_max_hw_queues": int(os.environ["GPU_MAX_HW_QUEUES"]), "repair": bool(a.repair), "events": a.events}

    def steps(n, deframe):
        n += n % 2  # (x_next alternates between the two inputs: every run ends where the next one starts)
        prev = False
        pdus = 0
        for k in range(n):
            r = dem.work_pipelined(xs[k % 2], x_next=xs[(k + 1) % 2])
            if deframe:
                if prev:
                    pdus += len(hd.pdus(stream=s)[0])
                dem.wait(r["step"], stream=s)
                hd.work(r["bits"], r["produced"], stream=s)
                prev = True
        if deframe and prev:
            pdus += len(hd.pdus(stream=s)[0])
        dem.synchronize()
        return r, pdus

    # chain-like bits: one step's output (the chain warmed up on the way)
    r, _ = steps(a.warmup + 2, False)
    bits, prod = r["bits"].clone(), r["produced"].clone()
    torch.cuda.synchronize()
    nb = prod.cpu().numpy()
    res["bits_per_step"] = dict(total=int(nb.sum()), per_channel_mean=float(nb.mean()))

    # the deframer alone
    for _ in range(a.warmup):
        hd.work(bits, prod, stream=s)
    s.synchronize()
    ms = []
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.calls)]
    for e0, e1 in ev:
        e0.record(s)
        hd.work(bits, prod, stream=s)
        e1.record(s)
    s.synchronize()
    ms = sorted(e0.elapsed_time(e1) for e0, e1 in ev)
    recs, _, fix = hd.pdus(stream=s, with_repairs=True)
    res["deframer_alone_ms"] = dict(median=ms[len(ms) // 2], min=ms[0], max=ms[-1], calls=a.calls,
                                    pdus_per_call=int(len(recs)), repaired_per_call=int((fix >= 0).sum()),
                                    repaired_by_event=[int(((fix >= 0) & (fix >> 16 == e)).sum()) for e in range(3)])
    res["deframer_alone_gbit_s"] = res["bits_per_step"]["total"] / (res["deframer_alone_ms"]["median"] * 1e-3) / 1e9

    # the pipelined step without / with the deframer behind it (alternating runs, each after a warm-up)
    per = {False: [], True: []}
    npdus = 0
    for rep in range(3):
        for deframe in (False, True):
            steps(a.warmup, deframe)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            _, p = steps(a.steps, deframe)
            per[deframe].append((time.perf_counter() - t0) * 1e3 / a.steps)
            npdus = max(npdus, p)
    res["step_ms"] = dict(without=sorted(per[False]), with_deframer=sorted(per[True]), steps=a.steps,
                          pdus_in_run=npdus)
    res["step_cost_ms"] = float(np.median(per[True]) - np.median(per[False]))

    # the host deframer over the same bits: aisx_hdlc_work called directly (buffers allocated once per worker,
    # a fresh handle per channel; ctypes lets go of the interpreter lock for the call), one thread and 16
    hb = bits.cpu().numpy()
    rows = [np.ascontiguousarray(hb[c, : nb[c]]) for c in range(nchan)]
    L = _lib.lib()
    maxp = int(nb.max()) // 16 + 2

    def host(chans):
        buf = np.zeros(maxp * 66, dtype=np.uint8)
        offs = np.zeros(maxp + 1, dtype=np.int32)
        n, h, found = C.c_int(0), C.c_void_p(), 0
        for c in chans:
            check(L.aisx_hdlc_create(C.byref(h), 11, 64), "aisx_hdlc_create")
            if a.events != 1:
                check(L.aisx_hdlc_set_repair_events(h, rules.ctypes.data_as(C.c_void_p), rules.size, a.events), "aisx_hdlc_set_repair_events")
            else:
                check(L.aisx_hdlc_set_repair(h, rules.ctypes.data_as(C.c_void_p) if rules.size else None, rules.size), "aisx_hdlc_set_repair")
            rc = L.aisx_hdlc_work(h, rows[c].ctypes.data_as(C.c_void_p), int(nb[c]), buf.ctypes.data_as(C.c_void_p),
                                  buf.size, offs.ctypes.data_as(C.c_void_p), maxp, C.byref(n))
            L.aisx_hdlc_destroy(h)
            check(rc, "aisx_hdlc_work")
            found += n.value
        return found

    t0 = time.perf_counter()
    found1 = host(range(nchan))
    one = time.perf_counter() - t0
    with cf.ThreadPoolExecutor(max_workers=16) as ex:
        t0 = time.perf_counter()
        found16 = sum(ex.map(host, [range(k, nchan, 16) for k in range(16)]))
        pool = time.perf_counter() - t0
    assert found1 == found16
    res["host"] = dict(one_thread_ms=one * 1e3, one_thread_mbit_s=nb.sum() / one / 1e6, pool16_ms=pool * 1e3,
                       pool16_mbit_s=nb.sum() / pool / 1e6, pdus=found1,
                       note="aisx_hdlc_work through ctypes, buffers reused; the copy of the bits to the host is not counted")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
