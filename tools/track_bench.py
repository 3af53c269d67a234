"""Cost of the vessel table in device memory (aisx_track_batch_*) at the benchmark's shape, 4096 channels x 65536 samples
per step, behind the batched HDLC deframer and the field decoder, on one MI355X:

  update        the six kernels of one update over one step's decoded rows (the bench's PDU list), hipEvents around each
                call, after a warm-up: the steady state (every MMSI known) and the first call on an empty table
  one_mmsi      the same rows with one MMSI in every row (one ship heard by every receiver: the contention worst case)
  distinct      the same rows with a different MMSI in every row, on an empty table and again once they are known
  expire        a table of 2^20 vessels: an expire that removes none, and one that removes half
  step          the pipelined stock chain (ais_demod.work_pipelined) per step with the deframer and the decoder behind
                every step and (a) nothing read back but the counts, (b) the whole per-PDU table copied to the host,
                (c) the update and the changed vessels' rows read back; the three alternate in one process

--hw-queues N sets GPU_MAX_HW_QUEUES for this process (read by the HIP runtime at its first call); the pipelined chain
wants 8 or more.  Writes one JSON file (--out).
Usage: python tools/track_bench.py [--nchan 4096] [--calls 50] [--steps 20] [--hw-queues 8] --out F"""
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
    sys.exit("track_bench: --hw-queues must be an integer in 1..32")
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
    ap.add_argument("--capacity", type=int, default=1 << 20)
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
    hd = ais_amd.hdlc_deframer_batch(11, 64, nchan, cap, max_pdus)
    md = ais_amd.pdu_decode_batch(nchan, max_pdus, 64)
    vt = ais_amd.vessel_table_batch(a.capacity, max_pdus)
    s = torch.cuda.Stream()
    res = {"shape": dict(nchan=nchan, T=T, length_min=11, length_max=64, max_pdus=max_pdus, capacity=a.capacity),
           "device": torch.cuda.get_device_name(0), "gpu_max_hw_queues": int(os.environ["GPU_MAX_HW_QUEUES"])}
    stamp = [0]

    def steps(n, mode):
        n += n % 2  # (x_next alternates between the two inputs: every run ends where the next one starts)
        prev = False
        rows = 0

        def read():
            if mode == "table":
                return len(md.messages(stream=s))
            if mode == "track":
                return len(vt.changed_arrays(stream=s)[0])
            return len(md.columns(stream=s)["TYPE"])  # (the counts only)

        for k in range(n):
            r = dem.work_pipelined(xs[k % 2], x_next=xs[(k + 1) % 2])
            if prev:
                rows += read()
            dem.wait(r["step"], stream=s)
            hd.work(r["bits"], r["produced"], stream=s)
            md.work(hd, stream=s)
            if mode == "track":
                stamp[0] += 1
                vt.work(md, stamp[0], stream=s, deframer=hd)
            prev = True
        rows += read()
        dem.synchronize()
        return r, rows

    def timed(call, calls, before=None):
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(calls)]
        for e0, e1 in ev:
            if before:
                before()
            e0.record(s)
            call()
            e1.record(s)
        s.synchronize()
        ms = sorted(e0.elapsed_time(e1) for e0, e1 in ev)
        return dict(median=ms[len(ms) // 2], min=ms[0], max=ms[-1], calls=calls)

    # chain-like rows: one step's output deframed and decoded (the chain warmed up on the way)
    steps(a.warmup + 2, "none")
    torch.cuda.synchronize()
    table = md.messages(stream=s)
    nrows = len(table)
    c, stride, sp, n = md.results_device()
    pdus = hd.results_device()[0]

    def update(cols_ptr=c):
        stamp[0] += 1
        vt.work_device(cols_ptr, stride, sp, n + 4, stamp[0], pdus, stream=s)

    def empty():
        s.synchronize()
        vt.reset()

    res["rows_per_call"] = nrows
    res["distinct_mmsi_in_rows"] = int(len(np.unique(table["mmsi"])))
    first = timed(update, 5, before=empty)
    for _ in range(a.warmup):
        update()
    u1 = timed(update, a.calls)
    u2 = timed(update, a.calls)
    cnt = vt.get_counts(stream=s)
    res["update_ms"] = dict(u1 if u1["median"] <= u2["median"] else u2, runs=[u1["median"], u2["median"]], on_empty_table=first, counts=cnt)
    # the same rows with the MMSI column replaced (a copy of the decoder's columns: the stride stays)
    cols_view = md._views()[0]
    for name, mmsi in (("one_mmsi", torch.full((max_pdus,), 366123456, dtype=torch.int32, device=dev)),
                       ("distinct", torch.arange(1000, 1000 + max_pdus, dtype=torch.int32, device=dev))):
        alt = cols_view.clone()
        alt[ais_amd.MSG_COLUMNS.index("MMSI")] = mmsi
        torch.cuda.synchronize()
        on_empty = timed(lambda: update(alt.data_ptr()), 5, before=empty)
        for _ in range(a.warmup):
            update(alt.data_ptr())
        known = timed(lambda: update(alt.data_ptr()), a.calls)
        res[name + "_ms"] = dict(known, on_empty_table=on_empty, counts=vt.get_counts(stream=s))
        del alt
    # expire on a table of `capacity` vessels: filled max_pdus distinct MMSIs at a time, the stamp rising with the call
    empty()
    alt = cols_view.clone()
    alt[ais_amd.MSG_COLUMNS.index("FLAGS")] = 1  # (rows beyond the step's count were never written: make them all valid)
    fills = (a.capacity + max_pdus - 1) // max_pdus
    full_n = torch.tensor([max_pdus], dtype=torch.int32, device=dev)
    for k in range(fills):
        alt[ais_amd.MSG_COLUMNS.index("MMSI")] = torch.arange(k * max_pdus, (k + 1) * max_pdus, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        vt.work_device(alt.data_ptr(), stride, sp, full_n.data_ptr(), k, None, stream=s)
        s.synchronize()
    filled = vt.get_counts(stream=s)["vessels"]
    keep_all = timed(lambda: vt.expire(0, stream=s), 5)
    half = timed(lambda: vt.expire(fills // 2, stream=s), 1)
    res["expire_ms"] = dict(vessels=filled, removes_none=keep_all, removes_half=half, left=vt.get_counts(stream=s)["vessels"])
    del alt
    empty()

    # the pipelined step: counts only / whole-table copy / update + changed rows (alternating runs)
    per = {"none": [], "table": [], "track": []}
    rows = dict.fromkeys(per, 0)
    for rep in range(3):
        for mode in per:
            steps(a.warmup, mode)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            _, p = steps(a.steps, mode)
            per[mode].append((time.perf_counter() - t0) * 1e3 / a.steps)
            rows[mode] = max(rows[mode], p)
    res["step_ms"] = dict(decoder_only=sorted(per["none"]), decoder_table_copy=sorted(per["table"]),
                          decoder_update_changed=sorted(per["track"]), steps=a.steps, rows_read=rows,
                          vessels=vt.get_counts(stream=s)["vessels"])
    base = float(np.median(per["none"]))
    res["step_cost_ms"] = dict(table_copy=float(np.median(per["table"])) - base, update_changed=float(np.median(per["track"])) - base)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
