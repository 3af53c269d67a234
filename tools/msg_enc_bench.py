"""Cost of the batched field encoder (aisx_msg_enc_batch_*) at the benchmark's shape, 4096 channels x 65536 samples per
step, behind the deframer and the field decoder, on one MI355X:

  alone   the encoder's call (one memset of two counters and one kernel) over one step's decoded rows, hipEvents around
          each call, after a warm-up: without an index list, with one (the rows in reversed order), and beside
          aisx_msg_batch_process -- the decoder, its mirror -- on the same rows in the same run
  step    the pipelined stock chain (ais_demod.work_pipelined) per step with deframer -> decoder -> vessel table and the
          table's counts read back behind every step, against the same step with the changed vessels encoded as type 1
          on their channels, armoured in the standard form and the text read back; the two variants alternate

--hw-queues N sets GPU_MAX_HW_QUEUES for this process (read by the HIP runtime at its first call); the pipelined chain
wants 8 or more.  Writes one JSON file (--out).
Usage: python tools/msg_enc_bench.py [--nchan 4096] [--calls 50] [--steps 20] [--hw-queues 8] --out F"""
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
    sys.exit("msg_enc_bench: --hw-queues must be an integer in 1..32")
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
    max_pdus, capacity = 1 << 17, 1 << 19
    des = ["A", "B"] * (nchan // 2) + ["A"] * (nchan % 2)
    hd = ais_amd.hdlc_deframer_batch(11, 64, nchan, cap, max_pdus)
    md = ais_amd.pdu_decode_batch(nchan, max_pdus, 64)
    vt = ais_amd.vessel_table_batch(capacity, max_pdus)
    enc = ais_amd.pdu_encode_batch(nchan, max_pdus, max_pdus)    # over the decoder's rows
    chg = ais_amd.pdu_encode_batch(nchan, max_pdus, capacity)    # over the vessel table's changed list
    nm = ais_amd.pdu_to_nmea_batch(des, nchan, max_pdus, 64, standard=True)
    s = torch.cuda.Stream()
    res = {"shape": dict(nchan=nchan, T=T, length_min=11, length_max=64, max_pdus=max_pdus, capacity=capacity, designators="A / B"),
           "device": torch.cuda.get_device_name(0), "gpu_max_hw_queues": int(os.environ["GPU_MAX_HW_QUEUES"])}

    def steps(n, encode):
        n += n % 2  # (x_next alternates between the two inputs: every run ends where the next one starts)
        prev = False
        out = 0

        def read():
            if encode:
                return len(nm.sentences(stream=s)[1])
            return vt.get_counts(stream=s)["changed"]

        for k in range(n):
            r = dem.work_pipelined(xs[k % 2], x_next=xs[(k + 1) % 2])
            if prev:
                out += read()
            dem.wait(r["step"], stream=s)
            hd.work(r["bits"], r["produced"], stream=s)
            md.work(hd, stream=s)
            vt.work(md, k, stream=s, deframer=hd)
            if encode:
                chg.work(vt, as_type=1, changed_only=True, chan="table", stream=s)
                nm.work_device(*chg.results_device(), stream=s)
            prev = True
        out += read()
        dem.synchronize()
        return out

    # chain-like rows: one step's output deframed and decoded (the chain warmed up on the way)
    steps(a.warmup + 2, False)
    torch.cuda.synchronize()
    rows = len(md.messages(stream=s))
    idx = torch.arange(rows - 1, -1, -1, dtype=torch.int32, device="cuda")
    c, stride, sp, n = md.results_device()
    torch.cuda.synchronize()

    def timed(call):
        for _ in range(a.warmup):
            call()
        s.synchronize()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.calls)]
        for e0, e1 in ev:
            e0.record(s)
            call()
            e1.record(s)
        s.synchronize()
        ms = sorted(e0.elapsed_time(e1) for e0, e1 in ev)
        return dict(median=ms[len(ms) // 2], min=ms[0], max=ms[-1], calls=a.calls)

    res["alone_ms"] = dict(rows=rows)
    res["alone_ms"]["encode"] = timed(lambda: enc.work(md, stream=s))
    enc.pdus(stream=s)
    res["alone_ms"]["rows_encoded"], res["alone_ms"]["rows_refused"] = enc.counts["encoded"], enc.counts["refused"]
    res["alone_ms"]["encode_indexed"] = timed(lambda: enc.work_device(c, stride, sp, n + 4, idx.data_ptr(), stream=s))
    res["alone_ms"]["encode_as_type_1"] = timed(lambda: enc.work(md, as_type=1, stream=s))
    enc.pdus(stream=s)
    res["alone_ms"]["rows_encoded_as_type_1"] = enc.counts["encoded"]
    res["alone_ms"]["decode"] = timed(lambda: md.work(hd, stream=s))
    res["alone_ms"]["bytes_per_row"] = 4 * 37 + 48 + 56 + 24 + 4

    # the pipelined step: deframer + decoder + vessel table against the same + encoder + NMEA of the changed vessels
    per = {False: [], True: []}
    text = 0
    for rep in range(3):
        for encode in (False, True):
            vt.reset()
            steps(a.warmup, encode)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = steps(a.steps, encode)
            per[encode].append((time.perf_counter() - t0) * 1e3 / a.steps)
            if encode:
                text = max(text, out)
    res["step_ms"] = dict(decode_table=sorted(per[False]), decode_table_encode_nmea_text=sorted(per[True]), steps=a.steps,
                          text_bytes_in_run=text, changed_vessels_last_step=vt.get_counts(stream=s)["changed"])
    res["step_cost_ms"] = float(np.median(per[True]) - np.median(per[False]))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
