"""Cost of the batched NMEA parser (aisx_nmea_parse_batch_*) on one MI355X, on (a) the text the NMEA stage produces
for one step of the benchmark's shape (4096 channels x 65536 samples) and (b) that text repeated to about 256 MB:

  process      the median of --calls calls of the parser's twelve kernels, hipEvents around each call, after a warm-up
  host         aisx_nmea_parse_work over the same text, one thread
  floor        the bytes the passes must read and write (the text three times: count, index, parse; 40 bytes of line
               end, key, position and time per line; the payload characters and the octets once each) divided by the
               copy rate aisx_util_copy_GBs measures in the same run
  step         (a) only: the pipelined stock chain per step with the deframer, the NMEA stage and the text read-back
               behind every step, against the same with the parser queued behind the NMEA stage (the text's length
               handed over on the device); the two variants alternate in one process

  --kernels-only MB   no chain and no JSON: 4000 sentences of ais_amd.pdu_to_nmea (random payloads of 21, 21, 21, 53 or 20
               octets, designators A / B, seed 1) repeated to MB megabytes, parsed in one call six times -- the run to put
               under `rocprofv3 --kernel-trace --stats`, whose kernel table gives each of the twelve kernels' time
               (profiles/nmea_parse_kernel_stats.md holds the medians of such a run at 256)

--hw-queues N sets GPU_MAX_HW_QUEUES for this process; the pipelined chain wants 8 or more.  Writes one JSON file.
Usage: python tools/nmea_parse_bench.py [--nchan 4096] [--calls 50] [--steps 20] [--big-mb 256] [--hw-queues 8] --out F"""
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
    sys.exit("nmea_parse_bench: --hw-queues must be an integer in 1..32")
os.environ["GPU_MAX_HW_QUEUES"] = _q  # (before torch makes the first HIP call)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import ctypes as C  # noqa: E402

import ais_amd  # noqa: E402
from ais_amd import _lib  # noqa: E402
import bench  # noqa: E402


def timed(ps, fn, calls, warmup, s):
    for _ in range(warmup):
        fn()
    s.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(calls)]
    for e0, e1 in ev:
        e0.record(s)
        fn()
        e1.record(s)
    s.synchronize()
    ms = sorted(e0.elapsed_time(e1) for e0, e1 in ev)
    return dict(median=ms[len(ms) // 2], min=ms[0], max=ms[-1], calls=calls)


def host_ms(des, text):
    h = ais_amd.nmea_to_pdu(des, 64, ref_tail=True)
    t0 = time.perf_counter()
    recs, data, _, cnt = h.work(text)
    return (time.perf_counter() - t0) * 1e3, cnt, int(recs["len"].sum())


def floor_ms(nbytes, nlines, octets, gbs):
    traffic = 3 * nbytes + 40 * nlines + (octets * 4 + 2) // 3 + octets
    return dict(bytes=int(traffic), ms=traffic / (gbs * 1e9) * 1e3)


def kernels_only(mb):
    rng = np.random.default_rng(1)
    arm = [ais_amd.pdu_to_nmea("A"), ais_amd.pdu_to_nmea("B")]
    text = b"".join(arm[k % 2].msg_to_sentence(bytes(rng.integers(0, 256, int(rng.choice([21, 21, 21, 53, 20])), dtype=np.uint8)))
                    .encode("latin-1") + b"\n" for k in range(4000))
    big = text * max(1, (mb << 20) // len(text))
    nl = big.count(b"\n")
    ps = ais_amd.nmea_to_pdu_batch(["A", "B"], 64, len(big), nl, nl, ref_tail=True)
    d = torch.frombuffer(bytearray(big), dtype=torch.uint8).cuda()
    n = torch.tensor([len(big)], dtype=torch.int64, device="cuda")
    for _ in range(6):
        ps.work(d, n)
    torch.cuda.synchronize()
    print(json.dumps(dict(text_bytes=len(big), lines=nl, counts=ps.messages()[3])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nchan", type=int, default=4096)
    ap.add_argument("--T", type=int, default=65536)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--big-mb", type=int, default=256)
    ap.add_argument("--hw-queues", type=int, default=8)
    ap.add_argument("--kernels-only", type=int, default=0, metavar="MB")
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.kernels_only:
        return kernels_only(a.kernels_only)
    if not a.out:
        ap.error("--out is required")
    nchan, T, sps = a.nchan, a.T, 4
    dev = torch.device("cuda", 0)
    opts = dict(samples_per_symbol=sps, bits_per_sec=9600.0, clockrec_gain=0.04, omega_relative_limit=0.01, fftlen=1024)
    tmpl = ais_amd.modulate_vector_bc(ais_amd.gmsk_mod(sps, 0.4), [1, 1, 0, 0] * 7, [1])
    xs = [bench.make_input(nchan, T, "S", sps, dev, r, True) for r in range(2)]
    dem = ais_amd.ais_demod(opts, nchan=nchan, max_items=T, stages="stock", preamble_symbols=tmpl)
    cap = dem.clockrec.out_capacity
    max_pdus = 1 << 17
    des = ["A", "B"]
    hd = ais_amd.hdlc_deframer_batch(11, 64, nchan, cap, max_pdus)
    nm = ais_amd.pdu_to_nmea_batch(des * (nchan // 2) + ["A"] * (nchan % 2), nchan, max_pdus, 64)
    ps = ais_amd.nmea_to_pdu_batch(des, 64, min(nm.text_cap, 1 << 30), 2 * max_pdus, max_pdus, ref_tail=True)
    s = torch.cuda.Stream()
    gbs = C.c_float(0)
    _lib.check(_lib.lib().aisx_util_copy_GBs(1 << 28, 10, C.byref(gbs)), "copy rate")
    res = {"shape": dict(nchan=nchan, T=T, length_max=64, max_line=512, designators="A / B", ref_tail=True),
           "device": torch.cuda.get_device_name(0), "gpu_max_hw_queues": int(os.environ["GPU_MAX_HW_QUEUES"]),
           "copy_GBs": gbs.value}

    def steps(n, parse):
        n += n % 2  # (x_next alternates between the two inputs: every run ends where the next one starts)
        prev = False
        nrec = 0
        for k in range(n):
            r = dem.work_pipelined(xs[k % 2], x_next=xs[(k + 1) % 2])
            if prev:
                nrec += len(nm.sentences(stream=s)[0])
            dem.wait(r["step"], stream=s)
            hd.work(r["bits"], r["produced"], stream=s)
            nm.work(hd, stream=s)
            if parse:
                ps.work_nmea(nm, stream=s)
            prev = True
        nrec += len(nm.sentences(stream=s)[0])
        dem.synchronize()
        return nrec

    steps(a.warmup + 2, True)
    torch.cuda.synchronize()
    _, text = nm.sentences(stream=s)
    recs, data, _, cnt = ps.messages(stream=s)
    assert cnt["FOUND"] == cnt["KEPT"] > 0 and cnt["REJ_FRAGMENT"] == 0, cnt

    # (a) the step's text, parsed where the NMEA stage left it
    one = timed(ps, lambda: ps.work_nmea(nm, stream=s), a.calls, a.warmup, s)
    h_ms, h_cnt, octets = host_ms(des, text)
    assert h_cnt["FOUND"] == cnt["FOUND"] and h_cnt["LINES"] == cnt["LINES"]
    one.update(text_bytes=len(text), lines=cnt["LINES"], messages=cnt["FOUND"], host_one_thread_ms=h_ms,
               floor=floor_ms(len(text), cnt["LINES"], octets, gbs.value))
    res["step_text"] = one
    per = {False: [], True: []}
    for rep in range(3):
        for parse in (False, True):
            steps(a.warmup, parse)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            steps(a.steps, parse)
            per[parse].append((time.perf_counter() - t0) * 1e3 / a.steps)
    res["step_ms"] = dict(deframer_nmea_text=sorted(per[False]), with_parser=sorted(per[True]), steps=a.steps)
    res["step_cost_ms"] = float(np.median(per[True]) - np.median(per[False]))
    del dem, hd, nm, ps, xs
    torch.cuda.empty_cache()

    # (b) the same text repeated to about --big-mb MB, one call
    reps = max(1, (a.big_mb << 20) // len(text))
    big = text * reps
    nlines = big.count(b"\n")
    pb = ais_amd.nmea_to_pdu_batch(des, 64, len(big), nlines, nlines, ref_tail=True)
    d_big = torch.frombuffer(bytearray(big), dtype=torch.uint8).cuda()
    d_n = torch.tensor([len(big)], dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    two = timed(pb, lambda: pb.work(d_big, d_n, stream=s), a.calls, a.warmup, s)
    recs, data, _, bcnt = pb.messages(stream=s)
    h_ms, h_cnt, octets = host_ms(des, big)
    assert {k: v for k, v in h_cnt.items() if k != "KEPT"} == {k: v for k, v in bcnt.items() if k != "KEPT"}, (h_cnt, bcnt)
    two.update(text_bytes=len(big), lines=bcnt["LINES"], messages=bcnt["FOUND"], host_one_thread_ms=h_ms,
               floor=floor_ms(len(big), bcnt["LINES"], octets, gbs.value))
    res["big_text"] = two
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
