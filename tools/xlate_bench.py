"""Cost of the batched freq_xlating_fir_filter_ccf (aisx_xlate_*) at the shape that feeds the chain's default step,
2048 streams x 327 680 samples at 250 kS/s, two channels each (A / B at -+25 kHz), decimation 5, the stock 603-tap
low-pass: 4096 rows x 65 536 items per call, on one MI355X:

  alone      one call, hipEvents around it, median of --calls after a warm-up; against the packed-fma floor
             (4096 x 65 536 x 603 v_pk_fma_f32 lanes = 1.62e11 at 157 TF/s = 4.1 ms) and as bytes moved
  step       the stock receiver per pipelined step: filter one step ahead into a ring of AISX_CHAIN_DEPTH + 1 row
             buffers -> ais_demod.work_pipelined -> hdlc_deframer_batch -> pdu_to_nmea_batch with the text read back
             (INTEGRATION.md), against the same tail on rows filtered beforehand and against the chain alone; the
             variants alternate in one process.  Also as receivers x 250 kS/s in real time.
  wide       the 25 MS/s design (60 227 taps, decimation 512, centres on the 1024-lane grid) that the channelizer
             cross-check uses: 64 streams x 4 channels x 1024 outputs per call, where the plan leaves 12 of 256 lanes
             of a workgroup with work, against its own packed-fma floor
  --kernels-only   just --calls filter calls and --steps receiver steps (the run to put under rocprofv3)
  --stats F        merge a rocprofv3 --kernel-trace --stats kernel_stats.csv of a --kernels-only run into --out

The input: 8 seeded streams (tests/synth.py make_wideband: bursts on both channels, carrier offsets up to +-400 Hz, config 5's SNR)
repeated to 2048.  --hw-queues N sets GPU_MAX_HW_QUEUES for this process (the pipelined chain wants 8 or more).
Usage: python tools/xlate_bench.py [--streams 2048] [--calls 50] [--steps 20] [--hw-queues 8] --out F"""
import argparse
import csv
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
    sys.exit("xlate_bench: --hw-queues must be an integer in 1..32")
os.environ["GPU_MAX_HW_QUEUES"] = _q  # (before torch makes the first HIP call)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import ais_amd  # noqa: E402
from ais_amd import _lib  # noqa: E402

FS, D, T, NSEED = 250e3, 5, 65536, 8
FMA_FLOOR_MS = 4.1  # 4096 x 65 536 x 603 packed fmas at the 157 TF FP32 spec peak


def merge_stats(path, out):
    with open(out) as f:
        res = json.load(f)
    rows = list(csv.DictReader(open(path)))
    tot = sum(float(r["TotalDurationNs"]) for r in rows)
    kern = {r["Name"]: dict(calls=int(r["Calls"]), total_ms=float(r["TotalDurationNs"]) * 1e-6,
                            avg_ms=float(r["AverageNs"]) * 1e-6, share=float(r["TotalDurationNs"]) / tot) for r in rows}
    xl = {k: v for k, v in kern.items() if "k_xlate" in k}
    res["kernel_trace"] = dict(kernels=dict(sorted(kern.items(), key=lambda kv: -kv[1]["total_ms"])[:12]),
                               xlate=xl, xlate_share=sum(v["share"] for v in xl.values()),
                               note="rocprofv3 --kernel-trace --stats over a --kernels-only run (filter calls, then "
                                    "pipelined receiver steps); share = of all kernel time in that run")
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res["kernel_trace"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=2048)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--hw-queues", type=int, default=8)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--stats")
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.stats is not None:
        return merge_stats(a.stats, a.out)
    import synth

    ns, nch = a.streams, 2 * a.streams
    taps = ais_amd.firdes_low_pass(1.0, FS, 11e3, 1e3)
    sps = FS / D / 9600.0
    made = [synth.make_wideband(900 + s, 2 * T, [1, 9], fs=FS, nlanes=10, decim=D, group_delay=301, amp=1.0,
                                bursts_per_lane=3, cfo_max=400.0, noise_sigma=0.1, tail_frames=2000)[0] for s in range(NSEED)]
    base = torch.as_tensor(np.stack(made)).cuda()
    reps = ns // NSEED
    xs = [base[:, k * T * D:(k + 1) * T * D].repeat(reps, 1).contiguous() for k in range(2)]
    del base
    xl = ais_amd.freq_xlating_fir_filter_ccf(D, taps, (-25e3, 25e3), FS, nstreams=ns, max_items=T * D)
    s = torch.cuda.Stream()
    res = {"shape": dict(streams=ns, channels_per_stream=2, rows=nch, inputs_per_call=T * D, outputs_per_call=T, decim=D,
                         ntaps=int(taps.size), samp_rate=FS),
           "device": torch.cuda.get_device_name(0), "gpu_max_hw_queues": int(os.environ["GPU_MAX_HW_QUEUES"])}

    # the filter alone
    out = torch.empty((nch, T), dtype=torch.complex64, device="cuda")
    with torch.cuda.stream(s):
        for k in range(a.warmup):
            xl.work(xs[k % 2], out=out, stream=s)
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.calls)]
        for k, (e0, e1) in enumerate(ev):
            e0.record(s)
            xl.work(xs[k % 2], out=out, stream=s)
            e1.record(s)
    s.synchronize()
    ms = sorted(e0.elapsed_time(e1) for e0, e1 in ev)
    med = ms[len(ms) // 2]
    rd, wr = ns * T * D * 8, nch * T * 8
    res["alone_ms"] = dict(median=med, min=ms[0], max=ms[-1], calls=a.calls)
    res["alone_fraction_of_fma_floor"] = FMA_FLOOR_MS / med
    res["alone_GBps"] = (rd + wr) / med * 1e-6
    res["bytes"] = dict(read=rd, written=wr)

    # the 25 MS/s, decimation-512 design: R = 1 and a 6144-item window leave G = 12 lanes per workgroup
    wtaps = ais_amd.firdes_low_pass(1.0, 25e6, 11e3, 1e3)
    wns, wout = 64, 1024
    cen = [m * 25e6 / 1024 - (25e6 if m >= 512 else 0) for m in (3, 200, 511, 1000)]
    wx = (torch.randn((wns, 512 * wout), dtype=torch.complex64, device="cuda") * 0.3).contiguous()
    wf = ais_amd.freq_xlating_fir_filter_ccf(512, wtaps, cen, 25e6, nstreams=wns, max_items=512 * wout)
    wo = torch.empty((4 * wns, wout), dtype=torch.complex64, device="cuda")
    for _ in range(3):
        wf.work(wx, out=wo, stream=s)
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(10)]
    for e0, e1 in ev:
        e0.record(s)
        wf.work(wx, out=wo, stream=s)
        e1.record(s)
    s.synchronize()
    wms = sorted(e0.elapsed_time(e1) for e0, e1 in ev)[5]
    wfloor = 4 * wns * wout * wtaps.size * 4 / 157e12 * 1e3  # packed fmas x 4 flop at 157 TF/s, in ms
    res["wide"] = dict(streams=wns, channels=4, outputs=wout, decim=512, ntaps=int(wtaps.size), ms_median=wms,
                       floor_ms=wfloor, fraction_of_fma_floor=wfloor / wms, lanes_with_work=12)
    del wx, wo, wf

    # the receiver step
    opts = dict(samples_per_symbol=sps, bits_per_sec=9600.0, clockrec_gain=0.04, omega_relative_limit=0.01, fftlen=1024)
    tmpl = synth.resampled_template(ais_amd.modulate_vector_bc(ais_amd.gmsk_mod(40, 0.4), [1, 1, 0, 0] * 7, [1]), 40, sps)
    dem = ais_amd.ais_demod(opts, nchan=nch, max_items=T, stages="stock", preamble_symbols=tmpl)
    hd = ais_amd.hdlc_deframer_batch(11, 64, nch, dem.clockrec.out_capacity, 1 << 17)
    nm = ais_amd.pdu_to_nmea_batch(["A", "B"] * ns, nch, 1 << 17, 64)
    depth = _lib.lib().aisx_chain_depth()
    ring = [torch.empty((nch, T), dtype=torch.complex64, device="cuda") for _ in range(depth + 1)]
    pre = [xl.work(xs[k]) for k in range(2)]  # rows filtered beforehand, for the variants without the filter
    torch.cuda.synchronize()
    slot = dict(k=0, last={})  # ring position; ring slot -> the last chain step that read it

    def run(n, variant):
        """n pipelined steps (the last one with no x_next: runs are independent); variant 'chain' (the chain
        alone), 'tail' (+ deframer + NMEA + text read-back on rows filtered beforehand) or 'full' (+ the filter one
        step ahead into the ring)"""
        nbytes = 0
        h = dem._chain_handle()

        def filt():
            q = slot["k"] % (depth + 1)
            slot["k"] += 1
            if q in slot["last"]:  # refill only after the step that last read this buffer
                _lib.check(_lib.lib().aisx_chain_wait_input(h, slot["last"][q], torch.cuda.current_stream().cuda_stream, 0),
                           "wait_input")
            return q, xl.work(xs[slot["k"] % 2], out=ring[q])

        q, y = filt() if variant == "full" else (None, pre[0])
        for j in range(n):
            qn, yn = None, None
            if j + 1 < n:
                qn, yn = filt() if variant == "full" else (None, pre[(j + 1) % 2])
            r = dem.work_pipelined(y, x_next=yn)
            if q is not None:
                slot["last"][q] = r["step"]
            if variant != "chain":
                if j > 0:
                    nbytes += len(nm.sentences(stream=s)[1])
                dem.wait(r["step"], stream=s)
                hd.work(r["bits"], r["produced"], stream=s)
                nm.work(hd, stream=s)
            q, y = qn, yn
        if variant != "chain":
            nbytes += len(nm.sentences(stream=s)[1])
        dem.synchronize()
        torch.cuda.synchronize()
        return nbytes

    if a.kernels_only:
        run(a.steps, "full")
        print("kernels-only run done")
        return
    per = {"chain": [], "tail": [], "full": []}
    text = 0
    for rep in range(3):
        for v in ("chain", "tail", "full"):
            run(a.warmup, v)
            t0 = time.perf_counter()
            nb = run(a.steps, v)
            per[v].append((time.perf_counter() - t0) * 1e3 / a.steps)
            text = max(text, nb)
    med = {v: float(np.median(x)) for v, x in per.items()}
    res["step_ms"] = dict({v: sorted(x) for v, x in per.items()}, steps=a.steps, text_bytes_in_run=text)
    res["step_cost_ms"] = dict(filter=med["full"] - med["tail"], deframer_nmea_text=med["tail"] - med["chain"])
    secs = T * D / FS
    res["real_time"] = dict(seconds_of_iq_per_step=secs, receivers_full=ns * secs / (med["full"] * 1e-3),
                            receivers_chain_only=ns * secs / (med["chain"] * 1e-3),
                            note="receivers x 250 kS/s (two channels each) that one MI355X keeps up with")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
