"""Cost of the duplicate suppression in device memory (aisx_dedup_batch_*) at the benchmark's shape, 4096 channels x 65536
samples per step, behind the batched HDLC deframer, on one MI355X:

  process       the five kernels of one call over one step's PDU list (the bench's), hipEvents around each call, after a
                warm-up, in three versions -- the list as it is, every payload made distinct, every payload the same --
                and, with window 2, in two states: on a handle that remembers nothing (every first copy is kept and
                enters its set) and call after call (one call in three keeps, two find everything in the window)
  yardsticks    in the same run: the vessel table's update over the same step's decoded rows, and the NMEA stage over the
                same list
  one_mmsi      the table's worst case -- the same rows with one MMSI in every row -- against the same rows with every
                payload the same run through the suppression first (dedup + decode + update of what is kept)
  step          the pipelined stock chain (ais_demod.work_pipelined) per step with (a) deframer, NMEA, read-back and (b)
                deframer, dedup (window 0), NMEA, read-back; the two alternate in one process.  The bench's input repeats
                a few unique channels over all of them, so a known share of a step's PDUs are duplicates: the host form
                counts them (list_counts)

--plain-only measures (a) alone and needs nothing of the suppression: run from a checkout of the parent commit in the same
session, its JSON goes in with --parent-json, for the step without dedup against the parent's.
--hw-queues N sets GPU_MAX_HW_QUEUES for this process (read by the HIP runtime at its first call).
Usage: python tools/dedup_bench.py [--nchan 4096] [--calls 50] [--steps 20] [--hw-queues 8] [--parent-json F] --out F"""
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
    sys.exit("dedup_bench: --hw-queues must be an integer in 1..32")
os.environ["GPU_MAX_HW_QUEUES"] = _q  # (before torch makes the first HIP call)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import ais_amd  # noqa: E402
import bench  # noqa: E402

WINDOW = 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nchan", type=int, default=4096)
    ap.add_argument("--T", type=int, default=65536)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--hw-queues", type=int, default=8)
    ap.add_argument("--plain-only", action="store_true")
    ap.add_argument("--parent-json")
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
    nm = ais_amd.pdu_to_nmea_batch(["A", "B"] * (nchan // 2) + ["A"] * (nchan % 2), nchan, max_pdus, 64)
    dd = None if a.plain_only else ais_amd.pdu_dedup_batch(WINDOW, max_pdus, 64)
    # the step's own handle remembers nothing: the bench alternates two inputs, so any window would suppress every later
    # step whole and leave the NMEA stage idle, which live traffic (messages carry their time) does not do
    dd_step = None if a.plain_only else ais_amd.pdu_dedup_batch(0, max_pdus, 64)
    s = torch.cuda.Stream()
    res = {"shape": dict(nchan=nchan, T=T, length_min=11, length_max=64, max_pdus=max_pdus, window=WINDOW),
           "device": torch.cuda.get_device_name(0), "gpu_max_hw_queues": int(os.environ["GPU_MAX_HW_QUEUES"])}
    stamp = [0]

    def steps(n, dedup):
        n += n % 2  # (x_next alternates between the two inputs: every run ends where the next one starts)
        prev, recs = False, 0
        for k in range(n):
            r = dem.work_pipelined(xs[k % 2], x_next=xs[(k + 1) % 2])
            if prev:
                recs += len(nm.sentences(stream=s)[0])
            dem.wait(r["step"], stream=s)
            hd.work(r["bits"], r["produced"], stream=s)
            if dedup:
                stamp[0] += 1
                dd_step.work(hd, stamp[0], stream=s)
            nm.work(dd_step if dedup else hd, stream=s)
            prev = True
        recs += len(nm.sentences(stream=s)[0])
        dem.synchronize()
        return recs

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

    def step_runs(modes):
        per = {m: [] for m in modes}
        recs = dict.fromkeys(modes, 0)
        for rep in range(3):
            for m in modes:
                steps(a.warmup, m == "dedup")
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                n = steps(a.steps, m == "dedup")
                per[m].append((time.perf_counter() - t0) * 1e3 / (a.steps + a.steps % 2))
                recs[m] = n
        return per, recs

    steps(a.warmup + 2, False)  # the chain warmed up; the deframer holds one step's PDU list
    torch.cuda.synchronize()
    if a.plain_only:
        per, recs = step_runs(["plain"])
        res["step_ms"] = dict(deframer_nmea=sorted(per["plain"]), steps=a.steps, records_read=recs)
        _write(a.out, res)
        return

    md = ais_amd.pdu_decode_batch(nchan, max_pdus, 64)
    vt = ais_amd.vessel_table_batch(1 << 20, max_pdus)
    recs, data = hd.pdus(stream=s)
    n = len(recs)
    host = ais_amd.pdu_dedup(WINDOW)
    host.work_records(recs, data, 0)
    res["records_per_call"] = n
    res["list_counts"] = dict(host.counts, duplicate_share=1.0 - host.counts["kept"] / max(n, 1))

    # the three versions of the list, packed one payload behind the other
    def version(kind):
        r = recs.copy()
        if kind == "same":
            r["len"] = recs["len"][0]
            r["offset"] = recs["offset"][0]
            return r, data
        ln = recs["len"].astype(np.int64)
        r["offset"] = np.concatenate([[0], np.cumsum(ln)[:-1]])
        out = np.zeros(int(ln.sum()) + 8, dtype=np.uint8)
        for k in range(n):  # (n is a few ten thousand)
            out[r["offset"][k]:r["offset"][k] + ln[k]] = data[recs["offset"][k]:recs["offset"][k] + ln[k]]
            out[r["offset"][k]:r["offset"][k] + 4] = np.frombuffer(np.uint32(k).tobytes(), dtype=np.uint8)  # (len >= 11)
        return r, out

    pdus_ptr, bytes_ptr, count_ptr = hd.results_device()
    lists = {"as_it_is": (pdus_ptr, bytes_ptr, count_ptr + 4, None)}
    for kind in ("distinct", "same"):
        r, d = version(kind)
        t = (torch.from_numpy(r.view(np.uint8).copy()).to(dev), torch.from_numpy(np.ascontiguousarray(d)).to(dev),
             torch.tensor([n], dtype=torch.int32, device=dev))
        lists[kind] = (t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), t)
    torch.cuda.synchronize()

    def process(which):
        p, b, c, _ = lists[which]
        stamp[0] += 1
        dd.work_device(p, b, c, None, stamp[0], None, stream=s)

    def fresh():
        s.synchronize()
        dd.reset()

    res["process_ms"] = {}
    for which in lists:
        for _ in range(a.warmup):
            process(which)
        on_fresh = timed(lambda: process(which), a.calls, before=fresh)
        cnt_fresh = dd.get_counts(stream=s)
        fresh()
        calls = a.calls + (-a.calls) % (WINDOW + 1)  # (whole cycles of one keeping call and `window` suppressing ones)
        repeated = timed(lambda: process(which), calls)
        res["process_ms"][which] = dict(fresh_handle=on_fresh, counts_fresh=cnt_fresh, repeated=repeated,
                                        counts_last_repeated=dd.get_counts(stream=s))

    # the yardsticks, in the same run: the NMEA stage over the list, the table's update over its decoded rows
    res["nmea_ms"] = timed(lambda: nm.work(hd, stream=s), a.calls)
    md.work(hd, stream=s)
    c, stride, sp, cn = md.results_device()

    def update(cols_ptr=c, nrows_ptr=cn + 4, pdus=pdus_ptr):
        stamp[0] += 1
        vt.work_device(cols_ptr, stride, sp, nrows_ptr, stamp[0], pdus, stream=s)

    for _ in range(a.warmup):
        update()
    res["track_update_ms"] = dict(timed(update, a.calls), counts=vt.get_counts(stream=s))

    # the table's worst case: one MMSI in every row -- and the same rows behind the suppression (every payload the same)
    cols_view = md._views()[0]
    alt = cols_view.clone()
    alt[ais_amd.MSG_COLUMNS.index("MMSI")] = torch.full((max_pdus,), 366123456, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    for _ in range(a.warmup):
        update(alt.data_ptr())
    res["one_mmsi_ms"] = dict(update_alone=timed(lambda: update(alt.data_ptr()), a.calls), counts=vt.get_counts(stream=s))

    def deduped():
        stamp[0] += 1
        fresh_stamp = stamp[0]
        dd.work_device(lists["same"][0], lists["same"][1], lists["same"][2], None, fresh_stamp, None, stream=s)
        md.work(dd, stream=s)
        c2, stride2, sp2, cn2 = md.results_device()
        vt.work_device(c2, stride2, sp2, cn2 + 4, fresh_stamp, dd.results_device()[0], stream=s)

    fresh()
    for _ in range(a.warmup):
        fresh()
        deduped()
    res["one_mmsi_ms"]["dedup_decode_update"] = timed(deduped, a.calls, before=fresh)
    res["one_mmsi_ms"]["counts_behind_dedup"] = vt.get_counts(stream=s)
    del alt

    # the pipelined step with and without the suppression (alternating runs)
    fresh()
    per, nrecs = step_runs(["plain", "dedup"])
    res["step_ms"] = dict(deframer_nmea=sorted(per["plain"]), deframer_dedup_nmea=sorted(per["dedup"]), steps=a.steps,
                          records_read=nrecs)
    res["step_cost_ms"] = dict(dedup=float(np.median(per["dedup"])) - float(np.median(per["plain"])))
    if a.parent_json:
        with open(a.parent_json) as f:
            res["parent_step_ms"] = json.load(f)["step_ms"]
    _write(a.out, res)


def _write(path, res):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
