"""Cost of the standard NMEA form (aisx_nmea_batch_create_std) against the reference form (aisx_nmea_batch_create) at
the benchmark's shape, 4096 channels x 65536 samples per step, behind the batched HDLC deframer, on one MI355X:

  alone    one handle of each form over one step's PDUs, the calls alternated one by one in one process, hipEvents
           around each; the median of --calls calls each, the text bytes each writes and the two ratios
  step     the pipelined stock chain (ais_demod.work_pipelined) per step with the deframer, the NMEA stage of one form
           and its text read-back behind every step; the two forms alternate in one process
  parent   with --parent-lib (the parent commit's libaisx.so): the reference-form call of that build and of this one on
           the same PDUs, in child processes that alternate (which goes first alternates too), --rounds times: the
           spread of the parent's own medians is the yardstick for "the default form is no slower"

--hw-queues N sets GPU_MAX_HW_QUEUES for this process and its children (read by the HIP runtime at its first call).
Usage: python tools/nmea_std_bench.py --out profiles/nmea_std_bench_q8.json [--parent-lib PATH] [--hw-queues 8]"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "gr-ais_amd"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

STATION, TIME = "rx-station-01", 1700000000  # a 13-byte station and a 10-digit time: a 33-byte tag block


def child(a):
    """one library, the reference form: the median of --calls calls over the PDUs of --pdus"""
    import numpy as np
    import torch

    import ais_amd  # noqa: F401  (GPU_MAX_HW_QUEUES)

    L = C.CDLL(a.lib)  # (after torch: one HIP runtime)
    vp, i32, lng = C.c_void_p, C.c_int, C.c_long
    L.aisx_nmea_batch_create.argtypes = [C.POINTER(vp), C.POINTER(C.c_char_p), i32, i32, i32, lng]
    L.aisx_nmea_batch_process.argtypes = [vp, vp, vp, vp, vp, vp]
    L.aisx_nmea_batch_destroy.argtypes = [vp]
    z = np.load(a.pdus)
    recs, data, nchan = z["recs"], z["data"], int(z["nchan"])
    des = (C.c_char_p * nchan)(*[b"AB"[c % 2:c % 2 + 1] for c in range(nchan)])
    h = vp()
    assert L.aisx_nmea_batch_create(C.byref(h), des, nchan, 1 << 17, 64, 0) == 0
    d_recs, d_data = torch.from_numpy(recs.view(np.uint8).copy()).cuda(), torch.from_numpy(data).cuda()
    d_n = torch.tensor([len(recs)], dtype=torch.int32, device="cuda")
    s = torch.cuda.Stream()
    torch.cuda.synchronize()

    def call():
        return L.aisx_nmea_batch_process(h, d_recs.data_ptr(), d_data.data_ptr(), d_n.data_ptr(), None, vp(s.cuda_stream))

    for _ in range(a.warmup):
        assert call() == 0
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.calls)]
    for e0, e1 in ev:
        e0.record(s)
        assert call() == 0
        e1.record(s)
    s.synchronize()
    ms = sorted(e0.elapsed_time(e1) for e0, e1 in ev)
    L.aisx_nmea_batch_destroy(h)
    print("RESULT " + json.dumps(dict(median=ms[len(ms) // 2], min=ms[0], max=ms[-1], calls=a.calls, pdus=len(recs))))


def run_child(args, limit):
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__)] + args
    p = subprocess.run(cmd, capture_output=True, text=True)
    for line in p.stdout.split("\n"):
        if line.startswith("RESULT "):
            return json.loads(line[7:])
    sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
    raise SystemExit("nmea_std_bench: %s ended with status %d: stopping" % (" ".join(args), p.returncode))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--lib", default=os.path.join(ROOT, "gr-ais_amd", "lib", "libaisx.so"))
    ap.add_argument("--pdus")
    ap.add_argument("--parent-lib")
    ap.add_argument("--nchan", type=int, default=4096)
    ap.add_argument("--T", type=int, default=65536)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--hw-queues", type=int, default=8)
    ap.add_argument("--out")
    a = ap.parse_args()
    if not 1 <= a.hw_queues <= 32:
        sys.exit("nmea_std_bench: --hw-queues must be in 1..32")
    os.environ["GPU_MAX_HW_QUEUES"] = str(a.hw_queues)  # (before the first HIP call of this process and its children)
    if a.child:
        return child(a)

    import numpy as np
    import torch

    import ais_amd
    import bench

    nchan, T, sps = a.nchan, a.T, 4
    dev = torch.device("cuda", 0)
    opts = dict(samples_per_symbol=sps, bits_per_sec=9600.0, clockrec_gain=0.04, omega_relative_limit=0.01, fftlen=1024)
    tmpl = ais_amd.modulate_vector_bc(ais_amd.gmsk_mod(sps, 0.4), [1, 1, 0, 0] * 7, [1])
    xs = [bench.make_input(nchan, T, "S", sps, dev, r, True) for r in range(2)]
    dem = ais_amd.ais_demod(opts, nchan=nchan, max_items=T, stages="stock", preamble_symbols=tmpl)
    max_pdus = 1 << 17
    des = ["A", "B"] * (nchan // 2) + ["A"] * (nchan % 2)
    hd = ais_amd.hdlc_deframer_batch(11, 64, nchan, dem.clockrec.out_capacity, max_pdus)
    forms = dict(reference=ais_amd.pdu_to_nmea_batch(des, nchan, max_pdus, 64),
                 standard=ais_amd.pdu_to_nmea_batch(des, nchan, max_pdus, 64, standard=True, stations=STATION))
    forms["standard"].set_time(TIME)
    s = torch.cuda.Stream()
    res = {"shape": dict(nchan=nchan, T=T, length_min=11, length_max=64, max_pdus=max_pdus, designators="A / B", station=STATION,
                         time=TIME),
           "device": torch.cuda.get_device_name(0), "gpu_max_hw_queues": a.hw_queues}

    def save():
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                json.dump(res, f, indent=1)

    def steps(n, nm):
        n += n % 2  # (x_next alternates between the two inputs: every run ends where the next one starts)
        prev, pdus = False, 0
        for k in range(n):
            r = dem.work_pipelined(xs[k % 2], x_next=xs[(k + 1) % 2])
            if prev:
                pdus += len(nm.sentences(stream=s)[0])
            dem.wait(r["step"], stream=s)
            hd.work(r["bits"], r["produced"], stream=s)
            nm.work(hd, stream=s)
            prev = True
        pdus += len(nm.sentences(stream=s)[0])
        dem.synchronize()
        return pdus

    # chain-like PDUs: one step's output deframed (the chain warmed up on the way)
    steps(a.warmup + 2, forms["reference"])
    torch.cuda.synchronize()
    recs, data = hd.pdus(stream=s)

    # one handle of each form over the deframer's last results, the calls alternated one by one
    for _ in range(a.warmup):
        for nm in forms.values():
            nm.work(hd, stream=s)
    s.synchronize()
    ev = {k: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.calls)] for k in forms}
    for i in range(a.calls):
        for k, nm in forms.items():
            ev[k][i][0].record(s)
            nm.work(hd, stream=s)
            ev[k][i][1].record(s)
    s.synchronize()
    alone = {}
    for k, nm in forms.items():
        ms = sorted(e0.elapsed_time(e1) for e0, e1 in ev[k])
        r, text = nm.sentences(stream=s)
        alone[k] = dict(median=ms[len(ms) // 2], min=ms[0], max=ms[-1], calls=a.calls, pdus_per_call=int(len(r)),
                        text_bytes_per_call=len(text), payload_bytes_per_call=int(r.size and recs["len"][: len(r)].sum()))
    alone["time_ratio"] = alone["standard"]["median"] / alone["reference"]["median"]
    alone["text_bytes_ratio"] = alone["standard"]["text_bytes_per_call"] / alone["reference"]["text_bytes_per_call"]
    res["alone_ms"] = alone
    print("alone: reference %.4f ms, standard %.4f ms (x %.3f), text bytes x %.3f" % (
        alone["reference"]["median"], alone["standard"]["median"], alone["time_ratio"], alone["text_bytes_ratio"]))
    save()

    # the pipelined step with each form behind the deframer (alternating runs)
    per = {k: [] for k in forms}
    for rep in range(3):
        for k, nm in forms.items():
            steps(a.warmup, nm)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            steps(a.steps, nm)
            per[k].append((time.perf_counter() - t0) * 1e3 / (a.steps + a.steps % 2))
    res["step_ms"] = dict({k: sorted(v) for k, v in per.items()}, steps=a.steps,
                          standard_minus_reference=float(np.median(per["standard"]) - np.median(per["reference"])))
    print("step: reference %s, standard %s" % ([round(v, 3) for v in sorted(per["reference"])], [round(v, 3) for v in sorted(per["standard"])]))
    save()

    # the reference-form call of the parent build and of this one, in alternating child processes
    if a.parent_lib:
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, "pdus.npz")
            np.savez(path, recs=recs, data=data, nchan=nchan)
            common = ["--child", "--pdus", path, "--calls", str(a.calls), "--warmup", str(a.warmup), "--hw-queues", str(a.hw_queues)]
            rounds = []
            for r in range(a.rounds):
                rnd = {}
                for k in (("parent", "this"), ("this", "parent"))[r % 2]:  # (which build goes first alternates too)
                    rnd[k] = run_child(common + ["--lib", a.parent_lib if k == "parent" else a.lib], 240)
                rounds.append(rnd)
                print("parent round %d: parent %.4f ms, this %.4f ms" % (r, rounds[-1]["parent"]["median"], rounds[-1]["this"]["median"]))
        pm, tm = [x["parent"]["median"] for x in rounds], [x["this"]["median"] for x in rounds]
        res["reference_form_against_parent"] = dict(rounds=rounds, parent_medians_ms=dict(min=min(pm), max=max(pm)),
                                                    this_medians_ms=dict(min=min(tm), max=max(tm)))
    else:
        res["reference_form_against_parent"] = "not measured: no --parent-lib given"
    save()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
