"""Cost of the host-fed receiver (ais_amd.ais_rx, aisx_rx_*) and of the filter's sample formats on one MI355X, at the
stock ais_rx shape (250 kS/s, decimation 5, 603 taps, A / B at -+25 kHz, blocks of 65 536 x 5 items per stream).

The driver (no GPU work of its own) runs every measurement as a child process under its own timeout and stops at the
first that fails:

  filter   aisx_xlate_process_fmt alone per format (median of --calls, hipEvents around each call), interleaved with
           aisx_xlate_process of another build of the library (--parent-lib: the parent commit's libaisx.so), each
           side --rounds times: the spread of the parent's own medians is the yardstick for "not slower"
  rx       per format and stream count: ms per block host-fed through slot() / submit() with pre-filled pinned slots
           (wall clock over --blocks blocks, results popped as they come), the time the host thread spent inside
           slot() and submit(), the achieved H2D rate, and the same blocks device-resident as converted fc32 through
           the hand-wired pipeline (filter one step ahead -> work_pipelined -> deframer -> NMEA);
           receivers in real time = streams x block duration / block time

The input: 8 seeded streams (tests/synth.py make_wideband) repeated, quantised on the host (cs16 2^-13, 8-bit 2^-5,
cu8 with bias 127.5).  Stream counts (--rx-streams): a pinned slot is streams x 327 680 items, three
of them are allocated; the default keeps fc32's three slots at 8 GB of pinned memory (1024 streams) and adds the
8-bit formats at the chain's default step (2048 streams, 1.34 GB per slot).
Usage: python tools/rx_bench.py --out profiles/rx_bench_q8.json [--parent-lib PATH] [--hw-queues 8]"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "gr-ais_amd"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

FS, D, T, NSEED = 250e3, 5, 65536, 8
FORMATS = ("cf32", "cs16", "cs8", "cu8")
ITEM = dict(cf32=8, cs16=4, cs8=2, cu8=2)
QUANT = dict(cf32=(1.0, 0.0), cs16=(2.0 ** -13, 0.0), cs8=(2.0 ** -5, 0.0), cu8=(2.0 ** -5, 127.5))


def seeds(nblocks):
    import numpy as np
    import synth

    made = [synth.make_wideband(900 + s, nblocks * T, [1, 9], fs=FS, nlanes=10, decim=D, group_delay=301, amp=1.0,
                                bursts_per_lane=3, cfo_max=400.0, noise_sigma=0.1, tail_frames=2000)[0] for s in range(NSEED)]
    return np.stack(made)


def quantise(x, fmt):
    import numpy as np

    if fmt == "cf32":
        return x
    scale, bias = QUANT[fmt]
    dt = dict(cs16=np.int16, cs8=np.int8, cu8=np.uint8)[fmt]
    v = np.ascontiguousarray(x).view(np.float32).reshape(x.shape[0], x.shape[1], 2)
    q = np.floor(v / np.float32(scale) + np.float32(128.0)) if fmt == "cu8" else np.rint(v / np.float32(scale))
    info = np.iinfo(dt)
    return np.clip(q, info.min, info.max).astype(dt)


def convert(raw, fmt):
    import numpy as np

    if fmt == "cf32":
        return raw
    scale, bias = QUANT[fmt]
    v = (raw.astype(np.float32) - np.float32(bias)) * np.float32(scale)
    return np.ascontiguousarray(v).view(np.complex64)[..., 0]


def child_filter(a):
    """one library, one format: the median of --calls filter calls at 2048 streams"""
    import numpy as np
    import torch

    import ais_amd  # noqa: F401  (GPU_MAX_HW_QUEUES)
    from ais_amd.blocks import firdes_low_pass

    L = C.CDLL(a.lib)  # (after torch: one HIP runtime)
    vp, i32, lng, f64, f32 = C.c_void_p, C.c_int, C.c_long, C.c_double, C.c_float
    L.aisx_xlate_create.argtypes = [C.POINTER(vp), i32, vp, i32, vp, i32, f64, i32, i32]
    L.aisx_xlate_process.argtypes = [vp, vp, lng, i32, vp, lng, C.POINTER(i32), vp]
    L.aisx_xlate_destroy.argtypes = [vp]
    ns = a.streams
    taps = firdes_low_pass(1.0, FS, 11e3, 1e3)
    fr = np.ascontiguousarray(np.broadcast_to(np.array([[-25e3, 25e3]]), (ns, 2)))
    h = vp()
    assert L.aisx_xlate_create(C.byref(h), D, taps.ctypes.data, taps.size, fr.ctypes.data, 2, FS, ns, T * D) == 0
    raw = quantise(seeds(1)[:, :T * D], a.fmt)
    x = torch.as_tensor(raw).cuda().repeat(*((ns // NSEED, 1) + ((1,) if a.fmt != "cf32" else ()))).contiguous()
    out = torch.empty((2 * ns, T), dtype=torch.complex64, device="cuda")
    s = torch.cuda.Stream()
    sp = vp(s.cuda_stream)
    n = i32(0)
    if a.fmt == "cf32" and not a.use_fmt_entry:
        def call():
            return L.aisx_xlate_process(h, x.data_ptr(), T * D, T * D, out.data_ptr(), T, C.byref(n), sp)
    else:
        L.aisx_xlate_process_fmt.argtypes = [vp, vp, i32, f32, f32, lng, i32, vp, lng, C.POINTER(i32), vp]
        scale, bias = QUANT[a.fmt]

        def call():
            return L.aisx_xlate_process_fmt(h, x.data_ptr(), FORMATS.index(a.fmt), scale, bias, T * D, T * D, out.data_ptr(), T,
                                            C.byref(n), sp)
    for _ in range(a.warmup):
        assert call() == 0
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.calls)]
    for e0, e1 in ev:
        e0.record(s)
        assert call() == 0
        e1.record(s)
    s.synchronize()
    ms = sorted(e0.elapsed_time(e1) for e0, e1 in ev)
    L.aisx_xlate_destroy(h)
    print("RESULT " + json.dumps(dict(median=ms[len(ms) // 2], min=ms[0], max=ms[-1], calls=a.calls,
                                      read_GB=ns * T * D * ITEM[a.fmt] * 1e-9)))


def child_rx(a):
    import numpy as np
    import torch

    import ais_amd
    import synth
    from ais_amd import _lib

    ns, fmt = a.streams, a.fmt
    scale, bias = QUANT[fmt]
    sps = FS / D / 9600.0
    tmpl = synth.resampled_template(ais_amd.modulate_vector_bc(ais_amd.gmsk_mod(40, 0.4), [1, 1, 0, 0] * 7, [1]), 40, sps)
    raw = quantise(seeds(2), fmt)
    reps = ns // NSEED
    blocks = [np.ascontiguousarray(raw[:, k * T * D:(k + 1) * T * D]) for k in range(2)]
    res = dict(streams=ns, fmt=fmt, block_bytes=ns * T * D * ITEM[fmt])
    # host-fed
    t0 = time.perf_counter()
    rx = ais_amd.ais_rx((-25e3, 25e3), FS, ("A", "B"), nstreams=ns, fmt=fmt, scale=scale, bias=bias, block_items=T * D,
                        preamble_symbols=tmpl)
    res["create_s"] = time.perf_counter() - t0
    npdus = 0
    t_slot = t_sub = 0.0
    sub_max = 0.0

    def run(nblocks, fill):
        nonlocal npdus, t_slot, t_sub, sub_max
        for k in range(nblocks):
            t1 = time.perf_counter()
            sl = rx.slot()
            t2 = time.perf_counter()
            if fill:  # (the first time round the ring: afterwards the slots are full)
                sl.reshape((reps, NSEED) + sl.shape[1:])[...] = blocks[k % 2][None]
            t3 = time.perf_counter()
            rx.submit()
            t4 = time.perf_counter()
            if not fill:
                t_slot += t2 - t1
                t_sub += t4 - t3
                sub_max = max(sub_max, t4 - t3)
            while (r := rx.pop()) is not None:
                npdus += len(r[1])

    run(rx.input_slots * 2, True)  # (six blocks: every slot filled, and the warm-up)
    while rx.pop(wait=True) is not None:
        pass
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    run(a.blocks, False)
    rx.flush()
    while (r := rx.pop(wait=True)) is not None:
        npdus += len(r[1])
    dt = time.perf_counter() - t0
    ms = dt / a.blocks * 1e3
    res["host_fed"] = dict(ms_per_block=ms, blocks=a.blocks, h2d_GBps=res["block_bytes"] / ms * 1e-6,
                           receivers_real_time=ns * (T * D / FS) / (ms * 1e-3), host_ms_in_slot_per_block=t_slot / a.blocks * 1e3,
                           host_ms_in_submit_per_block=t_sub / a.blocks * 1e3, host_ms_in_submit_max=sub_max * 1e3, pdus=npdus,
                           status=rx.status)
    del rx
    torch.cuda.synchronize()
    # device-resident: the same blocks as converted fc32 through the hand-wired pipeline
    xs = [torch.as_tensor(convert(b, fmt)).cuda().repeat(reps, 1).contiguous() for b in blocks]
    nch = 2 * ns
    taps = ais_amd.firdes_low_pass(1.0, FS, 11e3, 1e3)
    xl = ais_amd.freq_xlating_fir_filter_ccf(D, taps, (-25e3, 25e3), FS, nstreams=ns, max_items=T * D)
    opts = dict(samples_per_symbol=sps, bits_per_sec=9600.0, clockrec_gain=0.04, omega_relative_limit=0.01, fftlen=1024)
    dem = ais_amd.ais_demod(opts, nchan=nch, max_items=T, stages="stock", preamble_symbols=tmpl)
    hd = ais_amd.hdlc_deframer_batch(11, 64, nch, dem.clockrec.out_capacity, 1 << 16)
    nm = ais_amd.pdu_to_nmea_batch(["A", "B"] * ns, nch, 1 << 16, 64)
    depth = _lib.lib().aisx_chain_depth()
    ring = [torch.empty((nch, T), dtype=torch.complex64, device="cuda") for _ in range(depth + 1)]
    cur, s = torch.cuda.current_stream(), torch.cuda.Stream()

    def filt(k):
        if k >= depth + 1:
            _lib.check(_lib.lib().aisx_chain_wait_input(dem._chain_handle(), k - depth - 1, C.c_void_p(cur.cuda_stream), 0), "wait_input")
        return xl.work(xs[k % 2], out=ring[k % (depth + 1)])

    def steps(k0, n, y_next):
        for k in range(k0, k0 + n):
            y = y_next
            y_next = filt(k + 1)
            r = dem.work_pipelined(y, x_next=y_next)
            if k > k0:
                nm.sentences(stream=s)
            dem.wait(r["step"], stream=s)
            hd.work(r["bits"], r["produced"], stream=s)
            nm.work(hd, stream=s)
        nm.sentences(stream=s)
        return y_next

    y_next = steps(0, 6, filt(0))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    steps(6, a.blocks, y_next)
    dem.synchronize()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / a.blocks * 1e3
    res["device_resident"] = dict(ms_per_block=ms, receivers_real_time=ns * (T * D / FS) / (ms * 1e-3))
    print("RESULT " + json.dumps(res))


def run_child(args, limit):
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__)] + args
    p = subprocess.run(cmd, capture_output=True, text=True)
    for line in p.stdout.split("\n"):
        if line.startswith("RESULT "):
            return json.loads(line[7:])
    sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
    raise SystemExit("rx_bench: %s ended with status %d: stopping" % (" ".join(args), p.returncode))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", choices=("filter", "rx"))
    ap.add_argument("--fmt", default="cf32")
    ap.add_argument("--lib", default=os.path.join(ROOT, "gr-ais_amd", "lib", "libaisx.so"))
    ap.add_argument("--use-fmt-entry", action="store_true")
    ap.add_argument("--parent-lib")
    ap.add_argument("--streams", type=int, default=2048)
    ap.add_argument("--rx-streams", type=int, default=1024)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--blocks", type=int, default=20)
    ap.add_argument("--hw-queues", type=int, default=8)
    ap.add_argument("--skip-rx", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    if not 1 <= a.hw_queues <= 32:
        sys.exit("rx_bench: --hw-queues must be in 1..32")
    os.environ["GPU_MAX_HW_QUEUES"] = str(a.hw_queues)  # (before the first HIP call of this process and its children)
    if a.child == "filter":
        return child_filter(a)
    if a.child == "rx":
        return child_rx(a)
    res = dict(shape=dict(samp_rate=FS, decim=D, ntaps=603, items_per_block=T * D, rows_per_stream=2), gpu_max_hw_queues=a.hw_queues,
               filter_alone=dict(streams=a.streams, rounds=[]), receiver=[])

    def save():
        if a.out:
            with open(a.out, "w") as f:
                json.dump(res, f, indent=1)

    common = ["--hw-queues", str(a.hw_queues), "--calls", str(a.calls), "--warmup", str(a.warmup), "--streams", str(a.streams)]
    for r in range(a.rounds):
        rnd = {}
        if a.parent_lib:
            rnd["parent_cf32"] = run_child(["--child", "filter", "--fmt", "cf32", "--lib", a.parent_lib] + common, 240)
        rnd["cf32"] = run_child(["--child", "filter", "--fmt", "cf32"] + common, 240)
        if r == 0:
            rnd["cf32_through_process_fmt"] = run_child(["--child", "filter", "--fmt", "cf32", "--use-fmt-entry"] + common, 240)
        for fmt in FORMATS[1:]:
            rnd[fmt] = run_child(["--child", "filter", "--fmt", fmt] + common, 240)
        res["filter_alone"]["rounds"].append(rnd)
        print("filter round %d: %s" % (r, {k: round(v["median"], 3) for k, v in rnd.items()}))
        save()
    fa = res["filter_alone"]
    for key in fa["rounds"][0]:
        meds = [rnd[key]["median"] for rnd in fa["rounds"] if key in rnd]
        fa[key + "_medians_ms"] = dict(min=min(meds), max=max(meds), n=len(meds))
    save()
    if not a.skip_rx:
        todo = [(fmt, a.rx_streams) for fmt in FORMATS] + [(fmt, 2048) for fmt in ("cs8", "cu8") if a.rx_streams != 2048]
        for fmt, ns in todo:
            r = run_child(["--child", "rx", "--fmt", fmt, "--streams", str(ns), "--blocks", str(a.blocks), "--hw-queues", str(a.hw_queues)], 420)
            res["receiver"].append(r)
            print("rx %s x %d: host-fed %.2f ms (%.1f GB/s), device-resident %.2f ms" % (
                fmt, ns, r["host_fed"]["ms_per_block"], r["host_fed"]["h2d_GBps"], r["device_resident"]["ms_per_block"]))
            save()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
