"""Cost of the batched burst transmitter (aisx_tx_batch_*) at the benchmark's shape, 4096 channels x 65536 samples at
5 samples per symbol, with synth.make_channel's occupancy (320-symbol slots, each occupied with probability 0.5 by one
burst of 21 octets), on one MI355X:

  render        k_tx_render over the whole window, hipEvents around each call, median of --calls after a warm-up
  empty         the same with an empty schedule (pure zero fill)
  accumulate    the same onto a tensor that holds a noise floor (reads and writes the tiles bursts touch)
  set_bursts    aisx_tx_batch_set_bursts for that schedule: host check and sort, upload, k_tx_frame, to the end of the
                kernel (wall clock: the call synchronises its stream for the upload)
  copy_GBs      aisx_util_copy_GBs in the same process: the write ceiling the render is reported against, as
                bytes written per second / (copy_GBs / 2) -- a copy moves every byte twice

Writes one JSON file (--out).  Usage: python tools/tx_bench.py [--nchan 4096] [--T 65536] [--calls 50] --out F"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "gr-ais_amd"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import ais_amd  # noqa: E402
from ais_amd import _lib  # noqa: E402


def schedule(nchan, T, sps, seed=1):
    """BURST_DTYPE array + bytes: per channel and slot of 320 symbols one 21-octet burst with probability 0.5"""
    rng = np.random.default_rng(seed)
    slot, dur, nb = int(320 * sps), int(np.ceil(276 * sps)) + 1, 21  # (276 symbols: 21 octets with every stuffed bit)
    nslots = T // slot
    occ = rng.random((nchan, nslots)) < 0.5
    c, s = np.nonzero(occ)
    n = c.size
    b = np.zeros(n, dtype=ais_amd.BURST_DTYPE)
    b["chan"], b["len"], b["offset"] = c, nb, np.arange(n) * nb
    b["start"] = s * slot + rng.integers(0, slot - dur, n)
    b["frac"] = np.minimum(rng.random(n).astype(np.float32), np.float32(0.99999))
    b["amp"] = 1.0
    b["cfo"] = rng.uniform(-500.0, 500.0, n) / (9600.0 * sps)
    b["phase"] = rng.uniform(-np.pi, np.pi, n)
    return b, rng.integers(0, 256, n * nb, dtype=np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nchan", type=int, default=4096)
    ap.add_argument("--T", type=int, default=65536)
    ap.add_argument("--sps", type=float, default=5.0)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    nchan, T = a.nchan, a.T
    b, data = schedule(nchan, T, a.sps)
    tx = ais_amd.ais_tx_batch(a.sps, nchan, max(len(b), 1))
    out = torch.empty((nchan, T), dtype=torch.complex64, device="cuda")
    s = torch.cuda.current_stream()
    res = {"shape": dict(nchan=nchan, T=T, sps=a.sps, bursts=int(len(b)), payload_octets=21, p_occ=0.5, slot_symbols=320),
           "device": torch.cuda.get_device_name(0), "bytes_written": int(out.numel() * 8)}

    def timed(fn):
        for _ in range(a.warmup):
            fn()
        s.synchronize()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.calls)]
        for e0, e1 in ev:
            e0.record(s)
            fn()
            e1.record(s)
        s.synchronize()
        ms = sorted(e0.elapsed_time(e1) for e0, e1 in ev)
        return dict(median=ms[len(ms) // 2], min=ms[0], max=ms[-1], calls=a.calls)

    gbs = C.c_float(0)
    _lib.check(_lib.lib().aisx_util_copy_GBs(out.numel() * 8 // 2, 20, C.byref(gbs)), "copy_GBs")
    res["copy_GBs"] = gbs.value

    tx.set_bursts_raw(b[:0], data[:0])
    res["empty_ms"] = timed(lambda: tx.render(0, T, out=out))
    wall = []
    for _ in range(5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        tx.set_bursts_raw(b, data)
        s.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
    res["set_bursts_ms"] = dict(median=sorted(wall)[2], min=min(wall), max=max(wall), calls=5,
                                note="host check and sort + upload + k_tx_frame, wall clock to the end of the kernel")
    res["render_ms"] = timed(lambda: tx.render(0, T, out=out))
    in_burst = float((out[:64] != 0).float().mean().item())
    out.normal_()
    res["accumulate_ms"] = timed(lambda: tx.render(0, T, out=out, accumulate=True))
    res["share_of_samples_in_bursts"] = in_burst
    half = gbs.value / 2.0
    for k in ("empty_ms", "render_ms"):
        w = res["bytes_written"] / (res[k]["median"] * 1e-3) / 1e9
        res[k]["written_GBs"] = w
        res[k]["fraction_of_write_ceiling"] = w / half
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
