"""The batched HDLC deframer's kernel bodies (gr-ais_amd/csrc/k_hdlc.h) on the CPU lane model
(tests/emul_hdlc), against the host deframer that is their specification (one ais_amd.hdlc_deframer_bp per
channel fed the same bits call by call) and, on the short streams, a Python restatement that also tells each
frame's end bit.  Plus the C ABI's argument checks and its refusal without a device.  -m "not gpu"."""
import ctypes as C

import numpy as np
import pytest

import hdlc_cases as hc
import torch  # noqa: F401  (before libaisx.so: one HIP runtime in the process)

emu = hc.emu


class EmuBatch:
    def __init__(self, lmin, lmax, nch, max_bits, max_pdus=4096):
        self.h = emu().emu_hdlc_create(lmin, lmax, nch, max_bits, max_pdus)
        assert self.h
        self.nch, self.max_pdus, self.lmax, self.max_bits = nch, max_pdus, lmax, max_bits

    def __del__(self):
        emu().emu_hdlc_destroy(self.h)

    def process(self, call, pad_front=0):
        rows, n = hc.pack(call, self.max_bits + 3, pad_front)
        emu().emu_hdlc_process(self.h, rows.ctypes.data, rows.strides[0], n.ctypes.data)

    def read(self):
        recs = np.zeros(self.max_pdus, dtype=hc.REC_DTYPE)
        data = np.zeros(self.max_pdus * (self.lmax - 1) + 1, dtype=np.uint8)
        cnt = np.zeros(3, dtype=np.int32)
        emu().emu_hdlc_read(self.h, recs.ctypes.data, data.ctypes.data, None, cnt.ctypes.data)
        return int(cnt[0]), int(cnt[2]), recs[: cnt[1]], data


def run_model(lmin, lmax, calls, pad_front=0, max_pdus=4096):
    nch = len(calls[0])
    b = EmuBatch(lmin, lmax, nch, max(max(len(x) for x in call) for call in calls) + 1, max_pdus)
    got = [[] for _ in range(nch)]
    for call in calls:
        b.process(call, pad_front)
        found, bad, recs, data = b.read()
        assert bad == 0 and found == len(recs)
        for c, lst in enumerate(hc.by_channel(recs, data, nch)):
            got[c] += lst
    return got


def check(lmin, lmax, calls, streams=None, pad_front=0):
    got = run_model(lmin, lmax, calls, pad_front)
    ref = hc.host_ref(lmin, lmax, calls)
    for c in range(len(got)):
        assert [p for _, p in got[c]] == ref[c], c
        if streams is not None:
            assert got[c] == hc.py_ref(lmin, lmax, streams[c]), c
    return sum(len(g) for g in got)


def test_random_bits_over_several_passes():
    rng = np.random.default_rng(1)
    # calls of up to 9 000 random bits (three passes of the kernel), every one or two thousand bits a frame of
    # random length around length_min .. length_max + 2 octets: good, too short, too long, cut by the noise
    def stream(lmin, lmax):
        s = []
        while len(s) < 25000:
            s += hc.noise(rng, int(rng.integers(0, 2000)))
            octs = int(rng.integers(max(lmin - 1, 2), lmax + 3))
            s += hc.frame_bits(bytes(rng.integers(0, 256, octs - 2).astype(np.uint8)))
        return s

    for lmin, lmax in ((2, 5), (11, 64), (3, 30)):
        streams = [stream(lmin, lmax) for _ in range(5)]
        cuts = [sorted(rng.integers(0, 25000, 2)) for _ in range(5)]
        calls = hc.split_calls(streams, cuts)
        calls = [[hc.as_bytes(rng, b, wild=(c % 2 == 1)) for c, b in enumerate(call)] for call in calls]
        found = check(lmin, lmax, calls)
        print("random bits, lmin %d lmax %d: %d PDUs" % (lmin, lmax, found))
        assert found > 10


def test_ais_frames_in_noise_and_misaligned_rows():
    rng = np.random.default_rng(2)
    streams, sent = zip(*[hc.ais_stream(rng, 6) for _ in range(6)])
    cuts = [sorted(rng.integers(0, len(s), 3)) for s in streams]
    calls = hc.split_calls(streams, cuts)
    for pad in (0, 5):
        check(11, 64, calls, streams, pad_front=pad)
    got = run_model(11, 64, calls)
    for c in range(6):
        assert [p for _, p in got[c]] == list(sent[c])


def test_adversarial_streams():
    rng = np.random.default_rng(3)
    for lmin, lmax in ((11, 64), (2, 2), (2, 9), (4, 40)):
        streams = [hc.adversarial_stream(rng, lmin, lmax) for _ in range(4)]
        calls = [[hc.as_bytes(rng, s, wild=True) for s in streams]]
        n = check(lmin, lmax, calls, streams)
        assert n >= 4 * 3, (lmin, lmax, n)


def test_long_frames_across_passes_and_calls():
    rng = np.random.default_rng(4)
    # frames up to length_max = 1024 octets (8 200 bits): longer than a pass of 4 096 bits
    streams = []
    for c in range(3):
        s = hc.noise(rng, 100)
        for octs in (1024, 1000, 1025, 700):
            s += hc.frame_bits(bytes(rng.integers(0, 256, octs - 2).astype(np.uint8))) + hc.noise(rng, 50)
        streams.append(s)
    cuts = [[len(s) // 3, len(s) // 3 + c, 2 * len(s) // 3] for c, s in enumerate(streams)]
    n = check(11, 1024, hc.split_calls(streams, cuts), streams)
    assert n == 3 * 3


def test_length_max_period():
    # after k * P data bits without a delimiter the frame restarts exactly where a good frame's bits begin: found
    # only if the drop recurs every P = 8 (length_max + 1) + 1 data bits, in one call and across calls split at the
    # drops (the open frame carried between calls)
    rng = np.random.default_rng(9)
    for lmax in (30, 64, 1024):
        for k in (1, 2):
            payload = bytes(rng.integers(0, 256, 20).astype(np.uint8))
            streams, cuts = hc.period_cases(rng, lmax, k, payload)
            assert [p for _, p in hc.py_ref(11, lmax, streams[0])] == [payload]
            n = check(11, lmax, hc.split_calls(streams, cuts), streams)
            assert n == len(streams), (lmax, k)


def test_split_at_every_offset_across_a_frame():
    rng = np.random.default_rng(5)
    lead = hc.noise(rng, 40)
    body = lead + hc.frame_bits(bytes(rng.integers(0, 256, 12).astype(np.uint8))) + hc.frame_bits(b"\x01\x02\x03\x04\x05\x06\x07\x08\x09") \
        + hc.noise(rng, 10)
    L = len(body)
    streams = [body] * (L + 1)
    # channel c: a call of c bits, then one of 0, 1 or 2 bits, then the rest
    cuts = [[c, min(L, c + c % 3)] for c in range(L + 1)]
    check(9, 64, hc.split_calls(streams, cuts), streams)


def test_overflow_keeps_a_prefix_and_bad_counts():
    rng = np.random.default_rng(6)
    streams, _ = zip(*[hc.ais_stream(rng, 4) for _ in range(5)])
    calls = [[np.asarray(s, dtype=np.uint8) for s in streams]] * 1
    full = run_model(11, 64, calls)
    flat = [(c, e, p) for c in range(5) for e, p in full[c]]
    b = EmuBatch(11, 64, 5, max(len(s) for s in streams) + 1, max_pdus=7)
    b.process(calls[0])
    found, bad, recs, data = b.read()
    assert found == len(flat) == 20 and len(recs) == 7 and bad == 0
    got = [(c, e, p) for c in range(5) for e, p in hc.by_channel(recs, data, 5)[c]]
    assert got == flat[:7]
    # a count outside [0, max_bits]: that channel is not advanced, the flag is raised once
    rows, n = hc.pack([np.zeros(3, np.uint8)] * 5, b.max_bits + 3)
    n[2] = b.max_bits + 1
    n[3] = -1
    emu().emu_hdlc_process(b.h, rows.ctypes.data, rows.strides[0], n.ctypes.data)
    assert b.read()[1] == 1
    emu().emu_hdlc_process(b.h, rows.ctypes.data, rows.strides[0], np.zeros(5, np.int32).ctypes.data)
    assert b.read()[1] == 0


def test_create_arguments_and_no_device():
    from ais_amd import _lib

    bad = [(1, 64, 4, 100, 10), (12, 11, 4, 100, 10), (11, 1025, 4, 100, 10), (11, 64, 0, 100, 10), (11, 64, 4, 0, 10),
           (11, 64, 4, 100, 0)]
    for a in bad:
        assert not emu().emu_hdlc_create(*a), a
    L = _lib.lib()
    h = C.c_void_p()
    for a in bad:
        assert L.aisx_hdlc_batch_create(C.byref(h), *a) == _lib.AISX_ERR_INVALID, a
    assert L.aisx_hdlc_batch_create(None, 11, 64, 4, 100, 10) == _lib.AISX_ERR_INVALID
    n = C.c_int(-1)
    L.aisx_device_count(C.byref(n))
    rc = L.aisx_hdlc_batch_create(C.byref(h), 11, 1024, 4, 100, 10)
    if n.value <= 0:
        assert rc == _lib.AISX_ERR_NO_DEVICE
    else:
        assert rc == _lib.AISX_OK
        assert L.aisx_hdlc_batch_destroy(h) == 0
    import ais_amd

    with pytest.raises(ValueError):
        ais_amd.hdlc_deframer_batch(1, 64, 4, 100, 10)
