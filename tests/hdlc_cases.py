"""Bit streams for the batched HDLC deframer's tests (tests/test_hdlc_batch_model.py on the CPU lane model,
tests/test_gpu_hdlc_batch.py on the device), the per-channel host reference (one ais_amd.hdlc_deframer_bp per
channel, the specification) and a small Python restatement of it that also tells the end bit of each frame."""
import numpy as np

import emul_load
import synth
from emul_load import i32, lng, vp

REC_DTYPE = np.dtype([("end_bit", "<u8"), ("offset", "<i8"), ("chan", "<i4"), ("len", "<i4")])
FLAG = [0, 1, 1, 1, 1, 1, 1, 0]


def emu():
    """the CPU lane model of the batched deframer (tests/emul_hdlc): one library for the plain, the single-bit and the
    event tests"""
    L = emul_load.load("emul_hdlc", [
        ("emu_hdlc_create", vp, [i32, i32, i32, i32, i32]),
        ("emu_hdlc_destroy", None, [vp]),
        ("emu_hdlc_set_repair", None, [vp, vp, i32, i32]),
        ("emu_hdlc_process", None, [vp, vp, lng, vp]),
        ("emu_hdlc_read", None, [vp, vp, vp, vp, vp]),
        ("emu_hdlc_syndrome_table", None, [vp]),
        ("emu_hdlc_plan", i32, [i32, i32, i32, i32, i32, vp]),
    ], extra_deps=["aisx_framing.cpp", "../../include/aisx.h"])
    assert L.emu_hdlc_rec_size() == REC_DTYPE.itemsize
    return L


def octets_to_bits(octets):
    return [(int(o) >> k) & 1 for o in octets for k in range(8)]


def frame_bits(payload, bad_fcs=False):
    """payload octets + FCS, bit-stuffed, between two flags (the closing flag's last 0 included)"""
    bits = octets_to_bits(payload)
    fcs = synth.crc16_hdlc(bits)
    if bad_fcs:
        fcs = list(fcs)
        fcs[3] ^= 1
    return FLAG + synth.bit_stuff(bits + fcs) + FLAG


def noise(rng, n):
    return list(rng.integers(0, 2, n))


def as_bytes(rng, bits, wild=False):
    """one bit per byte; wild: a one is any byte value 1..255 (the deframer takes nonzero as one)"""
    b = np.asarray(bits, dtype=np.uint8)
    if wild:
        b = np.where(b != 0, rng.integers(1, 256, b.size), 0).astype(np.uint8)
    return b


def ais_stream(rng, nframes, gap=(20, 400), lengths=(21, 21)):
    """frames of AIS-like payloads (lengths in octets) in random bits; returns the stream and the payloads sent"""
    bits, sent = noise(rng, int(rng.integers(*gap))), []
    for _ in range(nframes):
        p = bytes(rng.integers(0, 256, int(rng.integers(lengths[0], lengths[1] + 1))).astype(np.uint8))
        sent.append(p)
        bits += [0, 1] * 12 + frame_bits(p) + noise(rng, int(rng.integers(*gap)))
    return bits, sent


def adversarial_stream(rng, lmin, lmax):
    """runs of 5, 6, 7 and 9 ones; frames of lmin - 1 .. lmax + 2 octets; two frames sharing a flag; a bad FCS"""
    ones = lambda k: [0] + [1] * k + [0]
    bits = noise(rng, 30)
    for k in (5, 6, 7, 9, 6, 12):
        bits += ones(k) + noise(rng, 13)
    for octs in (lmin - 1, lmin, lmax, lmax + 1, lmax + 2):
        p = bytes(rng.integers(0, 256, max(octs - 2, 0)).astype(np.uint8))
        bits += frame_bits(p) + noise(rng, 17)
    a = bytes(rng.integers(0, 256, max(lmin, 3)).astype(np.uint8))
    b = bytes(rng.integers(0, 256, max(lmin, 3) + 1).astype(np.uint8))
    fa, fb = frame_bits(a), frame_bits(b)
    bits += fa[:-8] + fb[:-8] + FLAG[:-1] + ones(7) + frame_bits(a, bad_fcs=True) + frame_bits(b) + noise(rng, 9)
    return bits


def junk(rng, n):
    """n random bits without a run of five ones, the last a 0: every one of them is a data bit"""
    out, run = [], 0
    for k in range(n):
        b = int(rng.integers(0, 2)) if run < 4 and k < n - 1 else 0
        out.append(b)
        run = run + 1 if b else 0
    return out


def period_stream(rng, lmax, k, payload):
    """the length_max rule at work: a flag, k * P data bits (P = 8 (length_max + 1) + 1: every P-th data bit of a
    segment is dropped with the frame that outgrew length_max, and collection starts again behind it), then a good
    frame's stuffed bits and closing flag WITHOUT an opening flag -- the frame the last restart collects.  Returns
    the stream and the positions of the dropped bits."""
    P = 8 * (lmax + 1) + 1
    pre = noise(rng, 37) + FLAG
    bits = pre + junk(rng, k * P) + frame_bits(payload)[len(FLAG):]
    return bits, [len(pre) + m * P - 1 for m in range(1, k + 1)]


def period_cases(rng, lmax, k, payload):
    """period_stream fed in one call and split around every drop and inside the run of data bits: per-channel
    streams (all the same) and cuts (two per channel)"""
    s, drops = period_stream(rng, lmax, k, payload)
    cuts = [[len(s), len(s)], [0, 1]]
    for d in drops:
        cuts += [[d - 1, d], [d, d + 1], [d + 1, d + 2], [d - 8 * (lmax + 1) // 2, d]]
    return [s] * len(cuts), cuts


def host_ref(lmin, lmax, calls):
    """calls: list of per-call lists of per-channel bit arrays -> per channel, the PDUs (bytes) in order"""
    import ais_amd

    nch = len(calls[0])
    hs = [ais_amd.hdlc_deframer_bp(lmin, lmax) for _ in range(nch)]
    out = [[] for _ in range(nch)]
    for call in calls:
        for c in range(nch):
            out[c] += hs[c].work(call[c])
    return out


def py_ref(lmin, lmax, bits):
    """aisx_hdlc_work restated bit by bit: [(end_bit, payload bytes)]"""
    ones, frame, shift, nshift, res = 0, [], 0, 0, []

    def crc(octs):
        reg = 0xFFFF
        for o in octs:
            reg ^= o
            for _ in range(8):
                reg = (reg >> 1) ^ (0x8408 if reg & 1 else 0)
        return ~reg & 0xFFFF

    for i, b in enumerate(bits):
        bit = 1 if b else 0
        if ones < 5:
            if len(frame) > lmax:
                frame, shift, nshift = [], 0, 0
            else:
                shift = (shift >> 1) | (0x80 if bit else 0)
                nshift += 1
                if nshift == 8:
                    frame.append(shift)
                    shift, nshift = 0, 0
        elif bit:
            if len(frame) >= lmin:
                pl = len(frame) - 2
                if crc(frame[:pl]) == frame[pl] | (frame[pl + 1] << 8):
                    res.append((i, bytes(frame[:pl])))
            frame, shift, nshift = [], 0, 0
        ones = ones + 1 if bit else 0
    return res


def split_calls(streams, cuts):
    """streams[c] split at cuts[c] (a sorted list of positions per channel): list of calls of per-channel arrays"""
    ncalls = len(cuts[0]) + 1
    calls = [[None] * len(streams) for _ in range(ncalls)]
    for c, s in enumerate(streams):
        edges = [0] + list(cuts[c]) + [len(s)]
        for k in range(ncalls):
            calls[k][c] = np.asarray(s[edges[k]:edges[k + 1]], dtype=np.uint8)
    return calls


def pack(call, stride, pad_front=0):
    """per-channel arrays -> ([nch][stride] bytes, counts); pad_front shifts every row's start off 16-byte alignment"""
    nch = len(call)
    buf = np.zeros(nch * stride + pad_front + 64, dtype=np.uint8)
    rows = buf[pad_front:pad_front + nch * stride].reshape(nch, stride)
    for c, b in enumerate(call):
        rows[c, :len(b)] = b
    return rows, np.array([len(b) for b in call], dtype=np.int32)


def by_channel(recs, data, nch):
    """records + byte buffer -> per channel [(end_bit, bytes)], checking the order and the packing on the way"""
    out = [[] for _ in range(nch)]
    prev, off = (-1, -1), 0
    for r in recs:
        key = (int(r["chan"]), int(r["end_bit"]))
        assert key > prev, (key, prev)
        assert int(r["offset"]) == off
        prev, off = key, off + int(r["len"])
        out[key[0]].append((key[1], bytes(data[int(r["offset"]):int(r["offset"]) + int(r["len"])])))
    return out
