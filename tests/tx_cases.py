"""Shared cases of the transmitter tests (test_tx_model.py, test_gpu_tx.py): the payload set of the framing checks,
synth.py's construction of a burst's levels, and a scene with synth.make_channel's occupancy."""
import numpy as np

import synth


def synth_levels(payload, training_bits=28, ramp_syms=8, tail_syms=4):
    """the NRZ levels (0 / 1) of synth.make_burst (synth.py:90-102) for given payload octets"""
    bits = np.unpackbits(np.frombuffer(bytes(payload), np.uint8), bitorder="little").tolist()
    frame = bits + synth.crc16_hdlc(bits)
    data = synth.FLAG + synth.bit_stuff(frame) + synth.FLAG
    sync = [1 if b else -1 for b in ([1, 1, 0, 0] * 64)[:training_bits]]
    ramp = [(-1) ** k for k in range(ramp_syms)]
    lv = synth.nrzi_levels(data, start_level=sync[-1])
    return np.array([(v + 1) // 2 for v in ramp + sync + lv + [lv[-1]] * tail_syms], dtype=np.uint8)


def fcs_ends_in_five_ones():
    """a payload whose FCS ends in five 1s (the last bits sent before the closing flag: a stuffed 0 follows them)"""
    rng = np.random.default_rng(5)
    while True:
        p = rng.integers(0, 256, 21, dtype=np.uint8).tobytes()
        bits = np.unpackbits(np.frombuffer(p, np.uint8), bitorder="little").tolist()
        if synth.crc16_hdlc(bits)[-5:] == [1] * 5:
            return p


def payload_set(nrandom=200):
    rng = np.random.default_rng(20261018)
    out = [rng.integers(0, 256, int(rng.integers(1, 127)), dtype=np.uint8).tobytes() for _ in range(nrandom)]
    for n in (1, 21, 126):
        out += [b"\xff" * n, b"\x7e" * n, b"\x00" * n]
    out += [b"\x5a", fcs_ends_in_five_ones()]
    return out


def preamble_template(sps):
    """the 28-symbol training sequence as the receiver's correlator template (integer sps)"""
    lv = [1 if b else -1 for b in synth.sync_bits("P")]
    return synth.gmsk_waveform(np.array(lv, float), sps)[: len(lv) * sps].astype(np.complex64)


def make_scene(seed, nchan, T, sps, framer, p_occ=0.5, cfo_hz=500.0, fs=None, nbytes=21, slot_syms=320, chan_cfo=None):
    """synth.make_channel's occupancy: per channel, slots of slot_syms symbols, each occupied with probability p_occ
    by one burst of nbytes random octets at a random place in the slot, random frac, phase and |cfo| <= cfo_hz.
    Returns the arguments of set_bursts / gmsk_scene as a dict."""
    rng = np.random.default_rng(seed)
    fs = 9600.0 * sps if fs is None else fs
    slot = int(slot_syms * sps)
    pay, chan, start, frac, cfo, phase = [], [], [], [], [], []
    for c in range(nchan):
        for s0 in range(0, T - slot + 1, slot):
            if rng.random() >= p_occ:
                continue
            p = rng.integers(0, 256, nbytes, dtype=np.uint8).tobytes()
            dur = int(np.ceil(framer(p).size * sps)) + 1
            pay.append(p)
            chan.append(c)
            start.append(s0 + int(rng.integers(0, max(1, slot - dur))))
            frac.append(rng.random())
            cfo.append((rng.uniform(-cfo_hz, cfo_hz) + (chan_cfo[c] if chan_cfo is not None else 0.0)) / fs)
            phase.append(rng.uniform(-np.pi, np.pi))
    return dict(payloads=pay, chan=np.array(chan, np.int32), start=np.array(start, np.int64),
                frac=np.minimum(np.array(frac, np.float32), np.float32(0.99999)), cfo=np.array(cfo, np.float32),
                phase=np.array(phase, np.float32))
