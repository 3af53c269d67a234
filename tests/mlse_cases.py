"""Inputs and references shared by the sequence detector's tests (test_mlse_host.py, test_mlse_model.py,
test_gpu_mlse.py): the float64 restatement of the model, clean symbols from levels, the host form driven call by call,
and the noisy channels of tools/mlse_gain.py with the oracle chain's symbols."""
import math

import numpy as np

B, W = 64, 16
COUNTS = (0, 1, 15, 16, 17, 63, 64, 79, 80, 81, 143, 144, 145, 5000)
SPS = 4


def qpulse(v, bt, L=4):
    """include/aisx.h: the transmitter's phase pulse, in float64"""
    if v <= 0:
        return 0.0
    if v >= L:
        return 1.0
    beta = math.pi * bt * math.sqrt(2.0 / math.log(2.0))
    F = lambda x: x * math.erf(beta * x) + math.exp(-beta * beta * x * x) / (beta * math.sqrt(math.pi))  # noqa: E731
    G = lambda x: 0.5 + 0.5 * (F(x + 0.5) - F(x - 0.5))  # noqa: E731
    lo, hi = G(-0.5 * L), G(0.5 * L)
    return (G(v - 0.5 * L) - lo) / (hi - lo)


def model(bt=0.4):
    """(c0, c1, theta[p][q][r]) in float64"""
    c0, c1 = qpulse(2.5, bt) - qpulse(1.5, bt), qpulse(3.5, bt) - qpulse(2.5, bt)
    th = np.zeros((2, 2, 2))
    for p in range(2):
        for q in range(2):
            for r in range(2):
                th[p, q, r] = math.pi / 2 * (c0 * (2 * q - 1) + c1 * (2 * p - 1 + 2 * r - 1))
    return c0, c1, th


def clean_symbols(levels, bt=0.4):
    """levels b[-1], b[0], ..., b[N]: s[n] = exp(j sum_{m <= n} theta(b[m-1], b[m], b[m+1])), n = 0 .. N - 1, float64
    rounded to complex64"""
    _, _, th = model(bt)
    b = np.asarray(levels, dtype=np.int64)
    step = th[b[:-2], b[1:-1], b[2:]]
    return np.exp(1j * np.cumsum(step)).astype(np.complex64)


def levels_of(bits):
    """the detector's decided levels from its bits: bit[n] = 1 ^ b[n] ^ b[n-1] with b[-1] = 0"""
    return np.bitwise_xor.accumulate(np.asarray(bits, np.uint8) ^ 1)


def host_run(ais_amd, calls, flush=True, bt=0.4):
    """one host detector fed the symbol arrays of `calls` one after the other: the list of each call's bits, the
    flush's last"""
    det = ais_amd.mlse_detector(bt)
    out = [det.work(c) for c in calls]
    if flush:
        out.append(det.flush())
    return out


class TypedPayloads:
    """a numpy Generator whose 168-bit draws (synth.make_burst's payloads) carry message type 1, as
    tools/hdlc_repair_gain.py's"""

    def __init__(self, rng):
        self._rng = rng

    def __getattr__(self, name):
        return getattr(self._rng, name)

    def integers(self, low, high=None, size=None):
        v = self._rng.integers(low, high, size)
        if size == 168:
            v[2:8] = [1, 0, 0, 0, 0, 0]
        return v


def typed_channel(seed, T, ebn0):
    """synth.make_channel(seed, T, "S", SPS, amp=1.0, ebn0_db=ebn0, cfo_max=500.0) with every payload's message type set
    to 1 -- its loop restated, so that nothing in synth is replaced while other threads or later tests use it: the same
    draws in the same order, hence the samples of tools/hdlc_repair_gain.py's typed_channel"""
    import synth

    rng = np.random.default_rng(seed)
    fs = synth.FS_BAUD * SPS
    x = np.zeros(T, dtype=np.complex128)
    slot = synth.slot_samples("S", SPS)
    infos = []
    for s0 in range(0, T - slot + 1, slot):
        if rng.random() >= 0.5:
            continue
        iq, info = synth.make_burst(TypedPayloads(rng), "S", SPS)
        cfo = rng.uniform(-500.0, 500.0)
        ph = rng.uniform(-np.pi, np.pi)
        start = s0 + int(rng.integers(0, max(1, slot - iq.size)))
        n = np.arange(iq.size)
        x[start:start + iq.size] += iq * np.exp(1j * (2 * np.pi * cfo / fs * n + ph))
        info.update(start=start, cfo=cfo, phase=ph, amp=1.0)
        infos.append(info)
    sigma = np.sqrt(SPS / (10 ** (ebn0 / 10.0)) / 2.0)
    x += rng.normal(0, sigma, T) + 1j * rng.normal(0, sigma, T)
    return x.astype(np.complex64), infos


def stock_template():
    import ais_amd

    return ais_amd.modulate_vector_bc(ais_amd.gmsk_mod(SPS, 0.4), [1, 1, 0, 0] * 7, [1])


def noisy_channel(seed, T, ebn0, tmpl):
    """-> (bits of the plain bit tail, the oracle chain's symbols, the set of sent payloads)"""
    import oracle_py as orc

    x, infos = typed_channel(seed, T, ebn0)
    bits, syms, _ = orc.Demod(SPS, tmpl, stages=3).step(x, want_syms=True)
    bits = np.asarray(bits if bits is not None else [], np.uint8)
    syms = np.asarray(syms if syms is not None else [], np.complex64)
    sent = {np.packbits(np.array(i["payload"], np.uint8), bitorder="little").tobytes() for i in infos}
    return bits, syms, sent
