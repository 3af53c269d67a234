"""The transmit side: the inverse of the receive chain's framing stages and a GMSK burst modulator beside the
demodulator (GNU Radio pairs `hdlc_deframer_bp` with `hdlc_framer_pb` and `gmsk_demod` with `gmsk_mod`).

  hdlc_framer   payload octets -> the NRZ levels of one burst: ramp, training sequence, flag, bit-stuffed payload +
                CRC-16/X.25, flag, tail, NRZI-encoded (aisx_hdlc_frame, host);
  gmsk_burst    one burst's waveform, gmsk_scene a schedule of bursts on several channels, every sample from the
                closed form in double (aisx_tx_render_host, the specification);
  ais_tx_batch  the same on the device: a schedule of bursts rendered into [nchan][n] rows of any sample window by
                one kernel, at any real samples per symbol >= 2 (aisx_tx_batch_*).

An AIS simulator, a loop-back self-test for a receiver set-up, AtoN or test-beacon generation.  Noise is not part
of it: render with accumulate=True onto a torch.randn floor."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import check

BURST_DTYPE = np.dtype([("start", "<i8"), ("offset", "<i8"), ("chan", "<i4"), ("len", "<i4"), ("frac", "<f4"),
                        ("amp", "<f4"), ("cfo", "<f4"), ("phase", "<f4")])  # aisx_burst
assert BURST_DTYPE.itemsize == 40


def hdlc_framer(payload, training_bits=28, ramp_syms=8, tail_syms=4):
    """payload (1..1023 octets) -> uint8 array of the burst's NRZ levels, one 0 / 1 per symbol"""
    p = np.frombuffer(bytes(payload), dtype=np.uint8)
    n = C.c_int(0)
    L = _lib.lib(device=False)
    rc = L.aisx_hdlc_frame(p.ctypes.data_as(C.c_void_p), p.size, int(training_bits), int(ramp_syms), int(tail_syms), None, 0,
                           C.byref(n))
    if rc != _lib.AISX_ERR_OVERFLOW:
        check(rc, "hdlc_framer")
        raise ValueError("hdlc_framer: an empty burst")
    out = np.zeros(n.value, dtype=np.uint8)
    check(L.aisx_hdlc_frame(p.ctypes.data_as(C.c_void_p), p.size, int(training_bits), int(ramp_syms), int(tail_syms),
                            out.ctypes.data_as(C.c_void_p), out.size, C.byref(n)), "hdlc_framer")
    return out


def _schedule(payloads, chan, start, frac, amp, cfo, phase):
    """the arguments of set_bursts / gmsk_scene -> (aisx_burst array, payload bytes one behind the other)"""
    payloads = [bytes(p) for p in payloads]
    n = len(payloads)
    b = np.zeros(n, dtype=BURST_DTYPE)
    lens = np.array([len(p) for p in payloads], dtype=np.int64)
    b["len"] = lens
    b["offset"] = np.cumsum(lens) - lens
    for name, v in (("chan", chan), ("start", start), ("frac", frac), ("amp", amp), ("cfo", cfo), ("phase", phase)):
        b[name] = np.broadcast_to(np.asarray(v), (n,))
    data = np.frombuffer(b"".join(payloads), dtype=np.uint8) if n else np.zeros(0, np.uint8)
    return b, np.ascontiguousarray(data)


def gmsk_scene(payloads, chan, start, sps, nchan, t0, n, frac=0.0, amp=1.0, cfo=0.0, phase=0.0, bt=0.4, training_bits=28,
               ramp_syms=8, tail_syms=4, out=None, accumulate=False):
    """The host form of ais_tx_batch: complex64 [nchan][n], the sample window [t0, t0 + n) of the bursts
    (payloads[k] on channel chan[k], symbol 0 at sample start[k] + frac[k], cfo in cycles per sample, phase in
    radians; scalars apply to every burst).  Every sample is evaluated in double and rounded once."""
    b, data = _schedule(payloads, chan, start, frac, amp, cfo, phase)
    if out is None:
        out = np.zeros((int(nchan), int(n)), dtype=np.complex64)
        accumulate = False
    if out.dtype != np.complex64 or out.ndim != 2 or out.shape != (int(nchan), int(n)) or out.strides[1] != 8:
        raise ValueError("gmsk_scene: out must be complex64 [nchan][n] with unit item stride")
    check(_lib.lib(device=False).aisx_tx_render_host(float(sps), float(bt), int(training_bits), int(ramp_syms), int(tail_syms),
                                                     int(nchan), b.ctypes.data_as(C.c_void_p), b.size,
                                                     data.ctypes.data_as(C.c_void_p), data.size, int(t0), int(n),
                                                     out.ctypes.data_as(C.c_void_p), out.strides[0] // 8, int(bool(accumulate))),
          "gmsk_scene")
    return out


def gmsk_burst(payload, sps, bt=0.4, training_bits=28, ramp_syms=8, tail_syms=4, frac=0.0, amp=1.0, cfo=0.0, phase=0.0):
    """One burst from its first sample on: complex64 [ceil(nsyms * sps) + 1] (the last sample or two lie behind the
    burst and are zero)."""
    nsyms = hdlc_framer(payload, training_bits, ramp_syms, tail_syms).size
    n = int(np.ceil(nsyms * float(sps))) + 1
    return gmsk_scene([payload], 0, 0, sps, 1, 0, n, frac, amp, cfo, phase, bt, training_bits, ramp_syms, tail_syms)[0]


class ais_tx_batch:
    """A schedule of at most max_bursts AIS bursts of at most length_max payload octets on nchan channels, rendered on
    the device at sps samples per symbol (any real number >= 2):

        tx = ais_amd.ais_tx_batch(5.0, nchan, max_bursts)
        tx.set_bursts(payloads, chan, start, frac=..., amp=..., cfo=..., phase=...)
        x = torch.randn(nchan, n, dtype=torch.complex64, device="cuda") * sigma
        tx.render(t0, n, out=x, accumulate=True)         # bursts on a noise floor, ready for ais_demod

    render() is stateless in t0: a burst may begin before the window and end behind it, and the rows of one call and
    of any split of its window into calls are bit-identical.  Bursts that overlap in a channel add."""

    def __init__(self, sps, nchan, max_bursts, bt=0.4, training_bits=28, ramp_syms=8, tail_syms=4, length_max=64):
        import torch  # noqa: F401  (before libaisx.so: _lib.lib)

        h = C.c_void_p()
        check(_lib.lib().aisx_tx_batch_create(C.byref(h), float(sps), float(bt), int(training_bits), int(ramp_syms),
                                              int(tail_syms), int(nchan), int(max_bursts), int(length_max)), "ais_tx_batch")
        self._h = h
        self.sps, self.bt, self.nchan, self.max_bursts, self.length_max = float(sps), float(bt), int(nchan), int(max_bursts), int(length_max)
        self.training_bits, self.ramp_syms, self.tail_syms = int(training_bits), int(ramp_syms), int(tail_syms)
        self.nbursts = 0

    def __del__(self):
        h = getattr(self, "_h", None)
        if h and _lib is not None:
            _lib.lib().aisx_tx_batch_destroy(h)
            self._h = None

    @staticmethod
    def _stream_ptr(stream):
        import torch

        s = stream if stream is not None else torch.cuda.current_stream()
        return C.c_void_p(s.cuda_stream)

    def set_bursts(self, payloads, chan, start, frac=0.0, amp=1.0, cfo=0.0, phase=0.0, stream=None):
        """Replaces the schedule: payloads[k] (bytes) on channel chan[k], symbol 0 at row sample start[k] + frac[k]
        (frac in [0, 1)), amplitude amp, carrier offset cfo in cycles per sample (|cfo| <= 0.5), phase in radians;
        scalars apply to every burst.  ValueError for a descriptor the handle cannot take: the schedule stays what
        it was.  Waits for the handle's last render; the framing kernel is queued on `stream`."""
        b, data = _schedule(payloads, chan, start, frac, amp, cfo, phase)
        self.set_bursts_raw(b, data, stream)

    def set_bursts_raw(self, bursts, data, stream=None):
        """the same from a BURST_DTYPE array and the payload bytes its offsets point into"""
        b = np.ascontiguousarray(bursts, dtype=BURST_DTYPE)
        data = np.ascontiguousarray(data, dtype=np.uint8)
        check(_lib.lib().aisx_tx_batch_set_bursts(self._h, b.ctypes.data_as(C.c_void_p), b.size, data.ctypes.data_as(C.c_void_p),
                                                  data.size, self._stream_ptr(stream)), "ais_tx_batch.set_bursts")
        self.nbursts = int(b.size)

    def render(self, t0, n, out=None, accumulate=False, stream=None):
        """complex64 device tensor [nchan][n]: the sample window [t0, t0 + n).  out: written in place (any row stride,
        unit item stride); accumulate=True adds to what out holds.  Queued on `stream` (default: the current one)."""
        import torch

        n = int(n)
        if out is None:
            if accumulate:
                raise ValueError("ais_tx_batch.render: accumulate needs out")
            out = torch.empty((self.nchan, n), dtype=torch.complex64, device="cuda")
        if (out.dtype != torch.complex64 or not out.is_cuda or out.dim() != 2 or tuple(out.shape) != (self.nchan, n) or
                (n > 1 and out.stride(1) != 1)):
            raise ValueError("ais_tx_batch.render: out must be a complex64 device tensor [nchan][n] with unit item stride")
        check(_lib.lib().aisx_tx_batch_render(self._h, int(t0), n, out.data_ptr(), out.stride(0) if self.nchan > 1 else max(out.stride(0), n),
                                              int(bool(accumulate)), self._stream_ptr(stream)), "ais_tx_batch.render")
        return out

    def levels(self, index, stream=None):
        """the NRZ levels the device framed for burst `index` of the last set_bursts (uint8, one per symbol): what
        hdlc_framer gives for its payload (synchronises `stream`)"""
        cap = 64 * ((self.training_bits + self.ramp_syms + self.tail_syms + 16 + 8 * (self.length_max + 2) * 6 // 5 + 63) // 64)
        out = np.zeros(cap, dtype=np.uint8)
        n = C.c_int(0)
        check(_lib.lib().aisx_tx_batch_read_levels(self._h, int(index), out.ctypes.data_as(C.c_void_p), cap, C.byref(n),
                                                   self._stream_ptr(stream)), "ais_tx_batch.levels")
        return out[: n.value].copy()
