"""Batched HDLC deframer on the device (aisx_hdlc_batch_*): the receive chain's `hdlc_deframer_bp(11, 64)`
(python/radio.py:64) for every channel of a chain step at once, behind `ais_demod.work_pipelined`.  Only the PDUs
whose CRC checks come back to the host; `pdu_to_nmea` stays there (it runs once per packet)."""
import ctypes as C

import numpy as np
import torch

from . import _lib
from ._lib import check

PDU_DTYPE = np.dtype([("end_bit", "<u8"), ("offset", "<i8"), ("chan", "<i4"), ("len", "<i4")])  # aisx_pdu


def _stream_ptr(stream=None):
    s = stream if stream is not None else torch.cuda.current_stream()
    return C.c_void_p(s.cuda_stream)


class hdlc_deframer_batch:
    """One `hdlc_deframer_bp(length_min, length_max)` per channel, nchan channels of at most max_bits bits per
    call, at most max_pdus PDUs per call (the rest are counted, not kept).  Per channel the results are exactly
    those of the host deframer fed the same bits call by call; records are ordered by channel, then by end_bit
    (the index of the closing bit in the channel's stream, counted from creation / reset).

    Behind the pipelined chain, on a stream `s` of the caller's:

        r = dem.work_pipelined(x_k, x_next)              # step k
        dem.wait(r["step"], stream=s)                    # 1. s waits for step k (the host does not block)
        hd.work(r["bits"], r["produced"], stream=s)      # 2. deframe step k on s, counts read on the device
        ...issue step k + 1, then...
        recs, data = hd.pdus(stream=s)                   # 3. step k's PDUs, read while step k + 1 runs

    The chain's own bit-tail stream is not enough on its own: a step whose front end emitted no whole vector
    writes its zero counts on another of the chain's streams; aisx_chain_wait orders every path.  A step's
    outputs rotate through AISX_CHAIN_DEPTH sets, so work() must be queued before the call that reuses them."""

    def __init__(self, length_min, length_max, nchan, max_bits, max_pdus):
        h = C.c_void_p()
        check(_lib.lib().aisx_hdlc_batch_create(C.byref(h), int(length_min), int(length_max), int(nchan), int(max_bits),
                                                int(max_pdus)), "hdlc_deframer_batch")
        self._h = h
        self.nchan, self.max_bits, self.max_pdus = int(nchan), int(max_bits), int(max_pdus)
        self.length_min, self.length_max = int(length_min), int(length_max)
        self.found = 0  # PDUs the last call found (kept or not)
        self._recs = np.zeros(self.max_pdus, dtype=PDU_DTYPE)  # read-back buffers, reused by every call
        self._data = np.zeros(self.max_pdus * (self.length_max - 1) + 1, dtype=np.uint8)

    def __del__(self):
        h = getattr(self, "_h", None)
        if h and _lib is not None:
            _lib.lib().aisx_hdlc_batch_destroy(h)
            self._h = None

    def reset(self):
        check(_lib.lib().aisx_hdlc_batch_reset(self._h), "hdlc_deframer_batch.reset")

    def work(self, bits, produced, stream=None):
        """bits: uint8 device tensor [nchan][>= max_bits], row c holding produced[c] bits (int32 device tensor
        [nchan]).  Queued on `stream` (default: the current one); nothing waits."""
        if bits.dtype != torch.uint8 or not bits.is_cuda or bits.dim() != 2 or bits.shape[0] != self.nchan or bits.stride(1) != 1:
            raise ValueError("hdlc_deframer_batch.work: bits must be a uint8 device tensor [nchan][n] with unit item stride")
        if produced.dtype != torch.int32 or not produced.is_cuda or produced.numel() != self.nchan or not produced.is_contiguous():
            raise ValueError("hdlc_deframer_batch.work: produced must be a contiguous int32 device tensor [nchan]")
        check(_lib.lib().aisx_hdlc_batch_process(self._h, bits.data_ptr(), bits.stride(0), produced.data_ptr(),
                                                 _stream_ptr(stream)), "hdlc_deframer_batch.work")

    def results_device(self):
        """device addresses of the last call's records (aisx_pdu [max_pdus]), bytes and counts (int [3]: found,
        kept, bad-count flag)"""
        p, b, n = C.c_void_p(), C.c_void_p(), C.c_void_p()
        check(_lib.lib().aisx_hdlc_batch_results_device(self._h, C.byref(p), C.byref(b), C.byref(n)),
              "hdlc_deframer_batch.results_device")
        return p.value, b.value, n.value

    def pdus(self, stream=None, as_list=False, overflow_ok=False):
        """The last call's PDUs (synchronises `stream`): (records, bytes) with records a PDU_DTYPE array (chan,
        end_bit, len, offset into bytes), or with as_list=True a list of (chan, end_bit, payload bytes).  When
        more than max_pdus were found, OverflowError -- or with overflow_ok=True the first max_pdus (self.found
        tells how many there were).  ValueError when a call since the last read met a count outside
        [0, max_bits] (that channel was not advanced)."""
        recs, data = self._recs, self._data
        n = C.c_int(0)
        rc = _lib.lib().aisx_hdlc_batch_read(self._h, recs.ctypes.data_as(C.c_void_p), self.max_pdus,
                                             data.ctypes.data_as(C.c_void_p), data.size, C.byref(n), _stream_ptr(stream))
        self.found = n.value
        if not (rc == _lib.AISX_ERR_OVERFLOW and overflow_ok):
            check(rc, "hdlc_deframer_batch.pdus")
        recs = recs[: min(n.value, self.max_pdus)].copy()
        nb = int(recs["offset"][-1] + recs["len"][-1]) if len(recs) else 0
        data = data[:nb].copy()
        if as_list:
            return [(int(r["chan"]), int(r["end_bit"]), bytes(data[r["offset"]:r["offset"] + r["len"]])) for r in recs]
        return recs, data
