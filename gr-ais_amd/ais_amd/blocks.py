"""Host-side mirror of the reference's block interface for the demod hot path.

Same names, constructor arguments and error behaviour as the reference's Python
bindings (swig/ais_swig.i:16-26 exposes ais.corr_est_cc, ais.freqest,
ais.msk_timing_recovery_cc; python/gmsk_sync.py and python/ais_demod.py are
Python hier blocks), with one addition: `nchan`, the number of independent
channels batched through one call.  All arithmetic happens in libaisx.so (HIP,
gfx950); torch is used only for device memory and streams.
"""
import ctypes as C
import math

import numpy as np
import torch

from . import _lib
from ._lib import check

TAG_DTYPE = np.dtype([("offset", "<u8"), ("value", "<f8"), ("key", "<i4"), ("chan", "<i4")])


def _stream_ptr(stream=None):
    s = stream if stream is not None else torch.cuda.current_stream()
    return C.c_void_p(s.cuda_stream)


def _dev_c64(x, nchan):
    if not isinstance(x, torch.Tensor):
        x = torch.as_tensor(np.ascontiguousarray(x, dtype=np.complex64))
    if x.dtype != torch.complex64:
        raise TypeError("expected complex64 (gr_complex) items, got %s" % x.dtype)
    if not x.is_cuda:
        x = x.cuda()
    x = x.reshape(nchan, -1)
    if x.stride(1) != 1:
        x = x.contiguous()
    return x


class corr_est_cc:
    """ais.corr_est_cc(symbols, sps, mark_delay, threshold=0.9)
    (include/ais/corr_est_cc.h:102-106, lib/corr_est_cc_impl.cc)."""

    def __init__(self, symbols, sps, mark_delay, threshold=0.9, nchan=1, max_items=65536, max_tags_per_chan=None):
        L = _lib.lib()
        s = np.ascontiguousarray(symbols, dtype=np.complex64)
        self.nchan, self.max_items = int(nchan), int(max_items)
        self._cap = int(max_tags_per_chan) if max_tags_per_chan else max(64, 4 * (self.max_items // 256))
        h = C.c_void_p()
        check(L.aisx_corr_create(C.byref(h), s.ctypes.data_as(C.c_void_p), s.size, float(sps), int(mark_delay),
                                 float(threshold), self.nchan, self.max_items, self._cap), "corr_est_cc")
        self._h = h
        self._N = s.size

    def __del__(self):
        h = getattr(self, "_h", None)
        if h and _lib is not None:  # (None while the interpreter shuts down: the process is going anyway)
            _lib.lib().aisx_corr_destroy(h)
            self._h = None

    # -- reference API ---------------------------------------------------
    def symbols(self):
        out = np.zeros(self._N, dtype=np.complex64)
        check(_lib.lib().aisx_corr_symbols(self._h, out.ctypes.data_as(C.c_void_p), out.size), "symbols")
        return out

    def set_symbols(self, symbols):
        s = np.ascontiguousarray(symbols, dtype=np.complex64)
        check(_lib.lib().aisx_corr_set_symbols(self._h, s.ctypes.data_as(C.c_void_p), s.size), "set_symbols")
        self._N = s.size

    def set_lds_claim(self, nbytes):
        """placement knob of the F = 4096 build (include/aisx.h: aisx_corr_set_lds_claim); results do not depend on it"""
        check(_lib.lib().aisx_corr_set_lds_claim(self._h, int(nbytes)), "set_lds_claim")

    def get_lds_claim(self):
        """(claim, used): the claim in force and the LDS a workgroup of the F = 4096 build uses (0: the F = 2048 build)"""
        b, u = C.c_int(0), C.c_int(0)
        check(_lib.lib().aisx_corr_get_lds_claim(self._h, C.byref(b), C.byref(u)), "get_lds_claim")
        return b.value, u.value

    def history(self):
        return _lib.lib().aisx_corr_history(self._h)

    def output_multiple(self):
        return _lib.lib().aisx_corr_output_multiple(self._h)

    def max_noutput_items(self):
        return _lib.lib().aisx_corr_max_noutput_items(self._h)

    def threshold(self):
        return _lib.lib().aisx_corr_threshold(self._h)

    def mark_delay(self):
        return _lib.lib().aisx_corr_mark_delay(self._h)

    def nitems_written(self, port=0):
        return _lib.lib().aisx_corr_nitems_written(self._h)

    def reset(self):
        check(_lib.lib().aisx_corr_reset(self._h), "reset")

    # -- batched device path ---------------------------------------------
    def work(self, x, want_corr=False, out=None, stream=None, corr=None):
        """One work() call on x[nchan][n] new items (device tensor).  Returns
        (out, corr|None); the tags of the call are read with tags().  out / corr: [nchan][n]
        device views to write into (rows may be strided); a given corr implies want_corr."""
        x = _dev_c64(x, self.nchan)
        n = x.shape[1]
        if out is None:
            out = torch.empty_like(x)
        if corr is not None:
            want_corr = True
            if corr.dtype != torch.complex64 or tuple(corr.shape) != tuple(x.shape) or corr.stride(1) != 1:
                raise ValueError("corr must be a complex64 [nchan][n] view with unit item stride")
        elif want_corr:
            corr = torch.empty_like(x)
        check(_lib.lib().aisx_corr_process(self._h, x.data_ptr(), x.stride(0), out.data_ptr(), out.stride(0),
                                           corr.data_ptr() if want_corr else None, corr.stride(0) if want_corr else 0,
                                           n, _stream_ptr(stream)), "corr_est_cc.work")
        return out, corr

    def set_profiling(self, on=True):
        check(_lib.lib().aisx_corr_set_profiling(self._h, 1 if on else 0), "set_profiling")

    def last_kernel_ms(self):
        ms = C.c_float(0)
        check(_lib.lib().aisx_corr_last_kernel_ms(self._h, C.byref(ms)), "last_kernel_ms")
        return ms.value

    def kernel_ms_history(self):
        buf = (C.c_float * 64)()
        n = C.c_int(0)
        check(_lib.lib().aisx_corr_kernel_ms_history(self._h, buf, 64, C.byref(n)), "kernel_ms_history")
        return [float(buf[i]) for i in range(n.value)]

    def tags_device(self):
        t, c, cap = C.c_void_p(), C.c_void_p(), C.c_int()
        check(_lib.lib().aisx_corr_tags_device(self._h, C.byref(t), C.byref(c), C.byref(cap)), "tags_device")
        return t, c, cap.value

    def tags(self, stream=None, allow_overflow=False, back=0):
        """Host copy of the last call's tags (back = 1, 2: of the call before / two before):
        structured array (offset,value,key,chan)."""
        cap = self.nchan * self._cap
        buf = np.zeros(cap, dtype=TAG_DTYPE)
        nt = C.c_int(0)
        rc = _lib.lib().aisx_corr_read_tags_back(self._h, int(back), buf.ctypes.data_as(C.c_void_p), cap, C.byref(nt),
                                                 _stream_ptr(stream))
        if not (allow_overflow and rc == _lib.AISX_ERR_OVERFLOW):
            check(rc, "corr_est_cc.tags")
        return buf[: nt.value].copy()

    # -- GNU Radio path (host pointers, one channel) ----------------------
    def work_host(self, in_with_history, noutput_items, nitems_written, want_corr=False, tag_cap=4096):
        a = np.ascontiguousarray(in_with_history, dtype=np.complex64)
        assert a.size >= noutput_items + self._N
        out = np.zeros(noutput_items, dtype=np.complex64)
        corr = np.zeros(noutput_items, dtype=np.complex64) if want_corr else None
        tags = np.zeros(tag_cap, dtype=TAG_DTYPE)
        nt = C.c_int(0)
        check(_lib.lib().aisx_corr_work_host(self._h, a.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p),
                                             corr.ctypes.data_as(C.c_void_p) if want_corr else None, noutput_items,
                                             nitems_written, tags.ctypes.data_as(C.c_void_p), tag_cap, C.byref(nt)),
              "corr_est_cc.work_host")
        return out, corr, tags[: nt.value].copy()


class msk_timing_recovery_cc:
    """ais.msk_timing_recovery_cc(sps, gain, limit, osps)
    (include/ais/msk_timing_recovery_cc.h:60-69, lib/msk_timing_recovery_cc_impl.cc)."""

    def __init__(self, sps, gain, limit, osps=1, nchan=1, max_items=65536):
        L = _lib.lib()
        self.nchan, self.max_items = int(nchan), int(max_items)
        h = C.c_void_p()
        check(L.aisx_msk_create(C.byref(h), float(sps), float(gain), float(limit), int(osps), self.nchan,
                                self.max_items), "msk_timing_recovery_cc")
        self._h = h
        self.out_capacity = L.aisx_msk_out_capacity(h)

    def __del__(self):
        h = getattr(self, "_h", None)
        if h and _lib is not None:  # (None while the interpreter shuts down: the process is going anyway)
            _lib.lib().aisx_msk_destroy(h)
            self._h = None

    def set_gain(self, gain):
        check(_lib.lib().aisx_msk_set_gain(self._h, float(gain)), "set_gain")

    def get_gain(self):
        return _lib.lib().aisx_msk_get_gain(self._h)

    def set_limit(self, limit):
        check(_lib.lib().aisx_msk_set_limit(self._h, float(limit)), "set_limit")
        self.out_capacity = _lib.lib().aisx_msk_out_capacity(self._h)

    def get_limit(self):
        return _lib.lib().aisx_msk_get_limit(self._h)

    def set_sps(self, sps):
        check(_lib.lib().aisx_msk_set_sps(self._h, float(sps)), "set_sps")
        self.out_capacity = _lib.lib().aisx_msk_out_capacity(self._h)

    def get_sps(self):
        return _lib.lib().aisx_msk_get_sps(self._h)

    def forecast(self, noutput_items):
        return _lib.lib().aisx_msk_forecast(self._h, int(noutput_items))

    def reset(self):
        check(_lib.lib().aisx_msk_reset(self._h), "reset")

    def work(self, x, tags_from=None, want_syms=True, want_aux=False, want_bits=True, stream=None, outs=None,
             tags_ptrs=None):
        """One stream step on x[nchan][n] new items.  `tags_from` = the
        corr_est_cc block whose last call produced the time_est tags (or None).
        Returns dict(syms, err, mu, bits, produced) of device tensors."""
        x = _dev_c64(x, self.nchan)
        n = x.shape[1]
        cap = self.out_capacity
        dev = x.device
        o = outs or {}
        syms = o.get("syms") if "syms" in o else (torch.empty((self.nchan, cap), dtype=torch.complex64, device=dev) if want_syms else None)
        err = o.get("err") if "err" in o else (torch.empty((self.nchan, cap), dtype=torch.float32, device=dev) if want_aux else None)
        mu = o.get("mu") if "mu" in o else (torch.empty((self.nchan, cap), dtype=torch.float32, device=dev) if want_aux else None)
        bits = o.get("bits") if "bits" in o else (torch.empty((self.nchan, cap), dtype=torch.uint8, device=dev) if want_bits else None)
        prod = o.get("produced") if "produced" in o else torch.empty(self.nchan, dtype=torch.int32, device=dev)
        stride = None
        for name, t, dt in (("syms", syms, torch.complex64), ("err", err, torch.float32), ("mu", mu, torch.float32),
                            ("bits", bits, torch.uint8)):
            if t is None:
                continue
            if (t.dim() != 2 or t.shape[0] != self.nchan or t.dtype != dt or t.stride(1) != 1 or not t.is_cuda
                    or t.shape[1] < 1 or t.stride(0) < t.shape[1]):
                raise ValueError("msk_timing_recovery_cc.work: outs[%r] must be a (nchan, cap) %s device tensor with "
                                 "unit inner stride" % (name, dt))
            if stride is None:
                stride, width = t.stride(0), t.shape[1]
            elif t.stride(0) != stride:
                raise ValueError("msk_timing_recovery_cc.work: all output tensors must share one row stride")
            else:
                width = min(width, t.shape[1])
        if prod.dim() != 1 or prod.shape[0] < self.nchan or prod.dtype != torch.int32 or not prod.is_cuda:
            raise ValueError("msk_timing_recovery_cc.work: outs['produced'] must be an int32 device tensor of nchan items")
        if stride is None:
            stride = width = cap
        if width < stride:
            # rows narrower than their stride (a column slice): the kernel bounds its writes by the
            # stride it is given, so hand it rows it owns entirely
            raise ValueError("msk_timing_recovery_cc.work: output rows must be as wide as their stride")
        if tags_ptrs is not None:
            tptr, cptr, tcap = tags_ptrs  # as returned by corr_est_cc.tags_device() right after its work()
        elif tags_from is not None:
            tptr, cptr, tcap = tags_from.tags_device()
        else:
            tptr, cptr, tcap = None, None, 0
        check(_lib.lib().aisx_msk_process_stream(
            self._h, x.data_ptr(), x.stride(0), n, tptr, cptr, tcap,
            syms.data_ptr() if syms is not None else None, err.data_ptr() if err is not None else None,
            mu.data_ptr() if mu is not None else None, bits.data_ptr() if bits is not None else None, stride,
            prod.data_ptr(), _stream_ptr(stream)), "msk_timing_recovery_cc.work")
        return dict(syms=syms, err=err, mu=mu, bits=bits, produced=prod)

    def set_tail_stream(self, stream):
        """Run the NRZI bit tail of every work() call on `stream` (None: back on the call's own
        stream).  The caller then alternates between two sets of output buffers (outs=) and orders
        its readers of `bits` after that stream (wait_tail)."""
        check(_lib.lib().aisx_msk_set_tail_stream(self._h, _stream_ptr(stream) if stream is not None else None,
                                                  1 if stream is not None else 0), "set_tail_stream")

    def wait_tail(self, stream=None):
        check(_lib.lib().aisx_msk_wait_tail(self._h, _stream_ptr(stream)), "wait_tail")

    def set_fused_tail(self, on):
        """The bit tail inside the recovery kernel's symbol flush (aisx_msk_set_fused_tail; default on).  Off: always
        the separate bit-tail kernel.  Results are identical; the two kinds of call may alternate."""
        check(_lib.lib().aisx_msk_set_fused_tail(self._h, 1 if on else 0), "set_fused_tail")

    def get_fused_tail(self):
        return bool(_lib.lib().aisx_msk_get_fused_tail(self._h))

    def set_pair_core(self, mode):
        """Schedule of the kernel's lock-step iteration pair (aisx_msk_set_pair_core): 1 (default) the hand-scheduled
        sequence, 0 the compiler's.  Results are identical; calls of either mode may alternate."""
        check(_lib.lib().aisx_msk_set_pair_core(self._h, int(mode)), "set_pair_core")

    def get_pair_core(self):
        return int(_lib.lib().aisx_msk_get_pair_core(self._h))

    def last_tail_fused(self):
        """Whether the last work() call that took bits computed them inside the recovery kernel."""
        return _lib.lib().aisx_msk_last_tail_fused(self._h) == 1

    def wait_prepass(self, stream=None):
        """`stream` waits until the last work() call's recovery kernel stands at the head of its queue
        (aisx_msk_wait_prepass): call it on the stream whose next kernels would otherwise take the
        LDS the recovery's workgroups need.  The first call only arms the event."""
        check(_lib.lib().aisx_msk_wait_prepass(self._h, _stream_ptr(stream)), "wait_prepass")

    def last_status(self, stream=None):
        st = C.c_int(0)
        check(_lib.lib().aisx_msk_last_status(self._h, C.byref(st), _stream_ptr(stream)), "last_status")
        return st.value

    def set_time_parallel(self, restart_points=64, join_kernel=-1, max_unit_items=0):
        """The time-parallel recovery (include/aisx.h: aisx_msk_set_time_parallel); restart_points=0 switches it off."""
        check(_lib.lib().aisx_msk_set_time_parallel(self._h, int(restart_points), int(join_kernel), int(max_unit_items)),
              "set_time_parallel")

    def set_max_noutput_items(self, m):
        """gr::block::set_max_noutput_items(): output items one general_work call is offered at most (0: what fits)."""
        check(_lib.lib().aisx_msk_set_max_noutput_items(self._h, int(m)), "set_max_noutput_items")

    def max_noutput_items(self):
        return _lib.lib().aisx_msk_get_max_noutput_items(self._h)

    def set_profiling(self, on=True):
        check(_lib.lib().aisx_msk_set_profiling(self._h, 1 if on else 0), "set_profiling")

    def kernel_ms_history(self):
        buf = (C.c_float * 64)()
        n = C.c_int(0)
        check(_lib.lib().aisx_msk_kernel_ms_history(self._h, buf, 64, C.byref(n)), "kernel_ms_history")
        return [float(buf[i]) for i in range(n.value)]

    def restart_stats(self, stream=None):
        """What the time-parallel recovery made of the last call (sums over the channels)."""
        a = (C.c_longlong * 10)()
        check(_lib.lib().aisx_msk_restart_stats(self._h, a, _stream_ptr(stream)), "restart_stats")
        return dict(restart_points=a[0], units_taken=a[1], symbols_from_units=a[2], units_ended_at_next=a[3],
                    units_ended_elsewhere=a[4], calls=a[5], links_equal=a[6], links=a[7], longest_unit_items=a[8],
                    unit_items=a[9])

    def general_work_host(self, noutput_items, ninput_items, buf, in_off, tags, nitems_read, in_has_lookahead=True):
        """GNU Radio path: in = &buf[in_off]; tags: structured array (TAG_DTYPE)."""
        buf = np.ascontiguousarray(buf, dtype=np.complex64)
        out = np.zeros(max(noutput_items, 1), np.complex64)
        err = np.zeros(max(noutput_items, 1), np.float32)
        mu = np.zeros(max(noutput_items, 1), np.float32)
        bits = np.zeros(max(noutput_items, 1), np.uint8)
        tags = np.ascontiguousarray(tags, dtype=TAG_DTYPE)
        cons, prod = C.c_int(0), C.c_int(0)
        inp = C.c_void_p(buf.ctypes.data + 8 * in_off)
        check(_lib.lib().aisx_msk_general_work_host(
            self._h, noutput_items, ninput_items, inp, out.ctypes.data_as(C.c_void_p), err.ctypes.data_as(C.c_void_p),
            mu.ctypes.data_as(C.c_void_p), bits.ctypes.data_as(C.c_void_p), tags.ctypes.data_as(C.c_void_p), tags.size,
            nitems_read, 1 if in_has_lookahead else 0, C.byref(cons), C.byref(prod)), "general_work_host")
        p = prod.value
        return out[:p], err[:p], mu[:p], bits[:p], cons.value


class square_and_fft_sync_cc:
    """ais.square_and_fft_sync_cc(samplerate, bits_per_sec, fftlen) (python/gmsk_sync.py:14-37),
    which owns ais.freqest(int(samplerate), int(bits_per_sec), fftlen) (lib/freqest_impl.cc)."""

    def __init__(self, samplerate, bits_per_sec, fftlen, nchan=1, max_items=65536):
        self.nchan, self.fftlen, self.max_items = int(nchan), int(fftlen), int(max_items)
        h = C.c_void_p()
        check(_lib.lib().aisx_freqsync_create(C.byref(h), float(samplerate), float(bits_per_sec), self.fftlen,
                                              self.nchan, self.max_items), "square_and_fft_sync_cc")
        self._h = h

    def __del__(self):
        h = getattr(self, "_h", None)
        if h and _lib is not None:  # (None while the interpreter shuts down: the process is going anyway)
            _lib.lib().aisx_freqsync_destroy(h)
            self._h = None

    def reset(self):
        check(_lib.lib().aisx_freqsync_reset(self._h), "reset")

    def estimate_ahead(self, x, stream=None, walk_stream=None):
        """Prepare the frequency estimates (on `stream`) and the NCO phase walk (on `walk_stream`,
        default: the same) of the next freq_sync_agc() call on exactly this tensor
        (aisx_freqsync_estimate_ahead): the serial walk of step k + 1 then runs beside the sample
        passes of step k.  Up to two preparations may wait (the second only behind a call whose
        length is a multiple of fftlen with nothing pending); they are consumed in order."""
        x = _dev_c64(x, self.nchan)
        check(_lib.lib().aisx_freqsync_estimate_ahead(self._h, x.data_ptr(), x.stride(0), x.shape[1], _stream_ptr(stream),
                                                      _stream_ptr(walk_stream) if walk_stream is not None else None),
              "estimate_ahead")

    def work(self, x, want_fhat=False, stream=None, out=None):
        """`out`: optional preallocated (nchan, >= n + fftlen) complex64 buffer the result is a view of."""
        x = _dev_c64(x, self.nchan)
        n = x.shape[1]
        cap = n + self.fftlen
        if out is None:
            out = torch.empty((self.nchan, cap), dtype=torch.complex64, device=x.device)
        elif out.shape[0] != self.nchan or out.shape[1] < cap or out.dtype != torch.complex64 or out.stride(1) != 1:
            raise ValueError("out must be a (nchan, >= n + fftlen) complex64 buffer")
        nv = cap // self.fftlen + 1
        fh = torch.empty((self.nchan, nv), dtype=torch.float32, device=x.device) if want_fhat else None
        nout = C.c_int(0)
        check(_lib.lib().aisx_freqsync_process(self._h, x.data_ptr(), x.stride(0), n, out.data_ptr(), out.stride(0),
                                               fh.data_ptr() if want_fhat else None, nv if want_fhat else 0,
                                               C.byref(nout), _stream_ptr(stream)), "square_and_fft_sync_cc.work")
        m = nout.value
        return out[:, :m], (fh[:, : m // self.fftlen] if want_fhat else None)


def freq_sync_agc(freq_sync, agc, x, want_fhat=False, stream=None, out=None):
    """freq_sync -> agc (the first two blocks of python/ais_demod.py:56) in one pass: the same
    result, bit for bit, as agc.work(freq_sync.work(x)[0]), without the hier block's output being
    stored (aisx_freqsync_agc_process).  Returns (agc output, fhat | None)."""
    x = _dev_c64(x, freq_sync.nchan)
    n = x.shape[1]
    cap = n + freq_sync.fftlen
    if out is None:
        out = torch.empty((freq_sync.nchan, cap), dtype=torch.complex64, device=x.device)
    elif out.shape[0] != freq_sync.nchan or out.shape[1] < cap or out.dtype != torch.complex64 or out.stride(1) != 1:
        raise ValueError("out must be a (nchan, >= n + fftlen) complex64 buffer")
    nv = cap // freq_sync.fftlen + 1
    fh = torch.empty((freq_sync.nchan, nv), dtype=torch.float32, device=x.device) if want_fhat else None
    nout = C.c_int(0)
    check(_lib.lib().aisx_freqsync_agc_process(freq_sync._h, agc._h, x.data_ptr(), x.stride(0), n, out.data_ptr(),
                                               out.stride(0), fh.data_ptr() if want_fhat else None, nv if want_fhat else 0,
                                               C.byref(nout), _stream_ptr(stream)), "freq_sync_agc")
    m = nout.value
    return out[:, :m], (fh[:, : m // freq_sync.fftlen] if want_fhat else None)


class freqest:
    """ais.freqest(sample_rate, data_rate, fftlen) (include/ais/freqest.h:49): consumes
    fft-shifted spectra, one float estimate per vector."""

    def __init__(self, sample_rate, data_rate, fftlen, nchan=1):
        # the block's own make(): d_offset / d_binsize from the float rate (lib/freqest_impl.cc:46-47), any fftlen >= 2
        self.nchan, self.fftlen = int(nchan), int(fftlen)
        h = C.c_void_p()
        check(_lib.lib().aisx_freqest_create_n(C.byref(h), float(sample_rate), int(data_rate), self.fftlen, self.nchan, 64), "freqest")
        self._h = h

    def __del__(self):
        if getattr(self, "_h", None):
            _lib.lib().aisx_freqsync_destroy(self._h)
            self._h = None

    def work(self, vecs, stream=None):
        v = _dev_c64(vecs, self.nchan)
        nvec = v.shape[1] // self.fftlen
        out = torch.empty((self.nchan, max(nvec, 1)), dtype=torch.float32, device=v.device)
        check(_lib.lib().aisx_freqest_work(self._h, v.data_ptr(), v.stride(0), out.data_ptr(), out.stride(0), nvec,
                                           _stream_ptr(stream)), "freqest.work")
        return out[:, :nvec]

    def work_host(self, vecs):
        """GNU Radio path: `vecs` = input_items[0], whole fftlen-vectors on the host; returns
        output_items[0] (one float per vector).  One call = one freqest::work call."""
        v = np.ascontiguousarray(vecs, dtype=np.complex64).reshape(-1)
        nvec = v.size // self.fftlen
        out = np.zeros(max(nvec, 1), dtype=np.float32)
        got = check(_lib.lib().aisx_freqest_work_host(self._h, nvec, v.ctypes.data_as(C.c_void_p),
                                                      out.ctypes.data_as(C.c_void_p)), "freqest.work_host")
        return out[:got]


class feedforward_agc_cc:
    """analog.feedforward_agc_cc(nsamples, reference) as used at python/ais_demod.py:35."""

    def __init__(self, nsamples, reference, nchan=1, max_items=65536):
        self.nchan = int(nchan)
        h = C.c_void_p()
        check(_lib.lib().aisx_agc_create(C.byref(h), int(nsamples), float(reference), self.nchan, int(max_items)),
              "feedforward_agc_cc")
        self._h = h

    def __del__(self):
        h = getattr(self, "_h", None)
        if h and _lib is not None:  # (None while the interpreter shuts down: the process is going anyway)
            _lib.lib().aisx_agc_destroy(h)
            self._h = None

    def reset(self):
        check(_lib.lib().aisx_agc_reset(self._h), "reset")

    def set_floor(self, floor_env):
        """initial max_env of the window search: 1e-4 (GNU Radio 3.7/3.8, the default) or 1e-12."""
        check(_lib.lib().aisx_agc_set_floor(self._h, float(floor_env)), "set_floor")

    def set_streaming(self, on):
        """on = False: the tile kernels for every call (the streaming kernel serves the stock window otherwise)."""
        check(_lib.lib().aisx_agc_set_streaming(self._h, 1 if on else 0), "set_streaming")

    def work(self, x, out=None, stream=None):
        x = _dev_c64(x, self.nchan)
        if out is None:
            out = torch.empty_like(x)
        check(_lib.lib().aisx_agc_process(self._h, x.data_ptr(), x.stride(0), out.data_ptr(), out.stride(0),
                                          x.shape[1], _stream_ptr(stream)), "feedforward_agc_cc.work")
        return out


_hwq_warned = False


def _warn_if_few_hw_queues():
    """The chain keeps four streams busy; the HIP runtime reads GPU_MAX_HW_QUEUES (default 4, shared by every
    stream of the process) at its first call.  Correct results either way -- but the streams then run in turn."""
    global _hwq_warned
    import os
    import warnings

    from . import HW_QUEUES_SET_TOO_LATE

    try:
        few = int(os.environ.get("GPU_MAX_HW_QUEUES", "4")) < 8
    except ValueError:
        few = True
    if (HW_QUEUES_SET_TOO_LATE or few) and not _hwq_warned:
        _hwq_warned = True
        warnings.warn("ais_amd: the pipelined chain wants GPU_MAX_HW_QUEUES >= 8 in the environment BEFORE the first HIP call "
                      "(%s); with the runtime's four hardware queues its streams share queues and the step is slower"
                      % ("the process had initialised torch.cuda before ais_amd was imported" if HW_QUEUES_SET_TOO_LATE
                         else "it is %s" % os.environ.get("GPU_MAX_HW_QUEUES", "unset")), RuntimeWarning, stacklevel=3)


class ais_demod:
    """ais.ais_demod(options) (python/ais_demod.py:21-56): the demod chain
    freq_sync -> agc -> corr_est (preamble_detect) -> msk timing recovery (clockrec)
    -> quadrature demod -> slicer -> diff decoder -> invert (:56), with the same
    option keys and constants, for `nchan` channels at once.

    `stages` selects the upstream conditioning: 'stock' (freq_sync + agc, the
    reference's connect order) or 'core' (corr_est -> msk only, the chain
    BASELINE.json's metric names)."""

    def __init__(self, options, nchan=1, max_items=65536, stages="stock", preamble_symbols=None, fused_front_end=False):
        from .modulate import gmsk_mod, modulate_vector_bc

        self._samples_per_symbol = options["samples_per_symbol"]
        self._bits_per_sec = options["bits_per_sec"]
        self._samplerate = self._samples_per_symbol * self._bits_per_sec
        self._clockrec_gain = options["clockrec_gain"]
        self._omega_relative_limit = options["omega_relative_limit"]
        self.fftlen = options["fftlen"]
        self.nchan = nchan
        self._max_items = int(max_items)
        self._chain = None
        self.stages = stages
        # freq_sync -> agc in one pass (freq_sync_agc): same results, bit for bit; off by default: the
        # separate NCO phase walk it needs is slower than fs_mix's in-kernel one when everything runs
        # in series on one stream -- it pays when the caller prepares it ahead (estimate_ahead, bench.py)
        self.fused_front_end = bool(fused_front_end)
        if stages == "stock":
            self.freq_sync = square_and_fft_sync_cc(self._samplerate, self._bits_per_sec, self.fftlen, nchan=nchan,
                                                    max_items=max_items)
            self.agc = feedforward_agc_cc(512, 2, nchan=nchan, max_items=max_items + self.fftlen)
        else:
            self.freq_sync = self.agc = None
        if preamble_symbols is None:
            self.preamble = [1, 1, 0, 0] * 7
            self.mod = gmsk_mod(int(self._samples_per_symbol), 0.4)
            self.mod_vector = modulate_vector_bc(self.mod.to_basic_block(), self.preamble, [1])
        else:
            self.mod_vector = np.asarray(preamble_symbols, dtype=np.complex64)
        self.preamble_detect = corr_est_cc(self.mod_vector, self._samples_per_symbol, 1, 0.9, nchan=nchan,
                                           max_items=max_items + self.fftlen)
        self.clockrec = msk_timing_recovery_cc(self._samples_per_symbol, self._clockrec_gain,
                                               self._omega_relative_limit, 1, nchan=nchan,
                                               max_items=max_items + self.fftlen)

    # -- pipelined step (aisx_chain_*): the path bench.py times ------------------------------
    def _chain_handle(self):
        if getattr(self, "_chain", None) is None:
            _warn_if_few_hw_queues()
            h = C.c_void_p()
            stock = self.stages == "stock"
            check(_lib.lib().aisx_chain_create(C.byref(h), self.freq_sync._h if stock else None, self.agc._h if stock else None,
                                               self.preamble_detect._h, self.clockrec._h, self.nchan, self._max_items,
                                               self.fftlen if stock else 0), "ais_demod chain")
            self._chain = h
            self._chain_outs = []
            self._chain_step = -1
        return self._chain

    def __del__(self):
        h = getattr(self, "_chain", None)
        if h and _lib is not None:
            _lib.lib().aisx_chain_destroy(h)  # (before the stage handles it borrows go)
            self._chain = None

    def work_pipelined(self, x, x_next=None, want_syms=False, outs=None, stream=None):
        """One step of the pipelined chain (aisx_chain_step) on x[nchan][n]: the same results as work(), bit
        for bit, with the sample passes of this step running beside the timing recovery of the
        previous one on the chain's own streams.  `x_next` = the NEXT step's input if it is
        already on the device (its frequency estimates and NCO phase walk are then prepared
        during this step; the next call must pass exactly that tensor, unchanged).
        Returns dict(bits, produced[, syms], step): device tensors that are complete once
        wait(step) has returned; AISX_CHAIN_DEPTH sets rotate, so a result must be consumed
        before the call three steps later.  Do not mix with work() on one object."""
        h = self._chain_handle()
        x = _dev_c64(x, self.nchan)
        nx = _dev_c64(x_next, self.nchan) if x_next is not None else None
        # (the chain reads its inputs asynchronously, on streams torch's allocator does not know of:
        # the tensors of the steps that may still be in flight stay referenced here)
        keep = getattr(self, "_chain_keep", None) or []
        keep.append((x, nx))
        self._chain_keep = keep[-(_lib.lib().aisx_chain_depth() + 1):]
        cap = self.clockrec.out_capacity
        if outs is None:
            depth = _lib.lib().aisx_chain_depth()
            while len(self._chain_outs) < depth:
                self._chain_outs.append(dict(
                    syms=torch.empty((self.nchan, cap), dtype=torch.complex64, device=x.device) if want_syms else None,
                    bits=torch.empty((self.nchan, cap), dtype=torch.uint8, device=x.device),
                    produced=torch.empty(self.nchan, dtype=torch.int32, device=x.device)))
            outs = self._chain_outs[(self._chain_step + 1) % depth]
            if want_syms and outs["syms"] is None:
                outs["syms"] = torch.empty((self.nchan, cap), dtype=torch.complex64, device=x.device)
        syms, bits, prod = outs.get("syms") if want_syms else None, outs["bits"], outs["produced"]
        step = C.c_longlong(0)
        check(_lib.lib().aisx_chain_step(
            h, x.data_ptr(), x.stride(0), x.shape[1], nx.data_ptr() if nx is not None else None,
            nx.stride(0) if nx is not None else 0, nx.shape[1] if nx is not None else 0,
            syms.data_ptr() if syms is not None else None, bits.data_ptr(), bits.stride(0), prod.data_ptr(),
            _stream_ptr(stream), C.byref(step)), "ais_demod.work_pipelined")
        self._chain_step = step.value
        return dict(bits=bits, produced=prod, syms=syms, step=step.value)

    def wait(self, step=None, stream=None, host=False):
        """`stream` (default: the current one) -- or the calling thread with host=True -- waits for the
        outputs of `step` (default: the last one issued)."""
        check(_lib.lib().aisx_chain_wait(self._chain_handle(), self._chain_step if step is None else step,
                                         None if host else _stream_ptr(stream), 1 if host else 0), "ais_demod.wait")

    def synchronize(self):
        check(_lib.lib().aisx_chain_synchronize(self._chain_handle()), "ais_demod.synchronize")

    def corr_output(self, step, chan0=0, nch=None, stream=None):
        """corr_est's delayed output of `step` (one of the last AISX_CHAIN_DEPTH), rows chan0 .. chan0 + nch - 1"""
        nch = self.nchan - chan0 if nch is None else nch
        out = torch.empty((nch, self._max_items + self.fftlen), dtype=torch.complex64, device="cuda")
        n = C.c_int(0)
        check(_lib.lib().aisx_chain_read_corr_output(self._chain_handle(), step, chan0, nch, out.data_ptr(), out.stride(0),
                                                     C.byref(n), _stream_ptr(stream)), "ais_demod.corr_output")
        return out[:, : n.value]

    def step_tags(self, step, stream=None):
        """corr_est's tags of pipelined step `step` (one of the last AISX_CHAIN_DEPTH) on the host, by step
        number (aisx_chain_read_tags): a step whose front end emitted no whole vector has none."""
        cap = self.nchan * self.preamble_detect._cap
        buf = np.zeros(cap, dtype=TAG_DTYPE)
        nt = C.c_int(0)
        check(_lib.lib().aisx_chain_read_tags(self._chain_handle(), int(step), buf.ctypes.data_as(C.c_void_p), cap, C.byref(nt),
                                              _stream_ptr(stream)), "ais_demod.step_tags")
        return buf[: nt.value].copy()

    def chain_stream(self, which):
        """the chain's streams as raw hipStream_t values: 0 sample passes, 1 timing recovery, 2 bit tail, 3 phase walk"""
        return _lib.lib().aisx_chain_stream(self._chain_handle(), which)

    def work(self, x, want_syms=False, stream=None):
        """One chain step on x[nchan][n].  Returns dict(bits, produced[, syms])."""
        y = _dev_c64(x, self.nchan)
        if self.stages == "stock":
            if self.fused_front_end:
                y, _ = freq_sync_agc(self.freq_sync, self.agc, y, stream=stream)
            else:
                y, _ = self.freq_sync.work(y, stream=stream)
            if y.shape[1] == 0:
                return dict(bits=None, produced=None, syms=None)
            if not self.fused_front_end:
                y = self.agc.work(y, stream=stream)
        y, _ = self.preamble_detect.work(y, stream=stream)
        r = self.clockrec.work(y, tags_from=self.preamble_detect, want_syms=want_syms, stream=stream)
        return r


def firdes_low_pass(gain, sampling_freq, cutoff_freq, transition_width):
    """filter.firdes.low_pass(gain, fs, cutoff, transition) with the default Hamming
    window, as python/radio.py:51 calls it ([GR] firdes.cc: windowed sinc, DC gain
    normalised).  Host side, init only."""
    ntaps = int(53.0 * sampling_freq / (22.0 * transition_width))
    if (ntaps & 1) == 0:
        ntaps += 1
    m = (ntaps - 1) // 2
    n = np.arange(-m, m + 1, dtype=np.float64)
    w = 0.54 - 0.46 * np.cos(2 * np.pi * np.arange(ntaps) / (ntaps - 1))
    fwt0 = 2 * np.pi * cutoff_freq / sampling_freq
    with np.errstate(invalid="ignore", divide="ignore"):
        taps = np.where(n == 0, fwt0 / np.pi, np.sin(n * fwt0) / (n * np.pi)) * w
    taps = taps.astype(np.float32).astype(np.float64)
    fmax = taps[m] + 2 * taps[m + 1:].sum()
    return (taps * (gain / fmax)).astype(np.float32)


class pfb_channelizer_ccf:
    """Wideband front end (BASELINE config 5): all `nlanes` uniformly spaced channels of
    one wideband stream at once; lane m is what
    freq_xlating_fir_filter_ccf(decim, taps, m*fs/nlanes, fs) (python/radio.py:52-54)
    would produce."""

    def __init__(self, nlanes, taps, decim=None, nstreams=1, max_frames=4096):
        t = np.ascontiguousarray(taps, dtype=np.float32)
        self.nlanes, self.decim, self.nstreams = int(nlanes), int(decim or nlanes), int(nstreams)
        h = C.c_void_p()
        check(_lib.lib().aisx_pfb_create(C.byref(h), self.nlanes, self.decim, t.ctypes.data_as(C.c_void_p), t.size,
                                         self.nstreams, int(max_frames)), "pfb_channelizer_ccf")
        self._h = h

    def __del__(self):
        h = getattr(self, "_h", None)
        if h and _lib is not None:  # (None while the interpreter shuts down: the process is going anyway)
            _lib.lib().aisx_pfb_destroy(h)
            self._h = None

    def work(self, x, stream=None):
        x = _dev_c64(x, self.nstreams)
        n = x.shape[1]
        nf = n // self.decim
        out = torch.empty((self.nstreams * self.nlanes, max(nf, 1)), dtype=torch.complex64, device=x.device)
        got = C.c_int(0)
        check(_lib.lib().aisx_pfb_process(self._h, x.data_ptr(), x.stride(0), n, out.data_ptr(), out.stride(0),
                                          C.byref(got), _stream_ptr(stream)), "pfb_channelizer_ccf.work")
        return out[:, : got.value]


class freq_xlating_fir_filter_ccf:
    """filter.freq_xlating_fir_filter_ccf(decimation, taps, center_freq, sampling_freq) (python/radio.py:49-54) for
    any decimation, real prototype and centre frequency, batched: `nstreams` input streams, and per stream one output
    channel per centre frequency.  `center_freq`: a float, a sequence of per-channel frequencies shared by all
    streams, or an (nstreams, nchan) array.  Output row s * nchan + c is stream s at centre c (the rows
    ais_demod.work_pipelined takes).  Streaming: any call length, any split of the input gives the same bits."""

    def __init__(self, decimation, taps, center_freq, sampling_freq, nstreams=1, max_items=1 << 20):
        t = np.ascontiguousarray(taps, dtype=np.float32).ravel()
        self.nstreams = int(nstreams)
        f = np.asarray(center_freq, dtype=np.float64)
        if f.ndim == 0:
            f = f.reshape(1, 1)
        if f.ndim == 1:
            f = f.reshape(1, -1)
        if f.ndim != 2 or f.shape[0] not in (1, self.nstreams) or f.shape[1] < 1:
            raise ValueError("freq_xlating_fir_filter_ccf: center_freq must be a float, a sequence of per-channel "
                             "frequencies or an (nstreams, nchan) array")
        f = np.ascontiguousarray(np.broadcast_to(f, (self.nstreams, f.shape[1])))
        self.decimation, self.nchan, self.sampling_freq = int(decimation), int(f.shape[1]), float(sampling_freq)
        self.max_items = int(max_items)
        h = C.c_void_p()
        check(_lib.lib().aisx_xlate_create(C.byref(h), self.decimation, t.ctypes.data_as(C.c_void_p), t.size,
                                           f.ctypes.data_as(C.c_void_p), self.nchan, self.sampling_freq, self.nstreams,
                                           self.max_items), "freq_xlating_fir_filter_ccf")
        self._h = h
        self.ntaps = t.size

    def __del__(self):
        h = getattr(self, "_h", None)
        if h and _lib is not None:
            _lib.lib().aisx_xlate_destroy(h)
            self._h = None

    def output_count(self, n):
        r = _lib.lib().aisx_xlate_output_count(self._h, int(n))
        check(min(r, 0), "freq_xlating_fir_filter_ccf.output_count")
        return r

    def center_freq(self, stream=0, chan=0):
        f = C.c_double(0.0)
        check(_lib.lib().aisx_xlate_center_freq(self._h, stream, chan, C.byref(f)), "freq_xlating_fir_filter_ccf.center_freq")
        return f.value

    def set_center_freq(self, f, stream=None, chan=None):
        """from the next call on (GNU Radio 3.8: the rotator goes on from its phase); stream / chan None = all"""
        for s in range(self.nstreams) if stream is None else [stream]:
            for c in range(self.nchan) if chan is None else [chan]:
                check(_lib.lib().aisx_xlate_set_center_freq(self._h, s, c, float(f)),
                      "freq_xlating_fir_filter_ccf.set_center_freq")

    def reset(self):
        check(_lib.lib().aisx_xlate_reset(self._h), "freq_xlating_fir_filter_ccf.reset")

    def work(self, x, out=None, stream=None, fmt=None, scale=1.0, bias=0.0):
        """x [nstreams][n] complex64 (a device tensor, any row stride); returns the [nstreams*nchan][nout] device
        tensor, or a view of `out` ([nstreams*nchan][>= nout], any row stride) holding the outputs.
        fmt "cs16" / "cs8" / "cu8": x is a device tensor [nstreams][n][2] of int16 / int8 / uint8 (re, im), taken as
        ((float)raw - bias) * scale where the filter stages its window (aisx_xlate_process_fmt): the same bits as
        work() on the converted values"""
        code = _fmt_code(fmt)
        if code == _lib.AISX_FMT_CF32:
            x = _dev_c64(x, self.nstreams)
        else:
            want = SAMPLE_FORMATS[code][2]
            if not isinstance(x, torch.Tensor) or not x.is_cuda or x.dtype != want or x.dim() != 3 or x.shape[0] != self.nstreams \
                    or x.shape[2] != 2:
                raise TypeError("freq_xlating_fir_filter_ccf.work: fmt %s takes a device tensor [%d][n][2] of %s"
                                % (SAMPLE_FORMATS[code][0], self.nstreams, want))
            if x.stride(2) != 1 or x.stride(1) != 2 or x.stride(0) % 2:
                x = x.contiguous()
        n = x.shape[1]
        nout = self.output_count(n)
        rows = self.nstreams * self.nchan
        if out is None:
            out = torch.empty((rows, max(nout, 1)), dtype=torch.complex64, device=x.device)
        elif out.dtype != torch.complex64 or out.dim() != 2 or out.shape[0] != rows or out.shape[1] < nout or out.stride(1) != 1:
            raise ValueError("freq_xlating_fir_filter_ccf.work: out must be complex64 [%d][>= %d] with unit column stride"
                             % (rows, nout))
        got = C.c_int(0)
        if code == _lib.AISX_FMT_CF32:
            check(_lib.lib().aisx_xlate_process(self._h, x.data_ptr(), x.stride(0), n, out.data_ptr(), out.stride(0),
                                                C.byref(got), _stream_ptr(stream)), "freq_xlating_fir_filter_ccf.work")
        else:
            check(_lib.lib().aisx_xlate_process_fmt(self._h, x.data_ptr(), code, float(scale), float(bias), x.stride(0) // 2, n,
                                                    out.data_ptr(), out.stride(0), C.byref(got), _stream_ptr(stream)),
                  "freq_xlating_fir_filter_ccf.work")
        return out[:, : got.value]


# AISX_FMT_* -> (name, numpy dtype of re / im, torch dtype)
SAMPLE_FORMATS = {
    _lib.AISX_FMT_CF32: ("cf32", np.float32, torch.float32),
    _lib.AISX_FMT_CS16: ("cs16", np.int16, torch.int16),
    _lib.AISX_FMT_CS8: ("cs8", np.int8, torch.int8),
    _lib.AISX_FMT_CU8: ("cu8", np.uint8, torch.uint8),
}


def _fmt_code(fmt):
    if fmt is None:
        return _lib.AISX_FMT_CF32
    for code, (name, _, _) in SAMPLE_FORMATS.items():
        if fmt == name or fmt == code:
            return code
    raise ValueError("unknown sample format %r: one of %s" % (fmt, [v[0] for v in SAMPLE_FORMATS.values()]))


class ais_rx:
    """ais_rx(freq, rate, designator) (python/radio.py:40-73): freq_xlating_fir_filter_ccf -> ais_demod ->
    hdlc_deframer_bp -> pdu_to_nmea, as one handle (aisx_rx_*) for `nstreams` sources at `rate`, fed from host memory
    in the source's own sample format.  `freq` / `designator`: a scalar, or one per centre of every stream
    (radio.py:88-89: (-25e3, 25e3) and ("A", "B")); `freq` may also be an (nstreams, ncentres) array.  Decimation
    int(rate / 48000), taps low_pass(1, rate, 11e3, 1e3), samples_per_symbol rate / decimation / 9600, gain 0.04, limit
    0.01, fftlen 1024, deframer (11, 64), as the reference sets them.

    fmt "cf32" (complex64 blocks) or "cs16" / "cs8" / "cu8" (blocks [nstreams][block_items][2] of int16 / int8 /
    uint8, value ((float)raw - bias) * scale).  Every block is block_items items per stream, a multiple of the
    decimation.  Output row s * ncentres + c (a record's chan) is stream s at centre c.

        rx = ais_amd.ais_rx((-25e3, 25e3), 250e3, ("A", "B"), nstreams=8, fmt="cu8", scale=1 / 128, bias=127.5)
        while True:
            source.read_into(rx.slot())          # the pinned slot: the copy to the device reads it in place
            rx.submit()                          # returns at once; block k is issued when block k + 1 arrives
            while (r := rx.pop()) is not None:   # (block, records, text) of every block that has finished
                sys.stdout.buffer.write(r[2])

    decode=True queues the ITU-R M.1371 field decoder behind the NMEA stage; pop_messages() then returns (block,
    records, text, messages) with one MSG_DTYPE row (mmsi, lon, lat, sog, cog, name ...) per record.

    tracks=capacity (implies decode=True) also keeps a vessel table of that many vessels on the device, merged from
    every block's messages behind the decoder with stamp = the block's number: read_tracks() gives the table,
    read_changed_tracks() the vessels the last issued block touched.

    detector="mlse" puts the 4-state sequence detector (ais_amd.mlse_detector_batch, BT = bt) between the timing recovery
    and the deframer: about 2 dB more sensitivity near the threshold.  It decides a symbol once 80 to
    143 later ones have arrived, so a burst that ends in a block's last 79 symbols comes out with the next block.

    repair=rules (ais_amd.AIS_REPAIR_RULES, or as ais_amd.hdlc_deframer_bp takes them) turns the deframer's single-bit
    repair on: a burst with one wrong bit still gives its sentence, and popped_repairs() tells which records of the
    block popped last were put right.  repair_events=mask (ais_amd.AIS_REPAIR_EVENTS: all) makes it the repair of one
    error event: one wrong bit, the two adjacent wrong bits one wrong decision of the differential slicer gives, and the
    two wrong bits two apart of the sequence detector's error event.  ais_amd.repair_mark reads a mark.

    nmea="standard" makes the text the standard form (ais_amd.pdu_to_nmea(..., standard=True): exact armouring, message
    ids, tag blocks) where the default, "reference", is the reference's text byte for byte.  stations: None, one str for
    every stream or nstreams str, the s: field of every sentence of that stream; t0: the second of block 0's first
    item, block b's sentences carry c: t0 + floor(b * block_items / rate) -- or no time for t0 < 0.

    dedup=window (0..15) puts the duplicate suppression (ais_amd.pdu_dedup_batch) between the deframer and the NMEA stage,
    with stamp = the block's number: of the PDUs of a block that carry one payload -- one transmission heard on several
    streams -- the first is kept, and a payload kept within the last `window` blocks is suppressed.  Records, text,
    messages and popped_repairs() are those of the kept records, the vessel table counts transmissions, and
    popped_dedup() gives the stage's counts for the block popped last.

    Each of these options is also an enable_*() method for a receiver that has not yet taken a slot or a block; the order
    of the calls does not matter, and one that raises leaves the receiver as it was.
    """

    def __init__(self, freq, rate, designator, nstreams=1, fmt="cf32", scale=1.0, bias=0.0, block_items=None,
                 preamble_symbols=None, taps=None, max_pdus_per_block=1 << 16, decode=False, tracks=None, repair=None,
                 detector=None, bt=0.4, repair_events=1, nmea="reference", stations=None, t0=-1, dedup=None):
        from .batch_framing import PDU_DTYPE
        from .modulate import gmsk_mod, modulate_vector_bc

        self.nstreams, self.rate = int(nstreams), float(rate)
        f = np.asarray(freq, dtype=np.float64)
        if f.ndim == 0:
            f = f.reshape(1, 1)
        if f.ndim == 1:
            f = f.reshape(1, -1)
        if f.ndim != 2 or f.shape[0] not in (1, self.nstreams) or f.shape[1] < 1:
            raise ValueError("ais_rx: freq must be a float, a sequence of per-centre frequencies or an (nstreams, "
                             "ncentres) array")
        f = np.ascontiguousarray(np.broadcast_to(f, (max(self.nstreams, 1), f.shape[1])))
        self.ncentres = int(f.shape[1])
        des = [designator] if isinstance(designator, (str, bytes)) else list(designator)
        des = [d.encode() if isinstance(d, str) else bytes(d) for d in des]
        if len(des) != self.ncentres:
            raise ValueError("ais_rx: %d designators for %d centres" % (len(des), self.ncentres))
        self.fmt = _fmt_code(fmt)
        self._item = np.dtype(np.complex64) if self.fmt == _lib.AISX_FMT_CF32 else np.dtype(SAMPLE_FORMATS[self.fmt][1])
        self.decimation = int(self.rate / 48000) if np.isfinite(self.rate) else 0
        if block_items is None:
            block_items = 65536 * max(self.decimation, 1)
        self.block_items = int(block_items)
        if taps is None and self.decimation >= 1:
            taps = firdes_low_pass(1.0, self.rate, 11e3, 1e3)
        t = np.ascontiguousarray(taps, dtype=np.float32).ravel() if taps is not None else None
        if preamble_symbols is None and self.decimation >= 1:
            sps = self.rate / self.decimation / 9600.0
            preamble_symbols = modulate_vector_bc(gmsk_mod(int(sps), 0.4).to_basic_block(), [1, 1, 0, 0] * 7, [1])
        sym = np.ascontiguousarray(preamble_symbols, dtype=np.complex64) if preamble_symbols is not None else np.zeros(1, np.complex64)
        _warn_if_few_hw_queues()
        h = C.c_void_p()
        check(_lib.lib().aisx_rx_create(C.byref(h), self.rate, self.nstreams, self.ncentres, f.ctypes.data_as(C.c_void_p),
                                        (C.c_char_p * len(des))(*des), self.fmt, float(scale), float(bias), self.block_items,
                                        t.ctypes.data_as(C.c_void_p) if t is not None else None, t.size if t is not None else 0,
                                        sym.ctypes.data_as(C.c_void_p), sym.size, int(max_pdus_per_block)), "ais_rx")
        self._h = h
        if nmea not in ("reference", "standard"):
            raise ValueError("ais_rx: nmea is 'reference' or 'standard'")
        if nmea == "reference" and (stations is not None or t0 >= 0):
            raise ValueError("ais_rx: stations and t0 belong to nmea='standard'")
        self.nmea = "reference"
        if nmea == "standard":
            self.enable_standard_nmea(stations, t0)  # (reads the geometry itself: the text of a block can be longer)
        else:
            self._read_geometry()
        self._recs = np.zeros(int(max_pdus_per_block), dtype=PDU_DTYPE)
        self.status = 0  # of the block popped last (AISX_MSK_ST_* | AISX_RX_ST_*)
        self.decode = False
        self._cols = self._strs = None
        self.tracks = 0
        self.repair = False
        self.detector = None
        if detector is not None:
            self.enable_detector(detector, bt)
        if repair is not None:
            self.enable_repair(repair, repair_events)
        if decode:
            self.enable_messages()
        if tracks:
            self.enable_tracks(tracks)
        self.dedup = None
        if dedup is not None:
            self.enable_dedup(dedup)

    def __del__(self):
        h = getattr(self, "_h", None)
        if h and _lib is not None:
            _lib.lib().aisx_rx_destroy(h)
            self._h = None

    def _shape(self):
        return (self.nstreams, self.block_items) if self.fmt == _lib.AISX_FMT_CF32 else (self.nstreams, self.block_items, 2)

    def _read_geometry(self):
        """the handle's geometry, and a text buffer for the longest text a block can give"""
        d, T, nch, nin, nres, tc = C.c_int(), C.c_int(), C.c_int(), C.c_int(), C.c_int(), C.c_long()
        check(_lib.lib().aisx_rx_geometry(self._h, C.byref(d), C.byref(T), C.byref(nch), C.byref(nin), C.byref(nres), C.byref(tc)),
              "ais_rx")
        self.items_per_block, self.nchan, self.input_slots, self.result_slots = T.value, nch.value, nin.value, nres.value
        self._text = np.zeros(max(tc.value, 1), dtype=np.uint8)

    def enable_standard_nmea(self, stations=None, t0=-1):
        """what nmea="standard", stations=, t0= does: from the first block on the text is the standard form, which can be
        longer (the text buffer is made again for it).  ValueError the second time, once a slot has been taken or a block
        pushed, and for a station the tag block cannot carry."""
        if stations is None or isinstance(stations, (str, bytes)):
            stations = [stations or ""] * self.nstreams
        sta = [x.encode() if isinstance(x, str) else bytes(x) for x in stations]
        if len(sta) != self.nstreams:
            raise ValueError("ais_rx: %d stations for %d streams" % (len(sta), self.nstreams))
        check(_lib.lib().aisx_rx_enable_standard_nmea(self._h, (C.c_char_p * len(sta))(*sta), int(t0)), "ais_rx")
        self.nmea = "standard"
        self._read_geometry()

    def slot(self):
        """the pinned host slot of the next block as a numpy view ([nstreams][block_items] complex64, or
        [nstreams][block_items][2] of the format's integer type): fill it, then submit().  Blocks only while every slot
        is still being copied from."""
        p, stride = C.c_void_p(), C.c_long()
        check(_lib.lib().aisx_rx_acquire(self._h, C.byref(p), C.byref(stride)), "ais_rx.slot")
        shape = self._shape()
        nbytes = int(np.prod(shape)) * self._item.itemsize
        buf = (C.c_char * nbytes).from_address(p.value)
        return np.frombuffer(buf, dtype=self._item).reshape(shape)

    def submit(self):
        """queues the slot filled last; returns the block's number.  OverflowError when every result slot waits to be
        popped (nothing was queued: pop(), then submit() again)."""
        b = C.c_longlong(-1)
        check(_lib.lib().aisx_rx_submit(self._h, C.byref(b)), "ais_rx.submit")
        return b.value

    def push(self, iq):
        """slot() + copy + submit() for a host array of the format's dtype, [nstreams][block_items] complex64 or
        [nstreams][block_items][2] integers"""
        a = np.asarray(iq)
        if a.dtype != self._item or a.shape != self._shape():
            raise TypeError("ais_rx.push: a block is %s of %s, got %s of %s" % (self._shape(), self._item, a.shape, a.dtype))
        a = np.ascontiguousarray(a)
        b = C.c_longlong(-1)
        check(_lib.lib().aisx_rx_push(self._h, a.ctypes.data_as(C.c_void_p), self.block_items, C.byref(b)), "ais_rx.push")
        return b.value

    def flush(self):
        """issues the block that waits for its successor (same results, no look-ahead for it)"""
        check(_lib.lib().aisx_rx_flush(self._h), "ais_rx.flush")

    def pop(self, wait=False):
        """(block, records, text) of the oldest finished block not yet popped -- records a PDU_DTYPE array (chan,
        end_bit, offset / len of each sentence in text), text the NMEA bytes, '\n' after every sentence -- or None when
        none has finished (wait=True: blocks until the next issued block has; None when none is issued)"""
        return self._pop(wait, False)

    def _pop(self, wait, messages):
        """pop() or pop_messages(): one call of the handle's, then the popped block out of the buffers"""
        from .framing import msg_table

        b, tl, nr, st = C.c_longlong(-1), C.c_long(0), C.c_int(0), C.c_int(0)
        args = (self._h, 1 if wait else 0, C.byref(b), self._text.ctypes.data_as(C.c_void_p), self._text.size, C.byref(tl),
                self._recs.ctypes.data_as(C.c_void_p), self._recs.size, C.byref(nr))
        if not messages:
            check(_lib.lib().aisx_rx_pop(*args, C.byref(st)), "ais_rx.pop")
        else:
            cols = self._cols.ctypes.data_as(C.c_void_p) if self.decode else None
            strs = self._strs.ctypes.data_as(C.c_void_p) if self.decode else None
            check(_lib.lib().aisx_rx_pop_messages(*args, cols, self._cols.shape[1] if self.decode else 0, strs, C.byref(st)),
                  "ais_rx.pop_messages")
        if b.value < 0:
            return None
        self.status = st.value
        r = (b.value, self._recs[: nr.value].copy(), self._text[: tl.value].tobytes())
        return r + (msg_table(self._cols, self._strs, nr.value),) if messages else r

    def enable_messages(self):
        """what decode=True does: from the first block on, the field decoder runs behind the NMEA stage and
        pop_messages() hands out the table.  ValueError once a slot has been taken or a block pushed."""
        from .framing import MSG_COLUMNS

        check(_lib.lib().aisx_rx_enable_messages(self._h), "ais_rx.enable_messages")
        if not self.decode:
            self._cols = np.zeros((len(MSG_COLUMNS), self._recs.size), dtype=np.int32)
            self._strs = np.zeros((self._recs.size, _lib.AISX_MSG_STR), dtype=np.uint8)
        self.decode = True

    def pop_messages(self, wait=False):
        """pop() plus the block's decoded messages: (block, records, text, messages), messages a MSG_DTYPE array
        with row i = ais_amd.msg_decode of record i's PDU.  Needs decode=True (ValueError otherwise)."""
        return self._pop(wait, True)

    def enable_repair(self, rules, events=1):
        """what repair=rules, repair_events=events does: the deframer repairs single-bit errors (events: the error events
        of the mask) by these rules from the first block on.  ValueError once a slot has been taken or a block pushed,
        and for rules the deframer (11, 64) cannot take or a bad mask."""
        from .framing import repair_rules

        r = repair_rules(rules)
        check(_lib.lib().aisx_rx_enable_repair_events(self._h, r.ctypes.data_as(C.c_void_p) if r.size else None, r.size, int(events)),
              "ais_rx.enable_repair")
        self.repair = True

    def enable_detector(self, detector="mlse", bt=0.4):
        """what detector="mlse" does: from the first block on the deframer reads the bits of the 4-state sequence
        detector (ais_amd.mlse_detector_batch) of BT = bt GMSK instead of the slicer's.  The detector holds back a
        channel's last 16 to 79 symbols until more input follows: flush() does not flush it.  ValueError for another
        name, and once a slot has been taken or a block pushed."""
        if detector != "mlse":
            raise ValueError("ais_rx: detector must be None or 'mlse', got %r" % (detector,))
        check(_lib.lib().aisx_rx_enable_mlse(self._h, float(bt)), "ais_rx.enable_detector")
        self.detector = "mlse"

    def popped_repairs(self):
        """the repair marks of the block popped last (by pop() or pop_messages()), one per record: an int32 array, -1 for
        a frame delivered as received, else the index of the first flipped bit in the frame (payload + FCS, bit 0 the first
        received) | event id << 16 (ais_amd.repair_mark).  Needs repair= (ValueError otherwise)."""
        fix = np.zeros(self._recs.size, dtype=np.int32)
        n = C.c_int(0)
        check(_lib.lib().aisx_rx_popped_repairs(self._h, fix.ctypes.data_as(C.c_void_p), fix.size, C.byref(n)),
              "ais_rx.popped_repairs")
        return fix[: n.value].copy()

    def enable_dedup(self, window):
        """what dedup=window does.  ValueError the second time, once a slot has been taken or a block pushed, and for a
        window outside [0, 15]."""
        check(_lib.lib().aisx_rx_enable_dedup(self._h, int(window)), "ais_rx.enable_dedup")
        self.dedup = int(window)

    def popped_dedup(self):
        """the duplicate suppression's counts for the block popped last, a dict of ais_amd.DEDUP_COUNTS (in, kept,
        dup_call, dup_window, bad_len).  Needs dedup= (ValueError otherwise)."""
        from .framing import DEDUP_COUNTS

        cnt = np.zeros(len(DEDUP_COUNTS), dtype=np.int32)
        check(_lib.lib().aisx_rx_popped_dedup(self._h, cnt.ctypes.data_as(C.c_void_p)), "ais_rx.popped_dedup")
        return {k: int(v) for k, v in zip(DEDUP_COUNTS, cnt)}

    def enable_tracks(self, capacity):
        """what tracks=capacity does: enable_messages(), and from the first block on the vessel table is updated
        behind the decoder.  ValueError once a slot has been taken or a block pushed."""
        check(_lib.lib().aisx_rx_enable_tracks(self._h, int(capacity)), "ais_rx.enable_tracks")
        self.enable_messages()
        self.tracks = int(capacity)

    def read_tracks(self, first=0, n=None):
        """(block, vessels): the table after the update of every block issued so far -- `block` the number of the
        last of them (-1: none) -- as a TRACK_DTYPE array of vessels [first, first + n).  Waits for the tail stream."""
        from .batch_framing import TRACK_COLUMNS, _track_table

        n = self.tracks if n is None else int(n)
        cols = np.zeros((len(TRACK_COLUMNS), max(n, 1)), dtype=np.int32)
        strs = np.zeros((max(n, 1), _lib.AISX_MSG_STR), dtype=np.uint8)
        nv, b = C.c_int(0), C.c_longlong(-1)
        check(_lib.lib().aisx_rx_read_tracks(self._h, int(first), n, cols.ctypes.data_as(C.c_void_p), cols.shape[1],
                                             strs.ctypes.data_as(C.c_void_p), C.byref(nv), C.byref(b)), "ais_rx.read_tracks")
        return b.value, _track_table(cols, strs, max(0, min(n, nv.value - int(first))))

    def read_changed_tracks(self):
        """(block, vessels): the vessels the last issued block's update merged a row into, as a TRACK_CHANGED_DTYPE
        array (field "vessel" = the index), ordered by the first row that touched each"""
        from .batch_framing import TRACK_COLUMNS, _track_table

        cap = max(self._recs.size, 1)
        idx = np.zeros(cap, dtype=np.int32)
        cols = np.zeros((len(TRACK_COLUMNS), cap), dtype=np.int32)
        strs = np.zeros((cap, _lib.AISX_MSG_STR), dtype=np.uint8)
        nc, b = C.c_int(0), C.c_longlong(-1)
        check(_lib.lib().aisx_rx_read_changed_tracks(self._h, idx.ctypes.data_as(C.c_void_p), cols.ctypes.data_as(C.c_void_p), cap,
                                                     strs.ctypes.data_as(C.c_void_p), cap, C.byref(nc), C.byref(b)),
              "ais_rx.read_changed_tracks")
        return b.value, _track_table(cols, strs, nc.value, idx)

    def set_center_freq(self, f, stream=None, chan=None):
        """from the next submitted block on; stream / chan None = all"""
        for s in range(self.nstreams) if stream is None else [stream]:
            for c in range(self.ncentres) if chan is None else [chan]:
                check(_lib.lib().aisx_rx_set_center_freq(self._h, s, c, float(f)), "ais_rx.set_center_freq")
