"""The batched freq_xlating_fir_filter_ccf reading the source's own sample format (k_xlate.h's loaders: cs16, cs8, cu8)
on the CPU lane model (tests/emul_xlate_fmt): raw integers over each format's full range, both extremes included,
through ragged calls; the outputs equal, bit for bit, the fc32 path fed numpy's conversion
(raw.astype(float32) - float32(bias)) * float32(scale).  Also a stream that changes format between calls, and the
argument checks of aisx_xlate_process_fmt and aisx_rx_create, which need no device.  -m "not gpu"."""
import ctypes as C

import numpy as np
import pytest

import emul_load
from emul_load import f32, f64, i32, lng, vp
import torch  # noqa: F401  (before libaisx.so: one HIP runtime in the process)
import xlate_cases as xc

NT = 64
CF32, CS16, CS8, CU8 = 0, 1, 2, 3
DTYPES = {CS16: np.int16, CS8: np.int8, CU8: np.uint8}
# (scale, bias) per format: powers of two and the RTL-SDR's half-integer bias, and values that round
PARAMS = {CS16: [(2.0 ** -13, 0.0), (1.0 / 3000.0, 0.25)], CS8: [(2.0 ** -6, 0.0), (0.013, -0.5)],
          CU8: [(2.0 ** -7, 127.5), (1.0 / 127.0, 127.4)]}


def emu():
    return emul_load.load("emul_xlate_fmt", [
        ("emu_xlate_fmt_create", vp, [i32, vp, i32, vp, i32, f64, i32, i32, i32]),
        ("emu_xlate_fmt_destroy", None, [vp]),
        ("emu_xlate_fmt_output_count", None, [vp, i32]),
        ("emu_xlate_fmt_item_bytes", None, [i32]),
        ("emu_xlate_fmt_process", None, [vp, vp, i32, f32, f32, lng, i32, vp, lng]),
    ])


class EmuFmt:
    def __init__(self, D, taps, freqs, fs, max_items, nt=NT):
        taps = np.ascontiguousarray(taps, np.float32)
        freqs = np.ascontiguousarray(freqs, np.float64)
        self.ns, self.nch = freqs.shape
        self.h = emu().emu_xlate_fmt_create(D, taps.ctypes.data, taps.size, freqs.ctypes.data, self.nch, fs, self.ns,
                                            max_items, nt)
        assert self.h

    def __del__(self):
        emu().emu_xlate_fmt_destroy(self.h)

    def work(self, x, fmt=CF32, scale=1.0, bias=0.0):
        """x [ns][n] complex64, or [ns][n][2] integers of the format (any row stride in items); returns [ns*nch][nout]"""
        n = x.shape[1]
        item = 8 if fmt == CF32 else 2 * x.dtype.itemsize
        assert x.strides[0] % item == 0 and emu().emu_xlate_fmt_item_bytes(fmt) == item
        cnt = emu().emu_xlate_fmt_output_count(self.h, n)
        out = np.zeros((self.ns * self.nch, cnt + 3), np.complex64)
        got = emu().emu_xlate_fmt_process(self.h, x.ctypes.data, fmt, scale, bias, x.strides[0] // item, n, out.ctypes.data,
                                          out.strides[0] // 8)
        assert got == cnt
        return out[:, :got]


def raw_input(rng, fmt, ns, N):
    """uniform over the format's whole range, both extremes placed where every call sequence meets them"""
    info = np.iinfo(DTYPES[fmt])
    r = rng.integers(info.min, info.max + 1, size=(ns, N, 2)).astype(DTYPES[fmt])
    r[:, 0, 0], r[:, 0, 1] = info.min, info.max
    r[:, N // 2, 0], r[:, N // 2, 1] = info.max, info.min
    r[:, -1, :] = info.min
    return r


def convert(raw, scale, bias):
    """the specification: two float32 operations, each rounded once"""
    v = (raw.astype(np.float32) - np.float32(bias)) * np.float32(scale)
    assert v.dtype == np.float32
    return np.ascontiguousarray(v).view(np.complex64)[..., 0]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def subset():
    """of xlate_cases.matrix(): decimations 1, 5, 50 (and 2, 7 while the tap count is small), which brings odd and even
    strides, one to three centres and one or two streams; plus the R = 2 case"""
    cases = [c for c in xc.matrix() if c["D"] in (1, 5, 50) or (c["D"] in (2, 7) and c["L"] <= 603)]
    assert {c["D"] for c in cases} >= {1, 5, 50} and {c["nch"] for c in cases} >= {1, 3}
    return cases


@pytest.mark.parametrize("fmt", [CS16, CS8, CU8])
def test_format_path_equals_fc32_path_on_numpy_conversion(fmt):
    n = 0
    for i, case in enumerate(subset()):
        taps = xc.lowpass(case["L"], case["D"])
        rng = np.random.default_rng(7000 + 10 * i + fmt)
        raw = raw_input(rng, fmt, case["ns"], case["N"])
        scale, bias = PARAMS[fmt][i % 2]
        x = convert(raw, scale, bias)
        sizes = xc.calls(case["D"], case["N"], case["max_items"])
        a = EmuFmt(case["D"], taps, case["freqs"], xc.FS, case["max_items"])
        b = EmuFmt(case["D"], taps, case["freqs"], xc.FS, case["max_items"])
        o = 0
        for s in sizes:
            ya = a.work(raw[:, o:o + s], fmt, scale, bias)
            yb = b.work(x[:, o:o + s])
            assert ya.shape == yb.shape and np.array_equal(bits(ya), bits(yb)), (case["D"], case["L"], o, s)
            o += s
        # split invariance carries over: the whole input in one call, from a wider (strided) buffer
        wide = np.zeros((case["ns"], case["N"] + 5, 2), raw.dtype)
        wide[:, :case["N"]] = raw
        g = EmuFmt(case["D"], taps, case["freqs"], xc.FS, case["N"])
        whole = g.work(wide[:, :case["N"]], fmt, scale, bias)
        h = EmuFmt(case["D"], taps, case["freqs"], xc.FS, case["N"])
        assert np.array_equal(bits(whole), bits(h.work(x)))
        n += 1
    print("format %d: %d cases bit for bit" % (fmt, n))


def test_stock_shape_with_the_device_plan():
    """ais_rx's shape on the device's 256 lanes (R = 4, the padded window), cu8 with the RTL-SDR's bias"""
    import ais_amd

    taps = ais_amd.firdes_low_pass(1.0, xc.FS, 11e3, 1e3)
    freqs = np.array([[-25e3, 25e3]] * 2)
    rng = np.random.default_rng(18)
    N = 5 * 1400 + 3
    raw = raw_input(rng, CU8, 2, N)
    x = convert(raw, 2.0 ** -7, 127.5)
    a = EmuFmt(5, taps, freqs, xc.FS, 1200, nt=256)
    b = EmuFmt(5, taps, freqs, xc.FS, N, nt=256)
    o, ys = 0, []
    for s in xc.calls(5, N, 1200):
        ys.append(a.work(raw[:, o:o + s], CU8, 2.0 ** -7, 127.5))
        o += s
    assert np.array_equal(bits(np.concatenate(ys, axis=1)), bits(b.work(x)))


def test_a_stream_may_change_format_between_calls():
    """the history is converted values: fc32, cs16, cu8, cs8, fc32 ... calls of one stream equal the all-fc32 run"""
    for D, L in ((5, 603), (1, 50), (50, 603)):
        taps = xc.lowpass(L, D)
        freqs = np.array([[25e3, -25e3, 12345.678]])
        rng = np.random.default_rng(31 + D)
        sizes = [s for s in xc.calls(D, 40 * D + 7, 2 * D + 29)]
        a = EmuFmt(D, taps, freqs, xc.FS, 2 * D + 29)
        b = EmuFmt(D, taps, freqs, xc.FS, 2 * D + 29)
        order = [CF32, CS16, CU8, CS8]
        for i, s in enumerate(sizes):
            fmt = order[i % 4]
            if fmt == CF32:
                x = xc.signal(rng, 1, s, freqs)
                ya = a.work(x)
            else:
                raw = raw_input(rng, fmt, 1, s)
                scale, bias = PARAMS[fmt][i % 2]
                x = convert(raw, scale, bias)
                ya = a.work(raw, fmt, scale, bias)
            assert np.array_equal(bits(ya), bits(b.work(x))), (D, L, i)


def test_fc32_loader_is_the_existing_model():
    """the default loader through the new model equals tests/emul_xlate's build of the same body"""
    import test_xlate_model as tm

    case = [c for c in xc.matrix() if c["D"] == 5 and c["L"] == 603][0]
    taps, x = xc.inputs(case)
    a = EmuFmt(case["D"], taps, case["freqs"], xc.FS, case["N"])
    b = tm.EmuXlate(case["D"], taps, case["freqs"], xc.FS, case["N"])
    assert np.array_equal(bits(a.work(x)), bits(b.work(x)))


def test_format_arguments_are_checked():
    taps = np.ones(8, np.float32)
    fr = np.zeros(2)
    h = emu().emu_xlate_fmt_create(5, taps.ctypes.data, 8, fr.ctypes.data, 2, 250e3, 1, 100, NT)
    raw = np.zeros((1, 10, 2), np.int16)
    out = np.zeros((2, 8), np.complex64)
    for fmt, scale, bias in ((4, 1.0, 0.0), (-1, 1.0, 0.0), (CS16, float("nan"), 0.0), (CS16, float("inf"), 0.0),
                             (CS8, 1.0, float("nan")), (CU8, 1.0, float("-inf"))):
        assert emu().emu_xlate_fmt_process(h, raw.ctypes.data, fmt, scale, bias, 10, 10, out.ctypes.data, 8) == -1
    assert emu().emu_xlate_fmt_process(h, raw.ctypes.data, CS16, 1.0, 0.0, 10, 10, out.ctypes.data, 8) == 2
    emu().emu_xlate_fmt_destroy(h)


def _rx_args(**kw):
    tmpl = np.ones(140, np.complex64)
    fr = np.array([[-25e3, 25e3]] * 2)
    des = (C.c_char_p * 2)(b"A", b"B")
    a = dict(rate=250e3, ns=2, nch=2, freqs=fr, des=des, fmt=CU8, scale=1 / 128.0, bias=127.5, block=5 * 4096, taps=None,
             ntaps=0, tmpl=tmpl, ntmpl=140, max_pdus=1024)
    a.update(kw)
    keep = (a["freqs"], a["tmpl"], a["taps"], des)
    return keep, (a["rate"], a["ns"], a["nch"], a["freqs"].ctypes.data if a["freqs"] is not None else None, a["des"], a["fmt"],
                  a["scale"], a["bias"], a["block"], a["taps"].ctypes.data if a["taps"] is not None else None, a["ntaps"],
                  a["tmpl"].ctypes.data if a["tmpl"] is not None else None, a["ntmpl"], a["max_pdus"])


def test_c_abi_argument_checks_and_no_device():
    from ais_amd import _lib

    L = _lib.lib()
    n = C.c_int(-1)
    L.aisx_device_count(C.byref(n))
    h = C.c_void_p()
    bad = [dict(rate=47999.0), dict(rate=float("nan")), dict(fmt=4), dict(fmt=-1), dict(scale=float("inf")),
           dict(bias=float("nan")), dict(block=5 * 4096 + 1), dict(block=0), dict(ns=0), dict(nch=0),
           dict(freqs=np.array([[-25e3, 125001.0]] * 2)), dict(freqs=None), dict(tmpl=None), dict(max_pdus=0),
           dict(des=(C.c_char_p * 2)(b"A", b"0123456789abcdefg")), dict(taps=np.ones(4, np.float32), ntaps=0)]
    for kw in bad:
        keep, args = _rx_args(**kw)
        assert L.aisx_rx_create(C.byref(h), *args) == _lib.AISX_ERR_INVALID, kw
        assert not h.value
    keep, ok = _rx_args()
    assert L.aisx_rx_create(None, *ok) == _lib.AISX_ERR_INVALID
    assert L.aisx_rx_destroy(None) == 0
    x = C.c_void_p(1)
    b, tl, nr = C.c_longlong(), C.c_long(), C.c_int()
    assert L.aisx_rx_acquire(None, C.byref(x), None) == _lib.AISX_ERR_INVALID
    assert L.aisx_rx_submit(None, None) == _lib.AISX_ERR_INVALID
    assert L.aisx_rx_push(None, x, 10, None) == _lib.AISX_ERR_INVALID
    assert L.aisx_rx_flush(None) == _lib.AISX_ERR_INVALID
    assert L.aisx_rx_pop(None, 0, C.byref(b), None, 0, C.byref(tl), None, 0, C.byref(nr), None) == _lib.AISX_ERR_INVALID
    assert L.aisx_rx_set_center_freq(None, 0, 0, 0.0) == _lib.AISX_ERR_INVALID
    assert L.aisx_xlate_process_fmt(None, x, CS16, 1.0, 0.0, 10, 10, x, 10, C.byref(n), None) == _lib.AISX_ERR_INVALID
    L.aisx_device_count(C.byref(n))
    rc = L.aisx_rx_create(C.byref(h), *ok)
    if n.value <= 0:
        assert rc == _lib.AISX_ERR_NO_DEVICE and not h.value
        import ais_amd

        with pytest.raises(_lib.NoDeviceError):
            ais_amd.ais_rx((-25e3, 25e3), 250e3, ("A", "B"), fmt="cu8", scale=1 / 128.0, bias=127.5, block_items=5 * 4096)
    else:
        assert rc == _lib.AISX_OK
        f = np.zeros(2)
        taps = np.ones(8, np.float32)
        xh = C.c_void_p()
        assert L.aisx_xlate_create(C.byref(xh), 5, taps.ctypes.data, 8, f.ctypes.data, 2, 250e3, 1, 100) == _lib.AISX_OK
        for fmt, scale, bias in ((4, 1.0, 0.0), (-1, 1.0, 0.0), (CS16, float("nan"), 0.0), (CS8, 1.0, float("inf"))):
            assert L.aisx_xlate_process_fmt(xh, x, fmt, scale, bias, 100, 100, x, 100, C.byref(n), None) == _lib.AISX_ERR_INVALID
        assert L.aisx_xlate_destroy(xh) == 0
        assert L.aisx_rx_submit(h, None) == _lib.AISX_ERR_INVALID  # (no slot acquired)
        assert L.aisx_rx_destroy(h) == 0


def test_python_arguments():
    import ais_amd

    with pytest.raises(ValueError):
        ais_amd.ais_rx((-25e3, 25e3), 250e3, ("A", "B"), fmt="cs12")
    with pytest.raises(ValueError):
        ais_amd.ais_rx((-25e3, 25e3), 250e3, ("A",))
    with pytest.raises(ValueError):
        ais_amd.ais_rx((-25e3, 25e3), 40e3, ("A", "B"))          # decimation 0
    with pytest.raises(ValueError):
        ais_amd.ais_rx((-25e3, 25e3), 250e3, ("A", "B"), block_items=1001)
    with pytest.raises(ValueError):
        ais_amd.ais_rx((-25e3, 130e3), 250e3, ("A", "B"))
    with pytest.raises(ValueError):
        ais_amd.ais_rx(0.0, 250e3, "A", nstreams=0)
