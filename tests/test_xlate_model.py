"""The batched freq_xlating_fir_filter_ccf's kernel body (gr-ais_amd/csrc/k_xlate.h) on the CPU lane model
(tests/emul_xlate) against the float64 filter of the oracle (orc_freq_xlating_fir): the matrix of decimations, tap
counts, centres and channel counts through ragged call sequences, split invariance bit for bit, retunes against the
closed form; plus the C ABI's argument checks and its refusal without a device.  -m "not gpu"."""
import ctypes as C

import numpy as np
import pytest

import emul_load
from emul_load import f64, i32, lng, vp
import torch  # noqa: F401  (before libaisx.so: one HIP runtime in the process)
import xlate_cases as xc

NT = 64  # lanes per workgroup in the model (the device runs 256: the plan follows)


def emu():
    return emul_load.load("emul_xlate", [
        ("emu_xlate_create", vp, [i32, vp, i32, vp, i32, f64, i32, i32, i32]),
        ("emu_xlate_destroy", None, [vp]),
        ("emu_xlate_plan", None, [vp, vp]),
        ("emu_xlate_output_count", None, [vp, i32]),
        ("emu_xlate_set_center_freq", None, [vp, i32, i32, f64]),
        ("emu_xlate_reset", None, [vp]),
        ("emu_xlate_process", None, [vp, vp, lng, i32, vp, lng]),
    ])


class EmuXlate:
    def __init__(self, D, taps, freqs, fs, max_items, nt=NT):
        taps = np.ascontiguousarray(taps, np.float32)
        freqs = np.ascontiguousarray(freqs, np.float64)
        self.ns, self.nch = freqs.shape
        self.h = emu().emu_xlate_create(D, taps.ctypes.data, taps.size, freqs.ctypes.data, self.nch, fs, self.ns,
                                        max_items, nt)
        assert self.h

    def __del__(self):
        emu().emu_xlate_destroy(self.h)

    def reset(self):
        emu().emu_xlate_reset(self.h)

    def plan(self):
        v = np.zeros(6, np.int32)
        emu().emu_xlate_plan(self.h, v.ctypes.data)
        return dict(zip(("R", "P", "S", "G", "U", "Utot"), v.tolist()))

    def work(self, x):
        """x [ns][n] (any row stride in elements); returns [ns*nch][nout]"""
        x = np.asarray(x, np.complex64)
        n = x.shape[1]
        cnt = emu().emu_xlate_output_count(self.h, n)
        out = np.zeros((self.ns * self.nch, cnt + 3), np.complex64)
        got = emu().emu_xlate_process(self.h, x.ctypes.data, x.strides[0] // 8, n, out.ctypes.data, out.strides[0] // 8)
        assert got == cnt
        return out[:, :got]


def run_calls(f, x, sizes):
    ys, o = [], 0
    for n in sizes:
        ys.append(f.work(x[:, o:o + n]))
        o += n
    return np.concatenate(ys, axis=1)


def test_matrix_against_float64():
    worst, plans = 0.0, set()
    for case in xc.matrix():
        taps, x = xc.inputs(case)
        f = EmuXlate(case["D"], taps, case["freqs"], xc.FS, case["max_items"])
        plans.add(tuple(f.plan().values()))
        y = run_calls(f, x, xc.calls(case["D"], case["N"], case["max_items"]))
        nout = -(-case["N"] // case["D"])
        assert y.shape == (case["ns"] * case["nch"], nout)
        w = xc.worst(y, xc.reference(case, taps, x, nout))
        assert w <= xc.GATE, (case["D"], case["L"], case["nch"], w)
        worst = max(worst, w)
        # split invariance: the whole input in one call gives the same bits
        g = EmuXlate(case["D"], taps, case["freqs"], xc.FS, case["N"])
        assert np.array_equal(g.work(x).view(np.uint32), y.view(np.uint32)), (case["D"], case["L"])
    print("lane model: %d cases, %d plans, worst max|y - y64| / max|y64| = %.2e" % (len(xc.matrix()), len(plans), worst))
    assert {p[0] for p in plans} == {1, 2, 8} and min(p[3] for p in plans) < NT  # (R, G) the tilings, few lanes


def test_stock_shape_with_the_device_plan():
    """ais_rx's shape (250 kS/s, decimation 5, firdes.low_pass(1, fs, 11e3, 1e3): 603 taps, A / B at -+25 kHz) with
    the device's 256 lanes per workgroup: R = 4 outputs per lane, the padded window"""
    import ais_amd

    taps = ais_amd.firdes_low_pass(1.0, xc.FS, 11e3, 1e3)
    assert taps.size == 603
    freqs = np.array([[-25e3, 25e3]] * 2)
    rng = np.random.default_rng(17)
    N = 5 * 1400 + 3
    x = xc.signal(rng, 2, N, freqs)
    f = EmuXlate(5, taps, freqs, xc.FS, 1200, nt=256)
    assert f.plan() == dict(R=4, P=20, S=21, G=256, U=618, Utot=618)
    y = run_calls(f, x, xc.calls(5, N, 1200))
    case = dict(D=5, ns=2, nch=2, freqs=freqs)
    w = xc.worst(y, xc.reference(case, taps, x, y.shape[1]))
    print("stock shape on the device plan: worst %.2e" % w)
    assert w <= xc.GATE
    g = EmuXlate(5, taps, freqs, xc.FS, N, nt=256)
    assert np.array_equal(g.work(x).view(np.uint32), y.view(np.uint32))


def test_strided_rows_and_reset():
    rng = np.random.default_rng(5)
    taps = xc.lowpass(603, 5)
    freqs = np.array([[-25e3, 25e3], [12345.678, 0.0]])
    x = xc.signal(rng, 2, 4000, freqs)
    wide = np.zeros((2, 4321), np.complex64)
    wide[:, :4000] = x
    f = EmuXlate(5, taps, freqs, xc.FS, 4000)
    a = f.work(wide[:, :4000])
    f.reset()
    b = f.work(x)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_retune_closed_form():
    rng = np.random.default_rng(9)
    D, taps = 5, xc.lowpass(603, 5)
    f_list = [25e3, -25e3, 12345.678]
    x = xc.signal(rng, 1, 5 * 700 + 3, np.array([f_list]))
    f = EmuXlate(D, taps, np.array([[f_list[0]]]), xc.FS, 2000)
    ys, k_list = [f.work(x[:, :1001])], []
    for i, (a, b) in enumerate(((1001, 2001), (2001, x.shape[1]))):
        k_list.append(sum(y.shape[1] for y in ys))
        assert emu().emu_xlate_set_center_freq(f.h, 0, 0, f_list[i + 1]) == 0
        ys.append(f.work(x[:, a:b]))
    y = np.concatenate(ys, axis=1)[0]
    y64 = xc.retune_reference(taps, D, x[0], f_list, k_list, y.size)
    w = float(np.max(np.abs(y - y64)) / np.max(np.abs(y64)))
    assert w <= xc.GATE, w


def test_create_arguments_and_no_device():
    from ais_amd import _lib

    taps = np.ones(8, np.float32)
    fr = np.zeros(4)
    ok = (5, taps.ctypes.data, 8, fr.ctypes.data, 2, 250e3, 2, 100)
    bad = [(0,) + ok[1:], (4097,) + ok[1:], (5, None) + ok[2:], (5, taps.ctypes.data, 0) + ok[3:],
           (5, taps.ctypes.data, 1 << 18) + ok[3:], ok[:3] + (None,) + ok[4:], ok[:4] + (0,) + ok[5:],
           ok[:5] + (0.0,) + ok[6:], ok[:5] + (float("nan"),) + ok[6:], ok[:6] + (0, 100), ok[:7] + (0,)]
    big = np.array([0.0, 0.0, 125001.0, 0.0])
    bad.append(ok[:3] + (big.ctypes.data,) + ok[4:])
    for args in bad:
        assert not emu().emu_xlate_create(*args, NT), args
    h0 = emu().emu_xlate_create(*ok, NT)
    assert h0
    assert emu().emu_xlate_set_center_freq(h0, 0, 2, 0.0) != 0 and emu().emu_xlate_set_center_freq(h0, 0, 0, 2e5) != 0
    emu().emu_xlate_destroy(h0)
    L = _lib.lib()
    h = C.c_void_p()
    for args in bad:
        assert L.aisx_xlate_create(C.byref(h), *args) == _lib.AISX_ERR_INVALID, args
    assert L.aisx_xlate_create(None, *ok) == _lib.AISX_ERR_INVALID
    assert L.aisx_xlate_destroy(None) == 0
    assert L.aisx_xlate_output_count(None, 5) == _lib.AISX_ERR_INVALID
    n = C.c_int(-1)
    L.aisx_device_count(C.byref(n))
    rc = L.aisx_xlate_create(C.byref(h), *ok)
    if n.value <= 0:
        assert rc == _lib.AISX_ERR_NO_DEVICE
    else:
        assert rc == _lib.AISX_OK
        assert L.aisx_xlate_output_count(h, -1) == _lib.AISX_ERR_INVALID
        assert L.aisx_xlate_set_center_freq(h, 2, 0, 0.0) == _lib.AISX_ERR_INVALID
        assert L.aisx_xlate_set_center_freq(h, 0, 0, 125001.0) == _lib.AISX_ERR_INVALID
        x = C.c_void_p(1)
        assert L.aisx_xlate_process(h, x, 100, 0, x, 100, C.byref(n), None) == _lib.AISX_ERR_INVALID
        assert L.aisx_xlate_process(h, x, 100, 101, x, 100, C.byref(n), None) == _lib.AISX_ERR_INVALID
        assert L.aisx_xlate_process(h, x, 50, 100, x, 100, C.byref(n), None) == _lib.AISX_ERR_INVALID
        assert L.aisx_xlate_process(h, x, 100, 100, x, 10, C.byref(n), None) == _lib.AISX_ERR_INVALID
        assert L.aisx_xlate_destroy(h) == 0
    import ais_amd

    with pytest.raises(ValueError):
        ais_amd.freq_xlating_fir_filter_ccf(5, taps, np.zeros((3, 2)), 250e3, nstreams=2)
    if n.value <= 0:
        with pytest.raises(_lib.NoDeviceError):
            ais_amd.freq_xlating_fir_filter_ccf(5, taps, (-25e3, 25e3), 250e3)
