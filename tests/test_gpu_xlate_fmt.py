"""-m gpu: the batched freq_xlating_fir_filter_ccf reading cs16 / cs8 / cu8 items (aisx_xlate_process_fmt, k_xlate.h's
integer loaders) on the device, every build: all cases of xlate_cases.matrix() -- R = 8, 4, 2 and 1 outputs per lane,
the reduced-lane plans of decimations 50 and 512, 1 to 5781 taps, 1 to 16 channels, 1 and 2 streams -- for each integer
format, with integers over the format's whole range (both extremes where every call sequence meets them), the stock
conversions and one whose scale is no power of two and whose bias float32 cannot hold.  Gate 1: bit for bit the
device's cf32 filter on numpy's (raw.astype(float32) - float32(bias)) * float32(scale), the specification of
include/aisx.h.  Gate 2: within xlate_cases.GATE of the float64 filter over the converted values formed in float64.
Then strided and offset raw rows, a stream that changes format between calls, rows that do not depend on their
position, and refused calls that leave the handle untouched."""
import ctypes as C

import numpy as np
import pytest

import test_xlate_fmt_model as fm
import xlate_cases as xc
from test_gpu_xlate import _bits, _dev

pytestmark = pytest.mark.gpu

FORMATS, CONVERSIONS = xc.FMT_CODES, xc.FMT_CONVERSIONS


@pytest.fixture(scope="module")
def ais():
    import torch

    assert torch.cuda.is_available(), "gpu tests need a visible MI355X"
    import ais_amd

    return ais_amd


def _filter(ais, case, taps, max_items, ns=None, freqs=None):
    return ais.freq_xlating_fir_filter_ccf(case["D"], taps, case["freqs"] if freqs is None else freqs, xc.FS,
                                           nstreams=case["ns"] if ns is None else ns, max_items=max_items)


def _run_fmt(f, raw_dev, sizes, fmt, scale, bias):
    import torch

    ys, o = [], 0
    for n in sizes:
        ys.append(f.work(raw_dev[:, o:o + n], fmt=fmt, scale=scale, bias=bias))
        o += n
    assert o == raw_dev.shape[1]
    return torch.cat(ys, dim=1).cpu().numpy()


@pytest.mark.parametrize("fmt", list(FORMATS))
def test_every_build_exact_and_against_float64(ais, fmt):
    """every case of the matrix x every conversion: the ragged calls on one handle and the single call on another equal
    the cf32 filter on numpy's conversion bit for bit, and stay within GATE of the float64 filter
    (achieved on the device: cs16 2.72e-06, cs8 2.17e-06, cu8 2.84e-06; the lane model gives the same three figures on
    the same inputs)"""
    import torch

    worst, where = 0.0, None
    cases = xc.matrix()
    for i, case in enumerate(cases):
        taps = xc.lowpass(case["L"], case["D"])
        nout = -(-case["N"] // case["D"])
        for j, (scale, bias) in enumerate(CONVERSIONS[fmt]):
            rng = np.random.default_rng(xc.fmt_seed(i, fmt, j))
            raw = fm.raw_input(rng, FORMATS[fmt], case["ns"], case["N"])
            info = np.iinfo(raw.dtype)
            assert raw.min() == info.min and raw.max() == info.max
            rawd = torch.as_tensor(raw).cuda()
            want = _filter(ais, case, taps, case["N"]).work(_dev(fm.convert(raw, scale, bias))).cpu().numpy()
            assert want.shape == (case["ns"] * case["nch"], nout)
            ragged = _run_fmt(_filter(ais, case, taps, case["max_items"]), rawd,
                              xc.calls(case["D"], case["N"], case["max_items"]), fmt, scale, bias)
            single = _run_fmt(_filter(ais, case, taps, case["N"]), rawd, [case["N"]], fmt, scale, bias)
            key = (fmt, case["D"], case["L"], case["nch"], case["ns"], scale, bias)
            # gate 1: exact
            assert ragged.shape == want.shape and np.array_equal(_bits(ragged), _bits(want)), key
            assert single.shape == want.shape and np.array_equal(_bits(single), _bits(want)), key
            # gate 2: against float64 (on the ragged run; the single call has the same bits by gate 1)
            w = xc.worst(ragged, xc.reference(case, taps, xc.converted64(raw, scale, bias), nout))
            if w > worst:
                worst, where = w, key
            assert w <= xc.GATE, (key, w)  # (achieved: 2.72e-06 / 2.17e-06 / 2.84e-06 for cs16 / cs8 / cu8)
    print("device %s: %d cases x %d conversions, worst max|y - y64| / max|y64| = %.2e at %s"
          % (fmt, len(cases), len(CONVERSIONS[fmt]), worst, where))
    assert worst <= xc.GATE


@pytest.mark.parametrize("fmt", list(FORMATS))
def test_strided_offset_raw_rows(ais, fmt):
    """rows aligned to one item only (2 bytes for cs8 / cu8, 4 for cs16): an odd row stride larger than n, the base
    advanced by an odd number of items; outputs into a wider buffer whose gaps keep their sentinel"""
    import torch

    for i, case in enumerate(xc.one_case_per_build()):
        taps = xc.lowpass(case["L"], case["D"])
        scale, bias = CONVERSIONS[fmt][1]
        ns, N = 3, case["N"]
        freqs = np.resize(case["freqs"], (ns, case["nch"]))
        raw = fm.raw_input(np.random.default_rng(300 + i), FORMATS[fmt], ns, N)
        rawd = torch.as_tensor(raw).cuda()
        f = _filter(ais, case, taps, N, ns=ns, freqs=freqs)
        want = f.work(rawd, fmt=fmt, scale=scale, bias=bias).cpu().numpy()
        W = N + 7 + (N % 2)                                   # odd
        big = torch.zeros((ns, W, 2), dtype=rawd.dtype, device="cuda")
        big[:, 3:3 + N] = rawd
        view = big[:, 3:3 + N]
        item = 2 * raw.dtype.itemsize
        assert W % 2 == 1 and view.stride(0) == 2 * W and (view.data_ptr() - big.data_ptr()) == 3 * item
        rows = ns * case["nch"]
        out = torch.full((rows, want.shape[1] + 5), 7.0 + 7.0j, dtype=torch.complex64, device="cuda")
        f.reset()  # (zero history, input index 0, rotators at 1: test_gpu_xlate.test_matrix_and_split_invariance pins it)
        got = f.work(view, out=out[:, 3:], fmt=fmt, scale=scale, bias=bias)
        assert got.data_ptr() == out[:, 3:].data_ptr()
        assert np.array_equal(_bits(got.cpu().numpy()), _bits(want)), (fmt, case["D"])
        o = out.cpu().numpy()
        assert (o[:, :3] == 7.0 + 7.0j).all() and (o[:, 3 + want.shape[1]:] == 7.0 + 7.0j).all(), (fmt, case["D"])


def test_a_stream_may_change_format_between_calls(ais):
    """the history is converted values: cf32, cs16, cu8, cs8, cf32 ... calls of one stream equal the all-cf32 run; on
    R = 8 (D = 1) and on R = 1 with 120 lanes (D = 50)"""
    import torch

    names = {v: k for k, v in FORMATS.items()}
    plans = dict(zip([(c["D"], c["L"]) for c in xc.matrix()], xc.device_plans()))
    assert plans[(1, 603)]["R"] == 8 and plans[(50, 603)]["R"] == 1
    for D, L in ((1, 603), (50, 603)):
        taps = xc.lowpass(L, D)
        freqs = np.array([[25e3, -25e3, 12345.678]])
        rng = np.random.default_rng(31 + D)
        sizes = xc.calls(D, 40 * D + 307, 2 * D + 29)
        assert len(sizes) >= 9
        a = ais.freq_xlating_fir_filter_ccf(D, taps, freqs, xc.FS, max_items=2 * D + 29)
        b = ais.freq_xlating_fir_filter_ccf(D, taps, freqs, xc.FS, max_items=2 * D + 29)
        order = [fm.CF32, fm.CS16, fm.CU8, fm.CS8]
        for i, s in enumerate(sizes):
            code = order[i % 4]
            if code == fm.CF32:
                x = xc.signal(rng, 1, s, freqs)
                ya = a.work(_dev(x))
            else:
                raw = fm.raw_input(rng, code, 1, s)
                scale, bias = CONVERSIONS[names[code]][i % 2]
                x = fm.convert(raw, scale, bias)
                ya = a.work(torch.as_tensor(raw).cuda(), fmt=names[code], scale=scale, bias=bias)
            yb = b.work(_dev(x))
            assert ya.shape == yb.shape and np.array_equal(_bits(ya.cpu().numpy()), _bits(yb.cpu().numpy())), (D, L, i)


@pytest.mark.parametrize("fmt", list(FORMATS))
def test_rows_do_not_depend_on_their_position(ais, fmt):
    """the same raw stream as stream 0 and as the last of five gives identical rows, for every build"""
    import torch

    for i, case in enumerate(xc.one_case_per_build()):
        taps = xc.lowpass(case["L"], case["D"])
        scale, bias = CONVERSIONS[fmt][1]
        ns, N = 5, case["N"]
        freqs = np.resize(case["freqs"], (ns, case["nch"]))
        freqs[ns - 1] = freqs[0]
        raw = fm.raw_input(np.random.default_rng(400 + i), FORMATS[fmt], ns, N)
        raw[ns - 1] = raw[0]
        f = _filter(ais, case, taps, case["max_items"], ns=ns, freqs=freqs)
        y = _run_fmt(f, torch.as_tensor(raw).cuda(), xc.calls(case["D"], N, case["max_items"]), fmt, scale, bias)
        nch = case["nch"]
        assert np.array_equal(_bits(y[:nch]), _bits(y[(ns - 1) * nch:])), (fmt, case["D"])
        assert not np.array_equal(_bits(y[:nch]), _bits(y[nch:2 * nch]))


def test_a_refused_call_leaves_the_handle_untouched(ais):
    """format 4, a NaN scale, an infinite bias and n > max_items return AISX_ERR_INVALID; the next valid call goes on
    bit-identically to a handle that never saw them (history, phase and output index untouched)"""
    import torch

    from ais_amd import _lib

    L = _lib.lib()
    case = [c for c in xc.matrix() if (c["D"], c["L"]) == (5, 603)][0]
    taps = xc.lowpass(case["L"], case["D"])
    scale, bias = CONVERSIONS["cs16"][1]
    raw = fm.raw_input(np.random.default_rng(55), fm.CS16, case["ns"], case["N"])
    rawd = torch.as_tensor(raw).cuda()
    sizes = xc.calls(case["D"], case["N"], case["max_items"])
    a = _filter(ais, case, taps, case["max_items"])
    b = _filter(ais, case, taps, case["max_items"])
    rows = case["ns"] * case["nch"]
    junk = torch.full((rows, case["max_items"] + 8), 7.0 + 7.0j, dtype=torch.complex64, device="cuda")
    bad = [(4, scale, bias, 13), (-1, scale, bias, 13), (fm.CS16, float("nan"), bias, 13), (fm.CS16, scale, float("inf"), 13),
           (fm.CS16, scale, float("-inf"), 13), (fm.CS16, scale, bias, case["max_items"] + 1), (fm.CS16, scale, bias, 0)]
    o = 0
    for k, n in enumerate(sizes):
        fmt_, sc_, bi_, n_ = bad[k % len(bad)]
        got = C.c_int(-7)
        rc = L.aisx_xlate_process_fmt(a._h, rawd.data_ptr(), fmt_, sc_, bi_, rawd.stride(0) // 2, n_, junk.data_ptr(),
                                      junk.stride(0), C.byref(got), None)
        assert rc == _lib.AISX_ERR_INVALID and got.value == -7, (k, rc)
        ya = a.work(rawd[:, o:o + n], fmt="cs16", scale=scale, bias=bias).cpu().numpy()
        yb = b.work(rawd[:, o:o + n], fmt="cs16", scale=scale, bias=bias).cpu().numpy()
        assert ya.shape == yb.shape and np.array_equal(_bits(ya), _bits(yb)), k
        o += n
    assert len(sizes) >= len(bad)
    assert (junk.cpu().numpy() == 7.0 + 7.0j).all()  # (a refused call writes nothing)
