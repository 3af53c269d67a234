"""-m "not gpu": what the device tests of the formatted filter and of the receiver's paths rest on.  The matrix that
test_gpu_xlate_fmt.py walks must reach every build launch<R> instantiates in aisx_xlate.hip -- R = 8, 4, 2, 1 -- and the
reduced-lane plan of large decimations (G < 256), on the device's 256 lanes; a later change of xlate_cases.matrix() or
of xlate_plan that drops one fails here, without a GPU.  The same full-range inputs run through the lane model
(tests/emul_xlate_fmt on the device's 256 lanes) against float64 with the project's gate, before the device is relied
on.  Both device modules import without a GPU."""
import numpy as np

import xlate_cases as xc


def test_the_matrix_reaches_every_build_on_the_device_plan():
    plans = xc.device_plans()
    cases = xc.matrix()
    assert len(plans) == len(cases) >= 34
    assert {p["R"] for p in plans} == {1, 2, 4, 8}
    assert {p["G"] for p in plans if p["R"] > 1} == {256}
    assert min(p["G"] for p in plans) < 16 and any(16 < p["G"] < 256 for p in plans)   # D = 512 and D = 50
    assert any(p["U"] < p["Utot"] for p in plans)                                       # a window cut into chunks
    assert {c["ns"] for c in cases} == {1, 2} and {c["nch"] for c in cases} == {1, 2, 3, 16}
    assert min(c["L"] for c in cases) == 1 and max(c["L"] for c in cases) == 5781
    # the cases the other tests of the file pick: one per build
    key = {(c["D"], c["L"]): (c["D"], p["R"], p["G"]) for c, p in zip(cases, plans)}
    per = {key[(c["D"], c["L"])] for c in xc.one_case_per_build()}
    assert per == {(1, 8, 256), (2, 8, 256), (5, 4, 256), (7, 2, 256), (50, 1, 120), (512, 1, 12)}


def test_the_conversions_round():
    """every format has the stock conversion and one whose subtraction and product both round in float32 (so that a
    fused or reordered conversion changes bits) and differ from the float64 value"""
    import test_xlate_fmt_model as fm

    assert xc.FMT_CODES == dict(cs16=fm.CS16, cs8=fm.CS8, cu8=fm.CU8)
    for fmt, code in xc.FMT_CODES.items():
        (s0, b0), (s1, b1) = xc.FMT_CONVERSIONS[fmt]
        assert np.log2(s0) == int(np.log2(s0)) and 2 * b0 == int(2 * b0)
        assert np.float32(s1) == s1 and np.float32(b1) == b1 and np.log2(s1) != int(np.log2(s1))
        info = np.iinfo(fm.DTYPES[code])
        raw = np.arange(info.min, info.max + 1).astype(fm.DTYPES[code])
        two = (raw.astype(np.float32) - np.float32(b1)) * np.float32(s1)
        exact = (raw.astype(np.float64) - np.float64(b1)) * np.float64(s1)
        fused = (raw.astype(np.float64) * np.float64(s1) - np.float64(np.float32(b1) * np.float32(s1))).astype(np.float32)
        assert np.count_nonzero(two != exact) > raw.size // 2
        assert np.count_nonzero(two != fused) > raw.size // 8, (fmt, np.count_nonzero(two != fused))


def test_full_range_inputs_stay_inside_the_gate_on_the_lane_model():
    """test_gpu_xlate_fmt's inputs (same seeds) through the lane model on the device's plan, every case, format and
    conversion: bit for bit the cf32 path on numpy's conversion, and within GATE of the float64 filter
    (achieved: cs16 2.72e-06, cs8 2.17e-06, cu8 2.84e-06 -- the device gives the same figures)"""
    import test_xlate_fmt_model as fm

    for fmt, code in xc.FMT_CODES.items():
        worst = 0.0
        for i, case in enumerate(xc.matrix()):
            taps = xc.lowpass(case["L"], case["D"])
            nout = -(-case["N"] // case["D"])
            for j, (scale, bias) in enumerate(xc.FMT_CONVERSIONS[fmt]):
                raw = fm.raw_input(np.random.default_rng(xc.fmt_seed(i, fmt, j)), code, case["ns"], case["N"])
                y = fm.EmuFmt(case["D"], taps, case["freqs"], xc.FS, case["N"], nt=256).work(raw, code, scale, bias)
                x = fm.convert(raw, scale, bias)
                assert np.array_equal(fm.bits(y), fm.bits(fm.EmuFmt(case["D"], taps, case["freqs"], xc.FS, case["N"], nt=256).work(x)))
                w = xc.worst(y, xc.reference(case, taps, xc.converted64(raw, scale, bias), nout))
                assert w <= xc.GATE, (fmt, case["D"], case["L"], scale, bias, w)
                worst = max(worst, w)
        print("lane model %s: worst max|y - y64| / max|y64| = %.2e" % (fmt, worst))


def test_the_device_modules_import():
    import test_gpu_rx_paths as tp
    import test_gpu_xlate_fmt as tf

    assert tp.pytestmark.name == "gpu" and tf.pytestmark.name == "gpu"
    assert callable(tp.gr.hand_wired) and callable(tp.tx._stock_inputs)
    assert len([n for n in dir(tp) if n.startswith("test_")]) >= 13 and len([n for n in dir(tf) if n.startswith("test_")]) >= 5
