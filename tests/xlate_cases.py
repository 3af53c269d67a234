"""Cases of the batched freq_xlating_fir_filter_ccf shared by the lane-model tests (test_xlate_model.py) and the
device tests (test_gpu_xlate.py): the matrix of decimations, tap counts, centres, channel counts and ragged call
sequences, the float64 reference (oracle_py.freq_xlating_fir, the oracle's orc_freq_xlating_fir) and the gate; and
what the tests of the integer sample formats share (test_gpu_xlate_fmt.py on the device, test_xlate_fmt_cases.py on the
lane model): the formats' conversions, the converted values in float64, the device's plan of every case."""
import numpy as np

import oracle_py as orc

FS = 250e3
CENTRES = [0.0, 25e3, -25e3, -FS / 2, float(np.nextafter(FS / 2, 0.0)), 12345.678]
DECIMS = [1, 2, 5, 7, 50, 512]
NCH = [1, 2, 3, 16]
GATE = 1e-5  # max|y - y64| <= GATE * max|y64| per row


def lowpass(L, D):
    """a Hamming-windowed sinc of L taps with its cutoff at 0.4 fs / D (L = 1: the identity)"""
    if L == 1:
        return np.ones(1, np.float32)
    n = np.arange(L) - (L - 1) / 2.0
    fc = 0.4 / D
    h = 2 * fc * np.sinc(2 * fc * n) * (0.54 - 0.46 * np.cos(2 * np.pi * np.arange(L) / (L - 1)))
    return (h / h.sum()).astype(np.float32)


def signal(rng, ns, N, freqs):
    """per stream: white noise plus a strong tone 300 Hz beside each of its centres (in band after the filter)"""
    m = np.arange(N)
    x = (rng.standard_normal((ns, N)) + 1j * rng.standard_normal((ns, N))) * 0.5
    for s in range(ns):
        for f in freqs[s]:
            x[s] += 2.0 * np.exp(2j * np.pi * (f + 300.0) / FS * m + 1j * rng.uniform(0, 2 * np.pi))
    return x.astype(np.complex64)


def calls(D, N, max_items, prime=13):
    """a ragged call sequence covering N inputs: 1, D-1, D, D+1, a prime and max_items, round and round"""
    sizes = [s for s in (1, D - 1, D, D + 1, prime, max_items) if 1 <= s <= max_items]
    out, k = [], 0
    while sum(out) < N:
        out.append(min(sizes[k % len(sizes)], N - sum(out)))
        k += 1
    return out


def matrix():
    """one case per (D, ntaps): channel counts and stream counts in turn, centres rotated so that every centre meets
    every decimation"""
    cases = []
    for D in DECIMS:
        for L in sorted({1, D - 1, D, D + 1, 603, 5781} - {0}):
            i = len(cases)
            nch = NCH[i % len(NCH)]
            ns = 1 if nch == 16 else 1 + i % 2
            rng = np.random.default_rng(1000 + i)
            freqs = np.empty((ns, nch))
            for s in range(ns):
                for c in range(nch):
                    k = i + s * nch + c
                    freqs[s, c] = CENTRES[k % len(CENTRES)] if c < len(CENTRES) else rng.uniform(-FS / 2, FS / 2)
            nout = 96 if L * D < 100000 else 40
            N = nout * D + int(rng.integers(0, D + 1))
            cases.append(dict(D=D, L=L, nch=nch, ns=ns, freqs=freqs, N=N, max_items=2 * D + 29, seed=2000 + i))
    # 8 D <= L < 24 D: two outputs per lane (xlate_plan's R = 2), on the device's plan as on the model's
    cases.append(dict(D=5, L=100, nch=2, ns=2, freqs=np.array([[25e3, -25e3], [12345.678, -FS / 2]]), N=5 * 96 + 2,
                      max_items=39, seed=2999))
    return cases


def inputs(case):
    rng = np.random.default_rng(case["seed"])
    return lowpass(case["L"], case["D"]), signal(rng, case["ns"], case["N"], case["freqs"])


def reference(case, taps, x, nout):
    """[ns * nch][nout]: the float64 filter per row"""
    rows = []
    for s in range(case["ns"]):
        for c in range(case["nch"]):
            rows.append(orc.freq_xlating_fir(taps, case["D"], float(case["freqs"][s, c]), FS, x[s], 0, nout))
    return np.array(rows).reshape(-1, nout)


def worst(y, y64):
    """max over rows of max|y - y64| / max|y64|"""
    w = 0.0
    for a, b in zip(y, y64):
        w = max(w, float(np.max(np.abs(a.astype(np.complex128) - b)) / max(np.max(np.abs(b)), 1e-30)))
    return w


def retune_reference(taps, D, x, f_list, k_list, nout):
    """the float64 filter after retunes: from output k_list[i] on, the filter at f_list[i + 1] times the product of
    e^{-j (w_old - w_new) D k_r} over the retunes so far (GNU Radio 3.8's rotator goes on from its phase)"""
    y = orc.freq_xlating_fir(taps, D, f_list[0], FS, x, 0, nout).astype(np.complex128)
    const = 1.0 + 0j
    for i, kr in enumerate(k_list):
        w_old, w_new = 2 * np.pi * f_list[i] / FS, 2 * np.pi * f_list[i + 1] / FS
        const *= np.exp(-1j * (w_old - w_new) * D * kr)
        y[kr:] = orc.freq_xlating_fir(taps, D, f_list[i + 1], FS, x, 0, nout)[kr:] * const
    return y


# ---- the integer sample formats (AISX_FMT_CS16 / CS8 / CU8) ----------------------------------------------------------

FMT_CODES = dict(cs16=1, cs8=2, cu8=3)
THIRD, TENTH = float(np.float32(1.0 / 3.0)), float(np.float32(0.1))
# (scale, bias): the stock receiver's (test_gpu_rx.quantise: 2^-13, and 2^-5 with the RTL-SDR's 127.5 for cu8), then a
# scale that is no power of two with a bias that float32 rounds: (raw - bias) rounds for most raw values and the
# product rounds again, so a conversion fused into one fma, or done in another order, changes bits
FMT_CONVERSIONS = dict(cs16=[(2.0 ** -13, 0.0), (THIRD, TENTH)], cs8=[(2.0 ** -5, 0.0), (THIRD, TENTH)],
                       cu8=[(2.0 ** -5, 127.5), (THIRD, TENTH)])


def fmt_seed(i, fmt, j):
    """the seed of case i's raw input in format fmt for conversion j: the device test and the lane-model test draw the
    same integers"""
    return 7000 + 10 * i + FMT_CODES[fmt] + 100000 * j


def converted64(raw, scale, bias):
    """[..., 2] integers -> the converted values formed in float64 (exact: at most 17 + 24 significant bits)"""
    v = (raw.astype(np.float64) - np.float64(np.float32(bias))) * np.float64(np.float32(scale))
    return v[..., 0] + 1j * v[..., 1]


def device_plans():
    """xlate_plan on the device's 256 lanes for every case of the matrix (R, P, S, G, U, Utot), through the lane
    model's binding of the same host code"""
    import test_xlate_model as tm

    return [tm.EmuXlate(c["D"], lowpass(c["L"], c["D"]), c["freqs"], FS, c["max_items"], nt=256).plan() for c in matrix()]


def one_case_per_build():
    """of the matrix, the 603-tap case of every decimation: R = 8, 8, 4, 2, then R = 1 on 120 and on 12 lanes"""
    return [c for c in matrix() if c["L"] == 603]
