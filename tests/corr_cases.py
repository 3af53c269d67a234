"""Shared cases of the correlator build matrix (tests/test_gpu_corr_builds.py on the device,
tests/test_emul_corr.py under the lane model): template lengths per product build, call
sequences with carried history, planted peaks on tile / segment / call edges, and the checks
every call makes -- the delayed pass-through against a plain shift of the stream, tags and
dense output against the oracle, and the dense output against a float64 correlation."""
import numpy as np

import oracle_py as orc
from parity import assert_tags_match, unit_template

# template lengths of the product's builds (gr-ais_amd/csrc/aisx_lib.hip: corr2d_pick, corr4f_pick)
F2048_RUNTIME = [1, 2, 99, 128, 129, 511, 512]   # k_corr2d_main<0>
F2048_FOLDED = [112, 140]                         # k_corr2d_main<112>, <140>
F4096_RUNTIME = [513, 640, 1000, 2047, 2048]      # k_corr4f_main<0>
F4096_FOLDED = [896, 1024, 1120, 1139]            # k_corr4f_main<896>, <1024>, <1120>, <1139>
ALL_LENGTHS = F2048_RUNTIME + F2048_FOLDED + F4096_RUNTIME + F4096_FOLDED

# resident workgroups per CU the product passes to corr_grid (aisx_corr_process)
WG_PER_CU = {2048: 4, 4096: 2}
# tiles per segment the long first call resolves to at 1 .. 3 channels (pinned by the grid test)
LONG_TPS = 7
# the many-channel cases: (N, channels) whose workgroups exceed one round of resident slots
MANY = [(2047, 517), (129, 1100)]
NOISE = 0.03


def fft_size(N):
    return 2048 if N <= 512 else 4096


def long_call(N):
    """the first call: 12 whole tiles and a ragged thirteenth (two segments of 7 and 6 tiles)"""
    return 12 * (fft_size(N) - N) + 517


def call_lengths(N):
    L = fft_size(N) - N
    lens = [long_call(N), 1, N - 1, N, N + 1, N // 2 + 1, 2 * L, 3 * L + 1, 5 * L + 123]
    return [n for n in lens if n > 0]


def many_call_lengths(N):
    L = fft_size(N) - N
    return [long_call(N), N + 1, 3 * L + 1]


def peak_positions(N, lens, nchan):
    """template start positions per channel (a peak's output index is start + N - 1): on tile edges of the
    long call, on its segment edge, at item 0 of every call and straddling every call edge; spaced so that no
    two planted templates overlap"""
    L = fft_size(N) - N
    starts = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(int)
    total = int(sum(lens))
    ends = [k * L for k in (1, 2, 3, 5)]                       # tile edges: first output of a tile ...
    a = [e - N + 1 for e in ends] + [int(s) - N + 1 for s in starts[1::2]]   # ... and item 0 of calls
    b = [e - N for e in ends] + [LONG_TPS * L - N + 1] + [int(s) - N // 2 for s in starts[1:]]
    c = [LONG_TPS * L - N, LONG_TPS * L - N + 2] + [int(s) - N + 1 for s in starts[2::2]] + [800, total - N - 2]
    sets = [a, b, c] if nchan >= 3 else [a + b + c]
    out = []
    for ch in range(nchan):
        keep, last = [], -10 ** 9
        for p in sorted(set(sets[ch % len(sets)])):
            if 0 <= p <= total - N and p - last >= N + 8:
                keep.append(p)
                last = p
        out.append(keep)
    return out


def make_stream(rng, N, lens, nchan):
    tmpl = unit_template(rng, N)
    total = int(sum(lens))
    x = (NOISE * (rng.normal(size=(nchan, total)) + 1j * rng.normal(size=(nchan, total)))).astype(np.complex64)
    for ch, plist in enumerate(peak_positions(N, lens, nchan)):
        for p in plist:
            x[ch, p:p + N] += (tmpl * np.exp(1j * rng.uniform(-3, 3))).astype(np.complex64)
    return tmpl, x


def corr64(x, tmpl):
    """corr[i] = sum_j conj(tmpl[N-1-j]) x[i-j] over the whole stream, zero before it, in float64"""
    N, n = tmpl.size, x.size
    m = 1 << int(np.ceil(np.log2(n + N)))
    h = np.conj(tmpl[::-1]).astype(np.complex128)
    return np.fft.ifft(np.fft.fft(x.astype(np.complex128), m) * np.fft.fft(h, m))[:n]


def rel_err(got, ref):
    return float(np.max(np.abs(got.astype(np.complex128) - ref)) / (np.max(np.abs(ref)) + 1e-300))


class Checker:
    """follows one handle's channels call by call.  x: the distinct input rows; src_of(row): which of them the
    handle's channel `row` carries (itself by default); rows: the channels compared (all by default)"""

    def __init__(self, tmpl, x, rows=None, src_of=None):
        self.tmpl, self.x, self.N = tmpl, x, tmpl.size
        self.src_of = src_of or (lambda r: r)
        self.rows = list(range(x.shape[0])) if rows is None else list(rows)
        self.orc = {r: orc.CorrEst(tmpl, 4.0, 1, 0.9) for r in self.rows}
        self.ref = {s: corr64(x[s], tmpl) for s in sorted({self.src_of(r) for r in self.rows})}
        self.k = 0
        self.ndet = 0
        self.errs = []   # (device vs float64, oracle vs float64) per dense call and row

    def check(self, out, corr, tags_of, n, floor):
        """out, corr: host [channels of the handle][n] (corr None: a sparse call); tags_of(row): that channel's tags"""
        k, N = self.k, self.N
        for r in self.rows:
            s = self.src_of(r)
            # the delayed pass-through: the stream shifted by N items, zeros before it
            want = np.zeros(n, np.complex64)
            lo = min(n, max(0, N - k))
            want[lo:] = self.x[s, k + lo - N:k + n - N]
            assert np.array_equal(out[r].view(np.uint64), want.view(np.uint64)), ("pass-through", r, k, n)
            oo, oc, ot = self.orc[r].work(self.x[s, k:k + n], want_corr=corr is not None)
            self.ndet += assert_tags_match(tags_of(r), ot)
            if corr is not None:
                assert np.max(np.abs(corr[r] - oc)) / (np.max(np.abs(oc)) + 1e-30) < 2e-6, ("oracle", r, k, n)
                ref = self.ref[s][k:k + n]
                e_dev, e_orc = rel_err(corr[r], ref), rel_err(oc, ref)
                self.errs.append((e_dev, e_orc))
                assert e_dev <= max(2 * e_orc, floor), ("float64", r, k, n, e_dev, e_orc)
        self.k += n
