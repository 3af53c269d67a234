"""-m gpu: every product build of the correlator (k_corr2d_main <112>, <140>, <0> at F = 2048;
k_corr4f_main <896>, <1024>, <1120>, <1139>, <0> at F = 4096) on the device, through the call
sequence of tests/corr_cases.py: a long call of two segments per channel (the grid is pinned by
tests/test_emul_corr.py::test_corr_matrix_grid_pin), calls of 1, N - 1, N, N + 1, N // 2 + 1,
2 L and 3 L + 1 items and a ragged last one, history carried throughout, dense and sparse calls
alternating on one handle, peaks on tile, segment and call edges.

Every call: the delayed pass-through equals a shift of the stream bit for bit; tags equal the
oracle's at exact offsets; the dense output is within 2e-6 of the oracle and, against a float64
correlation of the whole stream, within max(2 x the oracle's own error, FLOOR) of the slice's
maximum.  Measured on one MI355X over the whole matrix: device error at most 1.0e-6 (N = 2048),
at most 5.5e-7 for N <= 1139 and 2.5e-7 for N <= 140; the oracle's float32 FFT at most 1.1e-6 on the
same samples; the device up to 16 x the oracle's where the oracle is nearly exact (N = 2, 1e-7), else
below 5.6 x.  FLOOR = 2e-6 leaves 2x headroom on the worst device figure; a misplaced item, a wrong
twiddle or a stale history is an error of order 1.
"""
import numpy as np
import pytest

import corr_cases as cc

pytestmark = pytest.mark.gpu

FLOOR = 2e-6


@pytest.fixture(scope="module")
def ais():
    import torch

    assert torch.cuda.is_available(), "gpu tests need a visible MI355X"
    import ais_amd

    return ais_amd


def _views(torch, nchan, n, strided, fill):
    """[nchan][n] device rows: contiguous, or at an odd item offset (not 16-byte aligned) with row stride n + 3"""
    if not strided:
        return torch.full((nchan, n), fill, dtype=torch.complex64, device="cuda")
    buf = torch.full((1 + nchan * (n + 3),), fill, dtype=torch.complex64, device="cuda")
    v = buf[1:].view(nchan, n + 3)[:, :n]
    assert v.stride() == (n + 3, 1) and v.data_ptr() % 16 == 8
    return v


def _family(blk, N):
    # the F = 4096 build reports the LDS a workgroup uses, the F = 2048 one 0
    used = blk.get_lds_claim()[1]
    assert (used > 0) == (cc.fft_size(N) == 4096), (N, used)


def _run(ais, N, nchan, strided, lens, x_rows, tmpl, rows=None, src_of=None, check_copies=False):
    import torch

    src_of = src_of or (lambda r: r)
    chk = cc.Checker(tmpl, x_rows, rows=rows, src_of=src_of)
    blk = ais.corr_est_cc(tmpl, 4.0, 1, 0.9, nchan=nchan, max_items=max(lens), max_tags_per_chan=256)
    _family(blk, N)
    src = np.array([src_of(r) for r in range(nchan)])
    k = 0
    for i, n in enumerate(lens):
        dense = i % 2 == 0
        xin = _views(torch, nchan, n, strided, 7e9)
        xin.copy_(torch.as_tensor(x_rows[:, k:k + n]).cuda()[torch.as_tensor(src).cuda()])
        out = _views(torch, nchan, n, strided, -7e9)
        corr = _views(torch, nchan, n, strided, -5e9) if dense else None
        o, c = blk.work(xin, out=out, corr=corr)
        assert o is out and c is corr
        tags = blk.tags()
        outh = out.cpu().numpy()
        corrh = corr.cpu().numpy() if dense else None
        order = np.argsort(tags["chan"], kind="stable")
        tags = tags[order]
        bounds = np.searchsorted(tags["chan"], np.arange(nchan + 1))
        tags_of = lambda r: tags[bounds[r]:bounds[r + 1]]  # noqa: E731
        chk.check(outh, corrh, tags_of, n, FLOOR)
        if check_copies:
            # equal input rows give equal outputs wherever they sit
            first = {}
            for r in range(nchan):
                first.setdefault(src[r], r)
            f = np.array([first[s] for s in src])
            assert np.array_equal(outh.view(np.uint64), outh[f].view(np.uint64))
            if dense:
                assert np.array_equal(corrh.view(np.uint64), corrh[f].view(np.uint64))
            for r in range(nchan):
                a, b = tags_of(r), tags_of(f[r])
                assert all(np.array_equal(a[k_], b[k_]) for k_ in ("offset", "value", "key")), (r, f[r])
        k += n
        assert blk.nitems_written() == k
    return chk


@pytest.mark.parametrize("nchan,strided", [(1, False), (3, True)])
@pytest.mark.parametrize("N", cc.ALL_LENGTHS)
def test_corr_build_matrix(ais, N, nchan, strided):
    rng = np.random.default_rng(9000 + 7 * N + nchan)
    lens = cc.call_lengths(N)
    tmpl, x = cc.make_stream(rng, N, lens, nchan)
    chk = _run(ais, N, nchan, strided, lens, x, tmpl)
    e = np.array(chk.errs)
    print("corr64 N=%d nchan=%d: device %.3g oracle %.3g ratio %.3g" % (N, nchan, e[:, 0].max(), e[:, 1].max(),
                                                                        (e[:, 0] / e[:, 1]).max()))
    assert chk.ndet >= (3 if N > 2 else 1)


@pytest.mark.parametrize("N,nchan", cc.MANY)
def test_corr_build_many_channels(ais, N, nchan):
    # more workgroups than one round of resident slots, two segments each on the long call; rows are copies
    # of five seeded rows; oracle and float64 on the first row, the last and every 37th
    rng = np.random.default_rng(77 + N)
    lens = cc.many_call_lengths(N)
    nbase = 5
    tmpl, base = cc.make_stream(rng, N, lens, nbase)
    rows = sorted(set(range(0, nchan, 37)) | {nchan - 1})
    chk = _run(ais, N, nchan, False, lens, base, tmpl, rows=rows, src_of=lambda r: (r * 3) % nbase,
               check_copies=True)
    e = np.array(chk.errs)
    print("corr64 N=%d nchan=%d: device %.3g oracle %.3g" % (N, nchan, e[:, 0].max(), e[:, 1].max()))
    assert chk.ndet >= len(rows)
