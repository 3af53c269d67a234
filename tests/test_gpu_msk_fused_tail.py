"""-m gpu: the NRZI bit tail folded into the timing recovery's symbol flush (aisx_msk_set_fused_tail, k_msk.h
MskParams::bits) against a twin handle with the switch off (k_bittail over the symbols the kernel wrote), fed identical
samples and tags: bits (whole rows: nothing may be written behind `produced`), produced, symbols when asked for, and
the carried tail state (one more call behind the four).  Channels whose samples are finite are also held to the
oracle's chain (oracle_py.Demod, corr_est -> msk -> bit tail).

Shapes: 9 channels (a ragged wave of 8 + 1) and 33 (a second workgroup with one live channel); calls of 8 samples
(nothing produced: the state carries), 37 (fewer symbols than a flush: the drain alone), 1000, 4101 (odd symbol counts,
many flushes) and 600 more."""
import numpy as np
import pytest

import oracle_py as orc

pytestmark = pytest.mark.gpu

SPS = 4
LENS = [8, 37, 1000, 4101, 600]
# (channel, what): samples the slicer's plain test does not cover -- compared against the twin only
ODD = {2: "nan", 5: "zeros", 7: "tiny"}


@pytest.fixture(scope="module")
def ais():
    import torch

    assert torch.cuda.is_available()
    import ais_amd

    return ais_amd


_CACHE = {}


def _inputs(ais, nchan):
    """per call: corr_est's output rows and its tags as device tensors in the hand-over layout, from one corr_est
    handle over LENS; and the oracle chain's bits per call for the channels left as they are"""
    import torch
    import synth

    if nchan in _CACHE:
        return _CACHE[nchan]
    total = sum(LENS)
    tmpl = ais.modulate_vector_bc(ais.gmsk_mod(SPS, 0.4), [1, 1, 0, 0] * 7, [1])
    xs = np.stack([synth.make_channel(900 + c, total, "S", SPS, amp=1.0, cfo_max=10.0)[0] for c in range(nchan)])
    corr = ais.corr_est_cc(tmpl, SPS, 1, 0.9, nchan=nchan, max_items=max(LENS))
    cap = corr._cap
    calls, k = [], 0
    for L in LENS:
        y, _ = corr.work(torch.as_tensor(xs[:, k:k + L]).cuda())
        torch.cuda.synchronize()
        y = y.cpu().numpy().copy()
        for c, what in ODD.items():
            if c < nchan and L >= 1000:
                if what == "nan":
                    y[c, 400] = np.complex64(complex(np.nan, 1.0))
                elif what == "zeros":
                    y[c, 300:700] = 0
                else:
                    y[c, 300:700] *= np.float32(1e-10)  # products of neighbours ~1e-20: negative ones take the table
        t = corr.tags()
        tg = np.zeros((nchan, cap), dtype=ais.TAG_DTYPE)
        cnt = np.zeros(nchan, np.int32)
        for c in range(nchan):
            sel = t[t["chan"] == c]
            tg[c, : len(sel)] = sel
            cnt[c] = len(sel)
        calls.append(dict(y=torch.as_tensor(y).cuda(), tags=torch.as_tensor(tg.view(np.uint8).reshape(nchan, -1).copy()).cuda(),
                          cnt=torch.as_tensor(cnt).cuda(), cap=cap))
        k += L
    ref = {}
    for c in range(nchan):
        if c in ODD:
            continue
        o, k, ref[c] = orc.Demod(SPS, tmpl, stages=0), 0, []
        for L in LENS:
            ref[c].append(o.step(xs[c, k:k + L])[0])
            k += L
    _CACHE[nchan] = (calls, ref)
    return _CACHE[nchan]


def _run(ais, nchan, calls, fused, odd_stride, want_syms, tail):
    """one handle over the calls; fused[i]: the switch for call i.  Returns per call (produced, whole bit rows, symbols)"""
    import torch

    blk = ais.msk_timing_recovery_cc(float(SPS), 0.04, 0.01, 1, nchan=nchan, max_items=max(LENS))
    assert blk.get_fused_tail()  # the default
    ts = torch.cuda.Stream() if tail else None
    if tail:
        blk.set_tail_stream(ts)
    cap = blk.out_capacity
    width = (cap | 1) if odd_stride else cap + (cap & 1)
    sets = [dict(syms=torch.empty((nchan, width), dtype=torch.complex64, device="cuda") if want_syms else None,
                 bits=torch.empty((nchan, width), dtype=torch.uint8, device="cuda"),
                 produced=torch.empty(nchan, dtype=torch.int32, device="cuda")) for _ in range(2)]
    res = []
    for i, cl in enumerate(calls):
        o = sets[i & 1]
        o["bits"].fill_(0xAA)
        o["produced"].fill_(-1)
        if want_syms:
            o["syms"].fill_(0)
        blk.set_fused_tail(fused[i])
        blk.work(cl["y"], tags_ptrs=(cl["tags"].data_ptr(), cl["cnt"].data_ptr(), cl["cap"]), outs=o)
        assert blk.last_tail_fused() == bool(fused[i])  # (osps 1, no err / mu ports, 8 channels per wave: it applies)
        blk.wait_tail()  # (the current stream waits for the bits, wherever they were written)
        torch.cuda.current_stream().synchronize()
        prod = o["produced"].cpu().numpy().copy()
        res.append((prod, o["bits"].cpu().numpy().copy(),
                    [o["syms"][c, : prod[c]].cpu().numpy().copy() for c in range(nchan)] if want_syms else None))
    blk.last_status()
    return res


def _compare(nchan, got, twin, ref):
    nbits = 0
    for i, ((pg, bg, sg), (pt, bt, st)) in enumerate(zip(got, twin)):
        assert np.array_equal(pg, pt), i
        assert np.array_equal(bg, bt), (i, np.argwhere(bg != bt)[:4])  # whole rows, the untouched part included
        if sg is not None:
            for c in range(nchan):
                assert sg[c].view(np.uint32).tobytes() == st[c].view(np.uint32).tobytes(), (i, c)
        for c, rb in ref.items():
            assert pg[c] == len(rb[i]) and np.array_equal(bg[c, : pg[c]], rb[i]), (i, c)
        nbits += int(pg.sum())
    assert int(got[0][0].sum()) == 0 and 0 < got[1][0].max() < 16  # nothing produced; the drain alone
    assert nbits > nchan * sum(LENS) / SPS * 0.95


@pytest.mark.parametrize("nchan", [9, 33])
@pytest.mark.parametrize("odd_stride,want_syms,tail", [(False, True, False), (True, False, False), (False, False, True),
                                                       (True, True, True)])
def test_fused_tail_equals_the_bit_tail_kernel(ais, nchan, odd_stride, want_syms, tail):
    calls, ref = _inputs(ais, nchan)
    got = _run(ais, nchan, calls, [1] * len(LENS), odd_stride, want_syms, tail)
    twin = _run(ais, nchan, calls, [0] * len(LENS), odd_stride, want_syms, tail)
    _compare(nchan, got, twin, ref)


@pytest.mark.parametrize("nchan", [9, 33])
@pytest.mark.parametrize("odd_stride,want_syms,tail,first", [(False, False, True, 1), (True, True, False, 0), (True, False, True, 0)])
def test_fused_and_unfused_calls_alternate_on_one_handle(ais, nchan, odd_stride, want_syms, tail, first):
    calls, ref = _inputs(ais, nchan)
    got = _run(ais, nchan, calls, [(first + i) & 1 for i in range(len(LENS))], odd_stride, want_syms, tail)
    twin = _run(ais, nchan, calls, [0] * len(LENS), odd_stride, want_syms, tail)
    _compare(nchan, got, twin, ref)
