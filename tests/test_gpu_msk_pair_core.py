"""-m gpu: the hand-scheduled lock-step pair of the timing recovery (aisx_msk_set_pair_core mode 1, DevCtx::pair_core) against
the compiler-scheduled body (mode 0) on twin handles fed identically: symbols, bits (whole rows), produced counts and the
status word as bit patterns, call by call; the last call of every stream is the "one further call" that shows the carried
state.  The sps 4 cases are also held to oracle_py.MskStream.

Streams: calls of 4133, 64, 1 and 2309 items (shorter than a chunk, a single item, no multiples of 64) and 600 more;
9 channels (a full wave and a ragged one with one live channel) or 70."""
import numpy as np
import pytest

import oracle_py as orc

pytestmark = pytest.mark.gpu

LENS = [4133, 64, 1, 2309, 600]
TOTAL = sum(LENS)
ST_INTERP_RANGE = 1


@pytest.fixture(scope="module")
def ais():
    import torch

    assert torch.cuda.is_available()
    import ais_amd

    return ais_amd


_XS = {}


def _signal(nchan):
    import synth

    if nchan not in _XS:
        _XS[nchan] = np.stack([synth.make_channel(700 + c, TOTAL, "P", 4, amp=1.0, cfo_max=50.0)[0] for c in range(nchan)])
    return _XS[nchan]


def _tags(rows, chan, dtype):
    rows = sorted(rows, key=lambda r: r[0])
    t = np.zeros(len(rows), dtype=dtype)
    t["offset"] = [r[0] for r in rows]
    t["value"] = [r[1] for r in rows]
    t["key"] = [r[2] if len(r) > 2 else 2 for r in rows]
    t[dtype.names[3]] = chan
    return t


def _run(ais, xs, modes, sps=4.0, gain=0.04, limit=0.01, q=0, tags=None):
    """one handle over LENS, modes[i] the switch for call i -> per call (produced, symbols as bits, whole bit rows, status)"""
    import torch

    nchan = xs.shape[0]
    blk = ais.msk_timing_recovery_cc(sps, gain, limit, 1, nchan=nchan, max_items=max(LENS))
    assert blk.get_pair_core() == 1  # the default
    if q:
        blk.set_max_noutput_items(q)
    cap = blk.out_capacity
    res, k = [], 0
    for i, L in enumerate(LENS):
        outs = dict(syms=torch.zeros((nchan, cap), dtype=torch.complex64, device="cuda"),
                    bits=torch.full((nchan, cap), 0xAA, dtype=torch.uint8, device="cuda"),
                    produced=torch.full((nchan,), -1, dtype=torch.int32, device="cuda"))
        tp = None
        if tags is not None:
            tcap = 64
            tg = np.zeros((nchan, tcap), dtype=ais.TAG_DTYPE)
            cnt = np.zeros(nchan, np.int32)
            for c in range(nchan):
                sel = tags[c][(tags[c]["offset"] >= k) & (tags[c]["offset"] < k + L)]
                tg[c, : len(sel)] = sel
                cnt[c] = len(sel)
            keep = (torch.as_tensor(tg.view(np.uint8).reshape(nchan, -1).copy()).cuda(), torch.as_tensor(cnt).cuda())
            tp = (keep[0].data_ptr(), keep[1].data_ptr(), tcap)
        blk.set_pair_core(modes[i])
        assert blk.get_pair_core() == modes[i]
        blk.work(torch.as_tensor(xs[:, k:k + L].copy()).cuda(), outs=outs, tags_ptrs=tp)
        st = blk.last_status()
        torch.cuda.synchronize()
        prod = outs["produced"].cpu().numpy().copy()
        res.append((prod, outs["syms"].cpu().numpy().view(np.uint32).copy(), outs["bits"].cpu().numpy().copy(), st))
        k += L
    return res


def _same(got, twin, nan_ok=False):
    nsym = 0
    for i, ((pg, sg, bg, stg), (pt, st_, bt, stt)) in enumerate(zip(got, twin)):
        assert np.array_equal(pg, pt), i
        assert stg == stt, (i, stg, stt)
        if nan_ok:  # the same bits, or NaN on both sides
            fg, ft = sg.view(np.float32), st_.view(np.float32)
            assert np.all((sg == st_) | (np.isnan(fg) & np.isnan(ft))), i
        else:
            assert np.array_equal(sg, st_), (i, np.argwhere(sg != st_)[:4])
        assert np.array_equal(bg, bt), (i, np.argwhere(bg != bt)[:4])  # whole rows, the untouched part included
        nsym += int(pg.sum())
    return nsym


def _oracle(got, xs, sps, gain, limit, q, tags, channels):
    for c in channels:
        o, bt, k = orc.MskStream(sps, gain, limit, 1, max_noutput=q), orc.BitTail(), 0
        for i, L in enumerate(LENS):
            ot = np.zeros(0, orc.TAG_DTYPE)
            if tags is not None:
                sel = tags[c][(tags[c]["offset"] >= k) & (tags[c]["offset"] < k + L)]
                ot = np.zeros(len(sel), dtype=orc.TAG_DTYPE)
                ot["offset"], ot["value"], ot["key"] = sel["offset"], sel["value"], sel["key"]
            out = o.step(xs[c, k:k + L], ot)[0]
            p = got[i][0][c]
            assert p == len(out), (i, c)
            assert np.array_equal(got[i][1][c, : 2 * p], out.view(np.uint32)), (i, c)
            assert np.array_equal(got[i][2][c, :p], bt.process(out)), (i, c)
            k += L


_TWIN = {}


def _twin(ais, key, xs, **kw):
    """the mode 0 run of a configuration, computed once"""
    if key not in _TWIN:
        _TWIN[key] = _run(ais, xs, [0] * len(LENS), **kw)
    return _TWIN[key]


@pytest.mark.parametrize("q", [2, 3, 4, 5, 8, 17, 0])
def test_run_lengths(ais, q):
    # set_max_noutput_items(q) ends every general_work call after q symbols: lock-step runs of q - 1 pairs and the short
    # ones before each landing, of every parity (0: unset, runs of up to MSK_PAIRS_MAX)
    xs = _signal(9)
    got = _run(ais, xs, [1] * len(LENS), q=q)
    nsym = _same(got, _twin(ais, ("q", q), xs, q=q))
    assert got[-1][3] == 0 and nsym > 9 * TOTAL / 4 * 0.95
    _oracle(got, xs, 4.0, 0.04, 0.01, q, None, range(9))


def _tag_cases(nchan, dtype):
    """channel c takes case c % 6"""
    k1 = LENS[0]
    cases = [
        [],                                                                             # no tags
        [(1500 + 2 * j, v) for j, v in enumerate([0.3, -0.2, 0.7, 0.1, -0.6, 0.45, 0.0, 0.9])],  # four tag pairs, consecutive symbols
        [(0, 0.25), (k1, 0.5), (k1 + 64 + 1, -0.25)],                                   # at item 0 of a call
        [(64 * 10 - 1, 0.4), (64 * 20 - 8, -0.7), (64 * 30 - 4, 0.05), (k1 + 65 + 64 * 7 - 2, 0.6)],  # before a chunk boundary
        [(900, float("nan")), (901, 0.3), (3000, float("nan")), (5000, float("nan"))],  # NaN tags
        [(1200, -0.4), (2400, -1.0), (2404, -0.01), (6000, -0.99), (3100, 0.5, 1)],     # negative centres (and another key)
    ]
    return [_tags(cases[c % 6], c, dtype) for c in range(nchan)]


@pytest.mark.parametrize("q", [0, 5])
def test_tags(ais, q):
    xs = _signal(70)
    tags = _tag_cases(70, ais.TAG_DTYPE)
    got = _run(ais, xs, [1] * len(LENS), q=q, tags=tags)
    _same(got, _twin(ais, ("tags", q), xs, q=q, tags=tags))
    assert got[-1][3] == 0
    _oracle(got, xs, 4.0, 0.04, 0.01, q, tags, range(0, 70, 3))


@pytest.mark.parametrize("sps", [4.0, 3.0, 5.2083])
@pytest.mark.parametrize("gain,limit", [(0.04, 0.01), (0.2, 0.05)])
def test_loop_parameters(ais, sps, gain, limit):
    # (0.2, 0.05): the error clip at 3 and the omega clip at `limit` both engage
    xs = _signal(9)
    kw = dict(sps=sps, gain=gain, limit=limit)
    got = _run(ais, xs, [1] * len(LENS), **kw)
    nsym = _same(got, _twin(ais, ("par", sps, gain, limit), xs, **kw))
    assert nsym > 9 * TOTAL / sps * 0.9
    if sps == 4.0:
        _oracle(got, xs, sps, gain, limit, 0, None, range(9))


def test_non_finite_input(ais):
    xs = _signal(9).copy()
    xs[4, 1000] = np.complex64(complex(np.nan, 1.0))
    got = _run(ais, xs, [1] * len(LENS))
    twin = _twin(ais, ("nan",), xs)
    _same(got, twin, nan_ok=True)
    assert got[0][3] & ST_INTERP_RANGE and twin[0][3] & ST_INTERP_RANGE
    _oracle(got, xs, 4.0, 0.04, 0.01, 0, None, [0, 3, 5, 8])  # the neighbours of the channel are untouched


@pytest.mark.parametrize("first", [0, 1])
def test_mode_changes_between_calls(ais, first):
    xs = _signal(70)
    tags = _tag_cases(70, ais.TAG_DTYPE)
    got = _run(ais, xs, [(first + i) & 1 for i in range(len(LENS))], tags=tags)
    # (mode 1 throughout equals mode 0 throughout on this stream: test_tags[0])
    _same(got, _twin(ais, ("tags", 0), xs, q=0, tags=tags))
    assert got[-1][3] == 0
