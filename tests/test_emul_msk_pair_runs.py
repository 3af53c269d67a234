"""The plain lock-step pair loop of k_msk.h under the CPU lane model, where the builds with a symbol stage put the symbol
of a pair into the stage while the next pair loads (the first pair of a run writes the spare row, the last symbol is staged
at the run's exit): runs of every length from 1 to 16 pairs, forced by set_max_noutput_items(Q) (a general_work call of Q
symbols starts with a run of Q - 1 pairs), on streams whose symbol count passes the stage's wrap (32 symbols) many times,
with and without time_est tags -- symbols, counts and bits against the oracle, bit for bit."""
import numpy as np
import pytest

import emul_py as emu
import oracle_py as orc
import synth

LENS = [1100, 37, 1, 700]
TOTAL = sum(LENS)
NCHAN = 9  # a full wave of eight channels and a ragged one
_XS = []


def _signal():
    if not _XS:
        _XS.append(np.stack([synth.make_channel(310 + c, TOTAL, "P", 4, amp=1.0, cfo_max=50.0)[0] for c in range(NCHAN)]))
    return _XS[0]


def _tags(c, with_tags):
    rows = []
    if with_tags and c % 3:
        rng = np.random.default_rng(40 + c)
        for s0 in np.sort(rng.choice(np.arange(40, TOTAL - 40), size=6, replace=False)):
            for j in range(int(rng.integers(1, 5))):
                rows.append((int(s0) + 4 * j, float(rng.uniform(-1, 1))))
        rows.append((LENS[0], -0.5))  # item 0 of a call, negative centre
    rows.sort()
    t = np.zeros(len(rows), dtype=emu.TAG_DTYPE)
    t["offset"] = [r[0] for r in rows]
    t["value"] = [r[1] for r in rows]
    t["key"] = 2
    t["chan"] = c
    return t


def _check(q, lpw, with_tags):
    xs = _signal()
    e = emu.MskStream(4.0, 0.04, 0.01, 1, nchan=NCHAN, lpw=lpw, max_noutput=q)
    o = [orc.MskStream(4.0, 0.04, 0.01, 1, max_noutput=q) for _ in range(NCHAN)]
    bt = [orc.BitTail() for _ in range(NCHAN)]
    tags = [_tags(c, with_tags) for c in range(NCHAN)]
    k = nsym = 0
    for L in LENS:
        cap = 64
        tg = np.zeros((NCHAN, cap), dtype=emu.TAG_DTYPE)
        cnt = np.zeros(NCHAN, np.int32)
        new = []
        for c in range(NCHAN):
            sel = tags[c][(tags[c]["offset"] >= k) & (tags[c]["offset"] < k + L)]
            tg[c, : len(sel)] = sel
            cnt[c] = len(sel)
            new.append(sel)
        r = e.step(xs[:, k:k + L], tg, cnt)
        assert r["status"] == 0
        for c in range(NCHAN):
            ot = np.zeros(len(new[c]), dtype=orc.TAG_DTYPE)
            ot["offset"], ot["value"], ot["key"] = new[c]["offset"], new[c]["value"], new[c]["key"]
            out, _, _, cons = o[c].step(xs[c, k:k + L], ot)
            p = r["produced"][c]
            assert p == len(out) and r["consumed"][c] == cons, (L, c)
            assert np.array_equal(r["syms"][c, :p].view(np.uint32), out.view(np.uint32)), (L, c)
            assert np.array_equal(r["bits"][c, :p], bt[c].process(out)), (L, c)
            nsym += p
        k += L
    assert nsym > NCHAN * TOTAL / 4 * 0.9 > 8 * 32  # (the stage wraps every 32 symbols)


@pytest.mark.parametrize("q", list(range(2, 18)) + [0])
def test_emul_msk_runs_of_every_length(q):
    _check(q, 8, False)


@pytest.mark.parametrize("q,lpw", [(2, 8), (3, 8), (6, 8), (17, 8), (0, 8), (3, 4), (8, 4), (0, 4)])
def test_emul_msk_runs_with_tags(q, lpw):
    _check(q, lpw, True)
