"""The 4-state sequence detector's host form (ais_amd.mlse_detector, aisx_mlse_*; include/aisx.h states it): its model
against a float64 recomputation, clean symbols decided exactly, the windowed search against the exhaustive maximum,
every split of a stream into calls giving the same bytes, and what it recovers near the threshold beside the plain bit
tail -- the oracle chain's symbols of noisy synthetic channels, deframed by the oracle's deframer.  -m "not gpu"."""
import concurrent.futures as cf
import itertools

import numpy as np
import pytest

import mlse_cases as mc


@pytest.fixture(scope="module")
def ais():
    import ais_amd

    return ais_amd


def test_model(ais):
    c0, c1, rot = ais.mlse_detector(0.4).model()
    assert abs(c0 - 0.735928) < 1e-6 and abs(c1 - 0.131918) < 1e-6, (c0, c1)
    w0, w1, th = mc.model(0.4)
    assert abs(c0 - w0) < 1e-12 and abs(c1 - w1) < 1e-12
    assert np.array_equal(rot[..., 0], np.cos(th).astype(np.float32)) and np.array_equal(rot[..., 1], np.sin(th).astype(np.float32))
    assert np.array_equal(th[::-1, ::-1, ::-1], -th)  # theta(-P, -Q, -R) = -theta
    assert np.array_equal(rot[::-1, ::-1, ::-1, 0], rot[..., 0]) and np.array_equal(rot[::-1, ::-1, ::-1, 1], -rot[..., 1])
    for bt in (0.3, 0.5):  # another pulse, another table
        d0, d1, _ = ais.mlse_detector(bt).model()
        e0, e1, _ = mc.model(bt)
        assert abs(d0 - e0) < 1e-12 and abs(d1 - e1) < 1e-12 and abs(d0 - c0) > 1e-3
    for bt in (0.05, 1.5, float("nan")):
        with pytest.raises(ValueError):
            ais.mlse_detector(bt)


def test_clean_symbols_are_decided_exactly(ais):
    N = 300
    for seed in range(5):
        b = np.random.default_rng(seed).integers(0, 2, N + 2)  # b[-1], b[0], ..., b[N]
        bits = np.concatenate(mc.host_run(ais, [mc.clean_symbols(b)]))
        assert bits.size == N
        got = mc.levels_of(bits)
        assert np.array_equal(got[1:N - 1], b[2:N]), seed  # n = 1 .. N - 2 (b[n] is b[n + 1] of the array)


def _brute(s, rot):
    """-> (b[0..N-1] of the exhaustive maximum, its margin over the best sequence with another b[0..N-1])"""
    N = s.size
    s64 = s.astype(np.complex128)
    z = s64 * np.conj(np.concatenate([[0], s64[:-1]]))
    c, sn = rot[..., 0].astype(np.float64), rot[..., 1].astype(np.float64)
    seqs = np.array(list(itertools.product((0, 1), repeat=N + 1)), dtype=np.int64)  # b[0..N]
    tot = np.zeros(len(seqs))
    for n in range(1, N):  # (z[0] = 0)
        p, q, r = seqs[:, n - 1], seqs[:, n], seqs[:, n + 1]
        tot += z[n].real * c[p, q, r] + z[n].imag * sn[p, q, r]
    per_prefix = tot.reshape(-1, 2).max(axis=1)  # the maximum over b[N], per b[0..N-1]
    order = np.argsort(per_prefix)
    return seqs[2 * order[-1], :N], per_prefix[order[-1]] - per_prefix[order[-2]]


def test_against_brute_force(ais):
    rng = np.random.default_rng(11)
    rot = ais.mlse_detector(0.4).model()[2]
    ncases, left_out = 400, 0
    for k in range(ncases):
        N = int(rng.integers(4, 13))
        s = ((rng.normal(size=N) + 1j * rng.normal(size=N)) / np.sqrt(2)).astype(np.complex64)
        want, margin = _brute(s, rot)
        if margin < 1e-4:
            left_out += 1
            continue
        bits = np.concatenate(mc.host_run(ais, [s]))
        assert bits.size == N
        assert np.array_equal(mc.levels_of(bits), want), (k, N, margin)
    assert left_out <= ncases // 20, "%d of %d cases had a margin below 1e-4" % (left_out, ncases)


def test_every_split_gives_the_same_bytes(ais):
    rng = np.random.default_rng(4)
    N = 1000
    s = (rng.normal(size=N) + 1j * rng.normal(size=N)).astype(np.complex64)
    whole = mc.host_run(ais, [s])
    assert whole[0].size == 64 * ((N - 80) // 64 + 1) == 960 and whole[1].size == N - 960
    ref = np.concatenate(whole).tobytes()
    cuts = sorted(rng.integers(0, N + 1, 16).tolist() + [300, 300, 301, 640])  # (0- and 1-symbol calls among them)
    edges = [0] + cuts + [N]
    calls = [s[a:b] for a, b in zip(edges[:-1], edges[1:])]
    assert len(calls) == 21 and min(c.size for c in calls) == 0 and 1 in [c.size for c in calls]
    got = mc.host_run(ais, calls)
    assert b"".join(g.tobytes() for g in got) == ref and sum(g.size for g in got[:-1]) == 960
    seen = 0
    for c, g in zip(calls, got):  # block k comes out with the call that brings symbol 64 k + 79
        before, seen = seen, seen + c.size
        done = lambda n: 0 if n < 80 else 64 * ((n - 80) // 64 + 1)  # noqa: E731
        assert g.size == done(seen) - done(before)
    one = mc.host_run(ais, [s[k:k + 1] for k in range(N)])
    assert b"".join(g.tobytes() for g in one) == ref
    det = ais.mlse_detector()
    det.work(s[:500])
    det.reset()  # a reset forgets the stream
    assert np.concatenate([det.work(s), det.flush()]).tobytes() == ref
    assert det.flush().size == 0 and np.concatenate([det.work(s), det.flush()]).tobytes() == ref  # as new behind a flush


def _gain_one(args):
    import ais_amd
    import oracle_py as orc

    seed, ebn0, tmpl = args
    bits, syms, sent = mc.noisy_channel(seed, 131072, ebn0, tmpl)
    plain = orc.Hdlc(11, 64).work(bits)
    mbits = np.concatenate(mc.host_run(ais_amd, [syms]))
    assert mbits.size == bits.size
    mlse = orc.Hdlc(11, 64).work(mbits)
    return dict(sent=len(sent), plain=len(set(plain) & sent), mlse=len(set(mlse) & sent),
                plain_wrong=len([p for p in plain if p not in sent]), mlse_wrong=len([p for p in mlse if p not in sent]))


@pytest.fixture(scope="module")
def gain():
    tmpl = mc.stock_template()
    jobs = [(5000 + c, e, tmpl) for e in (14, 16) for c in range(4)]
    with cf.ThreadPoolExecutor(8) as ex:
        rows = list(ex.map(_gain_one, jobs))
    out = {}
    for (seed, e, _), r in zip(jobs, rows):
        t = out.setdefault(e, dict.fromkeys(r, 0))
        for k in r:
            t[k] += r[k]
    print("  " + "; ".join("%d dB: %s" % (e, out[e]) for e in out))
    return out


def test_gain_over_the_bit_tail(gain):
    """seeds 5000..5003, 131 072 samples at 4 per symbol: the sent payloads the oracle's deframer finds in the detector's
    bits against those it finds in the bit tail's"""
    assert gain[16]["plain"] >= 1 and gain[16]["mlse"] >= 1.5 * gain[16]["plain"], gain[16]
    assert gain[14]["mlse"] > gain[14]["plain"], gain[14]
    assert gain[14]["mlse_wrong"] <= 2 and gain[16]["mlse_wrong"] <= 2, gain
