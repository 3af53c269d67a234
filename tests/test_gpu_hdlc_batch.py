"""The batched HDLC deframer on the MI355X (aisx_hdlc_batch_*, ais_amd.hdlc_deframer_batch) against the host
deframer that is its specification (one ais_amd.hdlc_deframer_bp per channel fed the same bits call by call), on
the streams of tests/test_hdlc_batch_model.py at 1, 37 and 4096 channels, and behind the stock pipelined chain at
4096 channels, queued as its docstring says.  -m gpu."""
import concurrent.futures as cf

import numpy as np
import pytest

import hdlc_cases as hc

pytestmark = pytest.mark.gpu

SPS = 4
OPTS = dict(samples_per_symbol=SPS, bits_per_sec=9600.0, clockrec_gain=0.04, omega_relative_limit=0.01, fftlen=1024)


@pytest.fixture(scope="module")
def ais():
    import torch

    assert torch.cuda.is_available()
    import ais_amd

    return ais_amd


def _dev_call(call, stride, pad=0):
    import torch

    rows, n = hc.pack(call, stride)
    buf = torch.zeros(rows.size + pad + 64, dtype=torch.uint8, device="cuda")
    b = buf[pad:pad + rows.size].view(rows.shape[0], stride)
    b.copy_(torch.from_numpy(rows))
    return b, torch.from_numpy(n).cuda()


def _run(ais, lmin, lmax, calls, pad=0, max_pdus=1 << 16):
    nch = len(calls[0])
    stride = max(max(len(x) for x in call) for call in calls) + 5
    hd = ais.hdlc_deframer_batch(lmin, lmax, nch, stride, max_pdus)
    got = [[] for _ in range(nch)]
    for call in calls:
        b, n = _dev_call(call, stride, pad)
        hd.work(b, n)
        recs, data = hd.pdus()
        for c, lst in enumerate(hc.by_channel(recs, data, nch)):
            got[c] += lst
    return got


def _check(ais, lmin, lmax, calls, streams=None, pad=0):
    got = _run(ais, lmin, lmax, calls, pad)
    ref = hc.host_ref(lmin, lmax, calls)
    for c in range(len(got)):
        assert [p for _, p in got[c]] == ref[c], c
        if streams is not None:
            assert got[c] == hc.py_ref(lmin, lmax, streams[c]), c
    return sum(len(g) for g in got)


def _frames_in_noise(rng, nbits, lmin, lmax, every=2000, pool=None):
    s = []
    while len(s) < nbits:
        s += hc.noise(rng, int(rng.integers(0, every)))
        s += pool[int(rng.integers(0, len(pool)))] if pool else hc.frame_bits(
            bytes(rng.integers(0, 256, int(rng.integers(max(lmin - 1, 2), lmax + 3)) - 2).astype(np.uint8)))
    return s


@pytest.mark.parametrize("nch", [1, 37])
def test_model_cases_on_the_device(ais, nch):
    rng = np.random.default_rng(100 + nch)
    tot = 0
    for lmin, lmax in ((2, 5), (11, 64), (3, 30)):
        streams = [_frames_in_noise(rng, 20000, lmin, lmax) for _ in range(nch)]
        cuts = [sorted(rng.integers(0, 20000, 3)) for _ in range(nch)]
        calls = [[hc.as_bytes(rng, b, wild=(c % 2 == 1)) for c, b in enumerate(call)] for call in hc.split_calls(streams, cuts)]
        tot += _check(ais, lmin, lmax, calls, pad=3 * (lmin % 2))
    for lmin, lmax in ((11, 64), (2, 2), (2, 9), (4, 40)):
        streams = [hc.adversarial_stream(rng, lmin, lmax) for _ in range(nch)]
        tot += _check(ais, lmin, lmax, [[hc.as_bytes(rng, s, wild=True) for s in streams]], streams)
    streams = []
    for c in range(nch):
        s = hc.noise(rng, 100)
        for octs in (1024, 1025, 700):
            s += hc.frame_bits(bytes(rng.integers(0, 256, octs - 2).astype(np.uint8))) + hc.noise(rng, 50)
        streams.append(s)
    cuts = [[len(s) // 3, len(s) // 3 + c % 3, 2 * len(s) // 3] for c, s in enumerate(streams)]
    tot += _check(ais, 11, 1024, hc.split_calls(streams, cuts), streams)
    print("%d channels: %d PDUs identical to the host deframer" % (nch, tot))


def test_split_at_every_offset_across_a_frame(ais):
    rng = np.random.default_rng(5)
    body = hc.noise(rng, 40) + hc.frame_bits(bytes(rng.integers(0, 256, 12).astype(np.uint8))) + \
        hc.frame_bits(b"\x01\x02\x03\x04\x05\x06\x07\x08\x09") + hc.noise(rng, 10)
    L = len(body)
    streams = [body] * (L + 1)
    n = _check(ais, 9, 64, hc.split_calls(streams, [[c, min(L, c + c % 3)] for c in range(L + 1)]), streams)
    assert n == 2 * (L + 1)


def test_length_max_period(ais):
    rng = np.random.default_rng(9)
    for lmax in (30, 64, 1024):
        for k in (1, 2):
            payload = bytes(rng.integers(0, 256, 20).astype(np.uint8))
            streams, cuts = hc.period_cases(rng, lmax, k, payload)
            assert [p for _, p in hc.py_ref(11, lmax, streams[0])] == [payload]
            n = _check(ais, 11, lmax, hc.split_calls(streams, cuts), streams, pad=lmax % 7)
            assert n == len(streams), (lmax, k)


def _pool_frames(rng, k=64):
    return [hc.frame_bits(bytes(rng.integers(0, 256, int(rng.integers(12, 64))).astype(np.uint8))) for _ in range(k)]


def _big_calls(rng, nch, ncalls, nbits):
    """nch channels x ncalls calls of up to nbits: noise with AIS-sized frames, counts differing per channel"""
    pool = _pool_frames(rng)
    base = [np.asarray(_frames_in_noise(rng, ncalls * nbits, 11, 64, every=1500, pool=pool), np.uint8) for _ in range(61)]
    calls = [[None] * nch for _ in range(ncalls)]
    for c in range(nch):
        s = np.roll(base[c % 61], 977 * c)
        pos = 0
        for k in range(ncalls):
            n = nbits - int(rng.integers(0, 300))
            calls[k][c] = s[pos:pos + n]
            pos += n
    return calls


def _host_pool(lmin, lmax, calls):
    nch = len(calls[0])
    with cf.ThreadPoolExecutor(max_workers=16) as ex:
        def one(c):
            import ais_amd

            d = ais_amd.hdlc_deframer_bp(lmin, lmax)
            out = []
            for call in calls:
                out += d.work(call[c])
            return out
        return list(ex.map(one, range(nch)))


def test_4096_channels_many_calls_deterministic(ais):
    import torch

    rng = np.random.default_rng(7)
    nch, ncalls, nbits = 4096, 4, 16384
    calls = _big_calls(rng, nch, ncalls, nbits)
    stride = nbits + 16
    a = ais.hdlc_deframer_batch(11, 64, nch, stride, 1 << 16)
    b = ais.hdlc_deframer_batch(11, 64, nch, stride, 1 << 16)
    got = [[] for _ in range(nch)]
    for call in calls:
        x, n = _dev_call(call, stride, pad=7)
        a.work(x, n)
        b.work(x, n)
        ra, da = a.pdus()
        rb, db = b.pdus()
        assert ra.tobytes() == rb.tobytes() and da.tobytes() == db.tobytes()  # two handles, identical buffers
        for c, lst in enumerate(hc.by_channel(ra, da, nch)):
            got[c] += [p for _, p in lst]
    torch.cuda.synchronize()
    ref = _host_pool(11, 64, calls)
    assert got == ref
    print("4096 channels x %d calls: %d PDUs identical to the host deframer" % (ncalls, sum(len(g) for g in got)))


def test_overflow_bad_counts_reset_and_interleaving(ais):
    import torch

    rng = np.random.default_rng(8)
    nch, nbits = 37, 6000
    calls = _big_calls(rng, nch, 3, nbits)
    stride = nbits + 16
    full = _run(ais, 11, 64, calls)
    small = ais.hdlc_deframer_batch(11, 64, nch, stride, 5)
    other = ais.hdlc_deframer_batch(11, 64, nch, stride, 1 << 12)
    got = []
    for k, call in enumerate(calls):
        x, n = _dev_call(call, stride)
        small.work(x, n)  # two handles interleaved on one stream
        other.work(x, n)
        ro, do = other.pdus()
        if k == 0:
            with pytest.raises(OverflowError):
                small.pdus()
        rs, ds = small.pdus(overflow_ok=True)
        # overflow: a prefix of the full ordered list is kept, the stream state still advances exactly
        assert len(ro) > 5 and small.found == len(ro) and len(rs) == 5
        assert rs.tobytes() == ro[:5].tobytes() and ds.tobytes() == do[: ds.size].tobytes()
        got += [(int(r["chan"]), int(r["end_bit"]), bytes(do[r["offset"]:r["offset"] + r["len"]])) for r in ro]
    for c in range(nch):
        assert [(e, p) for ch, e, p in got if ch == c] == full[c], c
    # a call of 0 bits everywhere
    small.work(x, torch.zeros(nch, dtype=torch.int32, device="cuda"))
    assert small.pdus()[0].size == 0 and small.found == 0
    # after a reset the handle starts over; a count outside [0, max_bits] leaves that channel where it was and the
    # next read (only) says so
    ref = hc.host_ref(11, 64, calls[:1])
    x, n = _dev_call(calls[0], stride)
    n_bad = n.clone()
    n_bad[3] = stride + 1
    n_bad[4] = -2
    other.reset()
    other.work(x, n_bad)
    with pytest.raises(ValueError):
        other.pdus()
    ro, do = other.pdus()
    byc = hc.by_channel(ro, do, nch)
    assert all([p for _, p in byc[c]] == (ref[c] if c not in (3, 4) else []) for c in range(nch))
    n_34 = torch.zeros_like(n)
    n_34[3], n_34[4] = n[3], n[4]
    other.work(x, n_34)
    ro, do = other.pdus()
    byc = hc.by_channel(ro, do, nch)
    assert [p for _, p in byc[3]] == ref[3] and [p for _, p in byc[4]] == ref[4]
    assert sum(len(v) for v in byc) == len(ref[3]) + len(ref[4])


def _replicated(base, nchan):
    import torch

    nu, T = base.shape
    reps = nchan // nu
    x = torch.as_tensor(base).cuda().repeat(reps, 1)
    rot = torch.exp(1j * torch.linspace(0, 6.0, reps, device="cuda")).to(torch.complex64)
    rot[0] = 1.0
    return (x.view(reps, nu, T) * rot.view(-1, 1, 1)).reshape(nchan, T).contiguous()


def test_stock_chain_4096_channels_deframed_on_the_device(ais):
    """The pipelined stock chain at 4096 channels x 3 steps of 65536 samples with the deframer queued behind every
    step as documented (wait on a stream of ours, process there, read step k's PDUs after step k + 1 is issued).
    Every channel's PDUs equal the host deframer's over the same bits; on the own-waveform channels they are
    what was sent, and the C oracle's deframer over those bits finds the same."""
    import torch

    import oracle_py as orc
    import synth

    nchan, T, steps, K = 4096, 65536, 3, 16
    tmpl = ais.modulate_vector_bc(ais.gmsk_mod(SPS, 0.4), [1, 1, 0, 0] * 7, [1])
    made = [synth.make_channel(4100 + c, T * steps, "S", SPS, amp=0.3, cfo_max=500.0) for c in range(K)]
    xs = np.stack([m[0] for m in made])
    x_dev = [_replicated(xs[:, s * T:(s + 1) * T], nchan) for s in range(steps)]
    dem = ais.ais_demod(OPTS, nchan=nchan, max_items=T, stages="stock", preamble_symbols=tmpl)
    cap = dem.clockrec.out_capacity
    hd = ais.hdlc_deframer_batch(11, 64, nchan, cap, 1 << 16)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    res, gpu = [], [[] for _ in range(nchan)]

    def collect():
        recs, data = hd.pdus(stream=s)
        for c, lst in enumerate(hc.by_channel(recs, data, nchan)):
            gpu[c] += [p for _, p in lst]

    for k in range(steps):
        r = dem.work_pipelined(x_dev[k], x_next=x_dev[k + 1] if k + 1 < steps else None)
        res.append(r)
        if k > 0:
            collect()  # step k - 1's, while step k runs
        dem.wait(r["step"], stream=s)
        hd.work(r["bits"], r["produced"], stream=s)
    collect()
    dem.synchronize()
    bits = [(r["bits"].cpu().numpy(), r["produced"].cpu().numpy()) for r in res]
    calls = [[b[c, : p[c]] for c in range(nchan)] for b, p in bits]
    ref = _host_pool(11, 64, calls)
    assert gpu == ref
    npdu = sum(len(g) for g in gpu)
    sent_n = oracle_n = 0
    for c in range(K):
        sent = [np.packbits(np.array(i["payload"], np.uint8), bitorder="little").tobytes() for i in made[c][1]]
        o = orc.Hdlc(11, 64).work(np.concatenate([call[c] for call in calls]))
        assert o == gpu[c], c
        assert set(gpu[c]) <= set(sent), c
        sent_n += len(sent)
        oracle_n += len(o)
    print("chain 4096 x %d steps: %d PDUs on the device, identical to the host deframer; own-waveform channels: "
          "%d of %d sent recovered" % (steps, npdu, oracle_n, sent_n))
    assert oracle_n > 0
