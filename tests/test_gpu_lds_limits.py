"""-m gpu: handles of one kernel that ask for different dynamic-LDS sizes, interleaved.  The limit hipFuncSetAttribute
raises belongs to a kernel on a device, not to a handle (aisx_host.h: ensure_dyn_lds): a handle asking for less must not
lower it under one asking for more.  Every test runs the LARGER size first and asserts that order from the handles'
own getters, so that a later change to the kernels' sizes cannot quietly turn it into the raising order; every call is
held to the CPU oracle or to a twin handle, byte for byte -- a call that merely raises no error proves nothing."""
import ctypes as C
import threading

import numpy as np
import pytest

import oracle_py as orc
from parity import assert_tags_match, planted, unit_template

pytestmark = pytest.mark.gpu

OPTS = dict(samples_per_symbol=4, bits_per_sec=9600.0, clockrec_gain=0.04, omega_relative_limit=0.01, fftlen=1024)
DEFAULT_LIMIT = 64 * 1024  # the runtime's dynamic-LDS limit before any hipFuncSetAttribute
LDS_CU = 160 * 1024  # the MI355X's LDS per CU


@pytest.fixture(scope="module")
def ais():
    import torch

    assert torch.cuda.is_available(), "gpu tests need a visible MI355X"
    import ais_amd

    return ais_amd


def _dev(x):
    import torch

    return torch.as_tensor(np.ascontiguousarray(x)).cuda()


def _per_chan(tags, nchan):
    return [tags[tags["chan"] == c] for c in range(nchan)]


def _corr_total(blk):
    claim, used = blk.get_lds_claim()
    assert used > 0, "the F = 4096 build must serve this length"
    return used + claim


class _CorrCase:
    """a correlator handle with its own template, channel count and carried oracle, fed fresh planted input per call"""

    def __init__(self, ais, seed, N, nchan, n, claim=0, tmpl=None):
        self.rng = np.random.default_rng(seed)
        self.N, self.nchan, self.n = N, nchan, n
        self.tmpl = unit_template(self.rng, N) if tmpl is None else tmpl
        self.blk = ais.corr_est_cc(self.tmpl, 4.0, 1, 0.9, nchan=nchan, max_items=n, max_tags_per_chan=512)
        self.blk.set_lds_claim(claim)
        self.orc = [orc.CorrEst(self.tmpl, 4.0, 1, 0.9) for _ in range(nchan)]
        self.written = 0
        self.whole = 0  # templates planted whole so far: the detections to expect at least

    def next_input(self):
        n, N = self.n, self.N
        # per channel: two or three whole templates, one across the call's end on channel 0 (history carried)
        pos = [[300 + 7 * c, n // 2 - N // 3 + c, n - N // 2] if c == 0 else [200 + 11 * c, n - N - 5 - c]
               for c in range(self.nchan)]
        self.whole += sum(1 for pl in pos for p in pl if p + N <= n)
        return planted(self.rng, self.nchan, n, self.tmpl, pos)

    def check(self, x, out, corr, tags, live=True):
        """one call's results against the oracle's (live: the handle has made no later call); returns the detections
        compared"""
        ndet = 0
        per = _per_chan(tags, self.nchan)
        for c in range(self.nchan):
            oo, oc, ot = self.orc[c].work(x[c], want_corr=True)
            assert np.array_equal(out[c].view(np.uint32), oo.view(np.uint32)), c
            assert np.max(np.abs(corr[c] - oc)) / (np.max(np.abs(oc)) + 1e-30) < 2e-6, c
            ndet += assert_tags_match(per[c], ot)
        self.written += x.shape[1]
        assert not live or self.blk.nitems_written() == self.written
        return ndet

    def call(self):
        x = self.next_input()
        out, corr = self.blk.work(_dev(x), want_corr=True)
        return self.check(x, out.cpu().numpy(), corr.cpu().numpy(), self.blk.tags())


def test_corr_two_template_lengths_share_the_generic_build(ais):
    # N = 2000 and N = 600 have no build of their own: both launch k_corr4f_main<0> (aisx_lib.hip: corr4f_pick) with
    # cfz_lds_bytes(N) each.  A (larger) first, then B, then A again: B's first launch must not lower A's limit.
    a = _CorrCase(ais, 11, 2000, 5, 9000)
    b = _CorrCase(ais, 12, 600, 3, 7000)
    assert _corr_total(a.blk) > _corr_total(b.blk) > 0 and _corr_total(a.blk) > DEFAULT_LIMIT, (a.blk.get_lds_claim(),
                                                                                               b.blk.get_lds_claim())
    ndet = 0
    for case in (a, b, a, b, a):
        ndet += case.call()
    assert a.whole + b.whole >= 40 and ndet >= a.whole + b.whole


def test_corr_one_length_two_claims_claiming_handle_first(ais):
    # the mirror of test_gpu_corr_msk.py::test_corr_lds_claim_changes_placement_not_results: k_corr4f_main<896> with a
    # claim launches first, its bare twin (below the default limit) second, the claiming handle again third
    rng = np.random.default_rng(78)
    N, n, nchan = 896, 3 * 3200 + 517, 4
    tmpl = unit_template(rng, N)
    a = ais.corr_est_cc(tmpl, 4.0, 1, 0.9, nchan=nchan, max_items=n)
    b = ais.corr_est_cc(tmpl, 4.0, 1, 0.9, nchan=nchan, max_items=n)
    a.set_lds_claim(17408)
    ta, tb = a.get_lds_claim(), b.get_lds_claim()
    assert ta[1] == tb[1] > 0 and tb[0] == 0 and sum(ta) > DEFAULT_LIMIT and sum(ta) > sum(tb), (ta, tb)
    o = [orc.CorrEst(tmpl, 4.0, 1, 0.9) for _ in range(nchan)]
    ndet = 0
    for i in range(3):
        x = planted(rng, nchan, n, tmpl, [[700 + i, 5000, n - N // 2], [5 + i], [n - N - 3], [1234, 6000 + i]])
        xa = _dev(x)
        oa, ca = a.work(xa, want_corr=True)
        tga = a.tags()
        ob, cb = b.work(xa, want_corr=True)
        tgb = b.tags()
        oa, ca, ob, cb = (t.cpu().numpy() for t in (oa, ca, ob, cb))
        assert np.array_equal(oa.view(np.uint32), ob.view(np.uint32)), i
        assert np.array_equal(ca.view(np.uint32), cb.view(np.uint32)), i
        assert tga.tobytes() == tgb.tobytes(), i
        per = _per_chan(tga, nchan)
        for c in range(nchan):
            oo, _, ot = o[c].work(x[c], want_corr=True)
            assert np.array_equal(oa[c].view(np.uint32), oo.view(np.uint32)), (i, c)
            ndet += assert_tags_match(per[c], ot)
    assert ndet >= 3 * 6  # (the templates planted whole)


def _front_pair(ais, nchan, max_items, agc_claim, walk_claim):
    from ais_amd import _lib

    L = _lib.lib()
    fs = ais.square_and_fft_sync_cc(38400.0, 9600.0, 1024, nchan=nchan, max_items=max_items)
    agc = ais.feedforward_agc_cc(512, 2.0, nchan=nchan, max_items=max_items + 1024)
    assert L.aisx_agc_set_lds_claim(agc._h, agc_claim) == 0
    assert L.aisx_freqsync_set_walk_lds_claim(fs._h, walk_claim) == 0
    return fs, agc


def _front_totals(fs, agc):
    from ais_amd import _lib

    L = _lib.lib()
    a, ua, w, uw = C.c_int(-1), C.c_int(-1), C.c_int(-1), C.c_int(-1)
    assert L.aisx_agc_get_lds_claim(agc._h, C.byref(a), C.byref(ua)) == 0
    assert L.aisx_freqsync_get_walk_lds_claim(fs._h, C.byref(w), C.byref(uw)) == 0
    assert ua.value > 0 and uw.value > 0
    return ua.value + a.value, uw.value + w.value


def test_fused_front_end_two_pairs_with_different_claims(ais):
    # k_agcw<true> (the streaming AGC: W = 512 and whole 512-item blocks, k_agcw.h: agcw_applies) and k_fs_walk, two
    # freqsync + agc pairs: A with large claims, B with smaller ones that are still above the default limit (so that B
    # does ask for a limit of its own); A, B, A, B, every call bit-exact against the two oracle blocks
    import synth

    lens = [4096, 3072, 8192, 2048]
    pairs = []
    for seed, nchan, agc_claim, walk_claim in ((1500, 24, 96 * 1024, 100 * 1024), (1600, 16, 60 * 1024, 64 * 1024)):
        fs, agc = _front_pair(ais, nchan, max(lens), agc_claim, walk_claim)
        xs = np.stack([synth.make_channel(seed + c, sum(lens), "P", 4, amp=0.4, cfo_max=500.0)[0] for c in range(nchan)])
        ofs = [orc.FreqSync(38400.0, 9600.0, 1024) for _ in range(6)]
        oag = [orc.Agc(512, 2.0) for _ in range(6)]
        pairs.append(dict(fs=fs, agc=agc, xs=xs, ofs=ofs, oag=oag, k=0))
    (ta_agc, ta_walk), (tb_agc, tb_walk) = (_front_totals(p["fs"], p["agc"]) for p in pairs)
    assert ta_agc > tb_agc > DEFAULT_LIMIT and ta_walk > tb_walk > DEFAULT_LIMIT, (ta_agc, tb_agc, ta_walk, tb_walk)
    nout = 0
    for L in lens:
        for p in pairs:  # A, then B
            k = p["k"]
            assert L % 512 == 0
            y = ais.freq_sync_agc(p["fs"], p["agc"], _dev(p["xs"][:, k:k + L]))[0].cpu().numpy()
            assert y.shape[1] == L  # (whole vectors: nothing pending, the streaming kernel ran)
            for c in range(6):
                yo, _ = p["ofs"][c].process(p["xs"][c, k:k + L])
                want = p["oag"][c].work(yo)
                assert np.array_equal(y[c].view(np.uint32), want.view(np.uint32)), (L, c)
            nout += y.shape[1]
            p["k"] = k + L
    assert nout == 2 * sum(lens)


def test_two_pipelined_chains_with_different_front_end_claims(ais):
    """Two stock chains of different channel counts, stepped alternately with work_pipelined.  aisx_chain_create derives
    the front-end and walk claims (aisx_chain.hip: chain_front_claim); while the recovery leaves half of the CUs free --
    the only regime where the derived totals exceed the default limit -- the derived claim is the same for every channel
    count, so chain B's handles are given smaller claims, still above the default limit, by hand after creation.  Each
    chain's bits and tags equal those of a serial twin, and its first channels' bits the oracle chain's."""
    import synth
    from ais_amd import _lib

    L = _lib.lib()
    T, steps, K = 8192, 4, 8
    chains = []
    for seed, nchan in ((5100, 64), (5300, 40)):
        made = [synth.make_channel(seed + c, T * steps, "S", 4, amp=0.3, cfo_max=500.0) for c in range(nchan)]
        pipe = ais.ais_demod(OPTS, nchan=nchan, max_items=T, stages="stock")
        ser = ais.ais_demod(OPTS, nchan=nchan, max_items=T, stages="stock")
        pipe._chain_handle()  # (creates the chain: the claims are derived now)
        tmpl = np.asarray(pipe.mod_vector, dtype=np.complex64)
        chains.append(dict(nchan=nchan, xs=np.stack([m[0] for m in made]), pipe=pipe, ser=ser,
                           ora=[orc.Demod(4, tmpl, stages=3) for _ in range(K)], gb=[[] for _ in range(K)],
                           ob=[[] for _ in range(K)]))
    da, db = (_front_totals(ch["pipe"].freq_sync, ch["pipe"].agc) for ch in chains)
    assert da == db and min(da) > DEFAULT_LIMIT, (da, db)  # what the rule derives for both
    b = chains[1]["pipe"]
    ua, uw = C.c_int(0), C.c_int(0)
    assert L.aisx_agc_get_lds_claim(b.agc._h, None, C.byref(ua)) == 0
    assert L.aisx_freqsync_get_walk_lds_claim(b.freq_sync._h, None, C.byref(uw)) == 0
    assert L.aisx_agc_set_lds_claim(b.agc._h, 66 * 1024 - ua.value) == 0
    assert L.aisx_freqsync_set_walk_lds_claim(b.freq_sync._h, 66 * 1024 - uw.value) == 0
    ta, tb = (_front_totals(ch["pipe"].freq_sync, ch["pipe"].agc) for ch in chains)
    assert ta[0] > tb[0] > DEFAULT_LIMIT and ta[1] > tb[1] > DEFAULT_LIMIT, (ta, tb)
    nbits = 0
    for s in range(steps):
        got = []
        for ch in chains:  # A, then B: each step's launches of B follow A's
            xs = ch["xs"]
            x = _dev(xs[:, s * T:(s + 1) * T])
            nxt = _dev(xs[:, (s + 1) * T:(s + 2) * T]) if s + 1 < steps else None
            rs = ch["ser"].work(x)
            got.append((rs, ch["ser"].preamble_detect.tags(), ch["pipe"].work_pipelined(x, x_next=nxt)))
        for ch, (rs, ts, rp) in zip(chains, got):
            ch["pipe"].synchronize()
            ps, pp = rs["produced"].cpu().numpy(), rp["produced"].cpu().numpy()
            bs, bp = rs["bits"].cpu().numpy(), rp["bits"].cpu().numpy()
            assert np.array_equal(ps, pp), s
            for c in range(ch["nchan"]):
                assert np.array_equal(bs[c, :ps[c]], bp[c, :pp[c]]), (s, c)
            assert ts.tobytes() == ch["pipe"].step_tags(rp["step"]).tobytes(), s
            nbits += int(pp.sum())
            for c in range(K):
                ob, _, _ = ch["ora"][c].step(ch["xs"][c, s * T:(s + 1) * T])
                ch["gb"][c].append(bp[c, :pp[c]].copy())
                ch["ob"][c].append(ob)
    assert nbits > 0.9 * (64 + 40) * (steps * T - 1024) / 4
    for ch in chains:
        assert ch["pipe"].clockrec.last_status() == 0
        same = sum(int(np.array_equal(np.concatenate(ch["gb"][c]), np.concatenate(ch["ob"][c]))) for c in range(K))
        assert same >= K - 2, same  # (a time_est that differs in its last place may slip a symbol in the noise: parity.py)


def test_two_host_threads_drive_correlators_of_different_lengths(ais):
    # one correlator per host thread, each on its own stream (N = 2000 and N = 600: one kernel, two sizes); ctypes lets go
    # of the GIL in the foreign calls, so the two threads' launches -- and their raises of the kernel's limit -- overlap
    import torch

    ncalls = 20
    cases = [_CorrCase(ais, 21, 2000, 3, 6000), _CorrCase(ais, 22, 600, 2, 4000)]
    assert _corr_total(cases[0].blk) > _corr_total(cases[1].blk) and _corr_total(cases[0].blk) > DEFAULT_LIMIT
    inputs = [[case.next_input() for _ in range(ncalls)] for case in cases]
    dins = [[_dev(x) for x in xl] for xl in inputs]
    streams = [torch.cuda.Stream() for _ in cases]
    torch.cuda.synchronize()
    results = [[] for _ in cases]
    errors = []
    start = threading.Barrier(len(cases))

    def drive(i):
        try:
            start.wait()
            for x in dins[i]:
                out, corr = cases[i].blk.work(x, want_corr=True, stream=streams[i])
                results[i].append((out, corr, cases[i].blk.tags(stream=streams[i])))
        except BaseException as e:  # (re-raised in the test's own thread)
            errors.append(e)

    threads = [threading.Thread(target=drive, args=(i,)) for i in range(len(cases))]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    torch.cuda.synchronize()
    ndet = 0
    for i, case in enumerate(cases):
        assert len(results[i]) == ncalls
        for x, (out, corr, tags) in zip(inputs[i], results[i]):
            ndet += case.check(x, out.cpu().numpy(), corr.cpu().numpy(), tags, live=False)
        assert case.blk.nitems_written() == case.written
    assert cases[0].whole + cases[1].whole >= ncalls * 8 and ndet >= cases[0].whole + cases[1].whole


def _msk_run(ais, nchan, lens, seed, tp_join):
    """the timing recovery over calls `lens` on the current device (tp_join None: the serial kernel k_msk; 1 / 0: the
    time-parallel recovery with k_msk_ff / k_mskp_join as the join), bit-exact against orc.MskStream"""
    import torch
    import synth
    from test_emul_mskp import _tags_with_pairs

    rng = np.random.default_rng(seed)
    total = sum(lens)
    xs = np.stack([synth.make_channel(900 + c + seed, total, "P", 4, amp=1.0, cfo_max=50.0)[0] for c in range(nchan)])
    blk = ais.msk_timing_recovery_cc(4.0, 0.04, 0.01, 1, nchan=nchan, max_items=max(lens))
    if tp_join is not None:
        blk.set_time_parallel(64, join_kernel=tp_join, max_unit_items=16384)
    o = [orc.MskStream(4.0, 0.04, 0.01, 1) for _ in range(nchan)]
    all_tags = [_tags_with_pairs(rng, total, c, 4.0, 900, 0.3, 6, None) for c in range(nchan)]
    k = nsym = 0
    for L in lens:
        cap = max(len(t) for t in all_tags) + 1
        tg = np.zeros((nchan, cap), dtype=ais.TAG_DTYPE)
        cnt = np.zeros(nchan, np.int32)
        new = []
        for c in range(nchan):
            sel = all_tags[c][(all_tags[c]["offset"] >= k) & (all_tags[c]["offset"] < k + L)]
            for f in ("offset", "value", "key", "chan"):
                tg[f][c, : len(sel)] = sel[f]
            cnt[c] = len(sel)
            new.append(sel)
        d_tags = torch.as_tensor(tg.view(np.uint8).reshape(nchan, -1).copy()).cuda()
        d_cnt = torch.as_tensor(cnt).cuda()
        r = blk.work(_dev(xs[:, k:k + L]), tags_ptrs=(d_tags.data_ptr(), d_cnt.data_ptr(), cap))
        assert blk.last_status() == 0
        prod, syms = r["produced"].cpu().numpy(), r["syms"].cpu().numpy()
        for c in range(nchan):
            ot = np.zeros(len(new[c]), dtype=orc.TAG_DTYPE)
            ot["offset"], ot["value"], ot["key"] = new[c]["offset"], new[c]["value"], new[c]["key"]
            out, _, _, _ = o[c].step(xs[c, k:k + L], ot)
            assert prod[c] == len(out), (c, L)
            assert np.array_equal(syms[c, :prod[c]].view(np.uint32), out.view(np.uint32)), (c, L)
            nsym += prod[c]
        k += L
    return nsym


def test_timing_recovery_on_a_second_device(ais):
    # k_msk and the time-parallel kernels on device 0, then on device 1, in one process: the limit raised on device 0
    # is not device 1's (the recovery's ~92 KB need a raise of their own there)
    import torch
    from ais_amd import _lib

    L = _lib.lib()
    n = C.c_int(0)
    assert L.aisx_device_count(C.byref(n)) == 0
    if n.value < 2:
        pytest.skip("one device visible: the second-device case needs two")
    try:
        for d in (0, 1):
            assert L.aisx_set_device(d) == 0
            with torch.cuda.device(d):
                for join in (None, 1, 0):
                    assert _msk_run(ais, 40, [12000, 37, 6000], 31 + d, join) > 40 * 3500
    finally:
        assert L.aisx_set_device(0) == 0


def test_corr_refuses_a_size_the_device_cannot_give_and_changes_nothing(ais):
    # N = 2048 uses ~74 KB; a 96 KB claim on top is more than the part's 160 KB per CU: the call is refused before
    # anything is launched or any state of the handle moves, and after the claim is taken back the stream goes on as
    # if the refused call had never been made
    import torch

    case = _CorrCase(ais, 41, 2048, 3, 9000)
    ndet = case.call()
    case.blk.set_lds_claim(96 * 1024)
    claim, used = case.blk.get_lds_claim()
    assert claim == 96 * 1024 and used + claim > LDS_CU, (claim, used)
    tags_before = case.blk.tags().tobytes()
    written = case.blk.nitems_written()
    x = case.next_input()
    xd = _dev(x)
    out = torch.full_like(xd, complex(7.0, -7.0))
    corr = torch.full_like(xd, complex(-3.0, 3.0))
    from ais_amd import _lib

    L = _lib.lib()
    torch.cuda.synchronize()
    rc = L.aisx_corr_process(case.blk._h, xd.data_ptr(), xd.stride(0), out.data_ptr(), out.stride(0), corr.data_ptr(),
                             corr.stride(0), xd.shape[1], None)
    msg = L.aisx_last_error().decode()
    assert rc == _lib.AISX_ERR_INVALID, (rc, msg)
    assert str(used + claim) in msg and str(LDS_CU) in msg, msg
    torch.cuda.synchronize()
    assert bool((out == complex(7.0, -7.0)).all()) and bool((corr == complex(-3.0, 3.0)).all())  # nothing launched
    assert case.blk.nitems_written() == written
    assert case.blk.tags().tobytes() == tags_before
    with pytest.raises(ValueError):
        case.blk.work(xd)
    case.blk.set_lds_claim(0)
    # the same input again, now accepted: the oracle sees it as the second call of an uninterrupted stream
    o2, c2 = case.blk.work(xd, want_corr=True)
    ndet += case.check(x, o2.cpu().numpy(), c2.cpu().numpy(), case.blk.tags())
    ndet += case.call()
    assert ndet >= case.whole - 2  # (the refused call's input was drawn once and counted once, yet detected twice)
