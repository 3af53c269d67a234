"""-m gpu: the buffers a C-ABI handle re-allocates in mid-life (gr-ais_amd/csrc/aisx_host.h: DevBuf::reserve, the
time-parallel path's resources, the profiling ring) and handle teardown.  Every case drives ONE long-lived handle
through a size change and compares it, bit for bit, with the CPU oracle or with a handle that had the final size (or
no such change) from its first call.  Shapes are the smallest that take the paths: a staging buffer grows when a call
asks for more than any call before it, d_ct when a tag list is longer than ctag_cap + 1024 = 1088 records."""
import numpy as np
import pytest

import oracle_py as orc
from parity import assert_tags_match, planted, unit_template
from test_emul_mskp import _tags_with_pairs

pytestmark = pytest.mark.gpu

NCHAN, L, NCALLS = 8, 4096, 7


@pytest.fixture(scope="module")
def ais():
    import torch

    assert torch.cuda.is_available(), "gpu tests need a visible MI355X"
    import ais_amd

    return ais_amd


def _dev(x):
    import torch

    return torch.as_tensor(np.ascontiguousarray(x)).cuda()


@pytest.fixture(scope="module")
def stream8():
    """8 channels x 7 calls of 4096 items and their time_est tags (the recipe of tests/test_gpu_mskp.py); read-only."""
    import synth

    rng = np.random.default_rng(5)
    total = L * NCALLS
    xs = np.stack([synth.make_channel(900 + c, total, "P", 4, amp=1.0, cfo_max=50.0)[0] for c in range(NCHAN)])
    tags = [_tags_with_pairs(rng, total, c, 4.0, 900, 0.3, 6) for c in range(NCHAN)]
    xs.setflags(write=False)
    return xs, tags


def _call_tags(ais, tags, k, cap):
    """the tags of call k as the device hand-over takes them: (records[nchan][cap], counts[nchan], cap)"""
    import torch

    tg = np.zeros((NCHAN, cap), dtype=ais.TAG_DTYPE)
    cnt = np.zeros(NCHAN, np.int32)
    for c in range(NCHAN):
        sel = tags[c][(tags[c]["offset"] >= k * L) & (tags[c]["offset"] < (k + 1) * L)]
        assert len(sel) <= cap
        for f in ("offset", "value", "key", "chan"):
            tg[f][c, : len(sel)] = sel[f]
        cnt[c] = len(sel)
    return torch.as_tensor(tg.view(np.uint8).reshape(NCHAN, -1).copy()).cuda(), torch.as_tensor(cnt).cuda(), cap


def _run_msk(ais, xs, ncalls=NCALLS, tags=None, tag_caps=None, strides=None, tail=False, bits_only=False, tp_calls=()):
    """`ncalls` stream calls on one handle; per call (produced, bits[, syms]) as host arrays, and the handle's stats"""
    import torch

    blk = ais.msk_timing_recovery_cc(4.0, 0.04, 0.01, 1, nchan=NCHAN, max_items=L)
    ts = torch.cuda.Stream() if tail else None
    if tail:
        blk.set_tail_stream(ts)
    res, keep = [], []
    for k in range(ncalls):
        blk.set_time_parallel(4 if k in tp_calls else 0, 1, 0)
        stride = strides[k] if strides else blk.out_capacity
        outs = dict(bits=torch.zeros((NCHAN, stride), dtype=torch.uint8, device="cuda"),
                    produced=torch.zeros(NCHAN, dtype=torch.int32, device="cuda"))
        if not bits_only:
            outs["syms"] = torch.zeros((NCHAN, stride), dtype=torch.complex64, device="cuda")
        tp = _call_tags(ais, tags, k, tag_caps[k]) if tags is not None else None
        keep.append(tp)
        r = blk.work(_dev(xs[:, k * L:(k + 1) * L]), want_syms=not bits_only, outs=outs,
                     tags_ptrs=(tp[0].data_ptr(), tp[1].data_ptr(), tp[2]) if tp else None)
        res.append(r)
    blk.wait_tail()
    torch.cuda.synchronize()
    assert blk.last_status() == 0
    out = []
    for r in res:
        p = r["produced"].cpu().numpy()
        row = [p, [r["bits"][c, : p[c]].cpu().numpy() for c in range(NCHAN)]]
        if not bits_only:
            row.append([r["syms"][c, : p[c]].cpu().numpy().view(np.uint32) for c in range(NCHAN)])
        out.append(row)
    return out, blk.restart_stats()


def _same(a, b):
    assert len(a) == len(b)
    for k, (ra, rb) in enumerate(zip(a, b)):
        assert np.array_equal(ra[0], rb[0]) and ra[0].min() > 0, k
        for part_a, part_b in zip(ra[1:], rb[1:]):
            for c in range(NCHAN):
                assert np.array_equal(part_a[c], part_b[c]), (k, c)


@pytest.mark.parametrize("want_corr", [False, True])
def test_corr_work_host_staging_grows_and_is_reused(ais, want_corr):
    """aisx_corr_work_host with noutput_items 256, 4096, 256 on the 112-sample template: outputs and tags are the
    oracle's (tests/parity.py's tag tolerances) and, bit for bit, those of a handle fed the same items through the
    device entry point, which stages nothing."""
    rng = np.random.default_rng(21)
    N = 112
    tmpl = unit_template(rng, N)
    lens = [256, 4096, 256]
    x = planted(rng, 1, sum(lens), tmpl, [[60, 1000, 2500, 4400]], noise=0.05)[0]
    blk = ais.corr_est_cc(tmpl, 4.0, 1, 0.9, nchan=1, max_items=4096)
    twin = ais.corr_est_cc(tmpl, 4.0, 1, 0.9, nchan=1, max_items=4096)
    o = orc.CorrEst(tmpl, 4.0, 1, 0.9)
    hist, k, ndet = np.zeros(N, np.complex64), 0, 0
    for n in lens:
        buf = np.concatenate([hist, x[k:k + n]])
        out, corr, tags = blk.work_host(buf, n, k, want_corr=want_corr)
        oo, oc, ot = o.work(x[k:k + n], want_corr=want_corr)
        assert np.array_equal(out.view(np.uint32), oo.view(np.uint32))
        ndet += assert_tags_match(tags, ot)
        tout, tcorr = twin.work(_dev(x[None, k:k + n]), want_corr=want_corr)
        assert np.array_equal(out.view(np.uint32), tout.cpu().numpy()[0].view(np.uint32))
        assert tags.tobytes() == twin.tags().tobytes()
        if want_corr:
            assert np.max(np.abs(corr - oc)) / np.max(np.abs(oc)) < 2e-6  # (as tests/test_gpu_corr_msk.py)
            assert np.array_equal(corr.view(np.uint32), tcorr.cpu().numpy()[0].view(np.uint32))
        hist, k = buf[n:], k + n
    assert ndet >= 4


def test_msk_general_work_host_staging_grows_and_is_reused(ais):
    """aisx_msk_general_work_host with (noutput_items, ninput_items, ntags) = (64, 300, 0), (512, 2200, 3),
    (64, 300, 1): symbols, err, mu, bits, consumed and produced are the oracle's."""
    import synth

    rng = np.random.default_rng(8)
    x, _ = synth.make_channel(77, 6000, "P", 4, amp=1.0, cfo_max=50.0)
    buf = np.concatenate([np.zeros(1, np.complex64), x])
    blk = ais.msk_timing_recovery_cc(4.0, 0.04, 0.01, 1)
    o, bt = orc.Msk(4.0, 0.04, 0.01, 1), orc.BitTail()
    read = 0
    for nout, ninput, ntags in [(64, 300, 0), (512, 2200, 3), (64, 300, 1)]:
        assert ninput >= o.forecast(nout)
        tags = np.zeros(ntags, dtype=ais.TAG_DTYPE)
        tags["offset"] = read + np.sort(rng.choice(np.arange(10, ninput - 40), size=ntags, replace=False))
        tags["value"], tags["key"] = rng.uniform(-0.9, 0.9, ntags), 2
        ot = np.zeros(ntags, dtype=orc.TAG_DTYPE)
        ot["offset"], ot["value"], ot["key"] = tags["offset"], tags["value"], tags["key"]
        a = blk.general_work_host(nout, ninput, buf, 1 + read, tags, read)
        b = o.general_work(nout, ninput, buf, 1 + read, ot, read, want_aux=True)
        assert a[4] == b[3] and len(a[0]) == len(b[0]) > 0
        for i in range(3):
            assert np.array_equal(a[i].view(np.uint32), b[i].view(np.uint32))
        assert np.array_equal(a[3], bt.process(b[0]))
        read += a[4]


@pytest.mark.parametrize("tail", [False, True])
def test_msk_symbol_scratch_grows_with_the_output_stride(ais, stream8, tail):
    """bits only (the handle finds the symbols a home): out_stride = out_capacity for two calls, twice that for two,
    the first value again for two -- against a fresh handle driven at the larger stride throughout; once more with
    the bit tail on a stream of its own."""
    cap = ais.msk_timing_recovery_cc(4.0, 0.04, 0.01, 1, nchan=NCHAN, max_items=L).out_capacity
    got, _ = _run_msk(ais, stream8[0], 6, strides=[cap, cap, 2 * cap, 2 * cap, cap, cap], tail=tail, bits_only=True)
    want, _ = _run_msk(ais, stream8[0], 6, strides=[2 * cap] * 6, tail=tail, bits_only=True)
    _same(got, want)


def test_msk_compacted_tag_list_grows_in_mid_life(ais, stream8):
    """a caller tag list of tag_cap 2048 does not fit the 64 + 1024 records per channel d_ct starts with: after one call
    at tag_cap 64 the list is re-allocated; the same calls on a handle that saw 2048 from its first call."""
    xs, tags = stream8
    got, _ = _run_msk(ais, xs, 4, tags=tags, tag_caps=[64, 2048, 2048, 64])
    want, _ = _run_msk(ais, xs, 4, tags=tags, tag_caps=[2048] * 4)
    _same(got, want)


def test_msk_time_parallel_switched_on_and_off_in_mid_life(ais, stream8):
    """aisx_msk_set_time_parallel(h, 4, 1, 0) after two serial calls, three calls with it, two more without: the path's
    resources come into being on a handle that is already running, and its results are the serial kernel's."""
    xs, tags = stream8
    caps = [64] * NCALLS
    got, st = _run_msk(ais, xs, tags=tags, tag_caps=caps, tp_calls=(2, 3, 4))
    want, st0 = _run_msk(ais, xs, tags=tags, tag_caps=caps)
    assert st["calls"] == 3 and st0["calls"] == 0
    _same(got, want)


def test_profiling_rings_wrap_and_restart(ais, stream8):
    """70 calls with profiling on fill the 64-pair ring and wrap it: the history is 64 positive times, the last call's
    time reads, the 70th call's outputs are those of a handle without profiling; off and on again starts the count
    at zero."""
    rng = np.random.default_rng(3)
    tmpl = unit_template(rng, 112)
    x = _dev(planted(rng, 1, 256, tmpl, [[40]], noise=0.05))
    a, b = (ais.corr_est_cc(tmpl, 4.0, 1, 0.9, nchan=1, max_items=256) for _ in range(2))
    a.set_profiling(True)
    for _ in range(70):
        oa, ob = a.work(x)[0], b.work(x)[0]
    h = a.kernel_ms_history()
    assert len(h) == 64 and min(h) > 0 and a.last_kernel_ms() > 0
    assert np.array_equal(oa.cpu().numpy().view(np.uint32), ob.cpu().numpy().view(np.uint32))
    assert a.tags().tobytes() == b.tags().tobytes()
    a.set_profiling(False)
    a.set_profiling(True)
    assert a.kernel_ms_history() == []
    for _ in range(3):
        a.work(x)
    assert len(a.kernel_ms_history()) == 3
    with pytest.raises(Exception):
        b.kernel_ms_history()  # (never enabled: AISX_ERR_INVALID)

    xm = _dev(stream8[0][:, :256])
    c, d = (ais.msk_timing_recovery_cc(4.0, 0.04, 0.01, 1, nchan=NCHAN, max_items=256) for _ in range(2))
    c.set_profiling(True)
    for _ in range(70):
        rc, rd = c.work(xm), d.work(xm)
    h = c.kernel_ms_history()
    assert len(h) == 64 and min(h) > 0
    pc, pd = rc["produced"].cpu().numpy(), rd["produced"].cpu().numpy()
    assert np.array_equal(pc, pd) and pc.min() > 0
    for ch in range(NCHAN):
        assert np.array_equal(rc["bits"][ch, : pc[ch]].cpu().numpy(), rd["bits"][ch, : pd[ch]].cpu().numpy())
    c.set_profiling(False)
    c.set_profiling(True)
    assert c.kernel_ms_history() == []
    for _ in range(3):
        c.work(xm)
    assert len(c.kernel_ms_history()) == 3


def test_create_destroy_churn_then_the_core_demod(ais):
    """Twenty create / destroy cycles of every handle type at a small geometry (a double free or a resource destroyed
    while borrowed shows here or in what follows), then the core demod of the smoke run against the oracle."""
    import torch
    import synth

    opts = dict(samples_per_symbol=4, bits_per_sec=9600.0, clockrec_gain=0.04, omega_relative_limit=0.01, fftlen=1024)
    tmpl = ais.modulate_vector_bc(ais.gmsk_mod(4, 0.4), [1, 1, 0, 0] * 7, [1])
    taps = ais.firdes_low_pass(1.0, 192000.0, 11e3, 1e3)
    ptaps = ais.firdes_low_pass(1.0, 25e6, 11e3, 1e3)
    for i in range(20):
        nchan = 1 + i % 8
        for stages in ("core", "stock"):
            dem = ais.ais_demod(opts, nchan=nchan, max_items=1024, stages=stages, preamble_symbols=tmpl, fused_front_end=True)
            assert dem._chain_handle()
            del dem  # (the chain before the stages it borrows)
        made = [ais.freqest(38400.0, 9600, 512, nchan=nchan), ais.freqest(38400.0, 9600, 1024, nchan=nchan),
                ais.pfb_channelizer_ccf(1024, ptaps, decim=512, max_frames=1024),
                ais.freq_xlating_fir_filter_ccf(4, taps, (-25e3, 25e3), 192000.0, nstreams=1, max_items=4096),
                ais.hdlc_deframer_batch(11, 64, nchan, 1024, 64), ais.pdu_to_nmea_batch("A", nchan, 64, 64),
                ais.pdu_decode_batch(nchan, 64, 64),
                ais.ais_rx((-25e3, 25e3), 192000.0, ("A", "B"), block_items=4096, preamble_symbols=tmpl, taps=taps,
                           max_pdus_per_block=64, decode=bool(i & 1))]
        del made
    sps, nchan, T = 4, 8, 8192
    xs = np.stack([synth.make_channel(31 + c, T, "S", sps, amp=1.0, cfo_max=10.0)[0] for c in range(nchan)])
    dem = ais.ais_demod(opts, nchan=nchan, max_items=T, stages="core", preamble_symbols=tmpl)
    r = dem.work(torch.as_tensor(xs).cuda())
    prod, bits, tags = r["produced"].cpu().numpy(), r["bits"].cpu().numpy(), dem.preamble_detect.tags()
    ndet = 0
    for c in range(nchan):
        ob, _, ot = orc.Demod(sps, tmpl, stages=0).step(xs[c])
        ndet += assert_tags_match(tags[tags["chan"] == c], ot)
        assert prod[c] == len(ob) and np.array_equal(bits[c, : prod[c]], ob)
    assert ndet > 0
