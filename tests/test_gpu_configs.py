"""-m gpu: the BASELINE.json configurations at their stated sizes, through the C ABI.

  config 2   256 batched channels x 65536 samples, corr_est only, N = 896 and N = 112
  config 3   4096 channels x 65536, the whole python/ais_demod.py:56 flowgraph (freq_sync + agc in
             front, stock template N = 896)
  config 4   the per-GPU shape of 65536 channels on 8 GPUs: 8192 channels x 65536
  SURVEY D3  corr_est at the other samples-per-symbol values the reference is run with
             (python/radio.py:49-57, python/ais.grc:79; isps at lib/corr_est_cc_impl.cc:193,270)

Oracle comparison on a subset of channels (the CPU oracle runs ~2.4 MS/s on the stock chain),
size-independent properties on all of them.
"""
import os

import numpy as np
import pytest

import oracle_py as orc
from parity import assert_tags_match, compare_bursts, compare_detections

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

SPS = 4
OPTS = dict(samples_per_symbol=SPS, bits_per_sec=9600.0, clockrec_gain=0.04, omega_relative_limit=0.01, fftlen=1024)


@pytest.fixture(scope="module")
def ais():
    import torch

    assert torch.cuda.is_available(), "gpu tests need a visible MI355X"
    import ais_amd

    return ais_amd


def _dev(x):
    import torch

    return torch.as_tensor(np.ascontiguousarray(x)).cuda()


def _template(ais, family, sps=SPS):
    import synth

    if family == "S":
        return ais.modulate_vector_bc(ais.gmsk_mod(sps, 0.4), [1, 1, 0, 0] * 7, [1])
    lv = [1 if b else -1 for b in synth.sync_bits("P")]
    return synth.gmsk_waveform(np.array(lv, float), sps)[: len(lv) * sps].astype(np.complex64)


def _replicated(base, nchan):
    """channel c = base[c % len(base)] times a per-replica carrier phase (device side)."""
    import torch

    nu, T = base.shape
    reps = nchan // nu
    assert reps * nu == nchan
    x = _dev(base).repeat(reps, 1)
    rot = torch.exp(1j * torch.linspace(0, 6.0, reps, device="cuda")).to(torch.complex64)
    rot[0] = 1.0
    return (x.view(reps, nu, T) * rot.view(-1, 1, 1)).reshape(nchan, T).contiguous()


@pytest.mark.parametrize("family", ["S", "P"])
def test_config2_256_channels_corr_est_only(ais, family):
    import torch
    import synth

    nchan, T, nu = 256, 65536, 16
    tmpl = _template(ais, family)
    N = tmpl.size
    base = np.stack([synth.make_channel(2000 + c, 2 * T, family, SPS, amp=1.0, cfo_max=15.0 if family == "P" else 3.0)[0]
                     for c in range(nu)])
    blk = ais.corr_est_cc(tmpl, float(SPS), 1, 0.9, nchan=nchan, max_items=T, max_tags_per_chan=1024)
    ora = [orc.CorrEst(tmpl, float(SPS), 1, 0.9) for _ in range(nu)]
    ndet = 0
    prev = None
    for s in range(2):  # two calls: the second starts from a carried history
        chunk = base[:, s * T:(s + 1) * T]
        x = _replicated(chunk, nchan)
        out, _ = blk.work(x)
        torch.cuda.synchronize()
        # A2 on every channel: the output is the input delayed by N, bit for bit
        assert torch.equal(out[:, N:], x[:, : T - N])
        if prev is None:
            assert bool((out[:, :N] == 0).all())
        else:
            assert torch.equal(out[:, :N], prev[:, T - N:])
        prev = x
        tags = blk.tags()
        for c in range(nu):  # replica 0 (no rotation) against the oracle, offsets exact
            _, _, ot = ora[c].work(chunk[c])
            ndet += assert_tags_match(tags[tags["chan"] == c], ot)
        # |corr|^2 does not see the carrier phase: every replica finds the same detections (a peak
        # within rounding of the threshold may flip)
        cnt = np.bincount(tags["chan"][tags["key"] == 2], minlength=nchan).reshape(nchan // nu, nu)
        mism = int((cnt != cnt[0]).any(axis=1).sum())
        print("config 2 (%s) call %d: replica groups whose detection counts differ from group 0: %d of %d" % (family, s, mism, nchan // nu))
        assert mism <= 1  # (achieved: 0)
    print("config 2 (%s, N = %d): %d detections identical to the oracle on %d channels x 2 calls" % (family, N, ndet, nu))
    assert ndet > 20 * nu and blk.nitems_written() == 2 * T


def _stock_chain_against_oracle(ais, nchan, K, steps, seed0):
    """The whole flowgraph on `nchan` channels x 65536 samples per step, through the PIPELINED step the
    benchmark times (ais_demod.work_pipelined = aisx_chain_step: fused front end, frequency estimates
    and NCO phase walk prepared a step ahead, timing recovery and bit tail on their own streams).
    All `steps` steps are issued back to back -- nothing waits in between, the buffer rotation
    wraps -- and compared afterwards.  Channels 0..K-1 carry their own seeded waveform and are
    checked against the oracle with the gates of test_gpu_stages.py::test_stock_chain_full_length_steps;
    the others are replicas of them."""
    import torch
    import synth

    T = 65536
    assert steps <= 3  # (results of the last AISX_CHAIN_DEPTH steps stay readable)
    tmpl = _template(ais, "S")
    import concurrent.futures as cf

    pool = cf.ThreadPoolExecutor(max_workers=min(32, K))  # (numpy and the C oracle release the GIL)
    made = list(pool.map(lambda c: synth.make_channel(seed0 + c, T * steps, "S", SPS, amp=0.3, cfo_max=500.0), range(K)))
    xs = np.stack([m[0] for m in made])
    dem = ais.ais_demod(OPTS, nchan=nchan, max_items=T, stages="stock", preamble_symbols=tmpl)
    thr = dem.preamble_detect.threshold()
    ora = [orc.Demod(SPS, tmpl, stages=3) for _ in range(K)]
    omsk = [orc.MskStream(float(SPS), 0.04, 0.01, 1) for _ in range(K)]
    obt = [orc.BitTail() for _ in range(K)]
    gbits = [[] for _ in range(K)]
    obits = [[] for _ in range(K)]
    tot = dict(detections=0, matched=0, lone=0, lone_near_threshold=0)
    mag = tim = 0.0
    nsym = 0
    x_dev = [_replicated(xs[:, s * T:(s + 1) * T], nchan) for s in range(steps)]
    torch.cuda.synchronize()
    res = [dem.work_pipelined(x_dev[s], x_next=x_dev[s + 1] if s + 1 < steps else None, want_syms=True) for s in range(steps)]
    dem.synchronize()
    assert dem.clockrec.last_status() == 0
    for s in range(steps):
        chunk = xs[:, s * T:(s + 1) * T]
        r = res[s]
        tags = dem.preamble_detect.tags(back=steps - 1 - s)
        prod = r["produced"].cpu().numpy()
        # every channel: a symbol per ~sps samples, nothing truncated
        assert prod.min() > T // SPS - 64 and prod.max() < T // SPS + 64
        syms = r["syms"][:K].cpu().numpy()
        bits = r["bits"][:K].cpu().numpy()
        yo_h = dem.corr_output(r["step"], 0, K).cpu().numpy()
        assert yo_h.shape[1] == T
        order = np.argsort(tags["chan"], kind="stable")
        tsort = tags[order]
        lo = np.searchsorted(tsort["chan"], np.arange(K), "left")
        hi = np.searchsorted(tsort["chan"], np.arange(K), "right")

        def one(c):  # channel c of this step against its own oracle objects (independent of the other channels')
            tc = tsort[lo[c]:hi[c]]
            ob, _, ot = ora[c].step(chunk[c])
            d = compare_detections(tc, ot, thr)
            feed = np.zeros(len(tc), dtype=orc.TAG_DTYPE)
            feed["offset"], feed["value"], feed["key"] = tc["offset"], tc["value"], tc["key"]
            out, _, _, _ = omsk[c].step(yo_h[c], feed)
            assert prod[c] == len(out), (s, c)
            assert np.array_equal(syms[c, : prod[c]].view(np.uint32), out.view(np.uint32)), (s, c)
            assert np.array_equal(bits[c, : prod[c]], obt[c].process(out)), (s, c)
            return d, ob

        for c, (d, ob) in enumerate(pool.map(one, range(K))):
            for k in tot:
                tot[k] += d[k]
            mag, tim = max(mag, d["mag_rel_max"]), max(tim, d["time_est_abs_max"])
            gbits[c].append(bits[c, : prod[c]].copy())
            obits[c].append(ob)
            nsym += prod[c]
    ncmp = same = near = 0
    for c in range(K):
        a, b, d = compare_bursts(np.concatenate(gbits[c]), np.concatenate(obits[c]), made[c][1])
        ncmp, same, near = ncmp + a, same + b, near + d
    print("stock chain (pipelined step) at %d channels x %d steps: %d symbols bit-exact given equal tags on %d channels; %d "
          "detections, %d matched within +-1, %d seen by one side only (%d of them within 2e-5 of the threshold); mag rel max "
          "%.2e, time_est abs max %.2e; %d decoded bursts compared, %d identical in place, %d within +-4 bits"
          % (nchan, steps, nsym, K, tot["detections"], tot["matched"], tot["lone"], tot["lone_near_threshold"], mag, tim,
             ncmp, same, near))
    assert tot["matched"] > 50 * K * steps
    assert tot["lone"] == tot["lone_near_threshold"], "a detection away from the threshold is missing on one side"
    assert tot["lone"] <= max(2, tot["matched"] // 500)
    assert mag <= 1e-5 and tim <= 1e-4
    # Every burst the oracle's chain decodes is in the GPU's bit stream, bit for bit, within a few
    # positions of the same place.  "In place" is counted on the concatenated stream of all steps: one
    # symbol more or less in the noise BEFORE a burst (the two chains' time_est values differ in their
    # last place, ~3e-7, and the loop then free-runs on noise until the next tag) moves every later
    # burst of that channel by one position -- with the tags equal the symbols ARE bit-exact (above).
    # (round 2, 4096 x 2 steps: 453 of 453 in place; round 3, 8192 x 3 steps: 280 of 300, 300 of 300 within +-4)
    # (round 5: 93-100 % in place at every shape run; round 6 gate 0.9)
    assert ncmp > 8 * K * steps and near >= ncmp - tot["lone"] and same >= 0.9 * ncmp
    # PDU level, as the application sees it (python/radio.py:64-73: hdlc_deframer_bp(11, 64) behind the demodulator): every
    # frame the oracle's chain recovers with a good CRC the GPU's bit stream recovers too; what the GPU recovers beyond
    # those is bounded by the detections only one side saw, and every frame it recovers was transmitted
    npdu = nwant = 0
    for c in range(K):
        want = orc.Hdlc(11, 64).work(np.concatenate(obits[c]))
        have = ais.hdlc_deframer_bp(11, 64).work(np.concatenate(gbits[c]))
        sent = [np.packbits(np.array(i["payload"], np.uint8), bitorder="little").tobytes() for i in made[c][1]]
        assert set(want) <= set(have), (c, len(want), len(have))
        assert set(have) <= set(sent), c
        npdu, nwant = npdu + len(have), nwant + len(want)
    print("  PDUs with a good CRC: oracle %d, GPU %d on %d channels" % (nwant, npdu, K))
    assert nwant > 4 * K * steps and npdu - nwant <= tot["lone"]
    return dem, x_dev, res


def test_config3_4096_channels_stock_chain(ais):
    """BASELINE config 3 through the path bench.py times; three steps so that the rotation wraps.
    On top of the oracle gates: a twin object running the stages one after the other on one stream
    (square_and_fft_sync_cc.work -> agc.work -> corr_est.work -> msk.work, the two-block front end)
    gives the same bits on ALL 4096 channels."""
    import torch

    dem, x_dev, res = _stock_chain_against_oracle(ais, 4096, 64, 3, 3100)
    twin = ais.ais_demod(OPTS, nchan=4096, max_items=65536, stages="stock", preamble_symbols=_template(ais, "S"))
    for s, x in enumerate(x_dev):
        r = twin.work(x)
        torch.cuda.synchronize()
        assert torch.equal(r["produced"], res[s]["produced"]), s
        w = int(r["produced"].max())
        idx = torch.arange(w, device="cuda").view(1, -1) < r["produced"].view(-1, 1)
        assert torch.equal(r["bits"][:, :w][idx], res[s]["bits"][:, :w][idx]), s
        a, b = twin.preamble_detect.tags(), dem.preamble_detect.tags(back=len(x_dev) - 1 - s)
        assert np.array_equal(a, b), s


def test_config4_per_gpu_shape_8192_channels(ais):
    # 65536 channels on 8 GPUs = 8192 per GPU (BASELINE config 4; the ranks share nothing)
    _stock_chain_against_oracle(ais, 8192, 64, 3, 3300)


def test_config5_wideband_channelizer_to_nmea(ais):
    """BASELINE config 5 end to end: 25 MS/s wideband IQ -> 1024-lane polyphase channelizer (decim 512:
    48 828 S/s per lane, 5.086 samples per symbol) -> demod lanes -> HDLC deframer -> NMEA, against the
    reference's structure for ONE channel repeated per lane (python/radio.py:49-57,64-73:
    freq_xlating_fir_filter_ccf -> ais_demod -> hdlc_deframer_bp(11, 64) -> pdu_to_nmea) on the oracle.
    Two chains: corr_est -> msk only on lanes whose carrier offset is a few Hz (no freq_sync in
    front of the correlator), and the whole flowgraph (ais_rx's) on all signal lanes, through the
    pipelined step.  The template is the stock 224-symbol one at the lanes' fractional rate.
    Gates: every detection of the oracle on the GPU within +-1 item, peak values within 2e-4 (the
    channelizer's own tolerance: its fp32 sums over 60 227 taps run in another order than the
    oracle's double ones), every PDU the oracle recovers recovered by the GPU, every PDU equal to
    what was transmitted."""
    import concurrent.futures as cf

    import torch
    import synth

    fs, M, D, nfr = 25e6, 1024, 512, 8192
    sps = fs / D / 9600.0
    quiet = [3, 100, 333, 511, 512, 777]          # carrier offset within +-3 Hz
    drift = [200, 640, 900, 1023]                 # up to +-400 Hz: needs freq_sync
    lanes = quiet + drift
    cfo = {m: 3.0 for m in quiet}
    cfo.update({m: 400.0 for m in drift})
    x, infos = synth.make_wideband(55, nfr, lanes, fs=fs, nlanes=M, decim=D, amp=1.1, bursts_per_lane=2, cfo_max=cfo)
    taps = ais.firdes_low_pass(1.0, fs, 11e3, 1e3)
    tmpl = synth.resampled_template(ais.modulate_vector_bc(ais.gmsk_mod(40, 0.4), [1, 1, 0, 0] * 7, [1]), 40, sps)
    assert tmpl.size == 1139
    opts = dict(samples_per_symbol=sps, bits_per_sec=9600.0, clockrec_gain=0.04, omega_relative_limit=0.01, fftlen=1024)

    # GPU: one channelizer call, then 1024 demod lanes at once
    pfb = ais.pfb_channelizer_ccf(M, taps, decim=D, max_frames=nfr)
    lanes_dev = pfb.work(_dev(x))
    assert tuple(lanes_dev.shape) == (M, nfr)
    got = {}
    for stages in ("core", "stock"):
        dem = ais.ais_demod(opts, nchan=M, max_items=nfr, stages=stages, preamble_symbols=tmpl)
        r = dem.work_pipelined(lanes_dev)
        dem.wait(host=True)
        assert dem.clockrec.last_status() == 0
        got[stages] = (r["produced"].cpu().numpy(), r["bits"].cpu().numpy(), dem.preamble_detect.tags(),
                       dem.preamble_detect.threshold())
        del dem
    lanes_host = lanes_dev[lanes].cpu().numpy()

    # oracle: the reference's per-channel filter (double accumulation), then its chain, per lane
    def ref_lane(m):
        return orc.freq_xlating_fir(taps, D, m * fs / M, fs, x, 0, nfr)

    with cf.ThreadPoolExecutor(len(lanes)) as ex:
        yo = dict(zip(lanes, ex.map(ref_lane, lanes)))
    worst = max(float(np.max(np.abs(lanes_host[i] - yo[m])) / np.max(np.abs(yo[m]))) for i, m in enumerate(lanes))
    assert worst < 2e-4, worst
    nm = ais.pdu_to_nmea("A")
    stats = {}
    for stages, st, which in (("core", 0, quiet), ("stock", 3, lanes)):
        prod, bits, tags, thr = got[stages]
        tot = dict(detections=0, matched=0, lone=0, lone_near_threshold=0)
        mag = tim = 0.0
        npdu = nsent = 0
        for m in which:
            ob, _, ot = orc.Demod(sps, tmpl, stages=st).step(yo[m])
            d = compare_detections(tags[tags["chan"] == m], ot, thr, near_rel=5e-4)
            for k in tot:
                tot[k] += d[k]
            mag, tim = max(mag, d["mag_rel_max"]), max(tim, d["time_est_abs_max"])
            gb = bits[m, : prod[m]]
            assert abs(int(prod[m]) - len(ob)) <= 1, (stages, m)
            want = orc.Hdlc(11, 64).work(ob)
            have = ais.hdlc_deframer_bp(11, 64).work(gb)
            assert set(want) <= set(have), (stages, m, len(want), len(have))
            sent = [np.packbits(np.array(i["payload"], np.uint8), bitorder="little").tobytes() for i in infos[m]]
            assert set(have) <= set(sent), (stages, m)  # nothing decoded that was not transmitted
            for p in have:
                assert nm.msg_to_sentence(p) == orc.pdu_to_nmea("A", p)
            npdu += len(have)
            nsent += len(sent)
        stats[stages] = (tot, mag, tim, npdu, nsent)
        print("config 5 (%s, %d lanes of 1024): %d detections, %d matched within +-1, %d seen by one side only (%d near the "
              "threshold); mag rel max %.2e, time_est abs max %.2e; %d of %d transmitted frames decoded to NMEA, channelizer vs "
              "reference filter %.1e" % (stages, len(which), tot["detections"], tot["matched"], tot["lone"],
                                         tot["lone_near_threshold"], mag, tim, npdu, nsent, worst))
        assert tot["matched"] >= 2 * len(which) and tot["lone"] == tot["lone_near_threshold"]
        assert mag <= 2e-4 and tim <= 2e-3
        assert npdu >= nsent - 1
    # the lanes that carry nothing find nothing
    idle = np.setdiff1d(np.arange(M), lanes)
    assert not np.isin(got["core"][2]["chan"], idle).any()


def test_config4_rows_do_not_depend_on_their_position(ais):
    # 8192 channels whose upper half repeats the lower half: the same input row gives the same
    # bits and tags wherever it sits in the batch (workgroup, wave, lane)
    import torch
    import synth

    nchan, T, nu = 8192, 65536, 8
    tmpl = _template(ais, "S")
    base = np.stack([synth.make_channel(3500 + c, T, "S", SPS, amp=1.0, cfo_max=3.0)[0] for c in range(nu)])
    half = _replicated(base, nchan // 2)
    x = torch.cat([half, half], dim=0).contiguous()
    dem = ais.ais_demod(OPTS, nchan=nchan, max_items=T, stages="core", preamble_symbols=tmpl)
    r = dem.work(x)
    assert dem.clockrec.last_status() == 0
    prod = r["produced"]
    assert torch.equal(prod[: nchan // 2], prod[nchan // 2:])
    bits = r["bits"]
    m = int(prod.max())
    valid = torch.arange(m, device="cuda").view(1, -1) < prod[: nchan // 2].view(-1, 1)  # (rows are written up to `produced`)
    assert bool(((bits[: nchan // 2, :m] == bits[nchan // 2:, :m]) | ~valid).all())
    tags = dem.preamble_detect.tags()
    lo, hi = tags[tags["chan"] < nchan // 2], tags[tags["chan"] >= nchan // 2]
    assert len(lo) == len(hi) > 0
    assert np.array_equal(lo["offset"], hi["offset"]) and np.array_equal(lo["value"], hi["value"])
    assert np.array_equal(lo["chan"] + nchan // 2, hi["chan"])
    ob, _, ot = orc.Demod(SPS, tmpl, stages=0).step(base[0])
    assert_tags_match(tags[tags["chan"] == 0], ot, exact_offsets=False)
    assert int(prod[0]) == len(ob)


@pytest.mark.parametrize("sps_block,sps_signal", [(5.0, 5), (5.2083, 5), (3.0, 3), (4.4, 4)])
def test_corr_est_other_samples_per_symbol(ais, sps_block, sps_signal):
    # isps = (int)(sps + 0.5) steps the peak search (lib/corr_est_cc_impl.cc:193,270); the stock
    # receiver runs the block at 5.2083 sps against a 5 sps template (python/radio.py:49-57)
    import synth

    tmpl = _template(ais, "S", sps_signal)
    nchan, T = 12, 40000
    xs = np.stack([synth.make_channel(2600 + c, T, "S", sps_signal, amp=1.0, cfo_max=3.0)[0] for c in range(nchan)])
    blk = ais.corr_est_cc(tmpl, sps_block, 1, 0.9, nchan=nchan, max_items=T, max_tags_per_chan=2048)
    ora = [orc.CorrEst(tmpl, sps_block, 1, 0.9) for _ in range(nchan)]
    ndet = 0
    for lo, hi in ((0, 25000), (25000, 25001), (25001, T)):
        out, _ = blk.work(_dev(xs[:, lo:hi]))
        out = out.cpu().numpy()
        tags = blk.tags()
        for c in range(nchan):
            oo, _, ot = ora[c].work(xs[c, lo:hi])
            assert np.array_equal(out[c], oo)
            ndet += assert_tags_match(tags[tags["chan"] == c], ot)
    assert ndet > 2 * nchan


def test_set_symbols_with_a_new_length_follows_the_reference(ais):
    # lib/corr_est_cc_impl.cc:132-162: history, output multiple and mark_delay follow the new
    # length; taps are stored as given (no conjugate / reverse); d_thresh stays; the FFT filter
    # restarts from a zeroed tail while the delayed pass-through keeps the block's history
    from parity import planted, unit_template

    rng = np.random.default_rng(77)
    t1, t2, t3 = unit_template(rng, 200), unit_template(rng, 640), unit_template(rng, 96)
    nchan, n = 3, 6000
    blk = ais.corr_est_cc(t1, 4.0, 300, 0.5, nchan=nchan, max_items=n, max_tags_per_chan=1024)
    ora = [orc.CorrEst(t1, 4.0, 300, 0.5) for _ in range(nchan)]
    assert blk.mark_delay() == 199
    cur = t1
    for step, new in enumerate((None, t2, None, t3, t3)):
        if new is not None:
            blk.set_symbols(new)
            for o in ora:
                o.set_symbols(new)
            cur = new
            assert np.array_equal(blk.symbols(), new)
            assert blk.history() == new.size + 1 == ora[0].history
            assert blk.output_multiple() == ora[0].output_multiple
            assert blk.mark_delay() == ora[0].mark_delay and blk.threshold() == ora[0].threshold
        # set_symbols stores the taps as given, so a burst that matches them is conj(reverse(taps))
        sig = np.conj(cur[::-1]) if step > 0 and cur is not t1 else cur
        x = planted(rng, nchan, n, sig, [[500, 3000], [10], [n - sig.size - 5]], noise=0.05, amp=2.0)
        out, corr = blk.work(_dev(x), want_corr=True)
        out, corr = out.cpu().numpy(), corr.cpu().numpy()
        tags = blk.tags()
        for c in range(nchan):
            oo, oc, ot = ora[c].work(x[c], want_corr=True)
            assert np.array_equal(out[c], oo), (step, c)
            assert np.max(np.abs(corr[c] - oc)) / (np.max(np.abs(oc)) + 1e-30) < 2e-6, (step, c)
            assert_tags_match(tags[tags["chan"] == c], ot)
    with pytest.raises(ValueError):
        blk.set_symbols(unit_template(rng, 2500))


def test_agc_floor_both_values(ais):
    # [GR] feedforward_agc_cc: "float max_env = 1e-4; // avoid divide by zero, indirectly set max
    # gain" (live) vs the commented-out 1e-12: they differ only where a whole window stays below 1e-4
    rng = np.random.default_rng(9)
    nchan, n = 4, 9000
    x = (rng.normal(size=(nchan, n)) + 1j * rng.normal(size=(nchan, n))).astype(np.complex64)
    x[0, 2000:5000] *= 1e-6
    x[1, :] *= 3e-6
    x[2, 100:4000] = 0
    differs = 0
    for floor in (1e-4, 1e-12):
        blk = ais.feedforward_agc_cc(512, 2.0, nchan=nchan, max_items=n)
        if floor != 1e-4:
            blk.set_floor(floor)
        out = blk.work(_dev(x)).cpu().numpy()
        for c in range(nchan):
            want = orc.Agc(512, 2.0, floor=floor if floor != 1e-4 else None).work(x[c])
            assert np.array_equal(out[c].view(np.uint32), want.view(np.uint32)), (floor, c)
        differs += int(np.abs(out[1]).max() > 1.0)
    assert differs == 1  # the quiet channel is lifted to the reference level only with the 1e-12 floor
    with pytest.raises(ValueError):
        blk.set_floor(0.0)


def test_freqest_work_host_gnuradio_path(ais):
    # freqest::work as the scheduler calls it: host vectors in, one float per vector out; maxpos is
    # a local of the call (lib/freqest_impl.cc:68 vs :74): an all-zero first vector gives -9600 Hz
    fe = ais.freqest(38400.0, 9600, 1024, nchan=1)
    v = np.zeros((4, 1024), dtype=np.complex64)
    v[1, 394] = 5
    v[1, 650] = 4j
    v[3, 100] = v[3, 356] = 1
    got = fe.work_host(v)
    want = orc.FreqEst.make(38400.0, 9600, 1024).work(v)
    assert got.tolist() == want.tolist() == [-9600.0, 187.5, 187.5, want[3]]
    # a second call starts from maxpos = 0 again
    assert fe.work_host(v[2:3]).tolist() == [-9600.0]
    rng = np.random.default_rng(4)
    r = (rng.normal(size=(7, 1024)) + 1j * rng.normal(size=(7, 1024))).astype(np.complex64)
    assert np.array_equal(fe.work_host(r), orc.FreqEst.make(38400.0, 9600, 1024).work(r))
    with pytest.raises(ValueError):
        ais.freqest(38400.0, 9600, 1024, nchan=2).work_host(v)


@pytest.mark.parametrize("nchan", [2048, 4096, 8192])
def test_chain_front_end_claim_is_near_the_best_of_a_sweep(ais, nchan):
    # aisx_chain_create places the front-end kernel's workgroups by an LDS claim it derives from the part's CU count / LDS size
    # and the recovery kernel's launch (aisx_chain.hip: chain_front_claim; DESIGN_APPENDIX.md A.6 holds the full sweep of
    # tools/claim_sweep.py).  The gate: a step with the chain's own choice takes at most 2 % longer than the best of
    # {no claim, 24, 48, 63 KB} set by hand on the same chain object, medians of three interleaved runs of 20 steps;
    # a claim never changes a result (test_config3 / test_config4 run with it, their twins without).
    # The sweep runs in a process of its own with the eight hardware queues the chain's streams are made for (DESIGN.md
    # 4.8; the runtime reads GPU_MAX_HW_QUEUES once, at its first call, and this process has made that call): with
    # fewer, two of the streams share a queue and run in turn, and the kernels the claim places beside each other no
    # longer overlap.
    import json
    import subprocess
    import sys

    code = ("import json, sys; sys.path.insert(0, %r); import claim_sweep as cs; "
            "print(json.dumps(cs.sweep(%d, [0, 24, 48, 63], steps=20, reps=3)))" % (os.path.join(ROOT, "tools"), nchan))
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, GPU_MAX_HW_QUEUES="8"), capture_output=True,
                         text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    r = json.loads(out.stdout.strip().splitlines()[-1])
    print("claim sweep at %d channels: chosen %d B -> %.3f ms per step; by hand %s" % (
        nchan, r["chosen_claim_bytes"], r["ms_per_step"]["chosen"], {k: v for k, v in r["ms_per_step"].items() if k != "chosen"}))
    assert r["chosen_claim_bytes"] > 0
    assert r["ms_per_step"]["chosen"] <= 1.02 * r["best_of_sweep_ms"], r["ms_per_step"]
    assert r["ms_per_step"]["chosen"] <= 1.01 * r["ms_per_step"]["0"], r["ms_per_step"]  # never slower than no claim (1 % of scatter)
