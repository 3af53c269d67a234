"""-m gpu: the batched freq_xlating_fir_filter_ccf on the device (libaisx.so, k_xlate.h) against the float64 filter of
the oracle: the matrix of test_xlate_model.py through ragged calls, split invariance bit for bit, strided and unaligned
rows, rows that do not depend on their position, retunes against the closed form, more than 2^32 inputs, agreement
with pfb_channelizer_ccf on the 1024-lane grid; and the stock receiver (python/radio.py ais_rx) end to end, from IQ at
250 kS/s to NMEA text, pipelined one step ahead of the chain as INTEGRATION.md describes."""
import ctypes as C

import numpy as np
import pytest

import oracle_py as orc
import xlate_cases as xc
from parity import compare_detections

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ais():
    import torch

    assert torch.cuda.is_available(), "gpu tests need a visible MI355X"
    import ais_amd

    return ais_amd


def _dev(x):
    import torch

    return torch.as_tensor(np.ascontiguousarray(x)).cuda()


def _run_calls(f, x_dev, sizes):
    import torch

    ys, o = [], 0
    for n in sizes:
        ys.append(f.work(x_dev[:, o:o + n]))
        o += n
    return torch.cat(ys, dim=1).cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_matrix_and_split_invariance(ais):
    worst = 0.0
    for case in xc.matrix():
        taps, x = xc.inputs(case)
        xd = _dev(x)
        f = ais.freq_xlating_fir_filter_ccf(case["D"], taps, case["freqs"], xc.FS, nstreams=case["ns"],
                                            max_items=case["max_items"])
        y = _run_calls(f, xd, xc.calls(case["D"], case["N"], case["max_items"]))
        nout = -(-case["N"] // case["D"])
        assert y.shape == (case["ns"] * case["nch"], nout)
        w = xc.worst(y, xc.reference(case, taps, x, nout))
        assert w <= xc.GATE, (case["D"], case["L"], case["nch"], w)
        worst = max(worst, w)
        g = ais.freq_xlating_fir_filter_ccf(case["D"], taps, case["freqs"], xc.FS, nstreams=case["ns"], max_items=case["N"])
        assert np.array_equal(_bits(g.work(xd).cpu().numpy()), _bits(y)), (case["D"], case["L"])
        # another ragged split (primes), and after reset() the same bits again
        g.reset()
        assert np.array_equal(_bits(_run_calls(g, xd, xc.calls(case["D"], case["N"], case["N"], prime=31))), _bits(y))
    print("device: %d cases, worst max|y - y64| / max|y64| = %.2e" % (len(xc.matrix()), worst))


def test_strided_unaligned_rows(ais):
    import torch

    rng = np.random.default_rng(3)
    taps = ais.firdes_low_pass(1.0, xc.FS, 11e3, 1e3)
    freqs = np.array([[-25e3, 25e3, 12345.678]] * 3)
    N = 5 * 3000 + 2
    x = xc.signal(rng, 3, N, freqs)
    f = ais.freq_xlating_fir_filter_ccf(5, taps, freqs, xc.FS, nstreams=3, max_items=N)
    want = f.work(_dev(x)).cpu().numpy()
    big = torch.zeros((3, N + 7), dtype=torch.complex64, device="cuda")
    big[:, 1:1 + N] = _dev(x)                      # rows 8-byte aligned only, odd row stride
    out = torch.full((9, want.shape[1] + 5), 7.0 + 7.0j, dtype=torch.complex64, device="cuda")
    f.reset()
    got = f.work(big[:, 1:1 + N], out=out[:, 3:])
    assert got.data_ptr() == out[:, 3:].data_ptr()
    assert np.array_equal(_bits(got.cpu().numpy()), _bits(want))
    o = out.cpu().numpy()
    assert (o[:, :3] == 7.0 + 7.0j).all() and (o[:, 3 + want.shape[1]:] == 7.0 + 7.0j).all()  # nothing outside


def test_rows_do_not_depend_on_their_position(ais):
    rng = np.random.default_rng(4)
    taps = ais.firdes_low_pass(1.0, xc.FS, 11e3, 1e3)
    freqs = np.array([[-25e3, 25e3]] * 64)
    freqs[:32, 1] = freqs[32:, 1] = rng.uniform(-xc.FS / 2, xc.FS / 2, 32)
    x = xc.signal(rng, 32, 5 * 2500, freqs[:32])
    xx = np.concatenate([x, x])
    f = ais.freq_xlating_fir_filter_ccf(5, taps, freqs, xc.FS, nstreams=64, max_items=xx.shape[1])
    y = _run_calls(f, _dev(xx), [777, 5000, xx.shape[1] - 5777])
    assert np.array_equal(_bits(y[:64]), _bits(y[64:]))


def test_retune_twice_closed_form(ais):
    rng = np.random.default_rng(9)
    D, taps = 5, ais.firdes_low_pass(1.0, xc.FS, 11e3, 1e3)
    f_list = [25e3, -25e3, 12345.678]
    x = xc.signal(rng, 1, 5 * 4000 + 3, np.array([f_list]))
    xd = _dev(x)
    f = ais.freq_xlating_fir_filter_ccf(D, taps, f_list[0], xc.FS, max_items=12000)
    ys, k_list = [f.work(xd[:, :6001]).cpu().numpy()], []
    for i, (a, b) in enumerate(((6001, 12001), (12001, x.shape[1]))):
        k_list.append(sum(y.shape[1] for y in ys))
        f.set_center_freq(f_list[i + 1])
        assert f.center_freq() == f_list[i + 1]
        ys.append(f.work(xd[:, a:b]).cpu().numpy())
    y = np.concatenate(ys, axis=1)[0]
    y64 = xc.retune_reference(taps, D, x[0], f_list, k_list, y.size)
    w = float(np.max(np.abs(y - y64)) / np.max(np.abs(y64)))
    print("retuned twice: worst %.2e" % w)
    assert w <= xc.GATE, w


def test_more_than_2_to_the_32_inputs(ais):
    """one stream, 16 taps, decimation 64: 2^32 + 64 * 193 zeros in calls of 2^26, then a signal.  The tail equals the
    oracle on the signal alone times e^{-j w Z}: no 32-bit index, no phase drift."""
    import torch

    D, L, fc = 64, 16, 12345.678
    taps = xc.lowpass(L, D)
    big = 1 << 26
    Z = (1 << 32) + 64 * 193
    f = ais.freq_xlating_fir_filter_ccf(D, taps, fc, xc.FS, max_items=big)
    zeros = torch.zeros((1, big), dtype=torch.complex64, device="cuda")
    out = torch.empty((1, big // D), dtype=torch.complex64, device="cuda")
    left = Z
    while left:
        n = min(big, left)
        f.work(zeros[:, :n], out=out)
        left -= n
    rng = np.random.default_rng(12)
    sig = xc.signal(rng, 1, D * 300, np.array([[fc]]))
    y = f.work(_dev(sig)).cpu().numpy()[0]
    turns = (np.longdouble(fc) / np.longdouble(xc.FS) * np.longdouble(Z)) % 1
    y64 = orc.freq_xlating_fir(taps, D, fc, xc.FS, sig[0], 0, 300) * np.exp(-2j * np.pi * float(turns))
    w = float(np.max(np.abs(y - y64)) / np.max(np.abs(y64)))
    print("after %d inputs: worst %.2e" % (Z, w))
    assert y.size == 300 and w <= xc.GATE, w


def test_agrees_with_the_channelizer_on_its_grid(ais):
    fs, M, D, nfr = 25e6, 1024, 512, 256
    taps = ais.firdes_low_pass(1.0, fs, 11e3, 1e3)
    assert taps.size == 60227
    lanes = [3, 200, 511, 1000]
    cen = [m * fs / M if m < M // 2 else m * fs / M - fs for m in lanes]
    rng = np.random.default_rng(8)
    n = nfr * D
    t = np.arange(n)
    x = (rng.standard_normal(n) + 1j * rng.standard_normal(n)) * 0.3
    for c in cen:
        x += np.exp(2j * np.pi * (c + 2000.0) / fs * t)
    x = x.astype(np.complex64)
    pfb = ais.pfb_channelizer_ccf(M, taps, decim=D, max_frames=nfr)
    lanes_dev = pfb.work(_dev(x)).cpu().numpy()[lanes]
    f = ais.freq_xlating_fir_filter_ccf(D, taps, cen, fs, max_items=n)
    y = f.work(_dev(x[None, :])).cpu().numpy()
    assert y.shape == (4, nfr)
    w = max(float(np.max(np.abs(y[i] - lanes_dev[i])) / np.max(np.abs(lanes_dev[i]))) for i in range(4))
    print("against pfb_channelizer_ccf (60 227 taps, D = 512): %.2e" % w)
    assert w < 2e-4, w


# ---- the stock receiver end to end -----------------------------------------------------------------------------

FS_STOCK, DECIM, T, STEPS, NS = 250e3, 5, 65536, 5, 8  # (5 steps: the ring of 4 row buffers wraps)
SPS = FS_STOCK / DECIM / 9600.0


def _stock_inputs():
    import concurrent.futures as cf

    import synth

    # noise_sigma 0.1: config 5's SNR per channel (it runs sigma 1 at 25 MS/s, a hundred times the bandwidth)
    def one(s):
        return synth.make_wideband(700 + s, T * STEPS, [1, 9], fs=FS_STOCK, nlanes=10, decim=DECIM, group_delay=301,
                                   amp=1.0, bursts_per_lane=4, cfo_max=400.0, noise_sigma=0.1, tail_frames=3000)

    with cf.ThreadPoolExecutor(NS) as ex:
        made = list(ex.map(one, range(NS)))
    return np.stack([m[0] for m in made]), [m[1] for m in made]


def _template(ais):
    import synth

    return synth.resampled_template(ais.modulate_vector_bc(ais.gmsk_mod(40, 0.4), [1, 1, 0, 0] * 7, [1]), 40, SPS)


def _receiver(ais, x_steps, nstreams, overlap=True):
    """filter -> stock chain (work_pipelined) -> hdlc_deframer_batch -> pdu_to_nmea_batch for every step.  With overlap
    the filter runs one step ahead into a ring of AISX_CHAIN_DEPTH + 1 row buffers, each refilled only after
    aisx_chain_wait_input of the step that last read it; without, every step is filtered, issued and waited for on its
    own.  Returns the correlator's threshold and per step the tags, PDUs, NMEA records and text."""
    import torch

    from ais_amd import _lib

    taps = ais.firdes_low_pass(1.0, FS_STOCK, 11e3, 1e3)
    nch = 2 * nstreams
    xl = ais.freq_xlating_fir_filter_ccf(DECIM, taps, (-25e3, 25e3), FS_STOCK, nstreams=nstreams, max_items=T * DECIM)
    opts = dict(samples_per_symbol=SPS, bits_per_sec=9600.0, clockrec_gain=0.04, omega_relative_limit=0.01, fftlen=1024)
    dem = ais.ais_demod(opts, nchan=nch, max_items=T, stages="stock", preamble_symbols=_template(ais))
    hd = ais.hdlc_deframer_batch(11, 64, nch, dem.clockrec.out_capacity, 1 << 16)
    nm = ais.pdu_to_nmea_batch(["A", "B"] * nstreams, nch, 1 << 16, 64)
    depth = _lib.lib().aisx_chain_depth()
    ring = [torch.empty((nch, T), dtype=torch.complex64, device="cuda") for _ in range(depth + 1)]
    cur = torch.cuda.current_stream()
    s = torch.cuda.Stream()
    got = []

    def filt(k):
        if k >= depth + 1:  # the buffer was last read by step k - depth - 1
            _lib.check(_lib.lib().aisx_chain_wait_input(dem._chain_handle(), k - depth - 1, C.c_void_p(cur.cuda_stream), 0),
                       "wait_input")
        y = xl.work(x_steps[k], out=ring[k % (depth + 1)])
        assert y.shape[1] == T
        return y

    res = {}

    def collect(step):
        tags = dem.step_tags(step, stream=s)
        pdus = hd.pdus(stream=s, as_list=True)  # (synchronises s, which waited for the step)
        recs, text = nm.sentences(stream=s)
        got.append((tags, pdus, recs, text, res.pop(step)["produced"][:32].cpu().numpy()))

    y_next = filt(0)
    for k in range(STEPS):
        y = y_next
        y_next = filt(k + 1) if overlap and k + 1 < STEPS else None
        r = dem.work_pipelined(y, x_next=y_next)
        res[r["step"]] = r
        if overlap and k > 0:
            collect(k - 1)
        dem.wait(r["step"], stream=s)
        hd.work(r["bits"], r["produced"], stream=s)
        nm.work(hd, stream=s)
        if not overlap:
            collect(k)
            dem.synchronize()
            if k + 1 < STEPS:
                y_next = filt(k + 1)
    if overlap:
        collect(STEPS - 1)
    dem.synchronize()
    return dem.preamble_detect.threshold(), got


def _oracle_channel(ais, taps, tmpl, x_stream, f):
    yo = orc.freq_xlating_fir(taps, DECIM, f, FS_STOCK, x_stream, 0, T * STEPS)
    dm = orc.Demod(SPS, tmpl, stages=3)
    res = [dm.step(yo[k * T:(k + 1) * T]) for k in range(STEPS)]
    bits = np.concatenate([r[0] for r in res])
    return [r[2] for r in res], orc.Hdlc(11, 64).work(bits), [len(r[0]) for r in res]


def _check_against_oracle(ais, thr, got, xs, infos, nstreams_checked):
    import concurrent.futures as cf

    taps = ais.firdes_low_pass(1.0, FS_STOCK, 11e3, 1e3)
    tmpl = _template(ais)
    jobs = [(s, c) for s in range(nstreams_checked) for c in range(2)]
    with cf.ThreadPoolExecutor(len(jobs)) as ex:
        ora = dict(zip(jobs, ex.map(lambda j: _oracle_channel(ais, taps, tmpl, xs[j[0]], (-25e3, 25e3)[j[1]]), jobs)))
    tot = dict(detections=0, matched=0, lone=0, lone_near_threshold=0)
    nwant = nhave = nsent = 0
    des = ["A", "B"]
    mag = tim = 0.0
    missing, extra = [], []
    for (s, c), (otags, want, nbits) in ora.items():
        ch = 2 * s + c
        for k in range(STEPS):
            tags = got[k][0]
            d = compare_detections(tags[tags["chan"] == ch], otags[k], thr, near_rel=5e-4)
            for key in tot:
                tot[key] += d[key]
            mag, tim = max(mag, d["mag_rel_max"]), max(tim, d["time_est_abs_max"])
            if d["lone"] or d["matched"] != d["detections"]:
                print("  step %d chan %d: %s" % (k, ch, {key: d[key] for key in ("detections", "matched", "lone", "lone_near_threshold")}))
        # bits produced per step: the filter's rows differ from the float64 filter's in their last bits, and between
        # bursts the timing loop free-runs on noise, so its rate there follows its own history (measured: up to 22 of
        # ~12 580 symbols per step apart).  The loop bounds it: omega_relative_limit = 1 %
        prod = [int(got[k][4][ch]) for k in range(STEPS)]
        if prod != nbits:
            print("  chan %d: bits per step %s, oracle %s" % (ch, prod, nbits))
        assert all(abs(a - b) <= 0.01 * b + 1 for a, b in zip(prod, nbits)), (ch, prod, nbits)
        have = [p for k in range(STEPS) for (cc, _, p) in got[k][1] if cc == ch]
        sent = [np.packbits(np.array(i["payload"], np.uint8), bitorder="little").tobytes() for i in infos[s][9 if c == 0 else 1]]
        if not set(want) <= set(have):   # every PDU the oracle recovers
            missing.append((s, c, len(want), len(have), [i["start"] for i in infos[s][9 if c == 0 else 1]]))
        if not set(have) <= set(sent):   # nothing that was not transmitted
            extra.append((s, c))
        nwant, nhave, nsent = nwant + len(want), nhave + len(have), nsent + len(sent)
    print("  missing (stream, chan, oracle PDUs, device PDUs, burst starts):", missing, "extra:", extra)
    assert not missing and not extra
    # the NMEA text, byte for byte: every record's line is the oracle's armouring of its PDU
    import nmea_cases as nc

    for k in range(STEPS):
        tags, pdus, recs, text, _ = got[k]
        lines = nc.split(recs, text)
        assert len(lines) == len(pdus)
        for (ch, e, t), (ch2, e2, p) in zip(lines, pdus):
            assert (ch, e) == (ch2, e2)
            if ch < 2 * nstreams_checked:
                assert t == orc.pdu_to_nmea(des[ch % 2], p), (k, ch)
    print("stock receiver, %d channels checked: %d detections, %d matched within +-1, %d one side only (%d near the "
          "threshold); mag rel max %.2e, time_est abs max %.2e; PDUs: oracle %d, device %d, transmitted %d"
          % (2 * nstreams_checked, tot["detections"], tot["matched"], tot["lone"], tot["lone_near_threshold"], mag, tim, nwant,
             nhave, nsent))
    # config 5's gates (test_gpu_configs.py): a detection seen by one side only is one at the threshold, the matched ones
    # agree in peak and time_est, and nearly every transmitted frame comes out
    assert tot["lone"] == tot["lone_near_threshold"]
    assert tot["matched"] >= 0.99 * tot["detections"] and tot["matched"] >= 2 * STEPS * len(ora)
    assert mag <= 2e-4 and tim <= 2e-3
    assert nhave >= nsent - 1


def test_stock_receiver_end_to_end(ais):
    """8 streams at 250 kS/s, channels A (-25 kHz, lane 9) and B (+25 kHz, lane 1) with carrier offsets up to
    +-400 Hz, 5 steps of 65 536 items: against the oracle's per-channel path; the overlapped run gives the same bits as
    the steps issued one after the other."""
    import torch

    xs, infos = _stock_inputs()
    x_steps = [_dev(xs[:, k * T * DECIM:(k + 1) * T * DECIM]) for k in range(STEPS)]
    thr, got = _receiver(ais, x_steps, NS, overlap=True)
    _check_against_oracle(ais, thr, got, xs, infos, NS)
    _, seq = _receiver(ais, x_steps, NS, overlap=False)
    for k in range(STEPS):
        assert np.array_equal(got[k][0], seq[k][0]) and got[k][1] == seq[k][1] and got[k][3] == seq[k][3], k
    torch.cuda.synchronize()


def test_stock_receiver_bench_shape_twins(ais):
    """2048 streams x 2 channels (4096 rows x 65 536 items per step, the chain's default step), every stream a twin of
    one of the 8 seeded ones: the first 8 against the oracle, every twin's rows, PDUs and text equal to its original's"""
    import torch

    xs, infos = _stock_inputs()
    reps = 2048 // NS
    x_steps = [_dev(xs[:, k * T * DECIM:(k + 1) * T * DECIM]).repeat(reps, 1) for k in range(STEPS)]
    # the rows of the first 16 streams, filtered alone, against their twins in the big batch
    taps = ais.firdes_low_pass(1.0, FS_STOCK, 11e3, 1e3)
    xl = ais.freq_xlating_fir_filter_ccf(DECIM, taps, (-25e3, 25e3), FS_STOCK, nstreams=2048, max_items=T * DECIM)
    y = xl.work(x_steps[0])
    small = ais.freq_xlating_fir_filter_ccf(DECIM, taps, (-25e3, 25e3), FS_STOCK, nstreams=NS, max_items=T * DECIM)
    y0 = small.work(x_steps[0][:NS])
    assert torch.equal(y.view(reps, 2 * NS, T).view(torch.float32), y0.unsqueeze(0).expand(reps, -1, -1).view(torch.float32))
    del y, xl
    thr, got = _receiver(ais, x_steps, 2048, overlap=True)
    _check_against_oracle(ais, thr, got, xs, infos, NS)
    for k in range(STEPS):
        tags, pdus, recs, text, _ = got[k]
        per = {}
        for ch, e, p in pdus:
            per.setdefault(ch, []).append((e, p))
        for ch in range(2 * NS):
            base = per.get(ch, [])
            for r in range(1, reps):
                assert per.get(ch + 2 * NS * r, []) == base, (k, ch, r)
        assert len(pdus) == reps * sum(len(per.get(ch, [])) for ch in range(2 * NS))
