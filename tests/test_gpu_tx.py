"""The batched burst transmitter on the device (aisx_tx_batch_*, k_tx.h) against its host specification
(aisx_hdlc_frame, aisx_tx_render_host), and looped back through the receive chain.

Measured on an MI355X at the shapes of test_rows_against_host (3 channels x 4096 samples): max |device - host| is
printed by the test and quoted in DESIGN.md 4.9; ROWS_GATE is four times that figure."""
import numpy as np
import pytest

import tx_cases as tc

pytestmark = pytest.mark.gpu

# 4 x the largest max |device - host| measured on an MI355X over the three runs of test_rows_against_host
ROWS_MEASURED = 8.5e-7
ROWS_GATE = 4 * ROWS_MEASURED


@pytest.fixture(scope="module")
def ais():
    import torch

    assert torch.cuda.is_available(), "gpu tests need a visible MI355X"
    import ais_amd

    return ais_amd


def test_device_levels_equal_host_levels(ais):
    pay = tc.payload_set()
    tx = ais.ais_tx_batch(5.0, 4, len(pay), length_max=126)
    tx.set_bursts(pay, np.arange(len(pay)) % 4, np.arange(len(pay))[::-1] * 100)  # (sorting moves every burst)
    for k, p in enumerate(pay):
        assert np.array_equal(tx.levels(k), ais.hdlc_framer(p)), k
    tx24 = ais.ais_tx_batch(5.0, 1, 8, training_bits=24, ramp_syms=0, tail_syms=0, length_max=126)
    tx24.set_bursts(pay[-8:], 0, 0)
    for k, p in enumerate(pay[-8:]):
        assert np.array_equal(tx24.levels(k), ais.hdlc_framer(p, 24, 0, 0)), k


T0, N = 60000, 4096


def _row_cases(ais, sps):
    """3 channels x [T0, T0 + N): channel 0 a burst that began before T0, one across the tile boundary at item 2048
    with frac 0.999 and cfo +0.01 and one overlapping it with cfo -0.01; channel 1 two bursts abutting with no gap, one
    that ends behind T0 + N and a 1000-octet burst that began long before T0 (t - start above 60000 where sps lets a
    burst be that long: 49 500 samples is the most at sps 5); channel 2 empty."""
    rng = np.random.default_rng(11)
    p21 = [rng.integers(0, 256, 21, dtype=np.uint8).tobytes() for _ in range(6)]
    long_ = b"\xff" * 1000
    dur = lambda p: int(np.ceil(ais.hdlc_framer(p).size * sps))
    far = max(int(dur(long_) - 0.75 * N), 45000)  # the long burst ends inside the window
    ab = T0 + 300
    pay = [p21[0], p21[1], p21[2], p21[3], p21[4], p21[5], long_]
    chan = [0, 0, 0, 1, 1, 1, 1]
    start = [T0 - dur(p21[0]) // 2, T0 + 2048 - dur(p21[1]) // 2, T0 + 2048, ab, ab + dur(p21[3]), T0 + N - 600, T0 - far]
    frac = [0.0, 0.999, 0.25, 0.0, 0.0, 0.5, 0.125]
    cfo = [0.0, 0.01, -0.01, 0.001, -0.002, 0.0, 0.01]
    amp = [1.0, 0.7, 0.5, 1.0, 1.0, 0.3, 0.2]
    phase = [0.0, 1.0, -2.0, 3.0, 0.5, -0.5, 2.5]
    return dict(payloads=pay, chan=chan, start=start, frac=frac, cfo=cfo, amp=amp, phase=phase)


@pytest.fixture(scope="module")
def rows(ais):
    """sps -> (schedule, host rows), computed once"""
    out = {}
    for sps in (5.0, 5.2083, 26.0417):
        sc = _row_cases(ais, sps)
        out[sps] = (sc, ais.gmsk_scene(sc["payloads"], sc["chan"], sc["start"], sps, 3, T0, N, frac=sc["frac"], amp=sc["amp"],
                                       cfo=sc["cfo"], phase=sc["phase"]))
    return out


def _tx(ais, sps, sc, nchan=3):
    tx = ais.ais_tx_batch(sps, nchan, 16, length_max=1023)
    tx.set_bursts(sc["payloads"], sc["chan"], sc["start"], frac=sc["frac"], amp=sc["amp"], cfo=sc["cfo"], phase=sc["phase"])
    return tx


@pytest.mark.parametrize("sps", [5.0, 5.2083, 26.0417])
def test_rows_against_host(ais, rows, sps):
    sc, want = rows[sps]
    if sps > 20:
        assert T0 - sc["start"][-1] > 60000
    got = _tx(ais, sps, sc).render(T0, N).cpu().numpy()
    dev = np.abs(got.astype(np.complex128) - want.astype(np.complex128))
    print("tx rows at sps %g: max |device - host| = %.3e (channels: %s), %d samples in bursts"
          % (sps, dev.max(), ", ".join("%.2e" % v for v in dev.max(axis=1)), int((want != 0).sum())))
    assert (want[2] == 0).all() and (want[0] != 0).sum() > 2000 and (want[1] != 0).sum() > 2000
    assert np.array_equal(got[want == 0], want[want == 0]), "a sample outside every burst is not zero"
    assert dev.max() <= ROWS_GATE


def test_any_split_is_bit_identical(ais, rows):
    import torch

    for sps in (5.0, 5.2083):
        sc, _ = rows[sps]
        tx = _tx(ais, sps, sc)
        one = tx.render(T0, N)
        parts = torch.full((3, N), 7.0, dtype=torch.complex64, device="cuda")
        off = 0
        for n in (1, 63, 64, 1000, N - 1128):
            tx.render(T0 + off, n, out=parts[:, off:off + n])
            off += n
        assert off == N
        assert np.array_equal(one.cpu().numpy().view(np.uint64), parts.cpu().numpy().view(np.uint64))


def test_accumulate_adds_one_float_add(ais, rows):
    import torch

    sc, _ = rows[5.0]
    tx = _tx(ais, 5.0, sc)
    g = torch.Generator(device="cuda").manual_seed(3)
    base = torch.randn(3, N + 1, dtype=torch.complex64, device="cuda", generator=g)
    for view in (base[:, :N], base[:, 1:]):  # rows that begin on and off a 16-byte boundary
        want = view + tx.render(T0, N)
        got = view.clone()
        tx.render(T0, N, out=got, accumulate=True)
        assert torch.equal(got, want)
        keep = view.clone()  # (in place on a strided view)
        tx.render(T0, N, out=view, accumulate=True)
        assert torch.equal(view, want)
        view.copy_(keep)


def test_bad_descriptors_keep_the_schedule(ais, rows):
    sc, _ = rows[5.0]
    tx = _tx(ais, 5.0, sc)
    before = tx.render(T0, N).cpu().numpy()
    p = [b"\x01" * 21]
    for kw in (dict(chan=3), dict(chan=-1), dict(frac=1.0), dict(frac=-0.1), dict(cfo=0.6), dict(cfo=float("nan")),
               dict(amp=float("inf")), dict(phase=float("nan"))):
        a = dict(chan=0, frac=0.0, cfo=0.0, amp=1.0, phase=0.0)
        a.update(kw)
        with pytest.raises(ValueError):
            tx.set_bursts(p, a["chan"], 0, frac=a["frac"], amp=a["amp"], cfo=a["cfo"], phase=a["phase"])
    with pytest.raises(ValueError):
        tx.set_bursts([b"\x01" * 1024], 0, 0)  # longer than length_max
    with pytest.raises(ValueError):
        tx.set_bursts(p * 17, 0, 0)  # more than max_bursts
    b = np.zeros(1, dtype=ais.BURST_DTYPE)
    b["len"], b["offset"], b["amp"] = 21, 1, 1.0
    with pytest.raises(ValueError):
        tx.set_bursts_raw(b, np.zeros(21, np.uint8))  # offset + len beyond the bytes
    assert np.array_equal(tx.render(T0, N).cpu().numpy().view(np.uint64), before.view(np.uint64))
    tx.set_bursts([], [], [])
    assert not tx.render(T0, N).cpu().numpy().any()


def test_two_handles_used_alternately(ais, rows):
    a, b = _tx(ais, 5.0, rows[5.0][0]), _tx(ais, 5.2083, rows[5.2083][0])
    ra, rb = a.render(T0, N).cpu().numpy(), b.render(T0, N).cpu().numpy()
    assert not np.array_equal(ra, rb)
    for _ in range(2):
        xa, xb = a.render(T0, N), b.render(T0, N)
        assert np.array_equal(xa.cpu().numpy().view(np.uint64), ra.view(np.uint64))
        assert np.array_equal(xb.cpu().numpy().view(np.uint64), rb.view(np.uint64))


def test_loop_back_through_the_chain(ais):
    """4 channels x 32768 at sps 5 on a torch.randn floor at 20 dB Eb/N0, through ais_demod.work_pipelined and
    hdlc_deframer_batch: what the host-rendered scene recovers under the same noise the device-rendered one recovers,
    but for 1 % (a decision at the threshold may flip on a last-place difference); the host scene recovers >= 90 %.
    The noise is drawn by torch's host generator, the same on every machine, and the seeds are chosen: the stock chain at
    sps 5 loses a few bursts at 20 dB whatever made them (the oracle chain: 42 of 45 of synth.make_channel's own bursts),
    which is a coin's toss against 90 % of some forty.  Through the oracle chain the host-rendered scene gives 42 of 42
    with this noise and 40 of 42 with seeds 10 and 11; scene 41 gave 30, 34 and 31 of 34."""
    import torch

    sps, nchan, T = 5, 4, 32768
    sc = tc.make_scene(46, nchan, T - 2 * 320 * sps, sps, ais.hdlc_framer)
    tx = ais.ais_tx_batch(float(sps), nchan, len(sc["payloads"]))
    tx.set_bursts(**sc)
    noise = (torch.randn(nchan, T, dtype=torch.complex64, generator=torch.Generator().manual_seed(9)) * float(np.sqrt(sps / 100.0))).cuda()
    x_dev = noise.clone()
    tx.render(0, T, out=x_dev, accumulate=True)
    x_host = noise + torch.as_tensor(ais.gmsk_scene(sc["payloads"], sc["chan"], sc["start"], sps, nchan, 0, T, frac=sc["frac"],
                                                    cfo=sc["cfo"], phase=sc["phase"])).cuda()
    opts = dict(samples_per_symbol=sps, bits_per_sec=9600.0, clockrec_gain=0.04, omega_relative_limit=0.01, fftlen=1024)

    def recovered(x):
        dem = ais.ais_demod(opts, nchan=nchan, max_items=T, stages="stock", preamble_symbols=tc.preamble_template(sps))
        hd = ais.hdlc_deframer_batch(11, 64, nchan, dem.clockrec.out_capacity, 4096)
        r = dem.work_pipelined(x)
        dem.wait(r["step"])
        hd.work(r["bits"], r["produced"])
        return {(c, p) for c, _, p in hd.pdus(as_list=True)}

    sent = {(int(c), p) for c, p in zip(sc["chan"], sc["payloads"])}
    host, dev = recovered(x_host) & sent, recovered(x_dev) & sent
    print("tx loop-back: %d scheduled, host-rendered recovers %d, device-rendered %d, %d of the host's missing"
          % (len(sent), len(host), len(dev), len(host - dev)))
    assert len(host) >= 0.9 * len(sent)
    assert len(host - dev) <= 0.01 * len(host)


def test_loop_back_through_ais_rx(ais):
    """2 streams at 250 kS/s (sps 26.0417), the two AIS channels at -/+ 25 kHz as the bursts' cfo, 20 dB, converted to
    cs16, 3 blocks through ais_rx: the NMEA text holds pdu_to_nmea of >= 90 % of the payloads, under the right designator.
    Seeds chosen as in test_loop_back_through_the_chain: the oracle's filter and chain on the host-rendered scene give 42 of
    43 with this noise (40 of 43 with seed 10; scene 43: 38 and 39 of 42)."""
    import torch

    import synth

    fs, decim, items = 250e3, 5, 16384
    sps, T = fs / 9600.0, 3 * items * decim
    sc = tc.make_scene(47, 4, T - 4 * int(320 * sps), sps, ais.hdlc_framer, fs=fs, chan_cfo=[-25e3, 25e3] * 2)
    lane = sc["chan"].copy()  # virtual channel = stream * 2 + centre, as ais_rx numbers its rows
    sc["chan"] = lane // 2
    tx = ais.ais_tx_batch(sps, 2, len(sc["payloads"]))
    tx.set_bursts(**sc)
    x = (torch.randn(2, T, dtype=torch.complex64, generator=torch.Generator().manual_seed(11)) * float(np.sqrt(sps / 100.0))).cuda()
    tx.render(0, T, out=x, accumulate=True)
    raw = torch.view_as_real(x).cpu().numpy()
    assert np.abs(raw).max() < 3.9
    raw = np.rint(raw * 2.0 ** 13).astype(np.int16)
    tmpl = synth.resampled_template(synth.gmsk_waveform(np.array([1 if b else -1 for b in synth.sync_bits("P")], float), 40)[: 28 * 40],
                                    40, fs / decim / 9600.0)
    rx = ais.ais_rx((-25e3, 25e3), fs, ("A", "B"), nstreams=2, fmt="cs16", scale=2.0 ** -13, block_items=items * decim,
                    preamble_symbols=tmpl)
    text = b""
    for k in range(3):
        rx.push(raw[:, k * items * decim:(k + 1) * items * decim])
        while (r := rx.pop()) is not None:
            text += r[2]
    rx.flush()
    while (r := rx.pop(wait=True)) is not None:
        text += r[2]
    lines = set(text.decode("latin-1").split("\n"))
    want = [ais.pdu_to_nmea("AB"[v % 2]).msg_to_sentence(p) for v, p in zip(lane, sc["payloads"])]
    wrong = [ais.pdu_to_nmea("BA"[v % 2]).msg_to_sentence(p) for v, p in zip(lane, sc["payloads"])]
    found = sum(w in lines for w in want)
    print("tx through ais_rx: %d of %d scheduled payloads in the NMEA text" % (found, len(want)))
    assert len(want) >= 40 and found >= 0.9 * len(want)
    assert not any(w in lines for w in wrong)
