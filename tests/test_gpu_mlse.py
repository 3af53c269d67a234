"""-m gpu: the batched sequence detector (ais_amd.mlse_detector_batch, aisx_mlse_batch_*) against its host form
(ais_amd.mlse_detector), byte for byte per channel: ragged counts at every size where a window, a block or a wave's
tile begins or ends, over consecutive calls, flush and reset; two handles interleaved on one stream; bad counts; and
the receiver with detector="mlse" against the hand-wired chain -> detector -> deframer -> NMEA stage and against the
host forms on the same symbols, with the plain receiver unchanged beside it."""
import numpy as np
import pytest

import mlse_cases as mc
import nmea_cases as nc
import test_gpu_rx as gr
import test_gpu_xlate as tx

pytestmark = pytest.mark.gpu

NCHAN, MAX_SYMS, STRIDE = 6, 5000, 5008
# every count of mlse_cases.COUNTS, 5000 in several channels and calls (a wave's tile is 4096 symbols)
PLAN = [[5000, 0, 79, 80, 145, 1], [1, 5000, 15, 64, 16, 5000], [143, 17, 5000, 63, 0, 81], [64, 81, 144, 5000, 5000, 80]]


@pytest.fixture(scope="module")
def ais():
    import torch

    assert torch.cuda.is_available(), "gpu tests need a visible MI355X"
    import ais_amd

    return ais_amd


@pytest.fixture(scope="module")
def streams():
    """[NCHAN][20480] symbols: the oracle chain's symbols of one short noisy synthetic channel (repeated), clean symbols
    of random levels, complex noise of three scales, and a row with not-a-number and infinite items among noise"""
    rng = np.random.default_rng(21)
    n = 20480
    _, syms, _ = mc.noisy_channel(5000, 32768, 16, mc.stock_template())
    assert syms.size > 4000
    s = np.zeros((NCHAN, n), np.complex64)
    s[0] = np.resize(syms, n)
    s[1] = mc.clean_symbols(rng.integers(0, 2, n + 2))
    for c, scale in ((2, 1.0), (3, 1e-3), (4, 50.0), (5, 1.0)):
        s[c] = scale * (rng.normal(size=n) + 1j * rng.normal(size=n))
    s[5, rng.integers(0, n, 40)] = np.array([np.nan, np.inf, -np.inf, 0.0], np.float32)[rng.integers(0, 4, 40)]
    return s


def _dev(x):
    import torch

    return torch.as_tensor(np.ascontiguousarray(x)).cuda()


class Feeder:
    """hands a device handle and one host detector per channel the same symbols, call by call, and compares"""

    def __init__(self, ais, streams, nchan=NCHAN, max_syms=MAX_SYMS):
        self.ais, self.s, self.nchan = ais, streams, nchan
        self.det = ais.mlse_detector_batch(nchan, max_syms)
        self.host = [ais.mlse_detector() for _ in range(nchan)]
        self.pos = [0] * nchan
        self.total = self.fed = 0

    def stage(self, counts):
        """-> (device symbols [nchan][STRIDE] with junk behind each row's count, device counts, the host's slices)"""
        buf = np.full((self.nchan, STRIDE), np.complex64(7e5 - 3e5j))
        parts = []
        for c, n in enumerate(counts):
            k = n if 0 <= n <= self.det.max_syms else 0
            parts.append(self.s[c, self.pos[c]:self.pos[c] + k])
            buf[c, :k] = parts[-1]
            self.pos[c] += k
            self.fed += k
        return _dev(buf), _dev(np.asarray(counts, np.int32)), parts

    def check(self, out, want, what):
        bits, nb = out[0].cpu().numpy(), out[1].cpu().numpy()
        for c in range(self.nchan):
            assert nb[c] == want[c].size and bits[c, :nb[c]].tobytes() == want[c].tobytes(), (what, c, int(nb[c]), want[c].size)
            self.total += int(nb[c])

    def call(self, counts, stream=None):
        x, n, parts = self.stage(counts)
        self.check(self.det.process(x, n, stream=stream), [h.work(p) for h, p in zip(self.host, parts)], counts)

    def flush(self):
        self.check(self.det.flush(), [h.flush() for h in self.host], "flush")


def test_device_equals_the_host_form(ais, streams):
    f = Feeder(ais, streams)
    assert sorted(set(v for row in PLAN for v in row)) == sorted(mc.COUNTS)
    for counts in PLAN:
        f.call(counts)
    f.flush()
    f.flush()  # nothing is left: no bits
    f.call(PLAN[0])  # as new behind a flush
    f.det.reset()
    for h in f.host:
        h.reset()
    for counts in PLAN[1:3]:
        f.call(counts)
    f.flush()
    # every symbol fed came out as one bit, but those the reset dropped: fewer than 144 a channel
    assert f.det.status() == 0 and f.fed - 144 * NCHAN < f.total <= f.fed and f.fed > 50000


def test_two_handles_interleaved_on_one_stream(ais, streams):
    import torch

    a, b = Feeder(ais, streams), Feeder(ais, streams[::-1].copy())
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        for ca, cb in zip(PLAN, PLAN[::-1]):
            xa, na, pa = a.stage(ca)
            xb, nb, pb = b.stage(cb)
            oa = a.det.process(xa, na, stream=st)  # both queued before either is read
            ob = b.det.process(xb, nb, stream=st)
            a.check(oa, [h.work(p) for h, p in zip(a.host, pa)], ca)
            b.check(ob, [h.work(p) for h, p in zip(b.host, pb)], cb)
        oa, ob = a.det.flush(stream=st), b.det.flush(stream=st)
        a.check(oa, [h.flush() for h in a.host], "flush")
        b.check(ob, [h.flush() for h in b.host], "flush")
    st.synchronize()


def test_bad_counts_and_arguments(ais, streams):
    from ais_amd import _lib

    f = Feeder(ais, streams, nchan=3, max_syms=200)
    f.call([200, 150, 200])
    assert f.det.status() == 0
    f.call([-1, 200, 201])  # (the Feeder gives the host forms of channels 0 and 2 no symbols)
    assert f.det.status() == _lib.AISX_MLSE_ST_BAD_COUNT and f.det.status() == 0
    f.call([200, 200, 200])
    f.flush()
    assert f.det.status() == 0
    with pytest.raises(ValueError):
        ais.mlse_detector_batch(0, 100)
    with pytest.raises(ValueError):
        ais.mlse_detector_batch(2, 100, bt=2.0)
    x, n, _ = f.stage([0, 0, 0])
    with pytest.raises(ValueError):
        f.det.process(_dev(np.zeros((3, 150), np.complex64)), n)  # a row stride below max_syms
    with pytest.raises(ValueError):
        f.det.process(x, n[:2])


# ---- through the receiver ---------------------------------------------------------------------------------------------

NBLOCKS = 3


@pytest.fixture(scope="module")
def one_stream():
    import synth

    x, infos = synth.make_wideband(700, tx.T * NBLOCKS, [1, 9], fs=tx.FS_STOCK, nlanes=10, decim=tx.DECIM, group_delay=301, amp=1.0,
                                   bursts_per_lane=4, cfo_max=400.0, noise_sigma=0.1, tail_frames=3000)
    raw, scale, bias, _ = gr.quantise(x[None, :], "cu8")
    n = tx.T * tx.DECIM
    return dict(rb=[np.ascontiguousarray(raw[:, k * n:(k + 1) * n]) for k in range(NBLOCKS)], scale=scale, bias=bias)


def hand_wired_mlse(ais, x_blocks):
    """filter -> chain (symbols) -> detector -> deframer -> NMEA stage, every step on its own: per block (recs, text),
    the deframer's PDUs as (chan, end_bit, payload), and the step's symbols per channel"""
    import torch

    fs, decim = tx.FS_STOCK, tx.DECIM
    n = x_blocks[0].shape[1]
    xl = ais.freq_xlating_fir_filter_ccf(decim, ais.firdes_low_pass(1.0, fs, 11e3, 1e3), (-25e3, 25e3), fs, nstreams=1, max_items=n)
    opts = dict(samples_per_symbol=fs / decim / 9600.0, bits_per_sec=9600.0, clockrec_gain=0.04, omega_relative_limit=0.01, fftlen=1024)
    dem = ais.ais_demod(opts, nchan=2, max_items=n // decim, stages="stock", preamble_symbols=tx._template(ais))
    cap = dem.clockrec.out_capacity
    det = ais.mlse_detector_batch(2, cap)
    hd = ais.hdlc_deframer_batch(11, 64, 2, cap + 79, 1 << 16)
    nm = ais.pdu_to_nmea_batch(["A", "B"], 2, 1 << 16, 64)
    out = []
    for x in x_blocks:
        r = dem.work_pipelined(xl.work(x), want_syms=True)
        dem.wait(r["step"])
        bits, nbits = det.process(r["syms"], r["produced"])
        hd.work(bits, nbits)
        nm.work(hd)
        recs, text = nm.sentences()
        prod = r["produced"].cpu().numpy()
        syms = r["syms"].cpu().numpy()
        out.append((recs, text, hd.pdus(as_list=True), [syms[c, :prod[c]].copy() for c in range(2)]))
        dem.synchronize()
    torch.cuda.synchronize()
    assert det.status() == 0
    return out


def _run(rx, blocks):
    got = []
    for k, b in enumerate(blocks):
        assert rx.push(b) == k
    rx.flush()
    while (r := rx.pop(wait=True)) is not None:
        got.append(r + (rx.status,))
    return got


def test_receiver_with_the_detector(ais, one_stream):
    st = one_stream
    xb = [tx._dev(gr.convert(b, st["scale"], st["bias"])) for b in st["rb"]]
    want = hand_wired_mlse(ais, xb)
    kw = dict(nstreams=1, fmt="cu8", scale=st["scale"], bias=st["bias"], block_items=tx.T * tx.DECIM, preamble_symbols=tx._template(ais))
    rx = ais.ais_rx((-25e3, 25e3), tx.FS_STOCK, ("A", "B"), detector="mlse", **kw)
    assert rx.detector == "mlse"
    got = _run(rx, st["rb"])
    assert [g[0] for g in got] == list(range(NBLOCKS)) and sum(len(g[1]) for g in got) >= 1
    for (b, recs, text, status), (wrecs, wtext, _, _) in zip(got, want):
        assert status == 0 and text == wtext and recs.tobytes() == wrecs.tobytes(), b
        nc.split(recs, text)
    with pytest.raises(ValueError):
        rx.enable_detector("mlse")  # only before the first block
    with pytest.raises(ValueError):
        ais.ais_rx((-25e3, 25e3), tx.FS_STOCK, ("A", "B"), detector="viterbi", **kw)
    # every PDU is one the host detector and the host deframer find on the same symbols, at the same end bit
    for c in range(2):
        det, hd, seen, host = ais.mlse_detector(), ais.hdlc_deframer_bp(11, 64), 0, []
        dev = [(e, p) for w in want for (ch, e, p) in w[2] if ch == c]
        for w in want:
            bits = det.work(w[3][c])
            host += hd.work(bits)
            seen += bits.size
        assert [p for _, p in dev] == host and all(e < seen for e, _ in dev), c
    # the plain receiver beside it: the plain hand-wired path's bytes, as before
    plain = gr.hand_wired(ais, xb, 1)
    rx2 = ais.ais_rx((-25e3, 25e3), tx.FS_STOCK, ("A", "B"), **kw)
    assert rx2.detector is None
    got2 = _run(rx2, st["rb"])
    for (b, recs, text, status), (wrecs, wtext) in zip(got2, plain):
        assert status == 0 and text == wtext and recs.tobytes() == wrecs.tobytes(), b
    print("  sentences: detector %d, plain %d" % (sum(len(g[1]) for g in got), sum(len(g[1]) for g in got2)))


def test_receiver_with_the_detector_and_repair(ais, one_stream):
    """the deframer made again for the detector keeps the rules, whichever was enabled first"""
    st = one_stream
    kw = dict(nstreams=1, fmt="cu8", scale=st["scale"], bias=st["bias"], block_items=tx.T * tx.DECIM, preamble_symbols=tx._template(ais))
    texts = []
    for order in (0, 1):
        rx = ais.ais_rx((-25e3, 25e3), tx.FS_STOCK, ("A", "B"), **kw)
        for step in ((rx.enable_detector, lambda: rx.enable_repair(ais.AIS_REPAIR_RULES))[::1 if order == 0 else -1]):
            step()
        got = _run(rx, st["rb"])
        assert all(g[3] == 0 for g in got) and len(rx.popped_repairs()) == len(got[-1][1])
        texts.append([g[2] for g in got])
    assert texts[0] == texts[1] and sum(len(t) for t in texts[0]) > 0
