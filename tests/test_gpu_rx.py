"""-m gpu: the host-fed receiver (ais_amd.ais_rx, aisx_rx_*) and the filter's sample formats
(aisx_xlate_process_fmt) on the device.  Inputs: test_gpu_xlate's stock fixture (8 streams at 250 kS/s, 5 blocks of
65 536 x 5 items), quantised on the host to cs16 / cs8 / cu8.  The formatted filter equals the fc32 filter on numpy's
conversion bit for bit; text, records and block numbers popped from ais_rx equal, byte for byte, what the hand-wired
pipeline of test_gpu_xlate._receiver returns for the converted tensors (the same kernels on the same values; the
chain's results do not depend on look-ahead or overlap); ring wrap, back-pressure and retunes likewise.

PDUs on this fixture (recovered by the receiver / transmitted), measured, not gated for the quantised formats: the
test prints them; DESIGN.md 4.6c quotes the run (63 recovered of 64 transmitted for cf32, cs16, cs8 and cu8 alike; cs16 at
scale 2^-13, the 8-bit formats at 2^-5 for a peak of 2.152, no component clipped)."""
import ctypes as C

import numpy as np
import pytest

import test_gpu_xlate as tx

pytestmark = pytest.mark.gpu

FORMATS = ("cf32", "cs16", "cs8", "cu8")
DT = dict(cs16=np.int16, cs8=np.int8, cu8=np.uint8)


@pytest.fixture(scope="module")
def ais():
    import torch

    assert torch.cuda.is_available(), "gpu tests need a visible MI355X"
    import ais_amd

    return ais_amd


@pytest.fixture(scope="module")
def fixture():
    xs, infos = tx._stock_inputs()
    return xs, infos


def quantise(xs, fmt):
    """-> raw [ns][N][2] (or xs itself for cf32), scale, bias, clipped samples.  cs16: scale 2^-13; 8-bit: the power of
    two that holds the fixture's peak |re|, |im|; cu8 with the RTL-SDR's bias 127.5"""
    if fmt == "cf32":
        return xs, 1.0, 0.0, 0
    v = np.ascontiguousarray(xs).view(np.float32).reshape(xs.shape[0], xs.shape[1], 2)
    peak = float(np.max(np.abs(v)))
    info = np.iinfo(DT[fmt])
    if fmt == "cs16":
        scale = 2.0 ** -13
    else:
        scale = 2.0 ** int(np.ceil(np.log2(peak / 127.0)))
    bias = 127.5 if fmt == "cu8" else 0.0
    q = np.floor(v / np.float32(scale) + np.float32(128.0)) if fmt == "cu8" else np.rint(v / np.float32(scale))
    clipped = int(np.count_nonzero((q < info.min) | (q > info.max)))
    raw = np.clip(q, info.min, info.max).astype(DT[fmt])
    print("  %s: peak %.3f, scale 2^%d, bias %.1f, %d of %d components clipped" % (fmt, peak, int(np.log2(scale)), bias, clipped, q.size))
    return raw, scale, bias, clipped


def convert(raw, scale, bias):
    """the specification of the device's conversion (include/aisx.h)"""
    if raw.dtype == np.complex64:
        return raw
    v = (raw.astype(np.float32) - np.float32(bias)) * np.float32(scale)
    return np.ascontiguousarray(v).view(np.complex64)[..., 0]


def blocks_of(a, nblocks=tx.STEPS):
    n = tx.T * tx.DECIM
    return [np.ascontiguousarray(a[:, k * n:(k + 1) * n]) for k in range(nblocks)]


def make_rx(ais, fmt, scale, bias, nstreams=tx.NS):
    return ais.ais_rx((-25e3, 25e3), tx.FS_STOCK, ("A", "B"), nstreams=nstreams, fmt=fmt, scale=scale, bias=bias,
                      block_items=tx.T * tx.DECIM, preamble_symbols=tx._template(ais))


def same(popped, got):
    """popped: [(block, recs, text)] in pop order; got: the hand-wired pipeline's per-step tuples"""
    assert [p[0] for p in popped] == list(range(len(got)))
    for (b, recs, text), g in zip(popped, got):
        assert text == g[3], b
        assert recs.tobytes() == g[2].tobytes(), b


def hand_wired(ais, x_blocks, nstreams, retunes=(), fs=tx.FS_STOCK, freqs=(-25e3, 25e3), designators=("A", "B"), taps=None,
               template=None, max_pdus=1 << 16, counts=None):
    """test_gpu_xlate._receiver's wiring, every step on its own, for any number of blocks; retunes: (block, stream,
    chan, f) applied before that block is filtered.  Returns per block (recs, text).  The defaults are the stock
    receiver's; fs sets the decimation int(fs / 48000) and the samples per symbol as ais_rx does, freqs / designators
    are per centre of every stream, taps default to low_pass(1, fs, 11e3, 1e3), template to the stock one, the block
    length is x_blocks' own.  max_pdus below a block's PDUs: the kept prefix comes back (overflow_ok); counts, a list,
    receives per block (PDUs found, records kept)."""
    import torch

    decim = int(fs / 48000)
    sps = fs / decim / 9600.0
    if taps is None:
        taps = ais.firdes_low_pass(1.0, fs, 11e3, 1e3)
    if template is None:
        template = tx._template(ais)
    nch = len(freqs) * nstreams
    n = x_blocks[0].shape[1]
    xl = ais.freq_xlating_fir_filter_ccf(decim, taps, freqs, fs, nstreams=nstreams, max_items=n)
    opts = dict(samples_per_symbol=sps, bits_per_sec=9600.0, clockrec_gain=0.04, omega_relative_limit=0.01, fftlen=1024)
    dem = ais.ais_demod(opts, nchan=nch, max_items=n // decim, stages="stock", preamble_symbols=template)
    hd = ais.hdlc_deframer_batch(11, 64, nch, dem.clockrec.out_capacity, max_pdus)
    nm = ais.pdu_to_nmea_batch(list(designators) * nstreams, nch, max_pdus, 64)
    out = []
    for k, x in enumerate(x_blocks):
        for (kb, s, c, f) in retunes:
            if kb == k:
                xl.set_center_freq(f, stream=s, chan=c)
        y = xl.work(x)
        r = dem.work_pipelined(y)
        dem.wait(r["step"])
        hd.work(r["bits"], r["produced"])
        nm.work(hd)
        out.append(nm.sentences(overflow_ok=counts is not None))
        if counts is not None:
            counts.append((nm.found, len(out[-1][0])))
        dem.synchronize()
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("fmt", FORMATS[1:])
def test_formatted_filter_equals_filter_on_converted_values(ais, fixture, fmt):
    import torch

    xs, _ = fixture
    N = 2 * tx.T * tx.DECIM + 3
    raw, scale, bias, _ = quantise(xs[:, :N], fmt)
    x = tx._dev(convert(raw, scale, bias))
    rawd = torch.as_tensor(raw).cuda()
    taps = ais.firdes_low_pass(1.0, tx.FS_STOCK, 11e3, 1e3)
    for sizes in ([N], [1, 4, 5, 6, 13, 65536 * 5, N - 65536 * 5 - 29]):
        f = ais.freq_xlating_fir_filter_ccf(tx.DECIM, taps, (-25e3, 25e3), tx.FS_STOCK, nstreams=tx.NS, max_items=N)
        g = ais.freq_xlating_fir_filter_ccf(tx.DECIM, taps, (-25e3, 25e3), tx.FS_STOCK, nstreams=tx.NS, max_items=N)
        o = 0
        for n in sizes:
            ya = f.work(rawd[:, o:o + n], fmt=fmt, scale=scale, bias=bias)
            yb = g.work(x[:, o:o + n])
            assert ya.shape == yb.shape and torch.equal(ya.view(torch.float32), yb.view(torch.float32)), (fmt, o, n)
            o += n
        assert o == N


@pytest.mark.parametrize("fmt", FORMATS)
def test_receiver_equals_hand_wired_pipeline(ais, fixture, fmt):
    """pops taken late (after all blocks and a flush) and as early as they come: block numbers, records and text byte
    for byte those of test_gpu_xlate._receiver on the converted tensors"""
    xs, infos = fixture
    raw, scale, bias, clipped = quantise(xs, fmt)
    xc = convert(raw, scale, bias)
    x_steps = [tx._dev(b) for b in blocks_of(xc)]
    thr, got = tx._receiver(ais, x_steps, tx.NS, overlap=True)
    rb = blocks_of(raw)
    # late
    rx = make_rx(ais, fmt, scale, bias)
    assert [rx.push(b) for b in rb] == list(range(tx.STEPS))
    rx.flush()
    late = []
    while (r := rx.pop(wait=True)) is not None:
        late.append(r)
        assert rx.status == 0
    same(late, got)
    assert rx.pop() is None
    del rx
    # early, through the pinned slot
    rx = make_rx(ais, fmt, scale, bias)
    early = []
    for k, b in enumerate(rb):
        rx.slot()[...] = b
        assert rx.submit() == k
        while (r := rx.pop()) is not None:
            early.append(r)
    rx.flush()
    while (r := rx.pop(wait=True)) is not None:
        early.append(r)
    same(early, got)
    nhave = sum(len(p[1]) for p in late)
    nsent = sum(len(infos[s][lane]) for s in range(tx.NS) for lane in (9, 1))
    print("ais_rx %s (%d components clipped): PDUs recovered %d, transmitted %d" % (fmt, clipped, nhave, nsent))
    if fmt == "cf32":
        tx._check_against_oracle(ais, thr, got, xs, infos, tx.NS)


def test_ring_wrap_and_back_pressure(ais, fixture):
    """10 blocks (every ring wraps: 3 input slots, 2 raw buffers, 4 row buffers, 3 output sets, 8 result slots), nothing
    popped until the result ring is full: one more submit returns AISX_ERR_OVERFLOW with nothing queued, and after one
    pop the same slot submits; the run's text equals the hand-wired pipeline's"""
    xs, _ = fixture
    raw, scale, bias, _ = quantise(xs, "cu8")
    rb = blocks_of(raw) * 2
    want = hand_wired(ais, [tx._dev(convert(b, scale, bias)) for b in rb], tx.NS)
    rx = make_rx(ais, "cu8", scale, bias)
    assert rx.result_slots == 8 and len(rb) > rx.result_slots + 1
    for k in range(rx.result_slots + 1):     # blocks 0 .. 8: steps 0 .. 7 issued, the result ring is full
        assert rx.push(rb[k]) == k
    k = rx.result_slots + 1
    rx.slot()[...] = rb[k]
    with pytest.raises(OverflowError):
        rx.submit()
    with pytest.raises(OverflowError):
        rx.flush()
    popped = [rx.pop(wait=True)]
    assert popped[0][0] == 0
    assert rx.submit() == k                   # the same slot, still acquired
    while (r := rx.pop(wait=True)) is not None:
        popped.append(r)
    rx.flush()
    popped.append(rx.pop(wait=True))
    assert rx.pop(wait=True) is None
    assert [p[0] for p in popped] == list(range(len(rb)))
    for (b, recs, text), (wrecs, wtext) in zip(popped, want):
        assert text == wtext and recs.tobytes() == wrecs.tobytes(), b
    assert sum(len(p[1]) for p in popped) > 0


def test_retune_between_blocks(ais, fixture):
    """channel A of every stream moved off its signal before block 2 and back before block 3: as the hand-wired pipeline
    with set_center_freq at the same places"""
    xs, _ = fixture
    raw, scale, bias, _ = quantise(xs, "cs16")
    rb = blocks_of(raw)
    ret = [(2, s, 0, -15e3) for s in range(tx.NS)] + [(3, s, 0, -25e3) for s in range(tx.NS)]
    want = hand_wired(ais, [tx._dev(convert(b, scale, bias)) for b in rb], tx.NS, retunes=ret)
    plain = hand_wired(ais, [tx._dev(convert(b, scale, bias)) for b in rb], tx.NS)
    assert [w[1] for w in want] != [p[1] for p in plain]   # (the retune is visible in the text)
    rx = make_rx(ais, "cs16", scale, bias)
    popped = []
    for k, b in enumerate(rb):
        for (kb, s, c, f) in ret:
            if kb == k:
                rx.set_center_freq(f, stream=s, chan=c)
        rx.push(b)
        while (r := rx.pop()) is not None:
            popped.append(r)
    rx.flush()
    while (r := rx.pop(wait=True)) is not None:
        popped.append(r)
    assert [p[0] for p in popped] == list(range(len(rb)))
    for (b, recs, text), (wrecs, wtext) in zip(popped, want):
        assert text == wtext and recs.tobytes() == wrecs.tobytes(), b
    with pytest.raises(ValueError):
        rx.set_center_freq(130e3, stream=0, chan=0)
