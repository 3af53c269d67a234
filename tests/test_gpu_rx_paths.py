"""-m gpu: the host-fed receiver (ais_amd.ais_rx, aisx_rx_*) beyond its stock run: runs of one and two blocks, flush in
the middle of a run and twice in a row, pop buffers that are too small, the status word with a small
max_pdus_per_block, other geometries (one stream; one and three centres per stream; caller-supplied taps; 96 kS/s with
decimation 2; small blocks; blocks that are no multiple of the 1024-item transform), two receivers side by side,
a handle destroyed with blocks in flight, and the argument rules on a live handle.

The reference for text, records and block numbers is the hand-wired pipeline (test_gpu_rx.hand_wired: the filter, the
chain, the deframer and the NMEA stage called one after the other on numpy's conversion of the raw blocks), byte for
byte.  Every geometry that test_gpu_rx does not run is also held against the oracle once (oracle_lines: the float64
filter, the C demodulator, deframer and armouring on the same converted samples): every sentence the oracle recovers is
in the receiver's text, and every sentence in the receiver's text was transmitted."""
import ctypes as C

import numpy as np
import pytest

import nmea_cases as nc
import oracle_py as orc
import test_gpu_rx as gr
import test_gpu_xlate as tx

pytestmark = pytest.mark.gpu

OVERFLOW = -5  # AISX_ERR_OVERFLOW
INVALID = -1   # AISX_ERR_INVALID


@pytest.fixture(scope="module")
def ais():
    import torch

    assert torch.cuda.is_available(), "gpu tests need a visible MI355X"
    import ais_amd

    return ais_amd


@pytest.fixture(scope="module")
def fixture():
    return tx._stock_inputs()


_STOCK = {}


def stock(ais, fixture, fmt):
    """the stock fixture in `fmt`: its raw blocks, the conversion, and the hand-wired pipeline's (recs, text) per block"""
    if fmt not in _STOCK:
        raw, scale, bias, _ = gr.quantise(fixture[0], fmt)
        rb = gr.blocks_of(raw)
        want = gr.hand_wired(ais, [tx._dev(gr.convert(b, scale, bias)) for b in rb], tx.NS)
        assert sum(len(w[0]) for w in want) >= 60  # (the fixture gives 63 PDUs)
        _STOCK[fmt] = dict(rb=rb, scale=scale, bias=bias, want=want)
    return _STOCK[fmt]


def drain(rx, wait=True):
    out = []
    while (r := rx.pop(wait=wait)) is not None:
        out.append(r + (rx.status,))
    return out


def same(popped, want, first=0):
    """popped: [(block, recs, text, status)] in pop order = blocks first, first + 1, ... of the hand-wired run, status 0"""
    assert [p[0] for p in popped] == list(range(first, first + len(popped)))
    for (b, recs, text, status), (wrecs, wtext) in zip(popped, want[first:]):
        assert text == wtext, b
        assert recs.tobytes() == wrecs.tobytes(), b
        assert status == 0, (b, status)
        nc.split(recs, text)  # (the text is exactly the records' lines: text_len ends behind the last sentence)


def oracle_lines(taps, tmpl, fs, x_stream, f, des, nblocks, T):
    """the sentences of one channel from the oracle alone: float64 filter, C demodulator stepped by the same T,
    hdlc_deframer_bp(11, 64), pdu_to_nmea"""
    D = int(fs / 48000)
    yo = orc.freq_xlating_fir(taps, D, f, fs, x_stream, 0, T * nblocks)
    dm = orc.Demod(fs / D / 9600.0, tmpl, stages=3)
    bits = [dm.step(yo[k * T:(k + 1) * T])[0] for k in range(nblocks)]
    bits = np.concatenate([np.asarray(b, np.uint8) for b in bits if b is not None and len(b)])
    return [orc.pdu_to_nmea(des, p) for p in orc.Hdlc(11, 64).work(bits)]


def sent_lines(infos_lane, des):
    return [orc.pdu_to_nmea(des, np.packbits(np.array(i["payload"], np.uint8), bitorder="little").tobytes())
            for i in infos_lane]


def check_oracle(popped, x_conv, infos, fs, freqs, lanes, designators, taps, tmpl, T, need=1):
    """popped against the oracle per channel: oracle's sentences <= the receiver's <= the transmitted ones; lanes[c] is
    the key of channel c's bursts in infos[s] (None: nothing was transmitted there)"""
    import concurrent.futures as cf

    ns, nch, nblocks = x_conv.shape[0], len(freqs), len(popped)
    have = {}
    for (_, recs, text, _) in popped:
        for ch, _, t in nc.split(recs, text):
            have.setdefault(ch, []).append(t)
    jobs = [(s, c) for s in range(ns) for c in range(nch)]
    with cf.ThreadPoolExecutor(min(len(jobs), 16)) as ex:
        ora = list(ex.map(lambda j: oracle_lines(taps, tmpl, fs, x_conv[j[0]], freqs[j[1]], designators[j[1]], nblocks, T), jobs))
    nora = nhave = 0
    for (s, c), want in zip(jobs, ora):
        got = have.get(s * nch + c, [])
        sent = sent_lines(infos[s][lanes[c]], designators[c]) if lanes[c] is not None else []
        assert set(want) <= set(got), (s, c, len(want), len(got))
        assert set(got) <= set(sent), (s, c)
        nora, nhave = nora + len(want), nhave + len(got)
    print("  against the oracle: %d channels, sentences oracle %d, receiver %d" % (len(jobs), nora, nhave))
    assert nhave >= need and nora >= need
    return nhave


def run(rx, blocks, flush_after=(), early=False):
    """push the blocks (flush after the listed block numbers), pop as early as they come or all at the end"""
    popped = []
    for k, b in enumerate(blocks):
        assert rx.push(b) == k
        if k in flush_after:
            rx.flush()
        if early:
            popped += drain(rx, wait=False)
    rx.flush()
    return popped + drain(rx)


# ---- 1. short runs and flush -----------------------------------------------------------------------------------------


def test_short_runs_and_flush(ais, fixture):
    """the chain's results do not depend on look-ahead: a block issued by flush (no prepared look-ahead) followed by
    blocks issued with one gives the hand-wired run's blocks, wherever the flushes fall"""
    st = stock(ais, fixture, "cs16")
    rb, want = st["rb"], st["want"]
    rx = gr.make_rx(ais, "cs16", st["scale"], st["bias"])
    assert rx.pop() is None and rx.pop(wait=True) is None  # nothing pushed
    rx.flush()                                             # nothing pending
    assert rx.pop(wait=True) is None
    assert rx.push(rb[0]) == 0
    assert rx.pop(wait=True) is None                       # block 0 waits for its successor: not issued
    rx.flush()
    rx.flush()                                             # twice in a row: the second has nothing to issue
    one = drain(rx)
    assert len(one) == 1
    same(one, want)
    del rx
    rx = gr.make_rx(ais, "cs16", st["scale"], st["bias"])
    two = run(rx, rb[:2])
    assert len(two) == 2
    same(two, want)
    rx.flush()
    assert rx.pop(wait=True) is None
    del rx
    for flushes, early in (((1,), False), ((1,), True), ((0, 1, 2, 3, 4), False), ((0, 2), True)):
        rx = gr.make_rx(ais, "cs16", st["scale"], st["bias"])
        got = run(rx, rb, flush_after=flushes, early=early)
        assert len(got) == len(rb), (flushes, early)
        same(got, want)
        rx.flush()
        assert rx.pop(wait=True) is None
        del rx


# ---- 2. small pop buffers, through ctypes ----------------------------------------------------------------------------


def _cpop(rx, rec_cap, text_cap, wait=1):
    from ais_amd import _lib
    from ais_amd.batch_framing import PDU_DTYPE

    recs = np.zeros(rx._recs.size, PDU_DTYPE)        # (full-size behind the small capacities passed)
    text = np.full(rx._text.size, 0x7e, np.uint8)
    b, tl, nr, st = C.c_longlong(-9), C.c_long(-9), C.c_int(-9), C.c_int(-9)
    rc = _lib.lib().aisx_rx_pop(rx._h, wait, C.byref(b), text.ctypes.data if text_cap else None, text_cap, C.byref(tl),
                                recs.ctypes.data if rec_cap else None, rec_cap, C.byref(nr), C.byref(st))
    return rc, b.value, nr.value, tl.value, recs, text


def test_small_pop_buffers(ais, fixture):
    """AISX_ERR_OVERFLOW with *nrecs / *text_len = what is needed, and the block stays (include/aisx.h)"""
    st = stock(ais, fixture, "cu8")
    rb, want = st["rb"], st["want"]
    rx = gr.make_rx(ais, "cu8", st["scale"], st["bias"])
    for k, b in enumerate(rb):
        assert rx.push(b) == k
    rx.flush()
    k0 = next(k for k, w in enumerate(want) if len(w[0]) >= 2)
    popped = [rx.pop(wait=True) + (rx.status,) for _ in range(k0)]
    nrec, ntext = len(want[k0][0]), len(want[k0][1])
    for rec_cap, text_cap in ((0, 0), (nrec - 1, ntext), (nrec, ntext - 1), (nrec - 1, ntext - 1), (0, ntext), (nrec, 0)):
        rc, b, nr, tl, recs, text = _cpop(rx, rec_cap, text_cap)
        assert rc == OVERFLOW, (rec_cap, text_cap, rc)
        assert (nr, tl) == (nrec, ntext), (rec_cap, text_cap, nr, tl)
        assert b == -1                                               # no block was handed out
        assert not recs.tobytes().strip(b"\0") and (text == 0x7e).all()  # and nothing was written
    # exactly large enough: the same block, unchanged
    rc, b, nr, tl, recs, text = _cpop(rx, nrec, ntext)
    assert (rc, b, nr, tl) == (0, k0, nrec, ntext)
    assert recs[:nr].tobytes() == want[k0][0].tobytes() and text[:tl].tobytes() == want[k0][1]
    popped.append((b, recs[:nr].copy(), text[:tl].tobytes(), 0))
    popped += drain(rx)                                               # the remaining blocks, in order
    assert len(popped) == len(rb)
    same(popped, want)


# ---- 3. the status word and overflow ---------------------------------------------------------------------------------


def test_status_word_and_overflow(ais, fixture):
    """max_pdus_per_block below the PDUs of some blocks and not of others.  An overflowing block: the deframer keeps the
    first max_pdus of its list ordered by channel, then end_bit (the contract
    test_gpu_hdlc_batch.py::test_overflow_bad_counts_reset_and_interleaving pins), so AISX_RX_ST_HDLC_OVERFLOW is set,
    nrecs == max_pdus, and records and text are those of a hand-wired deframer and NMEA stage created with the same
    max_pdus -- which are the first max_pdus records of the unlimited run, their text ending behind the last kept
    sentence.  A block that fits: status 0, byte-identical to the unlimited run, also right after an overflowing one.

    AISX_RX_ST_NMEA_OVERFLOW cannot be reached: the receiver sizes the NMEA stage's text for the worst case of
    max_pdus records.  AISX_RX_ST_BAD_COUNT, and with it the two hipMemsetAsync calls that clear the stages' bad-input
    flags behind every block, cannot be reached through the public API with valid arguments either: the counts, channels
    and lengths the stages check come from the handle's own chain and deframer."""
    from ais_amd import _lib

    st = stock(ais, fixture, "cs8")
    rb = st["rb"] + st["rb"][:2]   # (7 blocks: the PDU counts cannot rise all the way, so one fitting block follows an overflowing one)
    xb = [tx._dev(gr.convert(b, st["scale"], st["bias"])) for b in rb]
    full = gr.hand_wired(ais, xb, tx.NS)
    n = [len(w[0]) for w in full]
    M = next((m for m in sorted(set(n)) if m >= 1 and any(n[k] > m >= n[k + 1] for k in range(len(n) - 1))), None)
    print("  PDUs per block %s, max_pdus_per_block %s" % (n, M))
    assert M is not None and M >= 1 and min(n) <= M < max(n)
    counts = []
    limited = gr.hand_wired(ais, xb, tx.NS, max_pdus=M, counts=counts)
    assert [c[0] for c in counts] == n and [c[1] for c in counts] == [min(v, M) for v in n]
    rx = ais.ais_rx((-25e3, 25e3), tx.FS_STOCK, ("A", "B"), nstreams=tx.NS, fmt="cs8", scale=st["scale"], bias=st["bias"],
                    block_items=tx.T * tx.DECIM, preamble_symbols=tx._template(ais), max_pdus_per_block=M)
    popped = run(rx, rb, early=True)
    assert [p[0] for p in popped] == list(range(len(rb)))
    after = 0
    for k, (b, recs, text, status) in enumerate(popped):
        lrecs, ltext = limited[k]
        assert recs.tobytes() == lrecs.tobytes() and text == ltext, k
        lines = nc.split(recs, text)
        if n[k] > M:
            assert status == _lib.AISX_RX_ST_HDLC_OVERFLOW, (k, status)
            assert len(recs) == M
            assert recs.tobytes() == full[k][0][:M].tobytes()          # the prefix of the ordered list
            assert lines == nc.split(*full[k])[:M] and full[k][1].startswith(text) and len(text) < len(full[k][1])
        else:
            assert status == 0, (k, status)
            assert recs.tobytes() == full[k][0].tobytes() and text == full[k][1], k
            after += k > 0 and n[k - 1] > M
    assert after >= 1


# ---- 4. geometries ---------------------------------------------------------------------------------------------------


def _sub(fixture, fmt, ns, nitems):
    xs, infos = fixture
    raw, scale, bias, _ = gr.quantise(xs[:ns, :nitems], fmt)
    return raw, scale, bias, gr.convert(raw, scale, bias), infos[:ns]


def _geometry(ais, fixture, fmt, ns, freqs, designators, lanes, block_items, nblocks, taps=None, need=1):
    raw, scale, bias, xc_, infos = _sub(fixture, fmt, ns, block_items * nblocks)
    rb = [np.ascontiguousarray(raw[:, k * block_items:(k + 1) * block_items]) for k in range(nblocks)]
    want = gr.hand_wired(ais, [tx._dev(gr.convert(b, scale, bias)) for b in rb], ns, freqs=freqs, designators=designators,
                         taps=taps)
    rx = ais.ais_rx(freqs, tx.FS_STOCK, designators, nstreams=ns, fmt=fmt, scale=scale, bias=bias, block_items=block_items,
                    preamble_symbols=tx._template(ais), taps=taps)
    assert (rx.items_per_block, rx.nchan) == (block_items // tx.DECIM, ns * len(freqs))
    popped = run(rx, rb, early=True)
    assert len(popped) == nblocks
    same(popped, want)
    t = ais.firdes_low_pass(1.0, tx.FS_STOCK, 11e3, 1e3) if taps is None else taps
    check_oracle(popped, xc_, infos, tx.FS_STOCK, freqs, lanes, designators, t, tx._template(ais), block_items // tx.DECIM, need)
    return popped


def test_one_stream(ais, fixture):
    _geometry(ais, fixture, "cu8", 1, (-25e3, 25e3), ("A", "B"), (9, 1), tx.T * tx.DECIM, 3)


def test_one_centre_per_stream(ais, fixture):
    _geometry(ais, fixture, "cs16", 4, (-25e3,), ("A",), (9,), tx.T * tx.DECIM, 3)


def test_three_centres_and_designators_of_every_length(ais, fixture):
    """designators cycle over a stream's centres (row r: designators[r % 3]): the empty string, 16 bytes, "AB"; the
    centre at 0 Hz carries nothing"""
    des = ("", "0123456789abcdef", "AB")
    popped = _geometry(ais, fixture, "cs8", 3, (-25e3, 25e3, 0.0), des, (9, 1, None), tx.T * tx.DECIM, 3, need=2)
    seen = set()
    for (_, recs, text, _) in popped:
        for ch, _, t in nc.split(recs, text):
            assert t.startswith("!AIVDM,1,1,,%s," % des[ch % 3]), (ch, t)
            seen.add(ch % 3)
    assert seen == {0, 1}


def test_small_blocks(ais, fixture):
    _geometry(ais, fixture, "cu8", tx.NS, (-25e3, 25e3), ("A", "B"), (9, 1), 4096 * tx.DECIM, 24)


def test_blocks_that_are_no_multiple_of_the_transform(ais, fixture):
    """block_items / decimation = 5000: include/aisx.h lets any multiple of the decimation through; the chain carries
    the items short of a whole 1024-item vector into the next block, with or without look-ahead"""
    _geometry(ais, fixture, "cs16", tx.NS, (-25e3, 25e3), ("A", "B"), (9, 1), 5000 * tx.DECIM, 20)


def test_caller_supplied_taps(ais, fixture):
    """taps equal to firdes_low_pass(1, fs, 11e3, 1e3) give the bytes of taps=None (the C low_pass of aisx_rx.hip is the
    Python one); a wider, shorter filter gives the hand-wired result for that filter"""
    own = ais.firdes_low_pass(1.0, tx.FS_STOCK, 11e3, 1e3)
    assert own.size == 603 and np.array_equal(own, orc.firdes_low_pass(1.0, tx.FS_STOCK, 11e3, 1e3))
    a = _geometry(ais, fixture, "cf32", 2, (-25e3, 25e3), ("A", "B"), (9, 1), tx.T * tx.DECIM, 3, taps=None)
    b = _geometry(ais, fixture, "cf32", 2, (-25e3, 25e3), ("A", "B"), (9, 1), tx.T * tx.DECIM, 3, taps=own)
    for (ba, ra, ta, _), (bb, rb_, tb, _) in zip(a, b):
        assert ba == bb and ra.tobytes() == rb_.tobytes() and ta == tb
    other = ais.firdes_low_pass(1.0, tx.FS_STOCK, 12e3, 3e3)
    assert other.size == 201
    c = _geometry(ais, fixture, "cf32", 2, (-25e3, 25e3), ("A", "B"), (9, 1), tx.T * tx.DECIM, 3, taps=other)
    assert [r.tobytes() for (_, r, _, _) in c] != [r.tobytes() for (_, r, _, _) in a]  # (another delay: other end bits)


def test_another_rate_and_decimation(ais):
    """96 kS/s: decimation 2, 5 samples per symbol, low_pass gives 231 taps (R = 8 where the stock shape plans R = 4),
    2 streams x 2 centres, 3 blocks of 16 384 x 2 items, cs16"""
    import synth
    import test_xlate_model as tm

    fs, D, T, nblocks, ns = 96e3, 2, 16384, 3, 2
    made = [synth.make_wideband(900 + s, T * nblocks, [25, 71], fs=fs, nlanes=96, decim=D, group_delay=115, amp=1.0,
                                bursts_per_lane=2, cfo_max=400.0, noise_sigma=0.1, tail_frames=3000) for s in range(ns)]
    xs, infos = np.stack([m[0] for m in made]), [m[1] for m in made]
    taps = ais.firdes_low_pass(1.0, fs, 11e3, 1e3)
    assert taps.size == 231 and np.array_equal(taps, orc.firdes_low_pass(1.0, fs, 11e3, 1e3))
    plan = tm.EmuXlate(D, taps, np.array([[-25e3, 25e3]] * ns), fs, T * D, nt=256).plan()
    assert plan["R"] == 8
    tmpl = np.asarray(ais.modulate_vector_bc(ais.gmsk_mod(5, 0.4), [1, 1, 0, 0] * 7, [1]), np.complex64)
    raw, scale, bias, _ = gr.quantise(xs, "cs16")
    xc_ = gr.convert(raw, scale, bias)
    rb = [np.ascontiguousarray(raw[:, k * T * D:(k + 1) * T * D]) for k in range(nblocks)]
    want = gr.hand_wired(ais, [tx._dev(gr.convert(b, scale, bias)) for b in rb], ns, fs=fs, template=tmpl)
    rx = ais.ais_rx((-25e3, 25e3), fs, ("A", "B"), nstreams=ns, fmt="cs16", scale=scale, bias=bias, block_items=T * D,
                    preamble_symbols=tmpl)
    assert (rx.decimation, rx.items_per_block, rx.nchan) == (D, T, 2 * ns)
    popped = run(rx, rb, early=True)
    assert len(popped) == nblocks
    same(popped, want)
    check_oracle(popped, xc_, infos, fs, (-25e3, 25e3), (71, 25), ("A", "B"), taps, tmpl, T, need=4)


# ---- 5. handles side by side, teardown -------------------------------------------------------------------------------


def test_two_receivers_side_by_side(ais, fixture):
    a, b = stock(ais, fixture, "cs16"), stock(ais, fixture, "cu8")
    ra = gr.make_rx(ais, "cs16", a["scale"], a["bias"])
    rb = gr.make_rx(ais, "cu8", b["scale"], b["bias"])
    pa, pb = [], []
    for k in range(tx.STEPS):
        assert ra.push(a["rb"][k]) == k
        assert rb.push(b["rb"][k]) == k
        pb += drain(rb, wait=False)
        pa += drain(ra, wait=False)
    rb.flush()
    pb += drain(rb)
    ra.flush()
    pa += drain(ra)
    assert len(pa) == len(pb) == tx.STEPS
    same(pa, a["want"])
    same(pb, b["want"])


def test_destroy_with_blocks_in_flight_then_a_fresh_handle(ais, fixture):
    """aisx_rx_destroy waits for what is in flight: result_slots blocks pushed, none popped, the handle deleted; a
    fresh handle then gives the whole run, and the same run once more gives the same bytes"""
    st = stock(ais, fixture, "cu8")
    rb = st["rb"] * 2
    rx = gr.make_rx(ais, "cu8", st["scale"], st["bias"])
    for k in range(rx.result_slots):
        assert rx.push(rb[k]) == k
    del rx
    runs = []
    for _ in range(2):
        rx = gr.make_rx(ais, "cu8", st["scale"], st["bias"])
        runs.append(run(rx, st["rb"]))
        assert len(runs[-1]) == tx.STEPS
        same(runs[-1], st["want"])
        del rx
    assert [(b, r.tobytes(), t, s) for (b, r, t, s) in runs[0]] == [(b, r.tobytes(), t, s) for (b, r, t, s) in runs[1]]


# ---- 6. argument rules on a live handle ------------------------------------------------------------------------------


def test_argument_rules_on_a_live_handle(ais, fixture):
    """submit without a slot, set_center_freq out of range, push with a short row stride: the error, and nothing
    queued or changed -- the run equals the one without those calls"""
    from ais_amd import _lib

    L = _lib.lib()
    st = stock(ais, fixture, "cs16")
    rb, want = st["rb"], st["want"]
    rx = gr.make_rx(ais, "cs16", st["scale"], st["bias"])
    b = C.c_longlong(-9)
    assert L.aisx_rx_submit(rx._h, C.byref(b)) == INVALID and b.value == -9      # before anything
    assert rx.pop(wait=True) is None
    assert rx.push(rb[0]) == 0
    assert L.aisx_rx_submit(rx._h, C.byref(b)) == INVALID and b.value == -9      # the slot went with block 0
    with pytest.raises(ValueError):
        rx.submit()
    short = np.ascontiguousarray(rb[1])
    assert L.aisx_rx_push(rx._h, short.ctypes.data, tx.T * tx.DECIM - 1, C.byref(b)) == INVALID and b.value == -9
    assert L.aisx_rx_push(rx._h, None, tx.T * tx.DECIM, C.byref(b)) == INVALID and b.value == -9
    assert rx.push(rb[1]) == 1
    for s, c, f in ((tx.NS, 0, -15e3), (-1, 0, -15e3), (0, 2, -15e3), (0, -1, -15e3), (0, 0, 125001.0), (0, 0, -130e3),
                    (0, 0, float("nan"))):
        assert L.aisx_rx_set_center_freq(rx._h, s, c, f) == INVALID, (s, c, f)
        with pytest.raises(ValueError):
            rx.set_center_freq(f, stream=s, chan=c)
    popped = drain(rx, wait=False)
    for k in range(2, tx.STEPS):
        assert rx.push(rb[k]) == k
        popped += drain(rx, wait=False)
    rx.flush()
    popped += drain(rx)
    assert len(popped) == tx.STEPS
    same(popped, want)
