"""-m gpu: repair of one error event by CRC syndrome in the batched HDLC deframer on the MI355X
(aisx_hdlc_batch_set_repair_events, ais_amd.hdlc_deframer_batch(repair=, events=)) against the host form that is its
specification (one ais_amd.hdlc_deframer_bp(repair=, events=) per channel fed the same bits call by call): the same PDUs,
order, bytes and marks; the marks through an overflow, the repaired PDUs through the NMEA stage, and the receiver handle
(ais_amd.ais_rx(repair=, repair_events=)) on a burst sent with two adjacent payload bits inverted, with the slicer and
with the sequence detector."""
import numpy as np
import pytest

import hdlc_cases as hc
import hdlc_events_cases as ec
import hdlc_repair_cases as rc

pytestmark = pytest.mark.gpu

R21 = {21: (1, 2, 3, 4, 9, 11, 18, 24)}


@pytest.fixture(scope="module")
def ais():
    import torch

    assert torch.cuda.is_available(), "gpu tests need a visible MI355X"
    import ais_amd

    return ais_amd


def _dev_call(call, stride, pad=0):
    import torch

    rows, n = hc.pack(call, stride)
    buf = torch.zeros(rows.size + pad + 64, dtype=torch.uint8, device="cuda")
    b = buf[pad:pad + rows.size].view(rows.shape[0], stride)
    b.copy_(torch.from_numpy(rows))
    return b, torch.from_numpy(n).cuda()


def _run(ais, lmin, lmax, calls, rules, events, pad=0, max_pdus=1 << 14, switches=None):
    """switches: {call index: (rules, events)} set before that call"""
    nch = len(calls[0])
    stride = max(max(len(x) for x in call) for call in calls) + 5
    hd = ais.hdlc_deframer_batch(lmin, lmax, nch, stride, max_pdus, repair=rules, events=events)
    hs = [ais.hdlc_deframer_bp(lmin, lmax, repair=rules, events=events) for _ in range(nch)]
    got, ref = [[] for _ in range(nch)], [[] for _ in range(nch)]
    for k, call in enumerate(calls):
        if switches and k in switches:
            hd.set_repair(*switches[k])
            for h in hs:
                h.set_repair(*switches[k])
        b, n = _dev_call(call, stride, pad)
        hd.work(b, n)
        recs, data, fix = hd.pdus(with_repairs=True)
        for c, lst in enumerate(rc.by_channel(recs, data, fix, nch)):
            got[c] += lst
            p, f = hs[c].work(call[c], with_repairs=True)
            ref[c] += list(zip(p, f))
    return got, ref


def _check(ais, lmin, lmax, calls, rules, events, pad=0, **kw):
    got, ref = _run(ais, lmin, lmax, calls, rules, events, pad, **kw)
    for c in range(len(got)):
        assert [(p, f) for _, p, f in got[c]] == ref[c], c
    return got


def _dev_marks(ptr, n):
    """n int32 at a device address, on the host"""
    import torch

    class Mem:
        __cuda_array_interface__ = dict(shape=(n,), typestr="<i4", data=(ptr, False), version=3)

    torch.cuda.synchronize()
    return torch.as_tensor(Mem(), device="cuda").cpu().numpy()


def _kinds(got):
    return [sum(f >= 0 and f >> 16 == e for g in got for _, _, f in g) for e in range(3)]


@pytest.mark.parametrize("nch", [1, 37])
def test_model_cases_on_the_device(ais, nch):
    rng = np.random.default_rng(400 + nch)
    # planted events of all three kinds and intact frames in noise, 5 000 - 9 000 bits per channel (more than one
    # 4096-bit pass) in 3 calls, rows off 16-byte alignment
    streams = [ec.event_stream(rng, int(rng.integers(5000, 9000)), rc.AIS_RULES, every=500) for _ in range(nch)]
    cuts = [sorted(rng.integers(0, len(s), 2)) for s in streams]
    calls = [[hc.as_bytes(rng, b, wild=(c % 2 == 1)) for c, b in enumerate(call)] for call in hc.split_calls(streams, cuts)]
    got = _check(ais, 11, 64, calls, rc.AIS_RULES, ec.ALL, pad=5)
    tot, kinds = sum(len(g) for g in got), _kinds(got)
    assert sum(kinds) >= 3 * nch ** 0.5 and tot > sum(kinds) and (nch == 1 or min(kinds) >= 3)
    assert got[0] == ec.py_ref(11, 64, streams[0], rc.AIS_RULES, ec.ALL)  # (end bits too, on one channel)
    _check(ais, 11, 64, calls, rc.AIS_RULES, ec.PAIR | ec.SKIP, pad=11)  # a mask without SINGLE
    # flips on the stuffed stream, length-only rules: equality with the host form is the only claim
    streams = [ec.event_stream(rng, 6000, rc.AIS_RULES, every=200, raw_flips=50) for _ in range(nch)]
    cuts = [sorted(rng.integers(0, 6000, 2)) for _ in range(nch)]
    got = _check(ais, 11, 64, hc.split_calls(streams, cuts), {k: None for k in rc.AIS_RULES}, ec.ALL)
    kinds = [a + b for a, b in zip(kinds, _kinds(got))]
    # a repaired frame across the pass boundary at bit 4096 and across both call boundaries (another offset per channel;
    # its pair sits in octets 7 and 8, its skip across the payload / FCS boundary), then two frames sharing a
    # delimiter, both repaired
    a, b = rc.typed_payload(rng, 21, 3), rc.typed_payload(rng, 21, 4)
    fa, fs = ec.event_frame(a, 63, 1), ec.event_frame(a, 166, 2)
    s = hc.junk(rng, 4096 - 100) + fa + hc.noise(rng, 700) + fs + hc.noise(rng, 500) + ec.event_frame(b, 0, 2)[:-8] + \
        ec.event_frame(a, 182, 1) + hc.noise(rng, 300)
    x0, x1 = 4096 - 100 + len(fa) + 700, 4096 - 100 + len(fa) + len(fs) + 1200
    cuts = [[x0 + (7 * c) % len(fs), x1 + (11 * c) % (2 * len(fa))] for c in range(nch)]
    got = _check(ais, 11, 64, hc.split_calls([s] * nch, cuts), R21, ec.ALL, pad=(3 if nch > 1 else 0))
    for g in got:
        assert [(p, f) for _, p, f in g if p in (a, b)] == [(a, ec.mark(63, 1)), (a, ec.mark(166, 2)), (b, ec.mark(0, 2)),
                                                            (a, ec.mark(182, 1))]
    print("%d channels: %d PDUs, repaired by kind %s, identical to the host form" % (nch, tot, kinds))


def test_mask_switched_between_calls(ais):
    """one stream in five calls per channel, a damaged frame of each kind closing in every call: off, all events, the
    single event (the single-bit kernel and its marks), pair and skip, off again"""
    rng = np.random.default_rng(51)
    nch = 5
    p = [rc.typed_payload(rng, 21, 1 + k) for k in range(3)]
    seg = lambda: hc.noise(rng, 200) + ec.event_frame(p[0], 40, 0) + hc.noise(rng, 90) + ec.event_frame(p[1], 100, 1) + \
        hc.noise(rng, 60) + ec.event_frame(p[2], 150, 2) + hc.noise(rng, 120)  # noqa: E731
    segs = [seg() for _ in range(5)]
    s = sum(segs, [])
    edges = np.cumsum([len(x) for x in segs])[:-1]
    cuts = [[int(e) - 30 * c for e in edges] for c in range(nch)]  # (a cut inside the noise that ends a segment)
    calls = hc.split_calls([s] * nch, cuts)
    sw = {1: (R21, ec.ALL), 2: (R21, ec.SINGLE), 3: (R21, ec.PAIR | ec.SKIP), 4: (None, ec.ALL)}
    got = _check(ais, 11, 64, calls, None, ec.SINGLE, switches=sw)
    m = [ec.mark(40, 0), ec.mark(100, 1), ec.mark(150, 2)]
    assert m[0] == 40
    for g in got:
        assert [(q, f) for _, q, f in g] == [(p[0], m[0]), (p[1], m[1]), (p[2], m[2]), (p[0], 40), (p[1], m[1]), (p[2], m[2])]
    # the old setter is the mask SINGLE; a bad mask or bad rules are refused and change nothing
    stride = len(s) + 5
    hd = ais.hdlc_deframer_batch(11, 64, 1, stride, 64, repair=R21, events=ec.SKIP)
    x, n = _dev_call([np.asarray(s, np.uint8)], stride)
    for bad in (0, 8, -1, 1 << 16):
        with pytest.raises(ValueError):
            hd.set_repair(R21, bad)
    with pytest.raises(ValueError):
        hd.set_repair({8: None}, ec.ALL)
    hd.work(x, n)
    assert hd.pdus(with_repairs=True)[2].tolist() == [m[2]] * 5
    hd.set_repair(R21)
    hd.work(x, n)
    assert hd.pdus(with_repairs=True)[2].tolist() == [40] * 5
    hd.set_repair(None, ec.ALL)
    hd.work(x, n)
    assert len(hd.pdus(with_repairs=True)[0]) == 0 and (_dev_marks(hd.repairs_device(), 64) == -1).all()


def test_four_frames_closing_in_one_word_and_the_long_frame_collision(ais):
    import test_hdlc_events_model as em

    rng = np.random.default_rng(52)
    # four minimal frames whose delimiters are bits 0, 21, 42 and 63 of a lane's word, each repaired; other alignments
    # (three and one, across the pass boundary at bit 4096)
    leads = (64 * 3 - 27, 64 * 3 - 27 + 1, 64 * 2 - 27 + 30, 64 * 63 - 27, 64 * 64 - 27)
    streams, m = [], None
    for lead in leads:
        s, m = em.four_in_a_word(rng, lead)
        streams.append(s)
    got = _check(ais, 2, 64, [[np.asarray(s, np.uint8) for s in streams]], {0: None}, ec.ALL, pad=9)
    for lead, g, s in zip(leads, got, streams):
        assert g == ec.py_ref(2, 64, s, {0: None}, ec.ALL)
        assert [(e, q, f) for e, q, f in g if f >= 0] == [(lead + 27 + 21 * k, b"", m) for k in range(4)]
    # a 1000-octet frame with a skip 7140 + d bits before its end comes out with the pair at d flipped: one channel,
    # two passes and a call boundary inside the frame
    for d in (0, 700):
        s, p, first = ec.collision_stream(rng, d)
        got = _check(ais, 11, 1024, hc.split_calls([s], [[len(s) // 2]]), {998: None}, ec.ALL)
        assert [f for _, _, f in got[0]] == [ec.mark(first, 1)] and got[0] == ec.py_ref(11, 1024, s, {998: None}, ec.ALL)
        got = _check(ais, 11, 1024, [[np.asarray(s, np.uint8)]], {998: None}, ec.SKIP, pad=1)
        assert [(q, f) for _, q, f in got[0]] == [(p, ec.mark(8000 - 1 - 7140 - d - 2, 2))]


def test_overflow_keeps_a_prefix_with_its_marks(ais):
    rng = np.random.default_rng(53)
    nch = 6
    streams = [ec.event_stream(rng, 5000, rc.AIS_RULES, every=150) for _ in range(nch)]
    calls = [[np.asarray(s, np.uint8) for s in streams]]
    full = _check(ais, 11, 64, calls, rc.AIS_RULES, ec.ALL)
    flat = [(c,) + t for c in range(nch) for t in full[c]]
    small = ais.hdlc_deframer_batch(11, 64, nch, max(len(s) for s in streams) + 5, 9, repair=rc.AIS_RULES, events=ec.ALL)
    x, n = _dev_call(calls[0], small.max_bits)
    small.work(x, n)
    with pytest.raises(OverflowError):
        small.pdus(with_repairs=True)
    recs, data, fix = small.pdus(overflow_ok=True, with_repairs=True)
    assert small.found == len(flat) > 9 and len(recs) == len(fix) == 9
    assert [(c,) + t for c in range(nch) for t in rc.by_channel(recs, data, fix, nch)[c]] == flat[:9]
    assert (fix >= 1 << 16).any()
    assert _dev_marks(small.repairs_device(), 9).tolist() == [t[3] for t in flat[:9]]


def test_repaired_pdus_through_the_nmea_stage(ais):
    """results_device / repairs_device feeding pdu_to_nmea_batch: a PDU repaired by an event is a PDU, and its text is the
    host pdu_to_nmea of the payload that was sent"""
    rng = np.random.default_rng(54)
    nch = 3
    sent = [[rc.typed_payload(rng, 21, 1 + k % 3) for k in range(5)] for _ in range(nch)]
    ev = [None, (0, 1), (7, 2), (166, 1), (170, 2)]  # (intact; type bits; across octets; across payload / FCS; in the FCS)
    streams = []
    for c in range(nch):
        s = hc.noise(rng, 50)
        for p, e in zip(sent[c], ev):
            s += (ec.event_frame(p) if e is None else ec.event_frame(p, *e)) + hc.junk(rng, 40 + c)
        streams.append(s)
    stride = max(len(s) for s in streams) + 5
    hd = ais.hdlc_deframer_batch(11, 64, nch, stride, 64, repair=R21, events=ais.AIS_REPAIR_EVENTS)
    nm = ais.pdu_to_nmea_batch(["A", "B", "C"], nch, 64, 64)
    x, n = _dev_call([np.asarray(s, np.uint8) for s in streams], stride)
    hd.work(x, n)
    nm.work(hd)
    lines = nm.sentences(as_list=True)
    marks = [-1 if e is None else ec.mark(*e) for e in ev] * nch
    want = [(c, ais.pdu_to_nmea("ABC"[c]).msg_to_sentence(p)) for c in range(nch) for p in sent[c]]
    assert [(c, t) for c, _, t in lines] == want
    assert list(_dev_marks(hd.repairs_device(), 64)[:len(want)]) == marks
    assert hd.pdus(with_repairs=True)[2].tolist() == marks
    assert [ais.repair_mark(v) for v in marks[:3]] == [(-1, ()), (0, (1, 1)), (7, (1, 0, 1))]


# ---- the receiver ------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("detector", [None, "mlse"])
def test_receiver_repairs_a_burst_with_an_adjacent_pair_flipped(ais, detector):
    """ais_rx(repair=AIS_REPAIR_RULES, repair_events=AIS_REPAIR_EVENTS) at test_gpu_hdlc_repair's geometry: one stream, two
    centres, 3 blocks of 65536 x 5 items, three bursts on the -25 kHz centre, the second sent with payload bits 77 and 78
    inverted.  With all events its sentence appears and popped_repairs() marks it; the same handle with the default
    events (the single bit) gives the other two alone.  With detector="mlse" the deframer is made again and keeps rules
    and mask."""
    import nmea_cases as nc
    import test_gpu_xlate as tx

    rng = np.random.default_rng(23)
    fs, D, T, nblocks, osf = tx.FS_STOCK, tx.DECIM, tx.T, 3, 40
    n = T * D * nblocks
    x = np.zeros(n, dtype=np.complex128)
    payloads, flip = [], 77
    for k, start in enumerate((40000, 330000, 520000)):
        p = rng.integers(0, 2, 168).tolist()
        p[2:8] = [1, 0, 0, 0, 0, 0]  # message type 1 (pdu[0] >> 2, bits packed LSB first)
        payloads.append(np.packbits(np.array(p, np.uint8), bitorder="little").tobytes())
        iq = _burst(p, (flip, flip + 1) if k == 1 else (), osf)
        dur = int(iq.size / osf * fs / 9600.0)
        tg = np.arange(dur) * (osf * 9600.0 / fs)
        ph = np.interp(tg, np.arange(iq.size), np.unwrap(np.angle(iq)))
        env = np.interp(tg, np.arange(iq.size), np.abs(iq))
        cfo, ph0 = rng.uniform(-300, 300), rng.uniform(-np.pi, np.pi)
        x[start:start + dur] += env * np.exp(1j * (ph + 2 * np.pi * ((-25e3 + cfo) / fs) * (start + np.arange(dur)) + ph0))
    x += rng.normal(0, 0.1 / np.sqrt(2), n) + 1j * rng.normal(0, 0.1 / np.sqrt(2), n)
    xs = x.astype(np.complex64)[None, :]
    blocks = [np.ascontiguousarray(xs[:, k * T * D:(k + 1) * T * D]) for k in range(nblocks)]
    line = [ais.pdu_to_nmea("A").msg_to_sentence(p) for p in payloads]

    def run(**kw):
        rx = ais.ais_rx((-25e3, 25e3), fs, ("A", "B"), nstreams=1, fmt="cf32", block_items=T * D,
                        preamble_symbols=tx._template(ais), repair=ais.AIS_REPAIR_RULES, detector=detector, **kw)
        out = []
        for k, b in enumerate(blocks):
            assert rx.push(b) == k
        rx.flush()
        while (r := rx.pop(wait=True)) is not None:
            out.append(r + (rx.popped_repairs(),))
        with pytest.raises(ValueError):
            rx.enable_repair(ais.AIS_REPAIR_RULES, ais.AIS_REPAIR_EVENTS)  # only before the first block
        assert all(len(fix) == len(recs) for _, recs, _, fix in out)
        return [(t, int(f)) for _, recs, text, fix in out for (_, _, t), f in zip(nc.split(recs, text), fix)]

    assert run() == [(line[0], -1), (line[2], -1)]
    assert run(repair_events=ais.AIS_REPAIR_EVENTS) == [(line[0], -1), (line[1], ec.mark(flip, 1)), (line[2], -1)]
    assert ais.repair_mark(ec.mark(flip, 1)) == (77, (1, 1))
    with pytest.raises(ValueError):
        run(repair_events=8)


def _burst(payload, flips, osf):
    """synth.make_burst's waveform (family S, osf samples per symbol, no timing offset) for a given payload, the payload
    bits `flips` inverted before stuffing and modulation; the FCS is the intact payload's"""
    import synth

    bits = list(payload)
    frame = bits + synth.crc16_hdlc(bits)
    for j in flips:
        frame[j] ^= 1
    data_bits = synth.FLAG + synth.bit_stuff(frame) + synth.FLAG
    sync_lv = [1 if b else -1 for b in synth.sync_bits("S")]
    data_lv = synth.nrzi_levels(data_bits, start_level=sync_lv[-1])
    levels = np.array([(-1) ** k for k in range(8)] + sync_lv + data_lv + [data_lv[-1]] * 4, dtype=np.float64)
    iq = synth.gmsk_waveform(levels, osf)[: len(levels) * osf]
    env = np.ones(iq.size)
    r = 8 * osf // 2
    env[:r] = np.linspace(0, 1, r, endpoint=False)
    env[-r:] = np.linspace(1, 0, r, endpoint=False)
    return iq * env
