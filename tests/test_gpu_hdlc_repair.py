"""-m gpu: single-bit repair by CRC syndrome in the batched HDLC deframer on the MI355X (aisx_hdlc_batch_set_repair,
ais_amd.hdlc_deframer_batch(repair=...)) against the host form that is its specification (one
ais_amd.hdlc_deframer_bp(repair=...) per channel fed the same bits call by call): the same PDUs, order, bytes and marks;
the marks through an overflow, the repaired PDUs through the NMEA stage, and the receiver handle
(ais_amd.ais_rx(repair=...)) on a burst sent with one wrong payload bit."""
import numpy as np
import pytest

import hdlc_cases as hc
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


def _run(ais, lmin, lmax, calls, rules, pad=0, max_pdus=1 << 14, switch_call=None, switch_rules=None):
    nch = len(calls[0])
    stride = max(max(len(x) for x in call) for call in calls) + 5
    hd = ais.hdlc_deframer_batch(lmin, lmax, nch, stride, max_pdus, repair=rules)
    got = [[] for _ in range(nch)]
    for k, call in enumerate(calls):
        if k == switch_call:
            hd.set_repair(switch_rules)
        b, n = _dev_call(call, stride, pad)
        hd.work(b, n)
        recs, data, fix = hd.pdus(with_repairs=True)
        for c, lst in enumerate(rc.by_channel(recs, data, fix, nch)):
            got[c] += lst
    return got


def _check(ais, lmin, lmax, calls, rules, pad=0, **kw):
    got = _run(ais, lmin, lmax, calls, rules, pad, **kw)
    ref = rc.host_ref(lmin, lmax, calls, rules, kw.get("switch_call"), kw.get("switch_rules"))
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


def _nfixed(got):
    return sum(f >= 0 for g in got for _, _, f in g)


@pytest.mark.parametrize("nch", [1, 37])
def test_model_cases_on_the_device(ais, nch):
    rng = np.random.default_rng(300 + nch)
    # repaired and intact frames in noise, 5 000 - 9 000 bits per channel (more than one 4096-bit pass) in 3 calls,
    # rows off 16-byte alignment
    streams = [rc.repair_stream(rng, int(rng.integers(5000, 9000)), rc.AIS_RULES, every=500) for _ in range(nch)]
    cuts = [sorted(rng.integers(0, len(s), 2)) for s in streams]
    calls = [[hc.as_bytes(rng, b, wild=(c % 2 == 1)) for c, b in enumerate(call)] for call in hc.split_calls(streams, cuts)]
    got = _check(ais, 11, 64, calls, rc.AIS_RULES, pad=5)
    tot, fixed = sum(len(g) for g in got), _nfixed(got)
    assert fixed >= 3 * nch ** 0.5 and tot > fixed
    assert got[0] == rc.py_ref(11, 64, streams[0], rc.AIS_RULES)  # (end bits too, on one channel)
    # flips on the stuffed stream, length-only rules: equality with the host form is the only claim
    streams = [rc.repair_stream(rng, 6000, rc.AIS_RULES, every=200, raw_flips=50) for _ in range(nch)]
    cuts = [sorted(rng.integers(0, 6000, 2)) for _ in range(nch)]
    got = _check(ais, 11, 64, hc.split_calls(streams, cuts), {k: None for k in rc.AIS_RULES})
    fixed += _nfixed(got)
    # a repaired frame across the pass boundary at bit 4096 and across both call boundaries (another offset per
    # channel), then two frames sharing a flag, the second repaired
    a, b = rc.typed_payload(rng, 21, 3), rc.typed_payload(rng, 21, 4)
    fa = rc.frame_bits(a, (90,))
    s = hc.junk(rng, 4096 - 100) + fa + hc.noise(rng, 700) + fa + hc.noise(rng, 500) + rc.frame_bits(b)[:-8] + \
        rc.frame_bits(a, (171,)) + hc.noise(rng, 300)
    x0, x1 = 4096 - 100 + len(fa) + 700, 4096 - 100 + 2 * len(fa) + 1200
    cuts = [[x0 + (7 * c) % len(fa), x1 + (11 * c) % (2 * len(fa))] for c in range(nch)]
    got = _check(ais, 11, 64, hc.split_calls([s] * nch, cuts), R21, pad=(3 if nch > 1 else 0))
    for g in got:
        assert [(p, f) for _, p, f in g if p in (a, b)] == [(a, 90), (a, 90), (b, -1), (a, 171)]
    # set_repair between calls with a frame open: off -> on before call 1, whose first bits close a damaged frame
    s = hc.noise(rng, 5000) + fa + hc.noise(rng, 600)
    cuts = [[5000 + 8 + (13 * c) % 150, 5000 + len(fa) + 300] for c in range(nch)]
    got = _check(ais, 11, 64, hc.split_calls([s] * nch, cuts), None, switch_call=1, switch_rules=R21)
    assert all((a, 90) in [(p, f) for _, p, f in g] for g in got)
    got = _check(ais, 11, 64, hc.split_calls([s] * nch, cuts), R21, switch_call=1, switch_rules=None)
    assert all(a not in [p for _, p, _ in g] and all(f == -1 for _, _, f in g) for g in got)
    print("%d channels: %d PDUs, %d repaired, identical to the host form" % (nch, tot, fixed))


def test_overflow_keeps_a_prefix_with_its_marks(ais):
    rng = np.random.default_rng(21)
    nch = 6
    streams = [rc.repair_stream(rng, 5000, rc.AIS_RULES, every=150) for _ in range(nch)]
    calls = [[np.asarray(s, np.uint8) for s in streams]]
    full = _check(ais, 11, 64, calls, rc.AIS_RULES)
    flat = [(c,) + t for c in range(nch) for t in full[c]]
    small = ais.hdlc_deframer_batch(11, 64, nch, max(len(s) for s in streams) + 5, 9, repair=rc.AIS_RULES)
    x, n = _dev_call(calls[0], small.max_bits)
    small.work(x, n)
    with pytest.raises(OverflowError):
        small.pdus(with_repairs=True)
    recs, data, fix = small.pdus(overflow_ok=True, with_repairs=True)
    assert small.found == len(flat) > 9 and len(recs) == len(fix) == 9
    assert [(c,) + t for c in range(nch) for t in rc.by_channel(recs, data, fix, nch)[c]] == flat[:9]
    assert (fix >= 0).any() and (fix < 0).any()
    # a handle that never had rules: every mark is -1; bad rules are refused and change nothing
    plain = ais.hdlc_deframer_batch(11, 64, nch, small.max_bits, 64)
    plain.work(x, n)
    recs, data, fix = plain.pdus(with_repairs=True)
    assert len(recs) >= 3 and (fix == -1).all()
    assert (_dev_marks(plain.repairs_device(), 64) == -1).all()
    for bad in ({8: None}, {63: None}, {k: None for k in range(9, 26)}):
        with pytest.raises(ValueError):
            small.set_repair(bad)
    small.work(x, n)
    r2, d2, f2 = small.pdus(overflow_ok=True, with_repairs=True)
    assert [(c,) + t for c in range(nch) for t in rc.by_channel(r2, d2, f2, nch)[c]] != []  # (still the rules it had:)
    assert (f2 >= 0).any()


def test_repaired_pdus_through_the_nmea_stage(ais):
    """results_device / repairs_device feeding pdu_to_nmea_batch: a repaired PDU is a PDU, and its text is the host
    pdu_to_nmea of the payload that was sent"""
    rng = np.random.default_rng(22)
    nch = 3
    sent = [[rc.typed_payload(rng, 21, 1 + k % 3) for k in range(4)] for _ in range(nch)]
    flips = [(), (0,), (100,), (170,)]
    streams = []
    for c in range(nch):
        s = hc.noise(rng, 50)
        for p, f in zip(sent[c], flips):
            s += rc.frame_bits(p, f) + hc.junk(rng, 40 + c)
        streams.append(s)
    stride = max(len(s) for s in streams) + 5
    hd = ais.hdlc_deframer_batch(11, 64, nch, stride, 64, repair=R21)
    nm = ais.pdu_to_nmea_batch(["A", "B", "C"], nch, 64, 64)
    x, n = _dev_call([np.asarray(s, np.uint8) for s in streams], stride)
    hd.work(x, n)
    nm.work(hd)
    lines = nm.sentences(as_list=True)
    marks = _dev_marks(hd.repairs_device(), 64)
    want = [(c, ais.pdu_to_nmea("ABC"[c]).msg_to_sentence(p)) for c in range(nch) for p in sent[c]]
    assert [(c, t) for c, _, t in lines] == want
    assert list(marks[:len(want)]) == [-1, 0, 100, 170] * nch
    assert hd.pdus(with_repairs=True)[2].tolist() == [-1, 0, 100, 170] * nch


# ---- the receiver ------------------------------------------------------------------------------------------------------


def _burst(payload, flip, osf):
    """synth.make_burst's waveform (family S, osf samples per symbol, no timing offset) for a given payload, payload bit
    `flip` inverted before stuffing and modulation; the FCS is the intact payload's"""
    import synth

    bits = list(payload)
    frame = bits + synth.crc16_hdlc(bits)
    if flip is not None:
        frame[flip] ^= 1
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


def test_receiver_repairs_a_burst_with_one_wrong_payload_bit(ais):
    """ais_rx(repair=AIS_REPAIR_RULES) at test_gpu_rx_paths.test_one_stream's geometry: one stream, two centres, 3 blocks
    of 65536 x 5 items.  Three bursts on the -25 kHz centre, the second sent with payload bit 77 inverted: with repair
    its sentence appears and popped_repairs() marks it; without, the text is the hand-wired pipeline's, byte for byte,
    and lacks it."""
    import synth
    import test_gpu_rx as gr
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
        iq = _burst(p, flip if k == 1 else None, osf)
        dur = int(iq.size / osf * fs / 9600.0)
        tg = np.arange(dur) * (osf * 9600.0 / fs)
        ph = np.interp(tg, np.arange(iq.size), np.unwrap(np.angle(iq)))
        env = np.interp(tg, np.arange(iq.size), np.abs(iq))
        cfo, ph0 = rng.uniform(-300, 300), rng.uniform(-np.pi, np.pi)
        x[start:start + dur] += env * np.exp(1j * (ph + 2 * np.pi * ((-25e3 + cfo) / fs) * (start + np.arange(dur)) + ph0))
    x += rng.normal(0, 0.1 / np.sqrt(2), n) + 1j * rng.normal(0, 0.1 / np.sqrt(2), n)
    xs = x.astype(np.complex64)[None, :]
    blocks = [np.ascontiguousarray(xs[:, k * T * D:(k + 1) * T * D]) for k in range(nblocks)]
    want = gr.hand_wired(ais, [tx._dev(b) for b in blocks], 1)
    line = [ais.pdu_to_nmea("A").msg_to_sentence(p) for p in payloads]
    plain_text = b"".join(w[1] for w in want).decode()
    assert line[0] in plain_text and line[2] in plain_text and line[1] not in plain_text

    def run(**kw):
        rx = ais.ais_rx((-25e3, 25e3), fs, ("A", "B"), nstreams=1, fmt="cf32", block_items=T * D,
                        preamble_symbols=tx._template(ais), **kw)
        out = []
        for k, b in enumerate(blocks):
            assert rx.push(b) == k
        rx.flush()
        while (r := rx.pop(wait=True)) is not None:
            out.append(r + ((rx.popped_repairs() if kw else None),))
        if not kw:
            with pytest.raises(ValueError):
                rx.popped_repairs()
        else:
            with pytest.raises(ValueError):
                rx.enable_repair(ais.AIS_REPAIR_RULES)  # only before the first block
        return out

    off = run()
    assert [(r.tobytes(), t) for _, r, t, _ in off] == [(r.tobytes(), t) for r, t in want]
    on = run(repair=ais.AIS_REPAIR_RULES)
    import nmea_cases as nc

    got = [(t, int(f)) for _, recs, text, fix in on for (_, _, t), f in zip(nc.split(recs, text), fix)]
    assert all(len(fix) == len(recs) for _, recs, _, fix in on)
    assert got == [(line[0], -1), (line[1], flip), (line[2], -1)]
