"""Repair of one error event by CRC syndrome in the HDLC deframers, -m "not gpu": the tables of
aisx_hdlc_event_table, the host form (aisx_hdlc_set_repair_events / aisx_hdlc_work_repair,
ais_amd.hdlc_deframer_bp(repair=, events=)) against the Python restatement of its rule (tests/hdlc_events_cases.py), its
false accepts on noise and what it recovers near the threshold, and the kernel bodies of gr-ais_amd/csrc/k_hdlc.h with
the event repair compiled in, on the CPU lane model (tests/emul_hdlc), against the host form bit for bit, marks
included."""
import concurrent.futures as cf
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import hdlc_cases as hc
import hdlc_events_cases as ec
import hdlc_repair_cases as rc
import mlse_cases as mc
import torch  # noqa: F401  (before libaisx.so: one HIP runtime in the process)

HERE = os.path.dirname(os.path.abspath(__file__))
EMUL = os.path.join(HERE, "emul_hdlc")
R21 = {21: (1, 2, 3, 4, 9, 11, 18, 24)}
REACH = 16383


def emu():
    L = hc.emu()
    assert L.emu_hdlc_rule_size() == rc.RULE_DTYPE.itemsize
    return L


class EmuBatch:
    def __init__(self, lmin, lmax, nch, max_bits, max_pdus=4096, rules=None, events=1):
        self.h = emu().emu_hdlc_create(lmin, lmax, nch, max_bits, max_pdus)
        assert self.h
        self.nch, self.max_pdus, self.lmax, self.max_bits = nch, max_pdus, lmax, max_bits
        self.set_repair(rules, events)

    def __del__(self):
        emu().emu_hdlc_destroy(self.h)

    def set_repair(self, rules, events=1):
        a = rc.rule_array(rules)
        emu().emu_hdlc_set_repair(self.h, a.ctypes.data if a.size else None, a.size, events)

    def process(self, call, pad_front=0):
        rows, n = hc.pack(call, self.max_bits + 3, pad_front)
        emu().emu_hdlc_process(self.h, rows.ctypes.data, rows.strides[0], n.ctypes.data)

    def read(self):
        recs = np.zeros(self.max_pdus, dtype=hc.REC_DTYPE)
        data = np.zeros(self.max_pdus * (self.lmax - 1) + 1, dtype=np.uint8)
        fix = np.full(self.max_pdus, -9, dtype=np.int32)
        cnt = np.zeros(3, dtype=np.int32)
        emu().emu_hdlc_read(self.h, recs.ctypes.data, data.ctypes.data, fix.ctypes.data, cnt.ctypes.data)
        return int(cnt[0]), int(cnt[2]), recs[: cnt[1]], data, fix[: cnt[1]]


def run_model(lmin, lmax, calls, rules, events, pad_front=0, max_pdus=4096, switch_call=None, switch_rules=None, switch_events=1):
    nch = len(calls[0])
    b = EmuBatch(lmin, lmax, nch, max(max(len(x) for x in call) for call in calls) + 1, max_pdus, rules, events)
    got = [[] for _ in range(nch)]
    for k, call in enumerate(calls):
        if k == switch_call:
            b.set_repair(switch_rules, switch_events)
        b.process(call, pad_front)
        found, bad, recs, data, fix = b.read()
        assert bad == 0 and found == len(recs)
        for c, lst in enumerate(rc.by_channel(recs, data, fix, nch)):
            got[c] += lst
    return got


def check(lmin, lmax, calls, rules, events, streams=None, pad_front=0, switch_call=None, switch_rules=None, switch_events=1,
          switch_pos=None):
    """the lane model against the host form (payloads and marks) and, given the streams, the restatement (end bits too)"""
    got = run_model(lmin, lmax, calls, rules, events, pad_front, switch_call=switch_call, switch_rules=switch_rules,
                    switch_events=switch_events)
    ref = ec.host_ref(lmin, lmax, calls, rules, events, switch_call, switch_rules, switch_events)
    for c in range(len(got)):
        assert [(p, f) for _, p, f in got[c]] == ref[c], c
        if streams is not None:
            sw = (switch_pos[c], switch_rules, switch_events) if switch_pos is not None else None
            assert got[c] == ec.py_ref(lmin, lmax, streams[c], rules, events, sw), c
    return got


def host(bits, rules, events, lmin=11, lmax=64):
    import ais_amd

    return ais_amd.hdlc_deframer_bp(lmin, lmax, repair=rules, events=events).work(np.asarray(bits, np.uint8), with_repairs=True)


def flipped(payload, idx):
    b = bytearray(payload)
    for j in idx:
        if j < 8 * len(b):
            b[j >> 3] ^= 1 << (j & 7)
    return bytes(b)


def four_in_a_word(rng, lead):
    """four 2-octet frames (no payload, the FCS of nothing: 16 zeros) whose FCS has a PAIR in its last two bits, each
    followed by three more ones, its delimiter and the zero the deframer drops behind it: 21 bits per frame, so that four
    delimiters span 64 bits -- the first `lead` + 27 bits into the stream.  Returns (stream, the frames' mark)"""
    unit = [0] * 14 + [1, 1] + [1, 1, 1] + [1] + [0]
    return hc.junk(rng, lead) + hc.FLAG + unit * 4 + hc.junk(rng, 40), ec.mark(14, 1)


def agrees(bits, rules, events, lmin=11, lmax=64):
    """the host form's (PDUs, marks) of the stream, asserted equal to the restatement's"""
    want = ec.py_ref(lmin, lmax, bits, rules, events)
    pdus, fix = host(bits, rules, events, lmin, lmax)
    assert list(zip(pdus, fix)) == [(p, f) for _, p, f in want]
    return list(zip(pdus, fix))


# ---- the tables --------------------------------------------------------------------------------------------------------


def _s():
    """s(d) for d < REACH + 2: 0x8000 and one step of the shift register per bit"""
    s = np.zeros(REACH + 2, dtype=np.int64)
    v = 0x8000
    for d in range(REACH + 2):
        s[d] = v
        v = (v >> 1) ^ (0x8408 if v & 1 else 0)
    return s


def test_event_tables():
    import ais_amd
    from ais_amd import _lib, framing

    s = _s()
    d = np.arange(REACH)
    syn = [s[:REACH], s[:REACH] ^ s[1:REACH + 1], s[:REACH] ^ s[2:REACH + 2]]
    single = np.zeros(65536, dtype=np.uint16)
    emu().emu_hdlc_syndrome_table(single.ctypes.data)
    for mask in ec.MASKS:
        ids = [e for e in range(3) if (mask >> e) & 1]
        best = np.full(65536, 1 << 30, dtype=np.int64)
        for e in ids:
            np.minimum.at(best, syn[e], d)
        want = np.zeros(65536, dtype=np.int64)
        claimed = np.zeros(65536, dtype=np.int64)
        for e in ids:
            win = best[syn[e]] == d
            want[syn[e][win]] = (e << 14) | (d[win] + 1)
            np.add.at(claimed, syn[e][win], 1)
        assert claimed.max() == 1 and want[0] == 0  # (no two events at the same distance share a syndrome; 0 is no error)
        tab = framing.event_table(mask)
        assert np.array_equal(tab.astype(np.int64), want), mask
    # the single event alone: hdlc_syndrome_table() wherever that is within reach
    assert np.array_equal(framing.event_table(ec.SINGLE), np.where(single <= REACH, single, 0))
    assert (single > REACH).any()
    # hdlc_syndrome_table() itself, by a walk of the CRC register of its own: 0x8000 for the frame's last bit, one step
    # per bit before it, the nearest bit where two give the same syndrome
    walk, v = np.zeros(65536, dtype=np.uint16), 0x8000
    for k in range(32767):
        if not walk[v]:
            walk[v] = k + 1
        v = (v >> 1) ^ (0x8408 if v & 1 else 0)
    assert np.array_equal(single, walk)
    # single syndromes are never pair or skip ones; pair at 0 and skip at 7140 collide, and the pair wins
    assert not set(syn[0].tolist()) & (set(syn[1].tolist()) | set(syn[2].tolist()))
    assert syn[1][0] == syn[2][7140]
    assert framing.event_table(6)[syn[1][0]] == (1 << 14) | 1 and framing.event_table(ec.ALL)[syn[1][0]] == (1 << 14) | 1
    assert framing.event_table(ec.SKIP)[syn[1][0]] == (2 << 14) | 7141
    assert all(syn[1][k] == syn[2][7140 + k] for k in range(0, REACH - 7142, 97))
    assert len(set(np.concatenate([x[:8208] for x in syn]).tolist())) == 23556  # of 3 x 8208 below the longest frame
    n = 8 * 892  # below 893 octets nothing collides
    assert len(set(np.concatenate([syn[0][:n], syn[1][: n - 1], syn[2][: n - 2]]).tolist())) == 3 * n - 3
    # a bad mask or no table
    L = _lib.lib(device=False)
    for bad in (0, 8, 9, -1, 1 << 16):
        assert L.aisx_hdlc_event_table(bad, tab.ctypes.data_as(C.c_void_p)) == _lib.AISX_ERR_INVALID
    assert L.aisx_hdlc_event_table(7, None) == _lib.AISX_ERR_INVALID
    assert ais_amd.AIS_REPAIR_EVENTS == 7 == ais_amd.REPAIR_SINGLE | ais_amd.REPAIR_PAIR | ais_amd.REPAIR_SKIP
    assert [ais_amd.repair_mark(m) for m in (-1, 0, 183, (1 << 16) | 5, (2 << 16) | 181)] == \
        [(-1, ()), (0, (1,)), (183, (1,)), (5, (1, 1)), (181, (1, 0, 1))]
    with pytest.raises(ValueError):
        ais_amd.repair_mark(3 << 16)


# ---- the host form against the restatement -----------------------------------------------------------------------------


def test_every_event_at_every_position_of_a_frame_on_the_host():
    """23 octets, so index 0 and the type bits, every octet boundary, the payload / FCS boundary (bits 167 | 168), events
    wholly in the FCS and the frame's last bit are all among the positions"""
    rng = np.random.default_rng(31)
    payload = rc.typed_payload(rng, 21, 18)
    other = rc.typed_payload(rng, 21, 19)  # a type R21 does not allow
    lead = hc.noise(rng, 23)
    made_allowed = 0
    for eid in range(3):
        lone = 1 << eid
        for first in range(184 - ec.SPAN[eid]):
            bits = lead + ec.event_frame(payload, first, eid) + [0, 1, 0]
            m = ec.mark(first, eid)
            for mask in (ec.ALL, lone, lone | (ec.SKIP if eid == 1 else ec.PAIR)):  # (the third: without SINGLE, or for it with PAIR)
                assert agrees(bits, R21, mask) == [(payload, m)], (eid, first, mask)
            for mask in (ec.ALL & ~lone, ):  # the event not enabled: no other event explains a frame this short
                assert agrees(bits, R21, mask) == [], (eid, first, mask)
            # sent with a type the rule does not allow: stays out, unless the flips themselves make the type an allowed
            # one -- then the repair restores the sent type and drops it all the same; the restatement decides
            assert agrees(lead + ec.event_frame(other, first, eid) + [0], R21, ec.ALL) == [], (eid, first)
            # sent with an allowed type, received -- through an event on the type bits -- with a disallowed one: repaired
            rx_type = (payload[0] ^ sum(1 << j for j in ec.flips_of(m) if j < 8)) >> 2
            made_allowed += first < 8 and not (rc.masks(R21)[21] >> rx_type) & 1
    assert made_allowed >= 4
    # single-bit marks are what the single-bit repair gives, and its setter is the mask SINGLE
    import ais_amd

    bits = lead + ec.event_frame(payload, 77, 0) + [0]
    a = ais_amd.hdlc_deframer_bp(11, 64, repair=R21).work(np.asarray(bits, np.uint8), with_repairs=True)
    assert a == host(bits, R21, ec.SINGLE) == ([payload], [77]) and agrees(bits, R21, ec.ALL) == [(payload, 77)]
    assert agrees(lead + ec.event_frame(payload) + [0], R21, ec.ALL) == [(payload, -1)]


def test_an_event_named_outside_a_short_frame():
    """a 13-octet frame whose FCS is off by the syndrome of an event further from the end than the frame is long"""
    rng = np.random.default_rng(32)
    s = _s()
    p = rc.typed_payload(rng, 11, 1)
    lead = hc.noise(rng, 19)
    n = 8 * 13
    seen = 0
    for eid in range(3):
        sp = ec.SPAN[eid]
        for d in sorted({n - sp - 1, n - sp, n - 1, n, n + 1, n + 40, 8000}):  # the first: the event's first bit is the frame's
            syn = int(s[d] ^ s[d + sp]) if sp else int(s[d])
            fcs_flips = tuple(8 * 11 + k for k in range(16) if (syn >> k) & 1)
            bits = lead + rc.frame_bits(p, fcs_flips) + [0]
            got = agrees(bits, {11: None}, ec.ALL)
            if d + sp < n:  # (inside: the frame's first bits are flipped, which the FCS as sent then fits)
                assert got == [(flipped(p, ec.flips_of(ec.mark(0, eid))), ec.mark(0, eid))]
                seen += 1
            else:
                assert got == [], (eid, d)
    assert seen == 3


def test_the_nearer_event_wins_in_a_long_frame():
    import ais_amd

    rng = np.random.default_rng(33)
    for d in (0, 5, 700):
        s, p, first = ec.collision_stream(rng, d)
        n = 8000
        skip_first = n - 1 - (7140 + d) - 2
        # all events: the pair at d is flipped, not the skip that was sent -- the payload comes out wrong in four bits
        # (d = 0 .. 15: the pair lies in the FCS, and only the skip's two), the mark says pair
        got = agrees(s, {998: None}, ec.ALL, 11, 1024)
        assert [f for _, f in got] == [ec.mark(first, 1)] and ais_amd.repair_mark(got[0][1]) == (first, (1, 1))
        wrong = np.unpackbits(np.frombuffer(got[0][0], np.uint8) ^ np.frombuffer(p, np.uint8), bitorder="little")
        assert sorted(np.flatnonzero(wrong)) == sorted(j for j in (skip_first, skip_first + 2, first, first + 1) if j < 8 * 998)
        # without PAIR the skip is found and the payload is the sent one
        assert agrees(s, {998: None}, ec.SKIP | ec.SINGLE, 11, 1024) == [(p, ec.mark(skip_first, 2))]


def test_rules_and_mask_on_the_host():
    import ais_amd
    from ais_amd import _lib

    rng = np.random.default_rng(34)
    lead = hc.noise(rng, 31)
    p21, p30 = rc.typed_payload(rng, 21, 1), rc.typed_payload(rng, 30, 1)
    bits = lead + ec.event_frame(p30, 77, 1) + lead + ec.event_frame(p21, 99, 2) + [0]
    assert agrees(bits, R21, ec.ALL) == [(p21, ec.mark(99, 2))]
    assert agrees(bits, {21: (1,), 30: None}, ec.ALL) == [(p30, ec.mark(77, 1)), (p21, ec.mark(99, 2))]
    assert agrees(bits, {21: (1,), 30: None}, ec.PAIR) == [(p30, ec.mark(77, 1))]
    assert agrees(bits, None, ec.ALL) == []
    # a bad mask is refused and leaves the handle as it was, rules and mask
    d = ais_amd.hdlc_deframer_bp(11, 64, repair=R21, events=ec.SKIP)
    b = np.asarray(bits, np.uint8)
    for bad in (0, 8, 15, -2, 1 << 20):
        with pytest.raises(ValueError):
            d.set_repair({30: None}, bad)
    with pytest.raises(ValueError):
        d.set_repair({8: None}, ec.ALL)
    L = _lib.lib(device=False)
    assert L.aisx_hdlc_set_repair_events(None, None, 0, 7) == _lib.AISX_ERR_INVALID
    assert L.aisx_hdlc_set_repair_events(d._h, None, 1, 7) == _lib.AISX_ERR_INVALID
    assert d.work(b, with_repairs=True) == ([p21], [ec.mark(99, 2)])
    # switched between calls: pair only, all, single (by the old setter), off
    d.set_repair({30: None}, ec.PAIR)
    assert d.work(b, with_repairs=True) == ([p30], [ec.mark(77, 1)])
    d.set_repair({21: None, 30: None}, ec.ALL)
    assert d.work(b, with_repairs=True) == ([p30, p21], [ec.mark(77, 1), ec.mark(99, 2)])
    d.set_repair({21: None, 30: None})
    assert d.work(b, with_repairs=True) == ([], [])
    assert d.work(np.asarray(lead + ec.event_frame(p21, 5, 0) + [0], np.uint8), with_repairs=True) == ([p21], [5])
    d.set_repair(None, ec.ALL)
    assert d.work(b, with_repairs=True) == ([], [])


def test_every_split_of_a_stream_into_calls_on_the_host():
    import ais_amd

    rng = np.random.default_rng(35)
    p, q = rc.typed_payload(rng, 21, 3), rc.typed_payload(rng, 12, 27)
    s = hc.noise(rng, 17) + ec.event_frame(p, 166, 2) + hc.noise(rng, 9) + ec.event_frame(q, 0, 1) + [0, 0]
    whole = agrees(s, rc.AIS_RULES, ec.ALL)
    assert whole == [(p, ec.mark(166, 2)), (q, ec.mark(0, 1))]
    b = np.asarray(s, np.uint8)
    for cut in range(len(s) + 1):
        d = ais_amd.hdlc_deframer_bp(11, 64, repair=rc.AIS_RULES, events=ec.ALL)
        a1, f1 = d.work(b[:cut], with_repairs=True)
        a2, f2 = d.work(b[cut:], with_repairs=True)
        assert list(zip(a1 + a2, f1 + f2)) == whole, cut
    # the mask switched at every position, SKIP before and PAIR behind: what holds when a frame closes decides
    ends = [e for e, _, _ in ec.py_ref(11, 64, s, rc.AIS_RULES, ec.ALL)]
    for cut in range(0, len(s) + 1, 3):
        d = ais_amd.hdlc_deframer_bp(11, 64, repair=rc.AIS_RULES, events=ec.SKIP)
        a1, f1 = d.work(b[:cut], with_repairs=True)
        d.set_repair(rc.AIS_RULES, ec.PAIR)
        a2, f2 = d.work(b[cut:], with_repairs=True)
        want = [(x, f) for _, x, f in ec.py_ref(11, 64, s, rc.AIS_RULES, ec.SKIP, (cut, rc.AIS_RULES, ec.PAIR))]
        assert list(zip(a1 + a2, f1 + f2)) == want == ([whole[0]] if cut > ends[0] else []) + ([whole[1]] if cut <= ends[1] else []), cut


# ---- noise and gain ----------------------------------------------------------------------------------------------------


def test_false_accepts_on_noise():
    """default_rng(1)'s 4 000 000 bits, deframer (11, 64): with the typed rules and all events at most 2 repaired PDUs (the
    plain CRC's own expectation there is 0.23); with lengths-only rules exactly what the restatement delivers"""
    import ais_amd

    bits = np.random.default_rng(1).integers(0, 2, 4000000).astype(np.uint8)
    any_type = {k: None for k in ais_amd.AIS_REPAIR_RULES}
    want = ec.py_ref(11, 64, bits.tolist(), any_type, ec.ALL)
    got = host(bits, any_type, ec.ALL)
    assert list(zip(*got)) == [(p, f) for _, p, f in want]
    nfix = sum(f >= 0 for f in got[1])
    typed = host(bits, ais_amd.AIS_REPAIR_RULES, ec.ALL)
    tm = rc.masks(ais_amd.AIS_REPAIR_RULES)
    assert list(zip(*typed)) == [(p, f) for _, p, f in want if f < 0 or (tm[len(p)] >> (p[0] >> 2)) & 1]
    ntyped = sum(f >= 0 for f in typed[1])
    print("4 Mbit of noise, all events: %d repaired with lengths-only rules, %d with the typed rules, %d plain CRC passes"
          % (nfix, ntyped, sum(f < 0 for f in typed[1])))
    assert ntyped <= 2
    assert 5 <= nfix <= 40  # (15 346 candidates x 3 x ~180 patterns / 65 536 x the share of the five lengths: about 15)


def _gain_one(args):
    import ais_amd

    seed, ebn0, tmpl, det = args
    bits, syms, sent = mc.noisy_channel(seed, 131072, ebn0, tmpl)
    if det:
        bits = np.concatenate(mc.host_run(ais_amd, [syms]))
    row = dict(sent=len(sent))
    for name, events in (("single", ec.SINGLE), ("all", ec.ALL)):
        pdus = ais_amd.hdlc_deframer_bp(11, 64, repair=ais_amd.AIS_REPAIR_RULES, events=events).work(bits)
        row[name] = len(set(pdus) & sent)
        row[name + "_unsent"] = len([p for p in pdus if p not in sent])
    return row


def test_gain_near_the_threshold():
    """seeds 5000..5003, 131 072 samples at 4 per symbol, AIS_REPAIR_RULES: from the bit tail at 16 dB all events recover
    at least 1.4 x the payloads the single event does and deliver nothing that was not sent; behind the sequence detector
    at 14 dB strictly more"""
    tmpl = mc.stock_template()
    jobs = [(5000 + c, e, tmpl, det) for e, det in ((16, False), (14, True)) for c in range(4)]
    with cf.ThreadPoolExecutor(8) as ex:
        rows = list(ex.map(_gain_one, jobs))
    tail = {k: sum(r[k] for r in rows[:4]) for k in rows[0]}
    mlse = {k: sum(r[k] for r in rows[4:]) for k in rows[0]}
    print("  bit tail, 16 dB: %s; detector, 14 dB: %s" % (tail, mlse))
    assert tail["all"] >= 1.4 * tail["single"] and tail["single"] > 0
    assert tail["all_unsent"] == 0
    assert mlse["all"] > mlse["single"]


# ---- the lane model against the host form ------------------------------------------------------------------------------


def test_lane_model_events_in_noise():
    rng = np.random.default_rng(41)
    streams = [ec.event_stream(rng, 9000, rc.AIS_RULES) for _ in range(5)]
    cuts = [sorted(rng.integers(0, 9000, 2)) for _ in range(5)]
    calls = [[hc.as_bytes(rng, b, wild=(c % 2 == 1)) for c, b in enumerate(call)] for call in hc.split_calls(streams, cuts)]
    got = check(11, 64, calls, rc.AIS_RULES, ec.ALL, streams)
    kinds = [sum(f >= 0 and f >> 16 == e for g in got for _, _, f in g) for e in range(3)]
    nfcs = sum(f >= 0 and (f & 0xFFFF) >= 8 * len(p) for g in got for _, p, f in g)
    print("events in noise: %d PDUs, repaired %s (%d in the FCS)" % (sum(len(g) for g in got), kinds, nfcs))
    assert min(kinds) >= 3 and nfcs >= 1 and sum(f < 0 for g in got for _, _, f in g) >= 3
    for mask in (ec.PAIR, ec.PAIR | ec.SKIP, ec.SINGLE | ec.SKIP):
        check(11, 64, calls, rc.AIS_RULES, mask, streams)
    # lengths-only rules, another geometry, misaligned rows; flips on the stuffed stream (equality is the only claim)
    check(9, 40, calls, {21: None, 12: None, 20: None, 17: None}, ec.ALL, streams, pad_front=5)
    streams = [ec.event_stream(rng, 6000, rc.AIS_RULES, every=200, raw_flips=50) for _ in range(4)]
    cuts = [sorted(rng.integers(0, 6000, 2)) for _ in range(4)]
    got = check(11, 64, hc.split_calls(streams, cuts), {k: None for k in rc.AIS_RULES}, ec.ALL, streams, pad_front=15)
    assert sum(f >= 0 for g in got for _, _, f in g) >= 5


def test_lane_model_every_position_of_a_frame():
    """one channel per position: every event at every position of a 23-octet frame, all events enabled, and the frames
    whose flips decide the type"""
    rng = np.random.default_rng(42)
    payload, other = rc.typed_payload(rng, 21, 18), rc.typed_payload(rng, 21, 19)
    lead = hc.noise(rng, 23)
    for eid in range(3):
        pos = list(range(184 - ec.SPAN[eid]))
        streams = [lead + ec.event_frame(payload, f, eid) + [0, 1, 0] for f in pos] + \
                  [lead + ec.event_frame(other, f, eid) + [0, 1, 0] for f in range(8)]
        got = check(11, 64, [[np.asarray(s, np.uint8) for s in streams]], R21, ec.ALL, streams)
        assert [[(p, f) for _, p, f in g] for g in got[: len(pos)]] == [[(payload, ec.mark(f, eid))] for f in pos]


def test_lane_model_short_frame_and_long_frame_collision():
    rng = np.random.default_rng(43)
    s = _s()
    p = rc.typed_payload(rng, 11, 1)
    streams = []
    for eid in range(3):
        for d in (8 * 13 - ec.SPAN[eid] - 1, 8 * 13 - ec.SPAN[eid], 8 * 13 + 1, 8000):
            syn = int(s[d] ^ s[d + ec.SPAN[eid]]) if eid else int(s[d])
            streams.append(hc.noise(rng, 11) + rc.frame_bits(p, tuple(88 + k for k in range(16) if (syn >> k) & 1)) + [0])
    got = check(11, 64, [[np.asarray(x, np.uint8) for x in streams]], {11: None}, ec.ALL, streams)
    assert [len(g) for g in got] == [1, 0, 0, 0] * 3
    # the 1000-octet frame: more than one pass, the open frame carried through them
    for d in (0, 700):
        x, p, first = ec.collision_stream(rng, d)
        got = check(11, 1024, [[np.asarray(x, np.uint8)]], {998: None}, ec.ALL, [x])
        assert [f for _, _, f in got[0]] == [ec.mark(first, 1)]
        cut = len(x) // 2
        check(11, 1024, hc.split_calls([x], [[cut]]), {998: None}, ec.SKIP, [x])


def test_lane_model_across_a_pass_and_every_call_boundary():
    rng = np.random.default_rng(44)
    p = rc.typed_payload(rng, 21, 3)
    fb = ec.event_frame(p, 63, 1)  # the pair sits in octets 7 and 8
    body = hc.junk(rng, 4096 - 100) + fb + hc.noise(rng, 20)
    got = check(11, 64, [[np.asarray(body, np.uint8)]], R21, ec.ALL, [body])
    assert [(q, f) for _, q, f in got[0]] == [(p, ec.mark(63, 1))]
    s = hc.noise(rng, 30) + fb + hc.noise(rng, 12)
    L = len(s)
    streams = [s] * (L + 1)
    got = check(11, 64, hc.split_calls(streams, [[c, min(L, c + c % 3)] for c in range(L + 1)]), R21, ec.ALL, streams)
    assert all((p, ec.mark(63, 1)) in [(q, f) for _, q, f in g] for g in got)


def test_lane_model_frames_sharing_a_flag_and_four_in_a_word():
    rng = np.random.default_rng(45)
    a, b = rc.typed_payload(rng, 21, 1), rc.typed_payload(rng, 21, 4)
    for (fa, ea), (fb, eb) in (((60, 1), (171, 2)), ((0, 2), (182, 1)), ((166, 2), (7, 1))):
        s = hc.noise(rng, 40) + ec.event_frame(a, fa, ea)[:-8] + ec.event_frame(b, fb, eb) + hc.noise(rng, 9)
        got = check(11, 64, [[np.asarray(s, np.uint8)] * 2], R21, ec.ALL, [s, s])
        assert [(q, f) for _, q, f in got[0]] == [(a, ec.mark(fa, ea)), (b, ec.mark(fb, eb))]
    # four minimal frames closing in one 64-bit word (delimiters at its bits 0, 21, 42 and 63), each repaired: the four
    # 16-bit slots of a lane's fixes word all in use; and at other alignments, three and one, two and two
    for lead in (64 * 3 - 27, 64 * 3 - 27 + 1, 64 * 2 - 27 + 30, 64 * 63 - 27, 64 * 64 - 27):
        s, m = four_in_a_word(rng, lead)
        got = check(2, 64, [[np.asarray(s, np.uint8)]], {0: None}, ec.ALL, [s])
        four = [(e, q, f) for e, q, f in got[0] if f >= 0]
        assert [(q, f) for _, q, f in four] == [(b"", m)] * 4 and [e for e, _, _ in four] == [lead + 27 + 21 * k for k in range(4)]
    assert host(s, {0: None}, ec.SINGLE, 2, 64)[1].count(m) == 0


def test_lane_model_switches_between_calls():
    rng = np.random.default_rng(46)
    p, q = rc.typed_payload(rng, 21, 1), rc.typed_payload(rng, 21, 2)
    s = hc.noise(rng, 25) + ec.event_frame(p, 17, 1) + hc.noise(rng, 33) + ec.event_frame(q, 140, 2) + hc.noise(rng, 8)
    first = 25 + 8 + 60  # inside the first frame
    second = len(s) - 8 - 8 - 50  # inside the second
    streams, cuts = [s, s], [[first, first], [second, second]]
    calls = hc.split_calls(streams, cuts)
    # off -> all events at call 1: the frame open at the switch is repaired (what holds when a frame closes decides)
    got = check(11, 64, calls, None, ec.SINGLE, streams, switch_call=1, switch_rules=R21, switch_events=ec.ALL, switch_pos=[first, second])
    assert [(x, f) for _, x, f in got[0]] == [(p, ec.mark(17, 1)), (q, ec.mark(140, 2))]
    assert [(x, f) for _, x, f in got[1]] == [(q, ec.mark(140, 2))]
    # pair only -> skip only; all -> the single event (the single-bit body and its table) -> nothing found; all -> off
    got = check(11, 64, calls, R21, ec.PAIR, streams, switch_call=1, switch_rules=R21, switch_events=ec.SKIP, switch_pos=[first, second])
    assert [(x, f) for _, x, f in got[0]] == [(q, ec.mark(140, 2))] and [(x, f) for _, x, f in got[1]] == [(p, ec.mark(17, 1)), (q, ec.mark(140, 2))]
    got = check(11, 64, calls, R21, ec.ALL, streams, switch_call=1, switch_rules=R21, switch_events=ec.SINGLE, switch_pos=[first, second])
    assert [(x, f) for _, x, f in got[0]] == [] and [(x, f) for _, x, f in got[1]] == [(p, ec.mark(17, 1))]
    got = check(11, 64, calls, R21, ec.ALL, streams, switch_call=1, switch_rules=None, switch_events=ec.ALL, switch_pos=[first, second])
    assert [(x, f) for _, x, f in got[0]] == [] and [(x, f) for _, x, f in got[1]] == [(p, ec.mark(17, 1))]


def test_lane_model_overflow_keeps_a_prefix_with_its_marks():
    rng = np.random.default_rng(47)
    streams = [ec.event_stream(rng, 4000, rc.AIS_RULES, every=150) for _ in range(5)]
    calls = [[np.asarray(s, np.uint8) for s in streams]]
    full = run_model(11, 64, calls, rc.AIS_RULES, ec.ALL)
    flat = [(c,) + t for c in range(5) for t in full[c]]
    assert len(flat) > 9 and sum(t[3] >= 1 << 16 for t in flat[:9]) >= 1
    b = EmuBatch(11, 64, 5, max(len(s) for s in streams) + 1, max_pdus=9, rules=rc.AIS_RULES, events=ec.ALL)
    b.process(calls[0])
    found, bad, recs, data, fix = b.read()
    assert found == len(flat) and len(recs) == 9 and bad == 0
    assert [(c,) + t for c in range(5) for t in rc.by_channel(recs, data, fix, 5)[c]] == flat[:9]


def test_lane_model_single_mask_on_the_single_bit_cases():
    """hdlc_repair_cases' streams under the mask SINGLE: the results and marks of the single-bit repair"""
    import test_hdlc_repair_model as old

    rng = np.random.default_rng(48)
    streams = [rc.repair_stream(rng, 7000, rc.AIS_RULES, every=300) for _ in range(4)]
    cuts = [sorted(rng.integers(0, 7000, 2)) for _ in range(4)]
    calls = hc.split_calls(streams, cuts)
    got = check(11, 64, calls, rc.AIS_RULES, ec.SINGLE, streams, pad_front=3)
    assert got == old.run_model(11, 64, calls, rc.AIS_RULES, pad_front=3)
    assert [[(p, f) for _, p, f in g] for g in got] == rc.host_ref(11, 64, calls, rc.AIS_RULES)
    assert all(g == rc.py_ref(11, 64, s, rc.AIS_RULES) for g, s in zip(got, streams))
    assert sum(f >= 0 for g in got for _, _, f in g) >= 10


def test_sanitizer_program_runs_clean():
    """tests/emul_hdlc `make san`: the host form and the lane model side by side in a stand-alone program under
    AddressSanitizer and UndefinedBehaviorSanitizer"""
    subprocess.check_call(["make", "-C", EMUL, "-s", "san"])
    r = subprocess.run([os.path.join(EMUL, "events_san")], capture_output=True, text=True)
    assert r.returncode == 0 and "events_san ok" in r.stdout, r.stdout + r.stderr
