"""Single-bit repair by CRC syndrome in the HDLC deframers, -m "not gpu": the host form (aisx_hdlc_set_repair /
aisx_hdlc_work_repair, ais_amd.hdlc_deframer_bp(repair=...)) against the Python restatement of its rule
(tests/hdlc_repair_cases.py), and the kernel bodies of gr-ais_amd/csrc/k_hdlc.h with the repair compiled in, on the CPU
lane model (tests/emul_hdlc), against the host form bit for bit, marks included."""

import numpy as np
import pytest

import hdlc_cases as hc
import hdlc_repair_cases as rc
import test_hdlc_batch_model as plain
import torch  # noqa: F401  (before libaisx.so: one HIP runtime in the process)

R21 = {21: (1, 2, 3, 4, 9, 11, 18, 24)}


def emu():
    L = hc.emu()
    assert L.emu_hdlc_rule_size() == rc.RULE_DTYPE.itemsize
    return L


class EmuBatch:
    def __init__(self, lmin, lmax, nch, max_bits, max_pdus=4096, rules=None):
        self.h = emu().emu_hdlc_create(lmin, lmax, nch, max_bits, max_pdus)
        assert self.h
        self.nch, self.max_pdus, self.lmax, self.max_bits = nch, max_pdus, lmax, max_bits
        self.set_repair(rules)

    def __del__(self):
        emu().emu_hdlc_destroy(self.h)

    def set_repair(self, rules):
        a = rc.rule_array(rules)
        emu().emu_hdlc_set_repair(self.h, a.ctypes.data if a.size else None, a.size, 1)

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


def run_model(lmin, lmax, calls, rules, pad_front=0, max_pdus=4096, switch_call=None, switch_rules=None):
    nch = len(calls[0])
    b = EmuBatch(lmin, lmax, nch, max(max(len(x) for x in call) for call in calls) + 1, max_pdus, rules)
    got = [[] for _ in range(nch)]
    for k, call in enumerate(calls):
        if k == switch_call:
            b.set_repair(switch_rules)
        b.process(call, pad_front)
        found, bad, recs, data, fix = b.read()
        assert bad == 0 and found == len(recs)
        for c, lst in enumerate(rc.by_channel(recs, data, fix, nch)):
            got[c] += lst
    return got


def check(lmin, lmax, calls, rules, streams=None, pad_front=0, switch_call=None, switch_rules=None, switch_pos=None):
    """the lane model against the host form (payloads and marks) and, given the streams, the restatement (end bits too)"""
    got = run_model(lmin, lmax, calls, rules, pad_front, switch_call=switch_call, switch_rules=switch_rules)
    ref = rc.host_ref(lmin, lmax, calls, rules, switch_call, switch_rules)
    for c in range(len(got)):
        assert [(p, f) for _, p, f in got[c]] == ref[c], c
        if streams is not None:
            sw = (switch_pos[c], switch_rules) if switch_pos is not None else None
            assert got[c] == rc.py_ref(lmin, lmax, streams[c], rules, sw), c
    return got


def host(bits, rules, lmin=11, lmax=64):
    import ais_amd

    return ais_amd.hdlc_deframer_bp(lmin, lmax, repair=rules).work(np.asarray(bits, np.uint8), with_repairs=True)


# ---- the host form against the restatement -----------------------------------------------------------------------------


def test_every_single_bit_of_a_frame_is_repaired_on_the_host():
    import ais_amd

    rng = np.random.default_rng(11)
    payload = rc.typed_payload(rng, 21, 18)
    lead = hc.noise(rng, 23)
    for i in range(184):
        bits = lead + rc.frame_bits(payload, (i,)) + [0, 1, 0]
        want = rc.py_ref(11, 64, bits, R21)
        pdus, fix = host(bits, R21)
        assert list(zip(pdus, fix)) == [(p, f) for _, p, f in want], i
        # the original payload, the flipped index (an FCS bit: the payload as received) -- a wrong type bit too: the
        # rule looks at the type AFTER the flip, which is the sent one again
        assert [w[1:] for w in want] == [(payload, i)], i
        assert host(bits, None) == ([], [])     # no rules: nothing
        assert ais_amd.hdlc_deframer_bp(11, 64).work(np.asarray(bits, np.uint8)) == []
        assert ais_amd.hdlc_deframer_bp(11, 64, repair=R21).work(np.asarray(bits, np.uint8)) == [payload]
    # a frame SENT with a type the rule does not allow stays out, also where one wrong type bit makes the received
    # type an allowed one (19 -> 18, 3, 11 ...): the restatement decides, the host agrees
    other = rc.typed_payload(rng, 21, 19)
    for i in range(184):
        bits = lead + rc.frame_bits(other, (i,)) + [0, 1, 0]
        assert rc.py_ref(11, 64, bits, R21) == [] and host(bits, R21) == ([], []), i
    assert host(lead + rc.frame_bits(other, (2,)) + [0], {21: None}) == ([other], [2])


def test_rules_on_the_host():
    import ais_amd
    from ais_amd import _lib

    rng = np.random.default_rng(12)
    lead = hc.noise(rng, 31)
    p21, p30 = rc.typed_payload(rng, 21, 1), rc.typed_payload(rng, 30, 1)
    # a length without a rule
    bits = lead + rc.frame_bits(p30, (77,)) + lead + rc.frame_bits(p21, (77,)) + [0]
    assert host(bits, R21) == ([p21], [77])
    assert host(bits, {21: (1,), 30: None}) == ([p30, p21], [77, 77])
    # a type outside the mask after the flip; a mask of all ones allows any content
    p7 = rc.typed_payload(rng, 21, 7)
    bits = lead + rc.frame_bits(p7, (100,)) + [0]
    assert host(bits, R21) == ([], []) and rc.py_ref(11, 64, bits, R21) == []
    assert host(bits, {21: None}) == ([p7], [100])
    assert host(lead + rc.frame_bits(p7) + [0], R21) == ([p7], [-1])  # (an intact frame is never subject to the rules)
    # two wrong bits: whatever comes out, host and restatement agree
    seen = 0
    for _ in range(300):
        a, b = (int(v) for v in rng.choice(184, 2, replace=False))
        bits = lead + rc.frame_bits(p21, (a, b)) + [0]
        want = rc.py_ref(11, 64, bits, {21: None})
        pdus, fix = host(bits, {21: None})
        assert list(zip(pdus, fix)) == [(p, f) for _, p, f in want]
        seen += len(want)
        assert all(p != p21 or f >= 168 for _, p, f in want)
    print("two wrong bits in 184: %d of 300 frames miscorrected" % seen)
    # bad rules are refused and leave the handle as it was
    d = ais_amd.hdlc_deframer_bp(11, 64, repair=R21)
    ok = lead + rc.frame_bits(p21, (5 * 8,)) + [0]
    for bad in ({8: None}, {63: None}, {21: None, 62: None, 9: None, 8: None}, {k: None for k in range(9, 26)}):
        with pytest.raises(ValueError):
            d.set_repair(bad)
    dup = np.zeros(2, rc.RULE_DTYPE)
    dup["payload_octets"] = 21
    with pytest.raises(ValueError):
        d.set_repair(dup)
    res = rc.rule_array({21: None})
    res["reserved"] = 1
    with pytest.raises(ValueError):
        d.set_repair(res)
    L = _lib.lib(device=False)
    assert L.aisx_hdlc_set_repair(d._h, None, 1) == _lib.AISX_ERR_INVALID
    assert L.aisx_hdlc_set_repair(None, None, 0) == _lib.AISX_ERR_INVALID
    assert d.work(np.asarray(ok, np.uint8), with_repairs=True) == ([p21], [40])
    d.set_repair({k: None for k in range(9, 25)})  # 16 rules, lengths 9 .. 62 are the limits
    d.set_repair({9: None, 62: None})
    d.set_repair(None)
    assert d.work(np.asarray(ok, np.uint8), with_repairs=True) == ([], [])
    assert {k: tuple(v) for k, v in ais_amd.AIS_REPAIR_RULES.items()} == rc.AIS_RULES
    assert np.array_equal(ais_amd.framing.repair_rules(ais_amd.AIS_REPAIR_RULES), rc.rule_array(rc.AIS_RULES))


# ---- the lane model against the host form ------------------------------------------------------------------------------


def test_repaired_and_intact_frames_in_noise():
    rng = np.random.default_rng(13)
    streams = [rc.repair_stream(rng, 9000, rc.AIS_RULES) for _ in range(5)]
    cuts = [sorted(rng.integers(0, 9000, 2)) for _ in range(5)]
    calls = [[hc.as_bytes(rng, b, wild=(c % 2 == 1)) for c, b in enumerate(call)] for call in hc.split_calls(streams, cuts)]
    got = check(11, 64, calls, rc.AIS_RULES, streams)
    nfix = sum(f >= 0 for g in got for _, _, f in g)
    nfcs = sum(f >= 8 * len(p) for g in got for _, p, f in g)
    print("frames in noise: %d PDUs, %d repaired (%d in the FCS)" % (sum(len(g) for g in got), nfix, nfcs))
    assert nfix >= 10 and nfcs >= 1 and sum(f < 0 for g in got for _, _, f in g) >= 5
    # the same streams with length-only rules and another deframer geometry
    check(9, 40, calls, {21: None, 12: None, 20: None, 17: None}, streams)


def test_raw_domain_flips():
    # inversions on the stuffed stream change flags and stuffing too: equality with the host form is the only claim
    rng = np.random.default_rng(14)
    streams = [rc.repair_stream(rng, 7000, rc.AIS_RULES, every=200, raw_flips=60) for _ in range(6)]
    cuts = [sorted(rng.integers(0, 7000, 2)) for _ in range(6)]
    got = check(11, 64, hc.split_calls(streams, cuts), {k: None for k in rc.AIS_RULES}, streams)
    assert sum(f >= 0 for g in got for _, _, f in g) >= 5


def test_repaired_frame_across_a_pass_and_every_call_boundary():
    rng = np.random.default_rng(15)
    p = rc.typed_payload(rng, 21, 3)
    fb = rc.frame_bits(p, (90,))
    # the frame straddles bit 4096 of the call (the kernel's pass boundary) ...
    body = hc.junk(rng, 4096 - 100) + fb + hc.noise(rng, 20)
    got = check(11, 64, [[np.asarray(body, np.uint8)]], R21, [body])
    assert [(q, f) for _, q, f in got[0]] == [(p, 90)]
    # ... and a call boundary at every offset across it: channel c's first call ends c bits into the stream
    s = hc.noise(rng, 30) + fb + hc.noise(rng, 12)
    L = len(s)
    streams = [s] * (L + 1)
    got = check(11, 64, hc.split_calls(streams, [[c, min(L, c + c % 3)] for c in range(L + 1)]), R21, streams)
    assert all((p, 90) in [(q, f) for _, q, f in g] for g in got)


def test_two_frames_sharing_a_flag_one_repaired():
    rng = np.random.default_rng(16)
    a, b = rc.typed_payload(rng, 21, 1), rc.typed_payload(rng, 21, 4)
    for fa, fb in (((60,), ()), ((), (171,)), ((3,), (183,))):
        s = hc.noise(rng, 40) + rc.frame_bits(a, fa)[:-8] + rc.frame_bits(b, fb) + hc.noise(rng, 9)
        got = check(11, 64, [[np.asarray(s, np.uint8)] * 2], R21, [s, s])
        assert [(q, f) for _, q, f in got[0]] == [(a, fa[0] if fa else -1), (b, fb[0] if fb else -1)]


def test_misaligned_rows():
    rng = np.random.default_rng(17)
    streams = [rc.repair_stream(rng, 5000, rc.AIS_RULES, every=300) for _ in range(4)]
    calls = hc.split_calls(streams, [sorted(rng.integers(0, 5000, 2)) for _ in range(4)])
    for pad in (1, 5, 15):
        check(11, 64, calls, rc.AIS_RULES, streams, pad_front=pad)


def test_set_repair_between_calls_with_a_frame_open():
    rng = np.random.default_rng(18)
    p, q = rc.typed_payload(rng, 21, 1), rc.typed_payload(rng, 21, 2)
    s = hc.noise(rng, 25) + rc.frame_bits(p, (17,)) + hc.noise(rng, 33) + rc.frame_bits(q, (140,)) + hc.noise(rng, 8)
    first = 25 + 8 + 60  # inside the first frame
    second = len(s) - 8 - 8 - 50  # inside the second
    streams, cuts = [s, s], [[first, first], [second, second]]
    calls = hc.split_calls(streams, cuts)
    # off -> on at call 1: the frame open at the switch is repaired (the rules apply when a frame closes)
    got = check(11, 64, calls, None, streams, switch_call=1, switch_rules=R21, switch_pos=[first, second])
    assert [(x, f) for _, x, f in got[0]] == [(p, 17), (q, 140)] and [(x, f) for _, x, f in got[1]] == [(q, 140)]
    # on -> off at call 1
    got = check(11, 64, calls, R21, streams, switch_call=1, switch_rules=None, switch_pos=[first, second])
    assert [(x, f) for _, x, f in got[0]] == [] and [(x, f) for _, x, f in got[1]] == [(p, 17)]


def test_overflow_keeps_a_prefix_with_its_marks():
    rng = np.random.default_rng(19)
    streams = [rc.repair_stream(rng, 4000, rc.AIS_RULES, every=150) for _ in range(5)]
    calls = [[np.asarray(s, np.uint8) for s in streams]]
    full = run_model(11, 64, calls, rc.AIS_RULES)
    flat = [(c,) + t for c in range(5) for t in full[c]]
    assert len(flat) > 9 and sum(t[3] >= 0 for t in flat[:9]) >= 1
    b = EmuBatch(11, 64, 5, max(len(s) for s in streams) + 1, max_pdus=9, rules=rc.AIS_RULES)
    b.process(calls[0])
    found, bad, recs, data, fix = b.read()
    assert found == len(flat) and len(recs) == 9 and bad == 0
    assert [(c,) + t for c in range(5) for t in rc.by_channel(recs, data, fix, 5)[c]] == flat[:9]


# ---- the off path ------------------------------------------------------------------------------------------------------


def test_without_rules_the_results_are_those_of_the_plain_model():
    rng = np.random.default_rng(20)
    cases = []
    streams = [hc.ais_stream(rng, 5)[0] for _ in range(4)]
    cases.append((11, 64, hc.split_calls(streams, [sorted(rng.integers(0, len(s), 2)) for s in streams])))
    for lmin, lmax in ((11, 64), (2, 9)):
        cases.append((lmin, lmax, [[hc.as_bytes(rng, hc.adversarial_stream(rng, lmin, lmax), wild=True) for _ in range(3)]]))
    s, cuts = hc.period_cases(rng, 30, 2, bytes(rng.integers(0, 256, 20).astype(np.uint8)))
    cases.append((11, 30, hc.split_calls(s, cuts)))
    n = 0
    for lmin, lmax, calls in cases:
        want = plain.run_model(lmin, lmax, calls)
        got = run_model(lmin, lmax, calls, None)
        assert [[(e, p) for e, p, _ in g] for g in got] == want
        assert all(f == -1 for g in got for _, _, f in g)
        n += sum(len(g) for g in got)
    assert n >= 30
    # a handle that had rules and lost them: the marks of an earlier call do not stay behind
    sr = rc.repair_stream(rng, 3000, rc.AIS_RULES, every=100)
    b = EmuBatch(11, 64, 1, len(sr) + 1, rules=rc.AIS_RULES)
    b.process([np.asarray(sr, np.uint8)])
    assert (b.read()[4] >= 0).any()
    b.set_repair(None)
    b.process([np.asarray(streams[0], np.uint8)])
    assert len(b.read()[4]) >= 4 and (b.read()[4] == -1).all()
