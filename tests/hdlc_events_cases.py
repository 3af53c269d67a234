"""Cases for the HDLC deframers' repair of one error event (tests/test_hdlc_events_model.py on the host form and the CPU
lane model, tests/test_gpu_hdlc_events.py on the device): a Python restatement of the host rule
(aisx_hdlc_set_repair_events, include/aisx.h) that also tells each frame's end bit, frames with planted events, and
streams of them in noise.

The restatement does not use the product's tables or the shift-register form of the syndromes: for a frame length it
computes the FCS check of every frame that differs from the all-zero frame in one bit (numpy, all positions at once),
takes an event's syndrome as the xor of its bits' by the CRC's linearity, and among the enabled events INSIDE the frame
that give a failed frame's syndrome picks the one whose last flipped bit is nearest the frame's end."""
import numpy as np

import hdlc_cases as hc
import hdlc_repair_cases as rc

SINGLE, PAIR, SKIP, ALL = 1, 2, 4, 7
MASKS = (1, 2, 3, 4, 5, 6, 7)
SPAN = (0, 1, 2)  # by event id
PATTERN = ((1,), (1, 1), (1, 0, 1))

_TABLE = np.zeros(256, dtype=np.int64)
for _v in range(256):
    _r = _v
    for _ in range(8):
        _r = (_r >> 1) ^ (0x8408 if _r & 1 else 0)
    _TABLE[_v] = _r
_BITS = {}
_EVENTS = {}


def bit_syndromes(got):
    """int array [8 * got]: (FCS check of the frame of `got` octets with only bit i set) xor (that of the all-zero
    frame) -- the linear part of the check: the CRC register started at 0 over the payload, xor the sent FCS"""
    if got not in _BITS:
        n, pl = 8 * got, got - 2
        reg = np.zeros(n, dtype=np.int64)
        idx = np.arange(n)
        for k in range(pl):
            byte = np.where(idx >> 3 == k, 1 << (idx & 7), 0)
            reg = (reg >> 8) ^ _TABLE[(reg ^ byte) & 0xFF]
        sent = np.where(idx >> 3 == pl, 1 << (idx & 7), 0) | np.where(idx >> 3 == pl + 1, 256 << (idx & 7), 0)
        _BITS[got] = reg ^ sent
    return _BITS[got]


def event_errors(got, events):
    """{syndrome: (first flipped bit, event id)} of the frames of `got` octets with one enabled event inside: where two
    give the same syndrome, the one whose last flipped bit is nearer the frame's end"""
    key = (got, events)
    if key not in _EVENTS:
        s = bit_syndromes(got)
        n = 8 * got
        best = {}
        for eid in range(3):
            if not (events >> eid) & 1:
                continue
            sp = SPAN[eid]
            syn = s[: n - sp] ^ s[sp:] if sp else s
            for first in range(n - sp):
                d = n - 1 - (first + sp)
                v = int(syn[first])
                assert v != 0
                if v not in best or d < best[v][0]:
                    assert v not in best or best[v][0] != d
                    best[v] = (d, first, eid)
        _EVENTS[key] = {v: (first, eid) for v, (d, first, eid) in best.items()}
    return _EVENTS[key]


def mark(first, eid):
    return first | (eid << 16)


def flips_of(m):
    """a mark -> the flipped bit indices"""
    first, eid = m & 0xFFFF, m >> 16
    return (first,) if eid == 0 else (first, first + SPAN[eid])


def py_ref(lmin, lmax, bits, rules=None, events=SINGLE, switch=None):
    """aisx_hdlc_work_repair on a handle with aisx_hdlc_set_repair_events(rules, events), restated bit by bit:
    [(end_bit, payload bytes, mark)]; switch = (bit position, rules, events): what holds from that position on"""
    m = rc.masks(rules)
    ones, frame, shift, nshift, res = 0, [], 0, 0, []
    for i, b in enumerate(bits):
        if switch is not None and i == switch[0]:
            m, events = rc.masks(switch[1]), switch[2]
        bit = 1 if b else 0
        if ones < 5:
            if len(frame) > lmax:
                frame, shift, nshift = [], 0, 0
            else:
                shift = (shift >> 1) | (0x80 if bit else 0)
                nshift += 1
                if nshift == 8:
                    frame.append(shift)
                    shift, nshift = 0, 0
        elif bit:
            got = len(frame)
            if got >= lmin:
                pl = got - 2
                s = rc.syndrome(frame)
                if s == 0:
                    res.append((i, bytes(frame[:pl]), -1))
                elif pl in m:
                    hit = event_errors(got, events).get(s)
                    if hit is not None:
                        f = list(frame)
                        for j in flips_of(mark(*hit)):
                            f[j >> 3] ^= 1 << (j & 7)
                        if (m[pl] >> (f[0] >> 2)) & 1:
                            res.append((i, bytes(f[:pl]), mark(*hit)))
            frame, shift, nshift = [], 0, 0
        ones = ones + 1 if bit else 0
    return res


def event_frame(payload, first=None, eid=0, more=()):
    """hdlc_repair_cases.frame_bits with event `eid` planted at bit `first` (None: intact) and the bits `more` flipped"""
    flips = () if first is None else flips_of(mark(first, eid))
    return rc.frame_bits(payload, tuple(flips) + tuple(more))


def host_ref(lmin, lmax, calls, rules=None, events=SINGLE, switch_call=None, switch_rules=None, switch_events=SINGLE):
    """one ais_amd.hdlc_deframer_bp per channel fed call by call (set_repair(switch_rules, switch_events) before call
    switch_call): per channel [(payload bytes, mark)]"""
    import ais_amd

    nch = len(calls[0])
    hs = [ais_amd.hdlc_deframer_bp(lmin, lmax, repair=rules, events=events) for _ in range(nch)]
    out = [[] for _ in range(nch)]
    for k, call in enumerate(calls):
        for c in range(nch):
            if k == switch_call:
                hs[c].set_repair(switch_rules, switch_events)
            p, f = hs[c].work(call[c], with_repairs=True)
            out[c] += list(zip(p, f))
    return out


def event_stream(rng, nbits, rules, every=700, raw_flips=0):
    """noise with frames of the rules' lengths and types (and some other lengths): intact, one planted event of each
    kind anywhere, at the frame's first bits (the type bits), at its last, across the payload / FCS boundary, one event
    and one more wrong bit, two events; raw_flips more inversions at random places of the stuffed stream"""
    m = rc.masks(rules)
    lens = sorted(m) + [17, 30]
    s = []
    while len(s) < nbits:
        s += hc.noise(rng, int(rng.integers(0, every)))
        octets = int(lens[int(rng.integers(0, len(lens)))])
        allowed = [t for t in range(64) if (m.get(octets, rc.ANY) >> t) & 1]
        p = rc.typed_payload(rng, octets, int(allowed[int(rng.integers(0, len(allowed)))]))
        n = 8 * (octets + 2)
        eid = int(rng.integers(0, 3))
        sp = SPAN[eid]
        kind = int(rng.integers(0, 10))
        if kind == 0:
            s += event_frame(p)
        elif kind == 1:
            s += event_frame(p, int(rng.integers(0, 8 - sp)), eid)
        elif kind == 2:
            s += event_frame(p, n - 1 - sp, eid)
        elif kind == 3:
            s += event_frame(p, 8 * octets - 1 - int(rng.integers(0, sp + 1)), eid)
        elif kind == 4:
            s += event_frame(p, int(rng.integers(0, n - sp)), eid, more=(int(rng.integers(0, n)),))
        elif kind == 5:
            a = int(rng.integers(0, n - 8))
            s += event_frame(p, a, eid, more=flips_of(mark(int(rng.integers(a + 3, n - 2)), int(rng.integers(0, 3)))))
        else:
            s += event_frame(p, int(rng.integers(0, n - sp)), eid)
    for _ in range(raw_flips):
        s[int(rng.integers(0, len(s)))] ^= 1
    return s


def collision_stream(rng, d, octets=1000):
    """a frame of `octets` octets (payload octets - 2, any type) with a SKIP planted 7140 + d bits before its last bit,
    between flags in noise; returns (stream, payload, the first bit of the PAIR at distance d that shares the syndrome)"""
    p = rc.typed_payload(rng, octets - 2, 1)
    n = 8 * octets
    last = n - 1 - (7140 + d)
    s = hc.noise(rng, 40) + event_frame(p, last - 2, 2) + hc.noise(rng, 30)
    return s, p, n - 1 - d - 1
