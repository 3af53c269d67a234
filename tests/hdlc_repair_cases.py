"""Cases for the HDLC deframer's single-bit repair (tests/test_hdlc_repair_model.py on the host form and the CPU lane
model, tests/test_gpu_hdlc_repair.py on the device): frames with chosen wrong bits, and a Python restatement of the host
rule (aisx_hdlc_set_repair, include/aisx.h) that also tells each frame's end bit.

The restatement does not use the product's syndrome table: for a frame length it computes the CRC of every frame that
differs from the all-zero frame in one bit, which by the CRC's linearity is the table's content for that length."""
import numpy as np

import hdlc_cases as hc
import synth

ANY = (1 << 64) - 1
RULE_DTYPE = np.dtype([("payload_octets", "<i4"), ("reserved", "<i4"), ("type_mask", "<u8")])
# ITU-R M.1371 fixed lengths (the issue's table; ais_amd.AIS_REPAIR_RULES must say the same)
AIS_RULES = {21: (1, 2, 3, 4, 9, 11, 18, 24), 53: (5,), 39: (19,), 20: (24,), 12: (27,)}


def masks(rules):
    """{payload octets: types or None / int mask} -> {payload octets: int mask}"""
    out = {}
    for octets, types in (rules or {}).items():
        if types is None:
            types = ANY
        if not isinstance(types, int):
            types = sum(1 << t for t in types)
        out[int(octets)] = types
    return out


def rule_array(rules):
    m = masks(rules)
    a = np.zeros(len(m), dtype=RULE_DTYPE)
    for k, (octets, mask) in enumerate(m.items()):
        a[k] = (octets, 0, mask)
    return a


def crc(octs):
    reg = 0xFFFF
    for o in octs:
        reg ^= o
        for _ in range(8):
            reg = (reg >> 1) ^ (0x8408 if reg & 1 else 0)
    return ~reg & 0xFFFF


def syndrome(frame):
    pl = len(frame) - 2
    return crc(frame[:pl]) ^ (frame[pl] | (frame[pl + 1] << 8))


_SINGLE = {}


def single_errors(got):
    """{syndrome: bit index} of the frames of `got` octets with one wrong bit"""
    if got not in _SINGLE:
        zero = syndrome([0] * got)
        tab = {}
        for i in range(8 * got):
            f = [0] * got
            f[i >> 3] = 1 << (i & 7)
            s = syndrome(f) ^ zero
            assert s not in tab and s != 0  # (every position has its own: frames here are far below 32767 bits)
            tab[s] = i
        _SINGLE[got] = tab
    return _SINGLE[got]


def py_ref(lmin, lmax, bits, rules=None, switch=None):
    """aisx_hdlc_work_repair restated bit by bit: [(end_bit, payload bytes, fix_bit)]; switch = (bit position, rules):
    the rules that hold from that position of the stream on (set_repair between two calls)"""
    m = masks(rules)
    ones, frame, shift, nshift, res = 0, [], 0, 0, []
    for i, b in enumerate(bits):
        if switch is not None and i == switch[0]:
            m = masks(switch[1])
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
                s = syndrome(frame)
                if s == 0:
                    res.append((i, bytes(frame[:pl]), -1))
                elif pl in m:
                    j = single_errors(got).get(s)
                    if j is not None:
                        f = list(frame)
                        f[j >> 3] ^= 1 << (j & 7)
                        if (m[pl] >> (f[0] >> 2)) & 1:
                            res.append((i, bytes(f[:pl]), j))
            frame, shift, nshift = [], 0, 0
        ones = ones + 1 if bit else 0
    return res


def frame_bits(payload, flips=()):
    """hdlc_cases.frame_bits with the frame's bits `flips` (indices into payload + FCS, bit 0 the first sent) inverted
    before stuffing; the FCS is the original payload's"""
    bits = hc.octets_to_bits(payload)
    bits = bits + list(synth.crc16_hdlc(bits))
    for i in flips:
        bits[i] ^= 1
    return hc.FLAG + synth.bit_stuff(bits) + hc.FLAG


def typed_payload(rng, octets, msg_type):
    """random payload octets whose message type (pdu[0] >> 2) is msg_type"""
    p = rng.integers(0, 256, octets).astype(np.uint8)
    p[0] = (msg_type << 2) | (int(p[0]) & 3)
    return bytes(p)


def host_ref(lmin, lmax, calls, rules=None, switch_call=None, switch_rules=None):
    """one ais_amd.hdlc_deframer_bp per channel fed call by call (set_repair(switch_rules) before call switch_call):
    per channel [(payload bytes, fix_bit)]"""
    import ais_amd

    nch = len(calls[0])
    hs = [ais_amd.hdlc_deframer_bp(lmin, lmax, repair=rules) for _ in range(nch)]
    out = [[] for _ in range(nch)]
    for k, call in enumerate(calls):
        for c in range(nch):
            if k == switch_call:
                hs[c].set_repair(switch_rules)
            p, f = hs[c].work(call[c], with_repairs=True)
            out[c] += list(zip(p, f))
    return out


def by_channel(recs, data, fix, nch):
    """hdlc_cases.by_channel with the marks: per channel [(end_bit, bytes, fix_bit)]"""
    plain = hc.by_channel(recs, data, nch)
    out, k = [[] for _ in range(nch)], 0
    for c in range(nch):
        for e, p in plain[c]:
            out[c].append((e, p, int(fix[k])))
            k += 1
    return out


def repair_stream(rng, nbits, rules, lmin=11, lmax=64, every=700, raw_flips=0):
    """noise with frames of the rules' lengths and types (and some other lengths): intact, one wrong bit, two wrong
    bits, a wrong bit on a type bit; raw_flips more inversions at random places of the stuffed stream"""
    m = masks(rules)
    lens = sorted(m) + [17, 30]
    s = []
    while len(s) < nbits:
        s += hc.noise(rng, int(rng.integers(0, every)))
        octets = int(lens[int(rng.integers(0, len(lens)))])
        allowed = [t for t in range(64) if (m.get(octets, ANY) >> t) & 1]
        p = typed_payload(rng, octets, int(allowed[int(rng.integers(0, len(allowed)))]))
        kind = int(rng.integers(0, 6))
        n = 8 * (octets + 2)
        flips = {0: (), 1: (int(rng.integers(0, n)),), 2: (int(rng.integers(0, n)),), 3: (int(rng.integers(0, n)),),
                 4: tuple(int(v) for v in rng.choice(n, 2, replace=False)), 5: (int(rng.integers(2, 8)),)}[kind]
        s += frame_bits(p, flips)
    for _ in range(raw_flips):
        s[int(rng.integers(0, len(s)))] ^= 1
    return s
