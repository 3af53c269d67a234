"""PDU lists for the standard-form NMEA armouring's tests (tests/test_nmea_std_model.py on the CPU lane model,
tests/test_gpu_nmea_std.py on the device), the pure-Python statement of the form (spec_sentence: include/aisx.h,
aisx_pdu_to_nmea_std) and the host reference per record, which is the specification of the device form.

A case is a dict as in nmea_cases.py -- designators, length_max, records [(chan, end_bit, payload)], optional text_cap /
npdus / nfound / max_pdus / bad -- plus stations (one per channel) and time (the call's c: value, -1 for none)."""
import numpy as np

from nmea_cases import D16, REC_DTYPE, _payload, pack, split  # noqa: F401

S15 = "STATION_15-byte"
T18 = 10 ** 18 - 1
MAX_OCTETS = 378


def spec_sentence(designator, payload, seq=0, station="", time=-1):
    """the standard form, from its statement in include/aisx.h alone (no call into the library): str"""
    n = len(payload)
    assert 1 <= n <= MAX_OCTETS and 0 <= seq <= 9 and -1 <= time < 10 ** 18 and len(station) <= 15
    P = -(-8 * n // 6)
    fill = 6 * P - 8 * n
    bits = [(payload[i // 8] >> (7 - i % 8)) & 1 for i in range(8 * n)] + [0] * fill
    chars = ""
    for k in range(P):
        v = int("".join(map(str, bits[6 * k:6 * k + 6])), 2)
        chars += chr(v + 48 if v < 40 else v + 56)
    F = -(-P // 56)

    def xor(s):
        x = 0
        for c in s.encode("latin-1"):
            x ^= c
        return "%02X" % x

    fields = ",".join(([("s:" + station)] if station else []) + ([("c:%d" % time)] if time >= 0 else []))
    tag = "\\%s*%s\\" % (fields, xor(fields)) if fields else ""
    out = []
    for f in range(1, F + 1):
        body = "AIVDM,%d,%d,%s,%s,%s,%d" % (F, f, str(seq) if F > 1 else "", designator, chars[56 * (f - 1):56 * f], fill if f == F else 0)
        out.append("%s!%s*%s" % (tag, body, xor(body)))
    return "\n".join(out)


def is_multi(payload):
    return 8 * len(payload) > 6 * 56


def host_sentence(designator, payload, seq, station, time):
    """the host function's text for one record ('' for an empty payload, which it refuses)"""
    import ais_amd

    if not len(payload):
        return ""
    nm = ais_amd.pdu_to_nmea(designator, standard=True, station=station, time=time)
    nm.next_id = seq
    return nm.msg_to_sentence(payload)


def expected(case, id0=0):
    """what a correct implementation writes, the counter standing at id0 before the call: [(chan, end_bit, text)] for the
    records kept, the whole stream, the number kept and the counter after the call"""
    des, sta, time = case["designators"], case["stations"], case.get("time", -1)
    out, stream, kept, nid = [], b"", 0, id0
    n = case.get("npdus", len(case["records"]))
    if n < 0 or n > case.get("max_pdus", len(case["records"])):
        return [], b"", 0, id0
    for c, e, p in case["records"][:n]:
        good = 0 <= c < len(des) and len(p) <= case["length_max"] - 1
        t = host_sentence(des[c], p, nid, sta[c], time) if good else ""
        add = (t + "\n").encode("latin-1") if t else b""
        if case.get("text_cap") and len(stream) + len(add) > case["text_cap"]:
            break
        out.append((c, e, t))
        stream += add
        kept += 1
        if good and is_multi(p):
            nid = (nid + 1) % 10
    return out, stream, kept, nid


def check_call(b, case):
    """one call of `case` on handle b -- the lane model's or the device's behind the same few methods (max_pdus, next_id,
    set_time, process, read) --, checked against the host function from the handle's counter on: the texts"""
    id0 = b.next_id()
    b.set_time(case.get("time", -1))
    recs, data = pack(case["records"], b.max_pdus)
    b.process(recs, data, case.get("npdus", len(case["records"])), case.get("nfound"))
    found, bad, recs, text = b.read()
    want, stream, kept, nid = expected(case, id0)
    assert bad == int(bool(case.get("bad"))), case["name"]
    assert len(recs) == kept
    n = case.get("npdus", len(case["records"]))
    assert found == (0 if n < 0 or n > b.max_pdus else case.get("nfound", n))
    got = split(recs, text)
    for g, w in zip(got, want):
        assert g == w, (case["name"], g, w)
    assert text == stream
    assert b.next_id() == nid
    assert b.read()[1] == 0  # (the flag is cleared by the read)
    return got


DES3, STA3 = ["", "B", D16], ["", "S", S15]


def every_length(rng, time=1700000000):
    """every payload length 1..378: fill counts 0 / 2 / 4, 1 to 9 fragments; designators of 0, 1 and 16 bytes with
    stations of 0, 1 and 15 bytes, so that a record's two lengths vary against each other"""
    recs = [((L + L // 3) % 3, 1000 + 7 * L, _payload(rng, L)) for L in range(1, MAX_OCTETS + 1)]
    return dict(name="every_length", designators=DES3, stations=[STA3[(c + 1) % 3] for c in range(3)], length_max=MAX_OCTETS + 1,
                records=recs, time=time)


def tails(rng):
    """payloads that end in all-ones and in all-zero bits, for each len % 3 and around the fragment edges"""
    recs = []
    for L in (1, 2, 3, 4, 5, 20, 21, 22, 41, 42, 43, 44, 53, 84, 85, 86, 377, 378):
        for tail in (b"\xff", b"\x00", b"\xff\xff", b"\x00\x00", b"\x01", b"\x80", b"\x0f", b"\x03"):
            p = (_payload(rng, L) + tail)[-L:] if L > len(tail) else tail[:L]
            recs.append((len(recs) % 3, 5 * len(recs), p))
    return dict(name="tails", designators=DES3, stations=STA3, length_max=MAX_OCTETS + 1, records=recs, time=9)


def longest_line():
    """the 135-byte line: a 43-byte tag block (15-byte station, 18-digit time), a 91-byte sentence (16-byte designator,
    56 characters, the id digit) and the newline -- and its neighbours one byte shorter in each part"""
    des, sta = [D16, D16[:15], D16], [S15, S15, S15[:14]]
    recs = [(k % 3, k, bytes([0xff - k] * L)) for k, L in enumerate((43, 43, 43, 378, 85, 84, 42, 1))]
    return dict(name="longest_line", designators=des, stations=sta, length_max=MAX_OCTETS + 1, records=recs, time=T18)


def many(rng, n, tile, time=10):
    """n short records, more than one scan tile of `tile` records, with multi-sentence records at the tile ends (the last
    records of a tile and the first of the next) and empty payloads among them"""
    des, sta = ["A", "B", "", D16], ["", "st1", S15, "x"]
    recs = []
    for i in range(n):
        at_edge = (i % tile) in (0, 1, tile - 2, tile - 1) or i == n - 1
        L = int(rng.integers(43, 60)) if at_edge else 0 if i % 97 == 5 else int(rng.integers(1, 9)) if i % 31 else int(rng.integers(43, 90))
        recs.append((i % 4, 3 * i, _payload(rng, L)))
    return dict(name="many", designators=des, stations=sta, length_max=128, records=recs, time=time)


def mixed(rng, time=-1):
    """AIS-sized records on 7 channels with empty payloads among them; every seventh record takes two sentences"""
    des = ["A", "B", "", D16, "AB", "C", "0"]
    sta = ["", "", "a", "b-_", S15, "Z9", ""]
    recs = []
    for i in range(300):
        L = 0 if i % 13 == 5 else 53 if i % 7 == 3 else int(rng.integers(1, 43))
        recs.append((i % 7, 3 * i, _payload(rng, L)))
    return dict(name="mixed", designators=des, stations=sta, length_max=64, records=recs, time=time)


def bad_records(rng):
    """a channel outside [0, nchan) and a payload longer than length_max - 1, multi-sentence ones among them: no text
    and no id for them, the others as usual, the read says INVALID once"""
    c = mixed(rng, time=0)
    recs = list(c["records"])
    recs[10] = (7, recs[10][1], _payload(rng, 53))
    recs[11] = (-1, recs[11][1], recs[11][2])
    recs[40] = (2, recs[40][1], _payload(rng, 64))
    return dict(c, name="bad_records", records=recs, bad=True)


def all_cases(rng):
    return [every_length(rng), tails(rng), longest_line(), mixed(rng), mixed(rng, time=T18), bad_records(rng)]
