"""PDU lists for the batched NMEA armouring's tests (tests/test_nmea_batch_model.py on the CPU lane model,
tests/test_gpu_nmea_batch.py on the device) and the host reference: aisx_pdu_to_nmea per record
(ais_amd.pdu_to_nmea(designator).msg_to_sentence), which is the specification.

A case is a dict: designators (one per channel), length_max, records (a list of (chan, end_bit, payload bytes) in
list order), optional text_cap / npdus (the count handed to the device, default len(records)) / nfound (a
producer's count) and what a read must then say (`bad`, `kept`)."""
import numpy as np

REC_DTYPE = np.dtype([("end_bit", "<u8"), ("offset", "<i8"), ("chan", "<i4"), ("len", "<i4")])  # aisx_pdu
D16 = "0123456789abcdef"


def host_sentence(designator, payload):
    """the host function's text for one record ('' for an empty payload, which it refuses)"""
    import ais_amd

    return ais_amd.pdu_to_nmea(designator).msg_to_sentence(payload) if len(payload) else ""


def pack(records, max_pdus=None, gap=3):
    """records -> (REC_DTYPE array [max(max_pdus, n)], payload bytes): payloads one behind the other with `gap`
    bytes between them (a reader that strays past a payload sees 0xA5, not the next one)"""
    n = len(records)
    recs = np.zeros(max(n, max_pdus or 0, 1), dtype=REC_DTYPE)
    data = bytearray()
    for i, (c, e, p) in enumerate(records):
        recs[i] = (e, len(data), c, len(p))
        data += bytes(p) + b"\xa5" * gap
    return recs, np.frombuffer(bytes(data) + b"\xa5" * 8, dtype=np.uint8).copy()


def expected(case):
    """the text of every record a correct implementation writes: [(chan, end_bit, text)] for the records kept,
    the whole stream (texts and newlines) and the number kept"""
    des = case["designators"]
    out, stream, kept = [], b"", 0
    n = case.get("npdus", len(case["records"]))
    if n < 0 or n > case.get("max_pdus", len(case["records"])):
        return [], b"", 0
    for c, e, p in case["records"][:n]:
        good = 0 <= c < len(des) and len(p) <= case["length_max"] - 1
        t = host_sentence(des[c], p) if good else ""
        add = (t + "\n").encode("latin-1") if t else b""
        if case.get("text_cap") and len(stream) + len(add) > case["text_cap"]:
            break
        out.append((c, e, t))
        stream += add
        kept += 1
    return out, stream, kept


def split(recs, text):
    """records read back + text -> [(chan, end_bit, text)], checking that the text is exactly the records' lines"""
    got, pos = [], 0
    for r in recs:
        o, n = int(r["offset"]), int(r["len"])
        assert o == pos, (o, pos)
        t = text[o:o + n]
        if n:
            assert text[o + n:o + n + 1] == b"\n"
            pos = o + n + 1
        got.append((int(r["chan"]), int(r["end_bit"]), t.decode("latin-1")))
    assert pos == len(text)
    return got


def _payload(rng, n):
    return bytes(rng.integers(0, 256, n).astype(np.uint8))


def every_length(rng):
    """every payload length 1..1023: fill counts 0 / 2 / 4, 1 to 25 fragments (9 -> 10 among them), texts of
    56, 57, 112 and 113 payload characters; three channels with designators of 0, 1 and 16 bytes"""
    des = ["", "B", D16]
    recs = [(L % 3, 1000 + 7 * L, _payload(rng, L)) for L in range(1, 1024)]
    return dict(name="every_length", designators=des, length_max=1024, records=recs)


def last_byte(rng):
    """every value of the last byte for each len % 3 (the padded group's quirks: the shift in eight bits, the
    signed-char wrap), designators differing per channel"""
    des = ["A", "B", "", D16, "xyz"]
    recs = []
    for L in (3, 4, 5, 6, 7, 8, 22, 23, 24):
        head = _payload(rng, L - 1)
        for v in range(256):
            recs.append(((v + L) % 5, 17 * v + L, head + bytes([v])))
    return dict(name="last_byte", designators=des, length_max=64, records=recs)


def mixed(rng, with_empty=True):
    """AIS-sized records on 7 channels with empty payloads among them (length_min = 2 lets one through)"""
    des = ["A", "B", "", D16, "AB", "C", "0"]
    recs = []
    for i in range(300):
        L = 0 if with_empty and i % 13 == 5 else int(rng.integers(1, 64))
        recs.append((i % 7, 3 * i, _payload(rng, L)))
    return dict(name="mixed", designators=des, length_max=64, records=recs)


def bad_records(rng):
    """a channel outside [0, nchan) and a payload longer than length_max - 1: no text for them, the others as
    usual, the read says INVALID once"""
    c = mixed(rng, with_empty=False)
    recs = list(c["records"])
    recs[10] = (7, recs[10][1], recs[10][2])
    recs[11] = (-1, recs[11][1], recs[11][2])
    recs[40] = (2, recs[40][1], _payload(rng, 64))
    return dict(c, name="bad_records", records=recs, bad=True)


def all_cases(rng):
    return [every_length(rng), last_byte(rng), mixed(rng), bad_records(rng)]
