"""The standard-form armouring on the host (aisx_pdu_to_nmea_std) against a pure-Python statement of the form
(nmea_std_cases.spec_sentence), byte for byte, its closed-form length and its refusals; and the round trip: the
standard text read back by the STRICT parser (ais_amd.nmea_to_pdu without ref_tail) returns every payload bit for bit,
where the reference form loses most payloads whose length is no multiple of three.  -m "not gpu"."""
import ctypes as C

import numpy as np
import pytest

import nmea_std_cases as sc
from nmea_std_cases import D16, S15, T18

DESIGNATORS = ["", "B", D16]
STATIONS = ["", "S", S15]
TIMES = [-1, 0, 9, 10, T18]


def std(designator, payload, seq=0, station="", time=-1):
    import ais_amd

    nm = ais_amd.pdu_to_nmea(designator, standard=True, station=station, time=time)
    nm.next_id = seq
    return nm.msg_to_sentence(payload)


def payloads(rng):
    """every length 1..378 with a random payload, one ending in all-ones and one ending in all-zero bits"""
    for L in range(1, sc.MAX_OCTETS + 1):
        p = bytes(rng.integers(0, 256, L).astype(np.uint8))
        k = min(L, 1 + L % 3)
        yield p
        yield p[:L - k] + b"\xff" * k
        yield p[:L - k] + b"\x00" * k


def test_matches_the_statement_of_the_form():
    from ais_amd.batch_framing import nmea_std_text_len

    rng = np.random.default_rng(21)
    n = 0
    for i, p in enumerate(payloads(rng)):
        # designator, station, time and id vary against each other and against the length
        d, s = DESIGNATORS[i % 3], STATIONS[(i // 3 + i) % 3]
        t, q = TIMES[(i // 2) % 5], (i // 5) % 10
        got = std(d, p, q, s, t)
        assert got == sc.spec_sentence(d, p, q, s, t), (len(p), d, s, t, q)
        assert len(got) == nmea_std_text_len(len(p), len(d), len(s), t)
        n += 1
    assert n == 3 * sc.MAX_OCTETS
    # every designator x station x time x id at the lengths where the form changes
    for L in (1, 2, 3, 41, 42, 43, 44, 84, 85, 377, 378):
        p = bytes(rng.integers(0, 256, L).astype(np.uint8))
        for d in DESIGNATORS:
            for s in STATIONS:
                for t in TIMES:
                    for q in range(10):
                        assert std(d, p, q, s, t) == sc.spec_sentence(d, p, q, s, t), (L, d, s, t, q)


def test_the_form_in_plain_sight():
    # 21 octets (no fill), 20 octets (four bits left: fill 2, 111100 -> 't'), 19 octets (fill 4, 110000 -> 'h'), two sentences
    assert std("A", bytes(21)) == "!AIVDM,1,1,,A,0000000000000000000000000000,0*26"
    assert std("B", b"\xff" * 20, station="x", time=5) == "\\s:x,c:5*71\\!AIVDM,1,1,,B," + "w" * 26 + "t,2*53"
    assert std("B", b"\xff" * 19) == "!AIVDM,1,1,,B," + "w" * 25 + "h,4*3E"
    two = std("A", b"\xff" * 43, seq=7, time=0).split("\n")
    assert two[0].startswith("\\c:0*69\\!AIVDM,2,1,7,A," + "w" * 56 + ",0*") and two[1].startswith("\\c:0*69\\!AIVDM,2,2,7,A,wh,4*")
    assert len(std(D16, b"\x00" * 43, 9, S15, T18).split("\n")[0]) == 134  # (with its newline: the 135-byte line)


def test_closed_form_length_in_the_library():
    from ais_amd import _lib

    L = _lib.lib(device=False)
    for n, d, s, t in [(1, 0, 0, -1), (43, 16, 15, T18), (378, 1, 0, 10), (42, 3, 15, -1), (0, 5, 5, 5)]:
        want = len(std("d" * d, b"\x5a" * n, 3, "s" * s, t)) if n else 0
        assert L.aisx_nmea_std_text_len(n, d, s, t) == want
    for n, d, s, t in [(379, 1, 0, -1), (-1, 1, 0, -1), (5, 1, 16, -1), (5, 1, 0, -2), (5, 1, 0, 10 ** 18)]:
        assert L.aisx_nmea_std_text_len(n, d, s, t) == _lib.AISX_ERR_INVALID


def test_refusals():
    from ais_amd import _lib

    L = _lib.lib(device=False)
    out = C.create_string_buffer(4096)

    def rc(p, seq=0, station=b"", time=-1, cap=4096):
        a = np.frombuffer(p, dtype=np.uint8) if len(p) else np.zeros(1, np.uint8)
        return L.aisx_pdu_to_nmea_std(b"A", a.ctypes.data_as(C.c_void_p), len(p), seq, station, time, out, cap)

    assert rc(b"\x01" * 378) > 0 and rc(b"\x01", 9, S15.encode(), T18) > 0
    assert rc(b"") == _lib.AISX_ERR_INVALID
    assert rc(b"\x01" * 379) == _lib.AISX_ERR_INVALID
    for bad in (b"a b", b"a,b", b"a*b", b"a\\b", b"\xe9", b"x" * 16, b"s:1"):
        assert rc(b"\x01", station=bad) == _lib.AISX_ERR_INVALID, bad
    assert rc(b"\x01", time=10 ** 18) == _lib.AISX_ERR_INVALID
    assert rc(b"\x01", time=-2) == _lib.AISX_ERR_INVALID
    assert rc(b"\x01", seq=10) == _lib.AISX_ERR_INVALID and rc(b"\x01", seq=-1) == _lib.AISX_ERR_INVALID
    assert rc(b"\x01" * 21, cap=10) == _lib.AISX_ERR_OVERFLOW
    assert L.aisx_pdu_to_nmea_std(b"A", None, 1, 0, b"", -1, out, 4096) == _lib.AISX_ERR_INVALID
    import ais_amd

    with pytest.raises(ValueError):
        ais_amd.pdu_to_nmea("A", standard=True, station="no good").msg_to_sentence(b"\x01")


def test_the_object_counts_its_ids():
    import ais_amd

    nm = ais_amd.pdu_to_nmea("A", standard=True)
    ids = []
    for k in range(25):
        s = nm.msg_to_sentence(b"\x11" * (53 if k % 2 else 21))
        if k % 2:
            ids.append(int(s.split(",")[3]))
        else:
            assert s.split(",")[3] == ""
    assert ids == [k % 10 for k in range(12)]
    # the default stays the reference's text
    assert ais_amd.pdu_to_nmea("A").msg_to_sentence(b"\xff" * 20) != std("A", b"\xff" * 20)
    assert ais_amd.pdu_to_nmea("A").msg_to_sentence(b"\x12" * 21) == std("A", b"\x12" * 21)


def test_round_trip_through_the_strict_parser():
    import ais_amd

    rng = np.random.default_rng(22)
    sent = []  # (chan, payload, time)
    text = []
    nms = {}
    for i, p in enumerate(payloads(rng)):
        c = i % 3
        s, t = STATIONS[(i // 3) % 3], TIMES[(i // 2) % 5]
        nm = nms.setdefault((c, s), ais_amd.pdu_to_nmea(DESIGNATORS[c], standard=True, station=s))
        text.append(nm.msg_to_sentence(p, time=t))
        sent.append((c, p, t))
    recs, data, times, counts = ais_amd.nmea_to_pdu(DESIGNATORS, 380).work(("\n".join(text) + "\n").encode("latin-1"))
    assert all(counts[k] == 0 for k in counts if k.startswith("REJ_")), counts
    assert counts["FOUND"] == counts["KEPT"] == len(sent) == len(recs) and counts["CARRIED"] == 0
    for r, tm, (c, p, t) in zip(recs, times, sent):
        assert int(r["chan"]) == c and int(r["len"]) == len(p) and int(tm) == t
        assert bytes(data[r["offset"]:r["offset"] + r["len"]]) == p
    assert counts["LINES"] == counts["SENTENCES"] == sum(t.count("\n") + 1 for t in text)


def test_the_reference_form_loses_type_5_payloads():
    """the defect the standard form is there for: 53-octet payloads (type 5) in the reference form, strict parsing"""
    import ais_amd

    rng = np.random.default_rng(0)
    nm = ais_amd.pdu_to_nmea("A")
    sent = [bytes(rng.integers(0, 256, 53).astype(np.uint8)) for _ in range(2000)]
    text = "".join(nm.msg_to_sentence(p) + "\n" for p in sent).encode("latin-1")
    recs, data, _, counts = ais_amd.nmea_to_pdu(["A"], 64).work(text)
    got = {bytes(data[r["offset"]:r["offset"] + r["len"]]) for r in recs}
    intact = sum(p in got for p in sent)
    print("reference form, 53 octets, strict parse: %d of 2000 read, %d intact" % (len(recs), intact))
    assert intact < 1000
    std_nm = ais_amd.pdu_to_nmea("A", standard=True)
    text = "".join(std_nm.msg_to_sentence(p) + "\n" for p in sent).encode("latin-1")
    recs, data, _, counts = ais_amd.nmea_to_pdu(["A"], 64).work(text)
    assert [bytes(data[r["offset"]:r["offset"] + r["len"]]) for r in recs] == sent
