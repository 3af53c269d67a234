"""The host NMEA parser (aisx_nmea_parse_*, ais_amd.nmea_to_pdu) against the independent Python statement of its
grammar, under every way of cutting the text into calls; round trips through both armourers; the decoder behind it."""
import numpy as np
import pytest

import ais_amd
import nmea_parse_cases as nc

CASES = nc.build_cases()


def run_host(text_pieces, ref_tail=False, max_line=nc.MAX_LINE, length_max=nc.LENGTH_MAX, designators=nc.DESIGNATORS):
    h = ais_amd.nmea_to_pdu(designators, length_max, max_line=max_line, ref_tail=ref_tail)
    out = []
    for piece in text_pieces:
        recs, data, times, cnt = h.work(piece)
        out.append((nc.as_tuples(recs, data, times), cnt))
    return out


def run_py(text_pieces, ref_tail=False, max_line=nc.MAX_LINE, length_max=nc.LENGTH_MAX, designators=nc.DESIGNATORS):
    h = nc.PyParser(designators, length_max, max_line, ref_tail)
    return [h.feed(piece) for piece in text_pieces]


def summed(calls):
    recs, tot = [], dict.fromkeys(nc.COUNT_NAMES, 0)
    for r, c in calls:
        recs += r
        for k in nc.COUNT_NAMES:
            tot[k] += c[k]
    del tot["CARRIED"]
    return recs, tot


@pytest.mark.parametrize("name,text", CASES, ids=[c[0] for c in CASES])
@pytest.mark.parametrize("ref_tail", [False, True])
def test_cases_against_python(name, text, ref_tail):
    whole = run_py([text], ref_tail)
    assert run_host([text], ref_tail) == whole
    rng = np.random.default_rng(len(text))
    for k in (1, 3, 17):
        pcs = nc.pieces(text, nc.random_cuts(rng, len(text), k))
        got = run_host(pcs, ref_tail)
        assert got == run_py(pcs, ref_tail)
        assert summed(got) == summed(whole)


def test_planted_rejects_count_where_expected():
    for name, ln, which in nc.planted_rejects():
        (recs, cnt), = run_host([nc.GOOD + b"\n" + ln + b"\n" + nc.GOOD + b"\r\n"])
        assert cnt["LINES"] == 3, name
        if which is None:
            assert cnt["FOUND"] == 3 and cnt["SENTENCES"] == 3, name
            continue
        assert cnt["FOUND"] == 2 and cnt[which] == 1, (name, cnt)
        assert sum(cnt[k] for k in nc.COUNT_NAMES if k.startswith("REJ_")) == 1, (name, cnt)
        assert [r[2] for r in recs] == [0, 2], name


def test_broken_groups():
    rng = np.random.default_rng(20240611)
    for name, lines, nmsg, nfrag in nc.broken_groups(rng):
        (recs, cnt), = run_host([b"".join(ln + b"\n" for ln in lines) + nc.GOOD + b"\n"])
        assert (cnt["FOUND"], cnt["REJ_FRAGMENT"]) == (nmsg + 1, nfrag), (name, cnt)


def test_every_cut_of_the_600_byte_text():
    text = nc.text600()
    assert 500 <= len(text) <= 700 and text.count(b"\n") == 8
    whole = summed(run_host([text]))
    assert whole == summed(run_py([text]))
    assert len(whole[0]) == 4 and whole[0][1][3] == 1700000000 and whole[0][2][3] == 99
    for cut in range(len(text) + 1):
        got = run_host([text[:cut], text[cut:]])
        assert summed(got) == whole, cut
    for cut in range(0, len(text), 7):  # and three pieces
        assert summed(run_host([text[:cut], text[cut:cut + 5], text[cut + 5:]])) == whole, cut


def test_round_trip_standard_armourer():
    rng = np.random.default_rng(1)
    h = ais_amd.nmea_to_pdu(["A"], 65, max_line=256)
    for n in range(1, 65):
        for nbits in (8 * n, 8 * n - int(rng.integers(1, 8))):
            bits = rng.integers(0, 2, nbits).tolist()
            text = b"".join(ln + b"\n" for ln in nc.armour_std(bits, b"A"))
            recs, data, _, cnt = h.work(text)
            assert cnt["FOUND"] == 1 and bytes(data) == nc.bits_to_octets(bits), (n, nbits)


def clear_tail(pdu):
    """a PDU as this project's armourer transmits it under REF_TAIL: the last 6 - fill bits cleared when fill > 0"""
    fill = (6 - (8 * len(pdu)) % 6) % 6
    if not fill:
        return bytes(pdu)
    v = int.from_bytes(pdu, "big")
    return ((v >> (6 - fill)) << (6 - fill)).to_bytes(len(pdu), "big")


def test_round_trip_own_armourer():
    rng = np.random.default_rng(2)
    arm = ais_amd.pdu_to_nmea("B")
    ref = ais_amd.nmea_to_pdu(["A", "B"], 65, max_line=256, ref_tail=True)
    std = ais_amd.nmea_to_pdu(["A", "B"], 65, max_line=256)
    for n in range(1, 65):
        for _ in range(4):
            pdu = bytes(rng.integers(0, 256, n, dtype=np.uint8))
            text = arm.msg_to_sentence(pdu).encode("latin-1") + b"\n"
            recs, data, _, cnt = ref.work(text)
            assert cnt["FOUND"] == 1 and recs["chan"][0] == 1 and bytes(data) == clear_tail(pdu), n
            recs, data, _, cnt = std.work(text)
            if n % 3 == 0:
                assert cnt["FOUND"] == 1 and bytes(data) == pdu, n


def test_arguments_reset_and_overflow():
    for bad in (dict(length_max=1), dict(length_max=1025), dict(max_line=63), dict(max_line=4097)):
        kw = dict(length_max=64, max_line=512)
        kw.update(bad)
        with pytest.raises(ValueError):
            ais_amd.nmea_to_pdu(["A"], kw["length_max"], max_line=kw["max_line"])
    with pytest.raises(ValueError):
        ais_amd.nmea_to_pdu(["A" * 17], 64)
    with pytest.raises(ValueError):
        ais_amd.nmea_to_pdu([], 64)
    text = nc.text600()
    whole, _ = summed(run_host([text]))
    h = ais_amd.nmea_to_pdu(nc.DESIGNATORS, nc.LENGTH_MAX, max_line=nc.MAX_LINE)
    # reset drops the open group, the partial line and the line index
    cut = text.index(b"\n", text.index(b"\n") + 1) + 10  # inside the group's second sentence
    _, _, _, cnt = h.work(text[:cut])
    assert cnt["CARRIED"] > 10
    h.reset()
    recs, data, times, cnt = h.work(text)
    assert nc.as_tuples(recs, data, times) == whole and cnt["CARRIED"] == 0
    # overflow by pdu_cap and by bytes_cap: a prefix is kept, the state advances
    for kw, kept in ((dict(pdu_cap=2), 2), (dict(pdu_cap=8, bytes_cap=whole[0][1] + whole[1][1] + 3), 2), (dict(pdu_cap=0), 0)):
        h.reset()
        with pytest.raises(OverflowError):
            h.work(text, **kw)
        h.reset()
        half = text.index(b"\n", 300) + 1
        recs, data, times, cnt = h.work(text[:half] + text[: text.index(b"\n") - 5], overflow_ok=True, **kw)
        assert cnt["FOUND"] == len([r for r in whole if r[2] < text[:half].count(b"\n")]) and cnt["KEPT"] == kept
        assert nc.as_tuples(recs, data, times) == whole[:kept]
        recs, data, times, cnt = h.work(text[text.index(b"\n") - 5: text.index(b"\n") + 1])
        assert cnt["FOUND"] == 1 and nc.as_tuples(recs, data, times)[0][4] == whole[0][4]


def pack(fields):
    bits = []
    for v, n in fields:
        bits += [int(b) for b in format(v & ((1 << n) - 1), "0%db" % n)]
    return bits


def sixbit(s, n):
    return [(ord(c) & 63, 6) for c in s.ljust(n, "@")]


def test_parsed_octets_decode_to_their_fields():
    t1 = pack([(1, 6), (0, 2), (366123456, 30), (5, 4), (-3, 8), (123, 10), (1, 1), (-73500000, 28), (24600000, 27),
               (2105, 12), (211, 9), (33, 6), (0, 2), (0, 3), (1, 1), (0x12345, 19)])
    t5 = pack([(5, 6), (0, 2), (244660123, 30), (0, 2), (9123456, 30)] + sixbit("PA1234", 7) + sixbit("EVER GIVEN", 20) +
              [(70, 8), (200, 9), (199, 9), (30, 6), (29, 6), (1, 4), (6, 4), (15, 5), (14, 5), (30, 6), (145, 8)] +
              sixbit("ROTTERDAM", 20) + [(0, 1), (0, 1)])
    t24 = pack([(24, 6), (0, 2), (338123456, 30), (0, 2)] + sixbit("SEA BREEZE", 20))
    assert (len(t1), len(t5), len(t24)) == (168, 424, 160)
    text = b"".join(ln + b"\n" for ln in nc.armour_std(t1, b"A") + nc.armour_std(t5, b"B", s=b"4") + nc.armour_std(t24, b"A"))
    assert text.count(b"\n") == 4
    recs, data, times, cnt = ais_amd.nmea_to_pdu(["A", "B"], 64).work(text)
    assert cnt["FOUND"] == 3 and recs["len"].tolist() == [21, 53, 20]
    m = [ais_amd.msg_decode(p[4]) for p in nc.as_tuples(recs, data, times)]
    assert (m[0]["TYPE"], m[0]["MMSI"], m[0]["SOG"], m[0]["LON"], m[0]["LAT"], m[0]["COG"], m[0]["ROT"]) == \
        (1, 366123456, 123, -73500000, 24600000, 2105, -3)
    assert (m[1]["TYPE"], m[1]["MMSI"], m[1]["IMO"], m[1]["SHIPTYPE"], m[1]["DRAUGHT"]) == (5, 244660123, 9123456, 70, 145)
    assert m[1]["callsign"].rstrip(b"@") == b"PA1234" and m[1]["name"].rstrip(b"@") == b"EVER GIVEN"
    assert m[1]["destination"].rstrip(b"@") == b"ROTTERDAM"
    assert (m[2]["TYPE"], m[2]["MMSI"], m[2]["PART"]) == (24, 338123456, 0) and m[2]["name"].rstrip(b"@") == b"SEA BREEZE"
