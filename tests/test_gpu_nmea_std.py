"""The standard-form NMEA armouring on the MI355X (aisx_nmea_batch_create_std, ais_amd.pdu_to_nmea_batch(standard=True))
against the host aisx_pdu_to_nmea_std that is its specification, byte for byte: the lists of tests/nmea_std_cases.py
written straight into device PDU lists (one of more than 8192 records, the device's scan tile), the 135-byte line, ids
over calls with the wrap, text_cap cuts, set_time between queued calls, reset and next_id, a handle of each form side by
side, and the loop deframer -> standard armourer -> strict parser on the device.  -m gpu."""
import numpy as np
import pytest

import hdlc_cases as hc
import nmea_cases as nc
import nmea_std_cases as sc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ais():
    import torch

    assert torch.cuda.is_available()
    import ais_amd

    return ais_amd


class DevNmeaStd:
    """the device handle behind the few methods nmea_std_cases.check_call drives (as the lane model's wrapper)"""

    def __init__(self, ais, case, stream=None):
        self.max_pdus = case.get("max_pdus", max(len(case["records"]), 1))
        self.nm = ais.pdu_to_nmea_batch(case["designators"], len(case["designators"]), self.max_pdus, case["length_max"],
                                        case.get("text_cap", 0), standard=True, stations=case["stations"])
        self.stream = stream
        self.keep = None

    def set_time(self, t):
        self.nm.set_time(t)

    def reset(self):
        self.nm.reset()

    def next_id(self):
        return self.nm.next_id(self.stream)

    def process(self, recs, data, npdus, nfound=None):
        import torch

        d_recs = torch.from_numpy(recs.view(np.uint8).copy()).cuda()
        d_data = torch.from_numpy(data).cuda()
        d_cnt = torch.tensor([npdus, nfound or 0], dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()  # (the copies ran on torch's stream)
        self.keep = (d_recs, d_data, d_cnt)
        self.nm.work_device(d_recs.data_ptr(), d_data.data_ptr(), d_cnt.data_ptr(), d_cnt.data_ptr() + 4 if nfound is not None else None,
                            stream=self.stream)

    def read(self):
        bad = 0
        try:
            recs, text = self.nm.sentences(stream=self.stream, overflow_ok=True)
        except ValueError:  # (once: the read clears the flag)
            bad = 1
            recs, text = self.nm.sentences(stream=self.stream, overflow_ok=True)
        return self.nm.found, bad, recs, text


def test_lists_on_the_device(ais):
    rng = np.random.default_rng(51)
    n = 0
    for case in sc.all_cases(rng):
        n += len(sc.check_call(DevNmeaStd(ais, case), case))
    base = sc.mixed(rng, time=1)
    sc.check_call(DevNmeaStd(ais, base), dict(base, name="zero", records=[]))
    sc.check_call(DevNmeaStd(ais, base), dict(base, name="zero_count", npdus=0))
    sc.check_call(DevNmeaStd(ais, base), dict(base, name="producer", npdus=100, nfound=250))
    for bad_n in (-1, len(base["records"]) + 1):
        b = DevNmeaStd(ais, base)
        sc.check_call(b, dict(base, npdus=bad_n, bad=True))
        sc.check_call(b, base)
    print("%d records identical to aisx_pdu_to_nmea_std" % n)


def test_more_than_one_scan_tile(ais):
    tile = 1024 * 8  # NM_SCAN_T x NM_ITEMS
    case = sc.many(np.random.default_rng(52), 2 * tile + 300, tile)
    multi = [sc.is_multi(p) for _, _, p in case["records"]]
    assert multi[tile - 1] and multi[tile] and multi[2 * tile - 1] and multi[2 * tile] and multi[-1]
    b = DevNmeaStd(ais, case)
    got = sc.check_call(b, case)
    assert len(got) == len(multi) > 8192 and b.next_id() == sum(multi) % 10
    sc.check_call(b, case)  # (the ids go on from there)


def test_the_longest_line(ais):
    case = sc.longest_line()
    got = sc.check_call(DevNmeaStd(ais, case), case)
    assert [len(g[2].split("\n")[0]) + 1 for g in got[:3]] == [135, 134, 134]
    assert len(got[3][2].split("\n")) == 9 and all(len(x) + 1 == 135 for x in got[3][2].split("\n")[:8])


def test_ids_over_calls_reset_and_next_id(ais):
    import torch

    rng = np.random.default_rng(53)
    case = sc.mixed(rng)
    case["records"] = case["records"][:270]
    nm = sum(sc.is_multi(p) for _, _, p in case["records"])
    assert nm % 10 != 0
    b = DevNmeaStd(ais, case, stream=torch.cuda.Stream())
    ids = []
    for k in range(3):  # (the counter wraps 9 -> 0 inside a call and stands between calls)
        got = sc.check_call(b, dict(case, time=(-1, 7, sc.T18)[k]))
        ids += [int(t.split("!")[1].split(",")[3]) for _, _, t in got if "\n" in t]
        assert b.next_id() == (k + 1) * nm % 10
    assert ids == [k % 10 for k in range(3 * nm)]
    b.reset()
    assert b.next_id() == 0
    recs, data = sc.pack(case["records"], b.max_pdus)
    b.process(recs, data, len(case["records"]))  # (the time is back at -1: channel 0 has no station, so no tag block)
    assert b.read()[3].startswith(b"!AIVDM")
    one = dict(case, records=[r for r in case["records"] if not sc.is_multi(r[2])])
    at = b.next_id()
    sc.check_call(b, one)
    assert b.next_id() == at
    # the three calls refuse a handle of the reference form, and a time out of range
    ref = ais.pdu_to_nmea_batch("A", 1, 4, 64)
    for f in (lambda: ref.set_time(1), ref.reset, ref.next_id, lambda: b.nm.set_time(10 ** 18), lambda: b.nm.set_time(-2)):
        with pytest.raises(ValueError):
            f()


def test_text_cap_cuts_around_a_multi_sentence_record(ais):
    rng = np.random.default_rng(54)
    base = sc.mixed(rng, time=3)
    want = sc.expected(base)[0]
    k = 150 + [sc.is_multi(p) for _, _, p in base["records"][150:]].index(True)
    before = sum(len(t) + 1 for _, _, t in want[:k] if t)
    whole = before + len(want[k][2]) + 1
    for cap, kept in ((before, k), (before + 1, k), (whole - 1, k), (whole, k + 1), (whole + 1, k + 1)):
        case = dict(base, name="cap %d" % cap, text_cap=cap)
        b = DevNmeaStd(ais, case)
        for rep in range(2):  # the second call's ids follow the ones written, not the ones cut
            got = sc.check_call(b, case)
        assert len(got) >= kept and all(not t for _, _, t in got[kept:])
        assert b.next_id() == 2 * sum(sc.is_multi(p) for _, _, p in base["records"][:kept]) % 10
        with pytest.raises(OverflowError):  # (what the wrapper's overflow_ok hides)
            b.nm.sentences()


def test_set_time_between_queued_calls(ais):
    """two calls queued on one stream with set_time between them and no synchronisation: each has its own time (the
    first call's text is copied aside on the same stream before the second overwrites it)"""
    import torch
    from ais_amd.batch_framing import _DevMem

    rng = np.random.default_rng(55)
    case = sc.mixed(rng)
    b = DevNmeaStd(ais, case, stream=torch.cuda.Stream())
    recs, data = sc.pack(case["records"], b.max_pdus)
    d_recs, d_data = torch.from_numpy(recs.view(np.uint8).copy()).cuda(), torch.from_numpy(data).cuda()
    d_cnt = torch.tensor([len(case["records"])], dtype=torch.int32, device="cuda")
    _, t_ptr, _ = b.nm.results_device()
    view = torch.as_tensor(_DevMem(b.nm, t_ptr, (b.nm.text_cap,), "|u1"), device=torch.device("cuda", torch.cuda.current_device()))
    torch.cuda.synchronize()  # (the uploads; from here on nothing waits until the read)
    b.nm.set_time(999)
    b.nm.work_device(d_recs.data_ptr(), d_data.data_ptr(), d_cnt.data_ptr(), stream=b.stream)
    with torch.cuda.stream(b.stream):
        aside = view.clone()
    b.nm.set_time(1000)  # (one digit more: every offset behind the first record moves)
    b.nm.work_device(d_recs.data_ptr(), d_data.data_ptr(), d_cnt.data_ptr(), stream=b.stream)
    _, _, _, second = b.read()
    _, s1, _, nid = sc.expected(dict(case, time=999), 0)
    _, s2, _, _ = sc.expected(dict(case, time=1000), nid)
    assert second == s2 and len(s1) < len(s2)
    assert aside[: len(s1)].cpu().numpy().tobytes() == s1


def test_a_handle_of_each_form_side_by_side(ais):
    import torch

    rng = np.random.default_rng(56)
    case = sc.mixed(rng, time=42)
    n = len(case["records"])
    std = DevNmeaStd(ais, case)
    ref = ais.pdu_to_nmea_batch(case["designators"], 7, n, 64)
    recs, data = sc.pack(case["records"], n)
    std.nm.set_time(42)
    std.process(recs, data, n)
    d_recs, d_data, d_cnt = std.keep
    for _ in range(2):  # interleaved on one stream over the same list
        ref.work_device(d_recs.data_ptr(), d_data.data_ptr(), d_cnt.data_ptr())
        std.nm.work_device(d_recs.data_ptr(), d_data.data_ptr(), d_cnt.data_ptr())
    torch.cuda.synchronize()
    _, s_std, _, nid = sc.expected(case, sc.expected(case, sc.expected(case, 0)[3])[3])
    assert std.read()[3] == s_std
    want_ref, s_ref, _ = nc.expected(case)
    r, t = ref.sentences()
    assert t == s_ref and nc.split(r, t) == want_ref
    # the reference form's handle is smaller: its worst case is not the standard form's
    assert ref.text_cap < std.nm.text_cap


def test_deframer_to_standard_text_to_strict_parser(ais):
    """the loop on the device: deframer -> standard armourer -> nmea_to_pdu_batch.work_nmea WITHOUT ref_tail; the parsed
    records and bytes are the deframer's, bit for bit, the times the armourer's"""
    import torch

    rng = np.random.default_rng(57)
    nch = 37
    base = [hc.ais_stream(rng, 6, lengths=(11, 62))[0] for _ in range(nch)]
    streams = [np.asarray(s, np.uint8) for s in base]
    stride = max(len(x) for x in streams) + 5
    rows, n = hc.pack(streams, stride)
    des = ["c%d" % c for c in range(nch)]
    sta = ["rx%d" % (c % 3) if c % 4 else "" for c in range(nch)]
    hd = ais.hdlc_deframer_batch(11, 64, nch, stride, 1 << 12)
    nm = ais.pdu_to_nmea_batch(des, nch, 1 << 12, 64, standard=True, stations=sta)
    ps = ais.nmea_to_pdu_batch(des, 64, nm.text_cap, 2 << 12, 1 << 12)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        b, nb = torch.from_numpy(rows).cuda(), torch.from_numpy(n).cuda()
    nm.set_time(1700000123)
    hd.work(b, nb, stream=s)
    nm.work(hd, stream=s)
    ps.work_nmea(nm, stream=s)
    pdus = hd.pdus(stream=s, as_list=True)
    recs, data, times, counts = ps.messages(stream=s)
    assert len(pdus) > 100 and any(sc.is_multi(p) for _, _, p in pdus) and any(len(p) % 3 for _, _, p in pdus)
    assert all(counts[k] == 0 for k in counts if k.startswith("REJ_")), counts
    assert counts["FOUND"] == counts["KEPT"] == len(pdus)
    got = [(int(r["chan"]), bytes(data[r["offset"]:r["offset"] + r["len"]])) for r in recs]
    assert got == [(c, p) for c, _, p in pdus]
    assert (times == 1700000123).all()
    # and the text is the host function's for those PDUs
    case = dict(designators=des, stations=sta, length_max=64, records=pdus, time=1700000123)
    assert nm.sentences(stream=s)[1] == sc.expected(case)[1]
