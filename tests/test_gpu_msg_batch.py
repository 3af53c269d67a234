"""The batched message-field decoder on the MI355X (aisx_msg_batch_*, ais_amd.pdu_decode_batch) against the host
aisx_msg_decode that is its specification, exactly, columns and strings: the cases of tests/msg_cases.py written
straight into device PDU lists (shuffled, gapped offsets: a payload at every byte alignment), the record counts at
which a wave, a workgroup and the table fill up, bad records and bad counts, a producer's overflow, behind the real
deframer, and two handles on two streams.  -m gpu."""
import numpy as np
import pytest

import hdlc_cases as hc
import msg_cases as mc

pytestmark = pytest.mark.gpu

NCOL = len(mc.COLUMNS)
FL = mc.COLUMNS.index("FLAGS")
GROUP = 256  # records one workgroup takes per pass (k_msg.h: MSG_T)


@pytest.fixture(scope="module")
def ais():
    import torch

    assert torch.cuda.is_available()
    import ais_amd

    return ais_amd


@pytest.fixture(scope="module")
def payloads():
    return mc.all_payloads(np.random.default_rng(41))


@pytest.fixture(scope="module")
def host_rows(ais, payloads):
    """aisx_msg_decode of every case, computed once"""
    return [mc.row_of(ais.msg_decode(p)) for p in payloads]


def _device_list(recs, data, npdus, nfound=0):
    import torch

    d_recs = torch.from_numpy(recs.view(np.uint8).copy()).cuda()
    d_data = torch.from_numpy(data).cuda()
    d_cnt = torch.tensor([npdus, nfound], dtype=torch.int32, device="cuda")
    return d_recs, d_data, d_cnt


def _work(md, dev, with_found=False, stream=None):
    d_recs, d_data, d_cnt = dev
    md.work_device(d_recs.data_ptr(), d_data.data_ptr(), d_cnt.data_ptr(), d_cnt.data_ptr() + 4 if with_found else None,
                   stream=stream)


def rows_of_messages(m):
    return [tuple(int(r[c.lower()]) for c in mc.COLUMNS) + (bytes(r["callsign"]), bytes(r["name"]), bytes(r["destination"]))
            for r in m]


def rows_of_columns(c):
    cols = np.stack([c[name].cpu().numpy() for name in mc.COLUMNS]) if len(c["TYPE"]) else np.zeros((NCOL, 0), np.int32)
    strs = c["strs"].cpu().numpy()
    out = []
    for i in range(cols.shape[1]):
        s = strs[i].tobytes()
        assert s[7:8] == b"\0"
        out.append(tuple(int(v) for v in cols[:, i]) + (s[0:7].rstrip(b"\0"), s[8:28].rstrip(b"\0"), s[28:48].rstrip(b"\0")))
    return out, strs


def test_cases_on_a_device_list(ais, payloads, host_rows):
    import torch

    rng = np.random.default_rng(42)
    n = len(payloads)
    recs, data = mc.pack(payloads, rng)
    assert {int(o) % 4 for o in recs["offset"][:n]} == {0, 1, 2, 3}
    md = ais.pdu_decode_batch(3, n, 64)
    dev = _device_list(recs, data, n)
    _work(md, dev)
    m = md.messages()
    assert md.found == n and len(m) == n
    got = rows_of_messages(m)
    for i, (g, w) in enumerate(zip(got, host_rows)):
        assert g == w, (i, payloads[i].hex())
    c = md.columns()
    assert set(c) == set(mc.COLUMNS) | {"strs"}
    assert all(c[k].dtype == torch.int32 and c[k].is_cuda and c[k].shape == (n,) for k in mc.COLUMNS)
    assert c["strs"].dtype == torch.uint8 and c["strs"].shape == (n, 48)
    got2, strs = rows_of_columns(c)
    assert got2 == host_rows
    nul = [i for i, w in enumerate(host_rows) if not (w[NCOL] or w[NCOL + 1] or w[NCOL + 2])]
    assert nul and not strs[nul].any()  # (absent strings are all NUL)
    # the views are the handle's memory: a filter on the device needs no copy
    sel = c["MMSI"][c["TYPE"] == 18].cpu().numpy()
    assert list(sel) == [w[2] for w in host_rows if w[0] == 18]
    print("%d records identical to aisx_msg_decode" % n)


def test_record_counts(ais, payloads, host_rows):
    """0, 1, 63, 64, 65 records, one workgroup's worth, one more, and max_pdus: the rows counted are written, the
    rest of the table is left alone"""
    import torch

    rng = np.random.default_rng(43)
    max_pdus = GROUP + 70
    recs, data = mc.pack(payloads[:max_pdus], rng)
    md = ais.pdu_decode_batch(3, max_pdus, 64)
    cp, stride, sp, _ = md.results_device()
    assert stride == max_pdus
    full = md._views()
    for n in (0, 1, 63, 64, 65, GROUP, GROUP + 1, max_pdus):
        full[0].fill_(0x5A5A5A5A)
        full[1].fill_(0x5A)
        torch.cuda.synchronize()
        dev = _device_list(recs, data, n, nfound=n)
        _work(md, dev, with_found=True)
        m = md.messages()
        assert len(m) == n and md.found == n
        assert rows_of_messages(m) == host_rows[:n]
        assert bool((full[0][:, n:] == 0x5A5A5A5A).all()) and bool((full[1][n:] == 0x5A).all())
        assert len(md.columns()["TYPE"]) == n


def test_bad_records_counts_and_overflow(ais, payloads, host_rows):
    import torch

    rng = np.random.default_rng(44)
    n = 150
    recs, data = mc.pack(payloads[:n], rng, nchan=3)
    recs["chan"][10] = 3
    recs["chan"][11] = -1
    recs["len"][70] = 64
    recs["len"][71] = -2
    recs["offset"][[10, 11, 70, 71]] = 1 << 40  # (no payload byte of a bad record is read)
    md = ais.pdu_decode_batch(3, n, 64)
    dev = _device_list(recs, data, n)
    _work(md, dev)
    with pytest.raises(ValueError):
        md.messages()
    m = md.messages()  # (the read cleared the flag)
    got = rows_of_messages(m)
    assert len(got) == n
    for i in range(n):
        if i in (10, 11, 70, 71):
            assert got[i] == tuple(4 if k == FL else mc.NA for k in range(NCOL)) + (b"", b"", b"")
        else:
            assert got[i] == host_rows[i]
    assert not md.columns()["strs"][[10, 11, 70, 71]].any()
    # a count outside [0, max_pdus]: no rows written, the flag raised once
    full = md._views()
    for bad_n in (-1, n + 1):
        full[0].fill_(0x5A5A5A5A)
        torch.cuda.synchronize()
        dev = _device_list(recs, data, bad_n)
        _work(md, dev)
        with pytest.raises(ValueError):
            md.messages()
        assert len(md.messages()) == 0 and md.found == 0
        assert bool((full[0] == 0x5A5A5A5A).all())
    # a producer that found more than max_pdus: overflow, the rows handed over are there
    good, gdata = mc.pack(payloads[:n], rng)
    dev = _device_list(good, gdata, n, nfound=n + 7)
    _work(md, dev, with_found=True)
    with pytest.raises(OverflowError):
        md.messages()
    m = md.messages(overflow_ok=True)
    assert md.found == n + 7 and rows_of_messages(m) == host_rows[:n]


def test_behind_the_deframer(ais):
    """one small step behind the real deframer: columns() equals the host decode of hd.pdus()"""
    import torch

    import test_gpu_nmea_batch as tn

    rng = np.random.default_rng(201)
    nch = 1
    streams = tn._streams(rng, nch)
    stride = max(len(x) for x in streams) + 5
    rows, n = hc.pack(streams, stride)
    hd = ais.hdlc_deframer_batch(11, 64, nch, stride, 1 << 12)
    md = ais.pdu_decode_batch(nch, 1 << 12, 64)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        b = torch.from_numpy(rows).cuda()
        nb = torch.from_numpy(n).cuda()
    hd.work(b, nb, stream=s)
    md.work(hd, stream=s)
    pdus = hd.pdus(stream=s, as_list=True)
    assert len(pdus) > 0
    want = [mc.row_of(ais.msg_decode(p)) for _, _, p in pdus]
    got, _ = rows_of_columns(md.columns(stream=s))
    assert got == want and md.found == len(pdus)
    assert rows_of_messages(md.messages(stream=s)) == want
    # the deframer's overflow surfaces in the read
    small = ais.hdlc_deframer_batch(11, 64, nch, stride, 2)
    small.work(b, nb, stream=s)
    md.work(small, stream=s)
    with pytest.raises(OverflowError):
        md.messages(stream=s)
    assert rows_of_messages(md.messages(stream=s, overflow_ok=True)) == want[:2] and md.found == len(pdus)


def test_two_handles_on_two_streams(ais, payloads, host_rows):
    import torch

    rng = np.random.default_rng(45)
    na, nb = 300, len(payloads) - 300
    ra, da = mc.pack(payloads[:na], rng)
    rb, db = mc.pack(payloads[na:], rng)
    a, b = ais.pdu_decode_batch(3, na, 64), ais.pdu_decode_batch(3, nb, 64)
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    dev_a, dev_b = _device_list(ra, da, na), _device_list(rb, db, nb)
    torch.cuda.synchronize()
    for _ in range(3):
        _work(a, dev_a, stream=sa)
        _work(b, dev_b, stream=sb)
    assert rows_of_messages(b.messages(stream=sb)) == host_rows[na:]
    assert rows_of_messages(a.messages(stream=sa)) == host_rows[:na]
