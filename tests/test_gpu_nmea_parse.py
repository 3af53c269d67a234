"""The batched NMEA parser on the MI355X (aisx_nmea_parse_batch_*, ais_amd.nmea_to_pdu_batch) against the host
aisx_nmea_parse_work that is its specification, bit for bit and call by call: the cases of tests/nmea_parse_cases.py
under cuts, a text cut at every byte, 64 KB in one call, the bounds and their refusal, and the device chain
deframer -> armourer -> parser -> decoder -> vessel table closed on itself.  -m gpu."""
import numpy as np
import pytest

import hdlc_cases as hc
import nmea_parse_cases as nc

pytestmark = pytest.mark.gpu

CASES = nc.build_cases()


@pytest.fixture(scope="module")
def ais():
    import torch

    assert torch.cuda.is_available()
    import ais_amd

    return ais_amd


def host_calls(pcs, ref_tail=False, pdu_cap=None, max_line=nc.MAX_LINE, designators=nc.DESIGNATORS):
    import ais_amd

    h = ais_amd.nmea_to_pdu(designators, nc.LENGTH_MAX, max_line=max_line, ref_tail=ref_tail)
    out = []
    for piece in pcs:
        recs, data, times, cnt = h.work(piece, pdu_cap=pdu_cap, overflow_ok=True)
        out.append((nc.as_tuples(recs, data, times), cnt))
    return out


def parser(ais, max_bytes=1 << 17, max_lines=4096, max_pdus=4096, ref_tail=False, max_line=nc.MAX_LINE, designators=nc.DESIGNATORS):
    return ais.nmea_to_pdu_batch(designators, nc.LENGTH_MAX, max_bytes, max_lines, max_pdus, max_line=max_line, ref_tail=ref_tail)


def dev_call(ps, piece, stream=None, **kw):
    ps.work(piece, stream=stream)
    recs, data, times, cnt = ps.messages(stream=stream, **kw)
    return nc.as_tuples(recs, data, times), cnt


def test_cases_whole_and_cut(ais):
    ncalls = 0
    for ref_tail in (False, True):
        ps = parser(ais, ref_tail=ref_tail)
        for name, text in CASES:
            rng = np.random.default_rng(len(text))
            for bounds in ([0, len(text)], nc.random_cuts(rng, len(text), 3), nc.random_cuts(rng, len(text), 17)):
                pcs = nc.pieces(text, bounds)
                ps.reset()
                want = host_calls(pcs, ref_tail)
                for k, piece in enumerate(pcs):
                    assert dev_call(ps, piece) == want[k], (name, ref_tail, bounds, k)
                    ncalls += 1
    print("%d calls identical to the host form" % ncalls)


def test_every_cut_of_the_600_byte_text(ais):
    text = nc.text600()
    ps = parser(ais, max_bytes=1024, max_lines=8, max_pdus=8)
    for cut in range(len(text) + 1):
        ps.reset()
        want = host_calls([text[:cut], text[cut:]])
        assert [dev_call(ps, text[:cut]), dev_call(ps, text[cut:])] == want, cut


def test_64k_in_one_call(ais):
    rng = np.random.default_rng(64)
    mixed = dict(CASES)["mixed"]
    lines = []
    while sum(len(x) + 1 for x in lines) < 64 * 1024:
        if rng.random() < 0.9:
            lines += nc.random_message(rng, nfrag=int(rng.integers(1, 3)), nbits=int(rng.integers(400, 505)))[0]
        else:
            lines.append(mixed.split(b"\n")[int(rng.integers(0, 100))])
    text = b"".join(ln + b"\n" for ln in lines)
    assert 700 <= len(lines) <= 1400
    ps = parser(ais)
    (want,) = host_calls([text])
    assert dev_call(ps, text) == want and want[1]["FOUND"] > 300
    # the same text as a device tensor at an address that is not 16-byte aligned
    import torch

    t = torch.zeros(len(text) + 16, dtype=torch.uint8, device="cuda")
    t[3:3 + len(text)].copy_(torch.frombuffer(bytearray(text), dtype=torch.uint8))
    ps.reset()
    ps.work(t[3:3 + len(text)])
    recs, data, times, cnt = ps.messages()
    assert (nc.as_tuples(recs, data, times), cnt) == want


def test_every_grid_stride_in_one_call(ais):
    """One call of more than 8 MB, 524 288 lines and 8192 records: every fixed grid takes a second turn on the device --
    count and index (2048 workgroups, tiles of 4096 bytes), parse and write (8192 waves), the group kernels (2048
    workgroups, tiles of 256 lines or sentences) -- with the grids the C ABI computes.  A group is left open at the end
    and completes in a second call."""
    rng = np.random.default_rng(8192)
    units = []
    for k in range(1200):
        r = rng.random()
        if r < 0.75:
            units.append(nc.random_message(rng, nfrag=1, nbits=int(rng.integers(1, 40)))[0])
        elif r < 0.9:
            units.append(nc.random_message(rng, nfrag=int(rng.integers(2, 5)), nbits=int(rng.integers(30, 90)))[0])
        elif r < 0.95:
            units.append([b"", b"$GPGGA,1*00", nc.GOOD[:-1] + b"0"][k % 3:k % 3 + 1])
        else:
            units.append(nc.random_message(rng, nfrag=3, nbits=60)[0][:2])  # a group that stays broken
    units = [b"".join(ln + b"\n" for ln in u) for u in units]
    tail = nc.armour_std(rng.integers(0, 2, 300).tolist(), b"B", [20, 20, 10], b"5", tag=b"c:31337")
    text = b"".join(units[i] for i in rng.integers(0, len(units), 440000)) + tail[0] + b"\n" + tail[1][:9]
    rest = tail[1][9:] + b"\n" + tail[2] + b"\n" + nc.GOOD + b"\n"
    nlines = text.count(b"\n")
    assert len(text) > 2048 * 4096 and nlines > 2048 * 256
    import ais_amd

    host = ais_amd.nmea_to_pdu(nc.DESIGNATORS, nc.LENGTH_MAX, max_line=nc.MAX_LINE)
    ps = parser(ais, max_bytes=len(text), max_lines=nlines, max_pdus=nlines)
    for piece in (text, rest):
        hr, hd, ht, hc_ = host.work(piece)
        ps.work(piece)
        dr, dd, dt, dc = ps.messages()
        assert dc == hc_ and np.array_equal(dr, hr) and np.array_equal(dd, hd) and np.array_equal(dt, ht)
    assert hc_["FOUND"] == 2 and ht[0] == 31337  # the group that was open, then the single
    ps.reset()
    host.reset()
    hr, hd, ht, hc_ = host.work(text)
    assert hc_["FOUND"] > 8192 and hc_["REJ_FRAGMENT"] > 0 and hc_["REJ_CHECKSUM"] > 0 and hc_["CARRIED"] > 9


def test_empty_partial_long_line_and_group_over_three_calls(ais):
    text = nc.text600()
    ps = parser(ais, max_line=512)
    hk = dict(max_line=512)
    assert dev_call(ps, b"") == host_calls([b""], **hk)[0]
    # only a partial line, then its end
    pcs = [text[:40], b"", text[40:]]
    assert [dev_call(ps, p) for p in pcs] == host_calls(pcs, **hk)
    # a line of 300 bytes with a tag block (more than four passes of a wave)
    ln = nc.padded_to(300)
    ps.reset()
    got = dev_call(ps, ln + b"\n")
    assert got == host_calls([ln + b"\n"], **hk)[0] and got[1]["FOUND"] == 1 and got[0][0][3] == 4242
    # a group whose fragments fall into three calls
    ends = [k + 1 for k, c in enumerate(text) if c == 10]
    pcs = [text[:ends[1]], text[ends[1]:ends[2]], text[ends[2]:]]
    ps.reset()
    got = [dev_call(ps, p) for p in pcs]
    assert got == host_calls(pcs, **hk) and got[0][1]["CARRIED"] > 0 and got[1][1]["CARRIED"] > got[0][1]["CARRIED"]
    assert sum(c["FOUND"] for _, c in got) == 4 and sum(c["REJ_FRAGMENT"] for _, c in got) == 0


def test_max_lines_and_refusal(ais):
    text = nc.text600()
    ps = parser(ais, max_bytes=1024, max_lines=8, max_pdus=8)
    cut = text.index(b"\n", 200) + 20
    want = host_calls([text[:cut], text[cut:]])
    assert dev_call(ps, text[:cut]) == want[0]
    ps.work(b"\n" * 9)  # max_lines + 1
    with pytest.raises(ValueError):
        ps.messages()
    recs, data, times, cnt = ps.messages()  # (the read cleared the flag)
    assert len(recs) == 0 and cnt["CARRIED"] == want[0][1]["CARRIED"] and cnt["LINES"] == 0
    import torch

    for n in (-1, 1025):  # a byte count out of range, handed over on the device
        ps.work(torch.zeros(1024, dtype=torch.uint8, device="cuda"), torch.tensor([n], dtype=torch.int64, device="cuda"))
        with pytest.raises(ValueError):
            ps.messages()
    assert dev_call(ps, text[cut:]) == want[1]  # the state was kept
    ps.reset()
    assert dev_call(ps, text) == host_calls([text])[0]  # exactly max_lines


def test_max_pdus_overflow(ais):
    text = b"".join(c[1] for c in CASES if c[0].startswith("fill-")) + nc.text600()[:50]
    rest = nc.text600()[50:]
    want = host_calls([text, rest], pdu_cap=4)
    ps = parser(ais, max_pdus=4)
    ps.work(text)
    with pytest.raises(OverflowError):
        ps.messages()
    recs, data, times, cnt = ps.messages(overflow_ok=True)
    assert (nc.as_tuples(recs, data, times), cnt) == want[0] and cnt["FOUND"] == 6 and cnt["KEPT"] == 4 and ps.found == 6
    assert dev_call(ps, rest) == want[1]


def _deframed(ais, nch, seed):
    import torch

    rng = np.random.default_rng(seed)
    streams = [np.asarray(hc.ais_stream(rng, 6, lengths=(11, 62))[0], np.uint8) for _ in range(nch)]
    stride = max(len(x) for x in streams) + 5
    hd = ais.hdlc_deframer_batch(11, 64, nch, stride, 1 << 12)
    rows, n = hc.pack(streams, stride)
    hd.work(torch.from_numpy(rows).cuda(), torch.from_numpy(n).cuda())
    return hd


def _cleared(pdu):
    fill = (6 - (8 * len(pdu)) % 6) % 6
    v = int.from_bytes(pdu, "big")
    return ((v >> (6 - fill)) << (6 - fill)).to_bytes(len(pdu), "big") if fill else bytes(pdu)


def test_device_chain_closes(ais):
    nch = 8
    des = [chr(65 + c) for c in range(nch)]
    hd = _deframed(ais, nch, 77)
    pdus = hd.pdus(as_list=True)
    assert len(pdus) >= 3 * nch
    nm = ais.pdu_to_nmea_batch(des, nch, 1 << 12, 64)
    ps = ais.nmea_to_pdu_batch(des, 64, nm.text_cap, 1 << 13, 1 << 12, ref_tail=True)
    md = ais.pdu_decode_batch(nch, 1 << 12, 64)
    vt = ais.vessel_table_batch(1 << 12, 1 << 12)
    nm.work(hd)
    ps.work_nmea(nm)
    md.work(ps)
    vt.work(md, 5, deframer=ps)
    recs, data, times, cnt = ps.messages()
    assert cnt["FOUND"] == cnt["KEPT"] == len(pdus) and cnt["REJ_FRAGMENT"] == 0 and cnt["CARRIED"] == 0
    got = nc.as_tuples(recs, data, times)
    assert [(g[0], g[4]) for g in got] == [(c, _cleared(p)) for c, _, p in pdus]
    rows = md.messages()
    assert len(rows) == len(pdus)
    for row, (_, _, p) in zip(rows, pdus):
        want = ais.msg_decode(_cleared(p))
        assert all(int(row[k.lower()]) == want[k] for k in ais.MSG_COLUMNS)
        assert (row["callsign"], row["name"], row["destination"]) == (want["callsign"], want["name"], want["destination"])
    host = ais.vessel_table(1 << 12)
    host.update(rows, None, 5, recs=recs)
    assert np.array_equal(vt.vessels(), host.vessels()) and len(host.vessels()) > 0


def test_two_handles_on_two_streams_and_teardown(ais):
    import torch

    a_text, b_text = dict(CASES)["mixed"], nc.text600() * 3
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    pa, pb = parser(ais), parser(ais)
    pca = nc.pieces(a_text, nc.random_cuts(np.random.default_rng(5), len(a_text), 4))
    pcb = nc.pieces(b_text, nc.random_cuts(np.random.default_rng(6), len(b_text), 4))
    wa, wb = host_calls(pca), host_calls(pcb)
    for k in range(5):
        pa.work(pca[k], stream=sa)
        pb.work(pcb[k], stream=sb)
        ra, rb = pa.messages(stream=sa), pb.messages(stream=sb)
        assert (nc.as_tuples(*ra[:3]), ra[3]) == wa[k] and (nc.as_tuples(*rb[:3]), rb[3]) == wb[k]
    # teardown with work queued
    for _ in range(4):
        pa.work(a_text, stream=sa)
    del pa
    torch.cuda.synchronize()
