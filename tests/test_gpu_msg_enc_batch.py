"""The field encoder on the MI355X (aisx_msg_enc_batch_*, ais_amd.pdu_encode_batch) against the host aisx_msg_encode
that is its specification, bit for bit -- bytes (all 56 per record), records, status and counts -- on the lane model's
cases (tests/test_msg_enc_model.py), two handles side by side and a call that overwrites another; then the loops on the
device: encoder -> decoder on 5000 mixed rows, the vessel table's snapshot through the standard armourer, the parser and
the decoder into a second vessel table, its changed list, and the dedup stage fed from the encoder's list.  -m gpu."""
import numpy as np
import pytest

import msg_cases as mc
import msg_enc_cases as ec
import test_msg_enc_model as tm

pytestmark = pytest.mark.gpu

NCOL = len(mc.COLUMNS)


@pytest.fixture(scope="module")
def ais():
    import torch

    assert torch.cuda.is_available()
    import ais_amd

    return ais_amd


@pytest.fixture(scope="module")
def rows():
    return tm.mixed_rows()


@pytest.fixture(scope="module")
def table(rows):
    """the lane model's table on the host and on the device: (cols, strs, n, device cols, device strs)"""
    import torch

    cols, strs, n = tm.wide_table(rows)
    return cols, strs, n, torch.from_numpy(cols).cuda(), torch.from_numpy(strs).cuda()


def dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run(enc, table, n, idx=None, chan=None, as_type=0, as_part=-1, stream=None):
    """queues one call on the device table; returns what has to stay alive until it has run"""
    import torch

    with torch.cuda.stream(stream or torch.cuda.current_stream()):
        keep = (torch.tensor([n], dtype=torch.int32, device="cuda"), dev(idx) if idx is not None else None,
                dev(chan) if chan is not None else None)
    enc.work((table[3], table[4], keep[0]) + ((keep[1],) if idx is not None else ()), as_type=as_type, as_part=as_part, chan=keep[2],
             stream=stream)
    return keep


def check(enc, want, n, stream=None):
    wrecs, wdata, wstatus = want
    recs, data = enc.pdus(stream=stream)
    status = enc.status(stream=stream)
    good = int((wstatus == 0).sum())
    assert enc.counts == dict(found=n, records=n, bad_input=0, encoded=good, refused=n - good)
    assert len(recs) == n and (status == wstatus).all()
    assert recs.tobytes() == wrecs.tobytes()
    assert (data.reshape(n, 56) == wdata).all()  # (all 56 bytes of every record)


def test_device_equals_the_host_function(ais, table):
    cols, strs, rows = table[:3]
    f = tm.host_row_encoder()
    for n in (0, 1, 63, 64, 65, 257, rows):
        enc = ais.pdu_encode_batch(3, rows, rows)
        keep = run(enc, table, n)
        check(enc, ec.expected_list(cols, strs, n, rows, 3, f), n)
    enc = ais.pdu_encode_batch(3, rows, rows)
    for n, a, p in ((rows, 0, -1), (300, 1, -1), (300, 5, -1), (65, 24, 0), (300, 24, -1), (300, 27, -1)):
        keep = run(enc, table, n, as_type=a, as_part=p)  # (a second call overwrites the first)
        check(enc, ec.expected_list(cols, strs, n, rows, 3, tm.host_row_encoder(a, p)), n)
    del keep


def test_device_index_list_and_channels(ais, table):
    cols, strs, rows = table[:3]
    rng = np.random.default_rng(9)
    nchan, max_rows = 4, 700
    idx = np.concatenate([np.arange(rows - 1, rows - 301, -1), rng.integers(0, 50, 200), [-1, rows, rows + 5, -(1 << 31), (1 << 31) - 1],
                          rng.integers(0, rows, 195)]).astype(np.int32)  # reversed, repeats, out of range
    by_row = rng.integers(0, nchan, rows).astype(np.int32)
    by_row[[3, 40, rows - 2]] = [nchan, -1, ec.NA]
    by_rec = rng.integers(0, nchan, max_rows).astype(np.int32)
    by_rec[[0, 64, 699]] = [nchan, -1, ec.NA]
    f = tm.host_row_encoder()
    enc = ais.pdu_encode_batch(nchan, max_rows, rows)
    keep = run(enc, table, max_rows, idx=idx)
    check(enc, ec.expected_list(cols, strs, max_rows, rows, nchan, f, idx=idx), max_rows)
    keep = run(enc, table, max_rows, idx=idx, chan=by_row)
    check(enc, ec.expected_list(cols, strs, max_rows, rows, nchan, f, idx=idx, chan=by_row), max_rows)
    keep = run(enc, table, max_rows, chan=by_rec)
    check(enc, ec.expected_list(cols, strs, max_rows, rows, nchan, f, chan=by_rec), max_rows)
    # a table smaller than the list: the rows beyond it are bad rows
    enc = ais.pdu_encode_batch(nchan, max_rows, 100)
    keep = run(enc, table, 130)
    check(enc, ec.expected_list(cols, strs, 130, 100, nchan, f), 130)
    assert (enc.status()[100:] == ec.BAD_ROW).all()
    del keep


def test_device_bad_row_count_and_arguments(ais, table):
    import torch

    cols, strs, rows = table[:3]
    for bad_n in (-1, 201):
        enc = ais.pdu_encode_batch(2, 200, rows)
        keep = run(enc, table, bad_n)
        with pytest.raises(ValueError):
            enc.pdus()
        assert enc.counts == dict(found=0, records=0, bad_input=1, encoded=0, refused=0)
        assert len(enc.pdus()[0]) == 0  # (said once; nothing was written)
        keep = run(enc, table, 70)  # the next call is clean
        check(enc, ec.expected_list(cols, strs, 70, rows, 2, tm.host_row_encoder()), 70)
    del keep
    enc = ais.pdu_encode_batch(2, 200, rows)
    n = torch.tensor([1], dtype=torch.int32, device="cuda")
    with pytest.raises(ValueError):  # col_stride below table_rows
        enc.work((table[3][:, : rows - 1].contiguous(), table[4], n))
    with pytest.raises(ValueError):  # strings not aligned
        enc.work_device(table[3].data_ptr(), table[3].shape[1], table[4].data_ptr() + 1, n.data_ptr())
    with pytest.raises(ValueError):
        enc.work((table[3], table[4], n), changed_only=True)
    for bad in ((0, 10, 10), (2, 0, 10), (2, 10, 0)):
        with pytest.raises(ValueError):
            ais.pdu_encode_batch(*bad)
    t = ais.pdu_encode_batch(1, 16, 16)  # create / destroy without a call; the read of a handle that never worked
    assert len(t.pdus()[0]) == 0 and t.counts["records"] == 0
    enc.work((table[3], None, n))  # no strings: all NUL
    want = ec.expected_list(cols, np.zeros_like(strs), 1, rows, 2, tm.host_row_encoder())
    check(enc, want, 1)


def test_two_handles_side_by_side(ais, table):
    import torch

    cols, strs, rows = table[:3]
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    a, b = ais.pdu_encode_batch(3, rows, rows), ais.pdu_encode_batch(1, 500, rows)
    idx = np.arange(499, -1, -1).astype(np.int32)
    keep = []
    for k in range(3):
        keep.append(run(a, table, rows - k, stream=sa))
        keep.append(run(b, table, 500 - k, idx=idx, as_type=18, stream=sb))
    check(a, ec.expected_list(cols, strs, rows - 2, rows, 3, tm.host_row_encoder()), rows - 2, stream=sa)
    check(b, ec.expected_list(cols, strs, 498, rows, 1, tm.host_row_encoder(18), idx=idx), 498, stream=sb)


def test_loop_on_the_device_encoder_to_decoder(ais, rows):
    """5000 mixed rows -> pdu_encode_batch -> pdu_decode_batch: every carried column and string is the input's (defaults
    for NA); a refused row comes back as FLAGS without COMPLETE"""
    import torch

    n = 5000
    many = [rows[(7 * i) % len(rows)] for i in range(n)]
    cols, strs = ec.table_of(many)
    enc = ais.pdu_encode_batch(1, n, n)
    md = ais.pdu_decode_batch(1, n, 64)
    d_cols, d_strs, d_n = dev(cols), dev(strs), torch.tensor([n], dtype=torch.int32, device="cuda")
    enc.work((d_cols, d_strs, d_n))
    md.work(enc)
    got = md.messages()
    status = enc.status()
    assert len(got) == n and md.found == n and enc.counts["encoded"] == int((status == 0).sum()) > n // 2
    want = {}  # (the rows repeat: the expectation is worked out once per distinct row)
    for i in range(n):
        k = (7 * i) % len(rows)
        if k not in want:
            want[k] = ec.expected_decode(many[i])
        w = want[k]
        assert (w is None) == (status[i] != 0), i
        if w is None:
            assert got["flags"][i] & 1 == 0 and got["mmsi"][i] == ec.NA
            continue
        assert got["flags"][i] == 1
        for name, v in w.items():
            assert got[name.lower()][i] == (v.rstrip(b"\0") if isinstance(v, bytes) else v), (i, name)


def _fleet(ais, rng, nships):
    """payloads of types 1 / 18 (positions) and 5 / 24A + 24B (static data) for nships MMSIs, in a shuffled order;
    {mmsi: (kind of position, kind of static)}"""
    def name(n):
        return bytes(rng.choice(np.frombuffer(b"ABCDEFGHIJKLMNOPQRSTUVWXYZ 0123456789", np.uint8), n))

    out, kinds = [], {}
    for k in range(nships):
        mmsi = 200000000 + 7919 * k
        pos, sta = ("a", "b", None)[k % 3 if k % 10 else 2], ("5", "24", None)[(k // 3) % 3]
        if pos is None and sta is None:
            pos = "a"
        kinds[mmsi] = (pos, sta)
        if pos:
            out.append(ais.msg_encode(ec.blank_row(
                TYPE=1 if pos == "a" else 18, MMSI=mmsi, SOG=int(rng.integers(0, 1023)), LON=int(rng.integers(-108000000, 108000000)),
                LAT=int(rng.integers(-54000000, 54000000)), COG=int(rng.integers(0, 3600)), HEADING=int(rng.integers(0, 360)),
                SECOND=int(rng.integers(0, 60)), ACCURACY=int(rng.integers(0, 2)), RAIM=int(rng.integers(0, 2)),
                RADIO=int(rng.integers(0, 1 << 19)))))
        if sta == "5":
            out.append(ais.msg_encode(ec.blank_row(
                TYPE=5, MMSI=mmsi, IMO=int(rng.integers(1, 1 << 30)), AIS_VERSION=1, callsign=name(7), name=name(20), destination=name(20),
                SHIPTYPE=int(rng.integers(1, 100)), TO_BOW=int(rng.integers(0, 512)), TO_STERN=int(rng.integers(0, 512)),
                TO_PORT=int(rng.integers(0, 64)), TO_STARBOARD=int(rng.integers(0, 64)), EPFD=1, MONTH=5, DAY=17, HOUR=11, MINUTE=30,
                DRAUGHT=int(rng.integers(0, 256)), DTE=0)))
        elif sta == "24":
            out.append(ais.msg_encode(ec.blank_row(TYPE=24, PART=0, MMSI=mmsi, name=name(20))))
            out.append(ais.msg_encode(ec.blank_row(TYPE=24, PART=1, MMSI=mmsi, callsign=name(7), SHIPTYPE=int(rng.integers(1, 100)),
                                                   TO_BOW=int(rng.integers(0, 512)), TO_STERN=int(rng.integers(0, 512)),
                                                   TO_PORT=int(rng.integers(0, 64)), TO_STARBOARD=int(rng.integers(0, 64)))))
    assert all(st == 0 for _, st in out)
    order = rng.permutation(len(out))
    return [out[i][0] for i in order], kinds


POSITION = ("LON", "LAT", "SOG", "COG", "HEADING", "SECOND", "ACCURACY", "RAIM")
STATIC = ("SHIPTYPE", "TO_BOW", "TO_STERN", "TO_PORT", "TO_STARBOARD")
STATIC_5 = ("IMO", "AIS_VERSION", "EPFD", "MONTH", "DAY", "HOUR", "MINUTE", "DRAUGHT", "DTE")


def test_snapshot_of_the_vessel_table(ais):
    """vessel table -> encoder (as type 1, then as type 5) -> standard armourer -> parser -> decoder -> a second vessel
    table: its position and static columns are the first's; then only what an update changed, in the changed list's
    order and on the vessels' channels"""
    import torch

    rng = np.random.default_rng(77)
    nships, cap, max_pdus = 300, 512, 1024
    payloads, kinds = _fleet(ais, rng, nships)
    recs, data = mc.pack(payloads, rng, nchan=2, max_pdus=max_pdus)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    md0, vt = ais.pdu_decode_batch(2, max_pdus, 64), ais.vessel_table_batch(cap, max_pdus)
    enc = ais.pdu_encode_batch(2, cap, cap)
    nm = ais.pdu_to_nmea_batch(["A", "B"], 2, cap, 64, standard=True)
    ps = ais.nmea_to_pdu_batch(["A", "B"], 64, nm.text_cap, 2 * cap, cap)
    md, vt2 = ais.pdu_decode_batch(2, cap, 64), ais.vessel_table_batch(cap, cap)
    with torch.cuda.stream(s):
        d_recs, d_data = dev(recs.view(np.uint8)), dev(data)
        d_cnt = torch.tensor([len(payloads)], dtype=torch.int32, device="cuda")
    md0.work_device(d_recs.data_ptr(), d_data.data_ptr(), d_cnt.data_ptr(), None, stream=s)
    vt.work_device(*md0.results_device()[:3], md0.results_device()[3] + 4, 1, d_recs.data_ptr(), stream=s)
    texts = []
    for k, as_type in enumerate((1, 5)):
        enc.work(vt, as_type=as_type, stream=s)  # nothing waits from here ...
        nm.work_device(*enc.results_device(), stream=s)
        ps.work_nmea(nm, stream=s)
        md.work(ps, stream=s)
        vt2.work(md, 2 + k, stream=s, deframer=ps)
        assert (enc.status(stream=s) == 0).all() and enc.counts["encoded"] == nships  # ... to here
        texts.append(nm.sentences(stream=s)[1])
        assert ps.messages(stream=s)[3]["KEPT"] == nships
    assert texts[0].count(b"!AIVDM") == nships and texts[1].count(b"!AIVDM") == 2 * nships  # (type 5: two sentences)
    first, second = vt.vessels(stream=s), vt2.vessels(stream=s)
    assert len(first) == len(second) == nships and (first["mmsi"] == second["mmsi"]).all()
    npos = nsta = 0
    for a, b in zip(first, second):
        pos, sta = kinds[int(a["mmsi"])]
        if pos:
            npos += 1
            assert all(a[c.lower()] == b[c.lower()] for c in POSITION), a["mmsi"]
        if sta:
            nsta += 1
            assert all(a[c.lower()] == b[c.lower()] for c in STATIC) and a["callsign"] == b["callsign"] and a["name"] == b["name"]
        if sta == "5":
            assert all(a[c.lower()] == b[c.lower()] for c in STATIC_5) and a["destination"] == b["destination"]
    assert npos > 200 and nsta > 150
    # a small update: exactly the changed vessels come out, in the changed list's order, on their channels
    upd = [ais.msg_encode(ec.blank_row(TYPE=1, MMSI=200000000 + 7919 * k, LON=k, LAT=-k, SOG=k))[0] for k in (250, 3, 77, 3, 120)]
    urecs, udata = mc.pack(upd, rng, nchan=2, max_pdus=max_pdus, shuffle=False)
    with torch.cuda.stream(s):
        d_recs, d_data = dev(urecs.view(np.uint8)), dev(udata)
        d_cnt = torch.tensor([len(upd)], dtype=torch.int32, device="cuda")
    md0.work_device(d_recs.data_ptr(), d_data.data_ptr(), d_cnt.data_ptr(), None, stream=s)
    vt.work_device(*md0.results_device()[:3], md0.results_device()[3] + 4, 9, d_recs.data_ptr(), stream=s)
    enc.work(vt, as_type=1, changed_only=True, chan="table", stream=s)
    out = enc.pdus(stream=s, as_list=True)
    changed = vt.changed(stream=s)
    assert [int(m) for m in changed["mmsi"]] == [200000000 + 7919 * k for k in (250, 3, 77, 120)]
    assert len(out) == 4 and enc.counts["encoded"] == 4
    for (chan, end_bit, p), v in zip(out, changed):
        d = ais.msg_decode(p)
        assert d["TYPE"] == 1 and d["MMSI"] == v["mmsi"] and (d["LON"], d["LAT"], d["SOG"]) == (v["lon"], v["lat"], v["sog"])
        assert chan == v["chan"]
    assert {c for c, _, _ in out} == {0, 1}


def test_dedup_keeps_one_of_two_identical_rows(ais):
    import torch

    rows = [ec.blank_row(TYPE=1, MMSI=1000 + k, LON=k * 1000, LAT=5) for k in (1, 2, 1, 3, 2, 4)]
    rows.append(ec.blank_row(TYPE=6, MMSI=9))  # refused: an empty record
    cols, strs = ec.table_of(rows)
    enc = ais.pdu_encode_batch(1, 16, 16)
    dd = ais.pdu_dedup_batch(1, 16, 64)
    wide = np.zeros((NCOL, 16), np.int32)
    wide[:, : len(rows)] = cols
    keep = (dev(wide), dev(strs), torch.tensor([len(rows)], dtype=torch.int32, device="cuda"))
    enc.work(keep)
    dd.work(enc, stamp=1)
    kept = dd.pdus()
    recs, data = enc.pdus()
    assert list(recs["len"]) == [21] * 6 + [0]
    got = [bytes(data[r["offset"]:r["offset"] + r["len"]]) for r in kept if r["len"]]
    assert got == [ais.msg_encode(rows[i])[0] for i in (0, 1, 3, 5)]
    assert dd.counts["in"] == 7 and dd.counts["kept"] == len(kept)
