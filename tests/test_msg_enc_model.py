"""The ITU-R M.1371 field encoder off the device: the host aisx_msg_encode (ais_amd.msg_encode) against the pure-Python
encoder of tests/msg_enc_cases.py, round trips through the decoders, the published sentences, the kernel body
(gr-ais_amd/csrc/k_msg_enc.h) on the CPU lane model (tests/emul_msg_enc) bit for bit against the host function, the same
comparison once in a stand-alone program built with AddressSanitizer and UndefinedBehaviorSanitizer
(tests/emul_msg_enc/enc_san.cpp: nothing of it is loaded into this process), the C ABI's argument checks and its refusal
without a device.  -m "not gpu"."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import emul_load
from emul_load import i32, vp
import msg_cases as mc
import msg_enc_cases as ec
import torch  # noqa: F401  (before libaisx.so: one HIP runtime in the process)

HERE = os.path.dirname(os.path.abspath(__file__))
EMUL = os.path.join(HERE, "emul_msg_enc")
CSRC = emul_load.CSRC
NCOL = len(mc.COLUMNS)


def emu():
    return emul_load.load("emul_msg_enc", [
        ("emu_msg_enc_create", vp, [i32, i32, i32]),
        ("emu_msg_enc_destroy", None, [vp]),
        ("emu_msg_enc_group_records", i32, []),
        ("emu_msg_enc_process", i32, [vp, vp, C.c_longlong, vp, vp, vp, vp, i32, i32]),
        ("emu_msg_enc_read", None, [vp, vp, vp, vp, vp]),
        ("emu_msg_enc_plan", i32, [i32, i32, i32, vp]),
    ], extra_deps=("aisx_msg_enc.cpp",))


@pytest.fixture(scope="module")
def cases():
    return ec.all_rows(np.random.default_rng(7))


@pytest.fixture(scope="module")
def host(cases):
    """aisx_msg_encode of every case, computed once: [(payload, status)]"""
    import ais_amd

    return [ais_amd.msg_encode(row, a, p) for row, a, p, _, _ in cases]


def test_flags_and_lengths():
    import ais_amd

    assert (ais_amd.MSG_ENC_NO_MMSI, ais_amd.MSG_ENC_NO_LAYOUT, ais_amd.MSG_ENC_RANGE, ais_amd.MSG_ENC_BAD_CHAR,
            ais_amd.MSG_ENC_BAD_ROW) == (1, 2, 4, 8, 16) == (ec.NO_MMSI, ec.NO_LAYOUT, ec.RANGE, ec.BAD_CHAR, ec.BAD_ROW)
    assert [ec.LENGTHS[k] for k in ("pos_a", "base", "static", "pos_b", "pos_b_ext", "aton", "24a", "24b", "24x", "long")] == \
        [21, 21, 53, 21, 39, 34, 20, 21, 20, 12]
    for layout, n in ec.LENGTHS.items():
        assert n == (mc.LAYOUTS[layout][0] + 7) // 8
        t, part = mc.LAYOUT_TYPE[layout]
        p, st = ais_amd.msg_encode(ec.blank_row(TYPE=t, PART=ec.NA if part is None else part, MMSI=1))
        assert st == 0 and len(p) == n, layout
    # the uncovered bits are exactly what no field of msg_cases.LAYOUTS covers
    for layout, gaps in ec.UNCOVERED.items():
        seen = np.zeros(8 * ec.LENGTHS[layout], dtype=bool)
        for name, start, width, _ in mc.fields(layout):
            seen[start:start + width] = True
        want = np.ones_like(seen)
        for a, b in gaps:
            want[a:b + 1] = False
        assert (seen == want).all(), layout


def test_host_function_equals_the_python_encoder(cases, host):
    assert len(cases) >= 400
    layouts = set()
    for (row, a, p, note, expect), (got, st) in zip(cases, host):
        want, wst = ec.encode(row, a, p)
        assert (got, st) == (want, wst), (note, got.hex(), want.hex(), st, wst)
        if expect is not None:
            assert st == expect, note
        assert (len(got) == 0) == (st != 0), note  # a refused row: len 0
        if st == 0:
            d = mc.decode(got)
            layouts.add(ec.layout_of(d["TYPE"], d["PART"]))
    assert layouts == set(ec.LENGTHS)


def test_defaults_and_type_27(cases, host):
    import ais_amd

    d = mc.decode(ais_amd.msg_encode(ec.blank_row(TYPE=1, MMSI=7))[0])
    assert [d[k] for k in ("NAV_STATUS", "ROT", "SOG", "LON", "LAT", "COG", "HEADING", "SECOND", "REPEAT", "ACCURACY", "RADIO")] == \
        [15, -128, 1023, 108600000, 54600000, 3600, 511, 60, 0, 0, 0]
    d = mc.decode(ais_amd.msg_encode(ec.blank_row(TYPE=4, MMSI=7))[0])
    assert (d["HOUR"], d["MINUTE"], d["SECOND"], d["YEAR"]) == (24, 60, 60, 0)
    assert mc.decode(ais_amd.msg_encode(ec.blank_row(TYPE=5, MMSI=7))[0])["DTE"] == 1
    d = mc.decode(ais_amd.msg_encode(ec.blank_row(TYPE=27, MMSI=7))[0])
    assert (d["LON"], d["LAT"], d["SOG"], d["COG"], d["NAV_STATUS"]) == (108600000, 54600000, 1023, 3600, 15)

    def enc27(**kw):
        p, st = ais_amd.msg_encode(ec.blank_row(TYPE=27, MMSI=7, **kw))
        return (st, None) if st else (0, mc.decode(p))

    for v, want in ((0, 0), (499, 0), (500, 1000), (501, 1000), (1499, 1000), (1500, 2000), (-499, 0), (-500, -1000), (-501, -1000)):
        assert enc27(LON=v)[1]["LON"] == want and enc27(LAT=v)[1]["LAT"] == want, v
    for v, want in ((0, 0), (4, 0), (5, 10), (614, 610), (615, 620), (1022, 620), (1023, 1023)):
        assert enc27(SOG=v)[1]["SOG"] == want, v
    assert enc27(SOG=1024)[0] == ec.RANGE and enc27(SOG=-1)[0] == ec.RANGE
    for v, want in ((0, 0), (3594, 3590), (3595, 0), (3599, 0), (3600, 3600), (4000, 3600)):
        assert enc27(COG=v)[1]["COG"] == want, v
    assert enc27(COG=-1)[0] == ec.RANGE
    assert enc27(LON=131072 * 1000)[0] == ec.RANGE and enc27(LAT=-65537 * 1000)[0] == ec.RANGE


def test_strings(cases, host):
    import ais_amd

    def enc(**kw):
        return ais_amd.msg_encode(ec.blank_row(TYPE=5, MMSI=7, **kw))

    p, st = enc()
    d = mc.decode(p)
    assert st == 0 and d["callsign"] == b"@" * 7 and d["name"] == b"@" * 20 and d["destination"] == b"@" * 20
    assert mc.decode(enc(name=b"AB\0CD")[0])["name"] == b"AB" + b"@" * 18  # (from the first NUL on, zeros)
    assert mc.decode(enc(name=b"\0XYZ")[0])["name"] == b"@" * 20
    assert mc.decode(enc(callsign=bytes([32, 63, 64, 95]))[0])["callsign"] == bytes([32, 63, 64, 95]) + b"@@@"
    for b in (31, 96, ord("a"), 127, 128, 255):
        assert enc(destination=bytes([65, b])) == (b"", ec.BAD_CHAR), b
    assert enc(name=b"AB\0a")[1] == 0  # (behind the NUL nothing is looked at)
    # byte [7] of a row's strings is ignored
    import ais_amd.framing as fr
    from ais_amd import _lib

    cols, strs = fr.msg_row(ec.blank_row(TYPE=5, MMSI=7, callsign=b"CALLSIG"))
    out = []
    for b7 in (0, ord("a"), 255):
        strs[7] = b7
        pdu = np.zeros(56, np.uint8)
        n, s = C.c_int(), C.c_int()
        assert _lib.lib(device=False).aisx_msg_encode(cols.ctypes.data, strs.ctypes.data, 0, -1, pdu.ctypes.data, 56, C.byref(n),
                                                      C.byref(s)) == 0
        out.append((pdu.tobytes(), n.value, s.value))
    assert out[0] == out[1] == out[2] and out[0][1:] == (53, 0)
    # strs = NULL: all NUL
    pdu = np.zeros(56, np.uint8)
    assert _lib.lib(device=False).aisx_msg_encode(cols.ctypes.data, None, 0, -1, pdu.ctypes.data, 56, C.byref(n), C.byref(s)) == 0
    assert (pdu[:53].tobytes(), s.value) == enc()


def test_statuses_and_overrides():
    import ais_amd
    from ais_amd import _lib

    ok = ec.blank_row(TYPE=1, MMSI=5)
    assert ais_amd.msg_encode(ec.blank_row(TYPE=1))[1] == ec.NO_MMSI
    assert ais_amd.msg_encode(ec.blank_row(TYPE=1, MMSI=1 << 30))[1] == ec.NO_MMSI | ec.RANGE
    for t in (6, 0, 64, ec.NA):
        assert ais_amd.msg_encode(ec.blank_row(TYPE=t, MMSI=5)) == (b"", ec.NO_LAYOUT), t
        assert ais_amd.msg_encode(ec.blank_row(TYPE=t)) == (b"", ec.NO_LAYOUT | ec.NO_MMSI), t
    assert ais_amd.msg_encode(ec.blank_row(TYPE=5, MMSI=5, IMO=1 << 30, name=b"x"))[1] == ec.RANGE | ec.BAD_CHAR
    # as_type and as_part override the columns; TYPE and PART are written as chosen; FLAGS is ignored
    p, st = ais_amd.msg_encode(ec.blank_row(TYPE=6, MMSI=5, FLAGS=7), as_type=18)
    assert st == 0 and len(p) == 21 and mc.decode(p)["TYPE"] == 18
    assert ais_amd.msg_encode(ok, as_type=64) == ais_amd.msg_encode(ok) == ais_amd.msg_encode(ok, as_type=-1)
    assert ais_amd.msg_encode(ok, as_type=6) == (b"", ec.NO_LAYOUT)
    row = ec.blank_row(TYPE=24, PART=1, MMSI=5, name=b"N", callsign=b"C")
    d = mc.decode(ais_amd.msg_encode(row)[0])
    assert (d["PART"], d["callsign"], d["name"]) == (1, b"C@@@@@@", b"")
    d = mc.decode(ais_amd.msg_encode(row, as_part=0)[0])
    assert (d["PART"], d["callsign"], d["name"]) == (0, b"", b"N" + b"@" * 19)
    p, st = ais_amd.msg_encode(ec.blank_row(TYPE=24, MMSI=5))
    assert st == 0 and len(p) == 20 and mc.decode(p)["PART"] == 3 and p[5:] == b"\0" * 15
    assert ais_amd.msg_encode(row, as_part=4) == (b"", ec.RANGE)
    # one MSG_DTYPE record works as a dict does
    rec = np.zeros(1, dtype=ais_amd.MSG_DTYPE)
    for c in mc.COLUMNS:
        rec[c.lower()] = row[c]
    rec["name"], rec["callsign"] = b"N", b"C"
    assert ais_amd.msg_encode(rec[0]) == ais_amd.msg_encode(row)
    # cap one short: AISX_ERR_OVERFLOW, nothing written
    import ais_amd.framing as fr

    cols, strs = fr.msg_row(ok)
    pdu = np.full(56, 0xEE, np.uint8)
    n, s = C.c_int(-7), C.c_int(-7)
    L = _lib.lib(device=False)
    assert L.aisx_msg_encode(cols.ctypes.data, strs.ctypes.data, 0, -1, pdu.ctypes.data, 20, C.byref(n), C.byref(s)) == _lib.AISX_ERR_OVERFLOW
    assert (pdu == 0xEE).all() and (n.value, s.value) == (-7, -7)
    assert L.aisx_msg_encode(cols.ctypes.data, strs.ctypes.data, 0, -1, pdu.ctypes.data, 21, C.byref(n), C.byref(s)) == 0
    assert (n.value, s.value) == (21, 0) and (pdu[21:] == 0xEE).all()
    cols[mc.COLUMNS.index("MMSI")] = -1  # a refused row writes nothing, whatever the cap
    pdu[:] = 0xEE
    assert L.aisx_msg_encode(cols.ctypes.data, strs.ctypes.data, 0, -1, pdu.ctypes.data, 0, C.byref(n), C.byref(s)) == 0
    assert (pdu == 0xEE).all() and (n.value, s.value) == (0, ec.NO_MMSI | ec.RANGE)


def test_round_trip_rows(cases, host):
    """decode(encode(row)) gives back every carried column and the strings, for every accepted row"""
    n = 0
    for (row, a, p, note, _), (got, st) in zip(cases, host):
        want = ec.expected_decode(row, a, p)
        assert (want is None) == (st != 0), note
        if st:
            continue
        d = mc.decode(got)
        assert d["FLAGS"] == 1 and ec.uncovered_are_zero(got, ec.layout_of(d["TYPE"], d["PART"])), note
        assert {k: d[k] for k in want} == want, note
        n += 1
    assert n > 300


def test_round_trip_payloads():
    """encode(decode(p)) == p for every COMPLETE payload of a layout, cut to the layout's length and with the
    uncovered bits zero; the three published sentences come back octet for octet.  Type 27 payloads are used as they
    are; one whose COG field holds 360..510, which the protocol does not use, decodes to 3600..5100 and by the rule
    (COG >= 3600 -> 511) comes back with 511 there and every other bit unchanged (msg_enc_cases.canonical)."""
    import ais_amd

    n = {}
    for p in mc.all_payloads(np.random.default_rng(41)):
        d = ais_amd.msg_decode(p)
        if d["FLAGS"] != 1:
            continue
        q = ec.canonical(p)
        layout = ec.layout_of(d["TYPE"], d["PART"])
        assert ais_amd.msg_encode(ais_amd.msg_decode(q)) == (q, 0), (layout, p.hex())
        assert ais_amd.msg_encode(d) == (q, 0), (layout, p.hex())
        n[layout] = n.get(layout, 0) + 1
    assert set(n) == set(ec.LENGTHS) and min(n.values()) >= 3, n
    for chars, _ in mc.PUBLISHED:
        p = mc.chars_to_payload(chars)
        d = ais_amd.msg_decode(p)
        assert ec.uncovered_are_zero(p, ec.layout_of(d["TYPE"], d["PART"]))
        assert ais_amd.msg_encode(d) == (p, 0), chars


# ---- the lane model ---------------------------------------------------------------------------------------------------
class EmuEnc:
    def __init__(self, nchan, max_rows, table_rows):
        self.h = emu().emu_msg_enc_create(nchan, max_rows, table_rows)
        assert self.h
        self.max_rows = max_rows

    def __del__(self):
        emu().emu_msg_enc_destroy(self.h)

    def process(self, cols, strs, nrows, idx=None, chan=None, as_type=0, as_part=-1):
        n = np.array([nrows], np.int32)
        assert cols.flags.c_contiguous and strs.flags.c_contiguous
        self.keep = (cols, strs, idx, chan, n)
        return emu().emu_msg_enc_process(self.h, cols.ctypes.data, cols.shape[1], strs.ctypes.data,
                                         idx.ctypes.data if idx is not None else None, n.ctypes.data,
                                         chan.ctypes.data if chan is not None else None, as_type, as_part)

    def read(self):
        recs = np.zeros(self.max_rows, dtype=mc.REC_DTYPE)
        data = np.zeros((self.max_rows, 56), dtype=np.uint8)
        status = np.zeros(self.max_rows, dtype=np.int32)
        cnt = np.zeros(5, dtype=np.int32)
        emu().emu_msg_enc_read(self.h, recs.ctypes.data, data.ctypes.data, status.ctypes.data, cnt.ctypes.data)
        return cnt, recs, data, status


def host_row_encoder(as_type=0, as_part=-1):
    """aisx_msg_encode on one row of a table: (cols [ncol], strs [48]) -> (bytes, status)"""
    from ais_amd import _lib

    L = _lib.lib(device=False)

    def f(c, s):
        c = np.ascontiguousarray(c, dtype=np.int32)
        s = np.ascontiguousarray(s, dtype=np.uint8)
        pdu = np.zeros(56, np.uint8)
        n, st = C.c_int(), C.c_int()
        assert L.aisx_msg_encode(c.ctypes.data, s.ctypes.data, as_type, as_part, pdu.ctypes.data, 56, C.byref(n), C.byref(st)) == 0
        return pdu[: n.value].tobytes(), st.value

    return f


def mixed_rows():
    """about 1000 mixed rows as dicts: the cases, and decoded payloads of every type and length"""
    import ais_amd

    rows = [c[0] for c in ec.all_rows(np.random.default_rng(7))]
    for p in mc.random_cases(np.random.default_rng(3), per_type=2) + mc.layout_cases(np.random.default_rng(4)):
        rows.append(ais_amd.msg_decode(p))
    return rows[:1003]


def wide_table(rows):
    """rows -> (cols with col_stride > n, strs with byte [7] set, n)"""
    cols, strs = ec.table_of(rows)
    wide = np.full((NCOL, len(rows) + 9), 0x77777777, dtype=np.int32)
    wide[:, : len(rows)] = cols
    strs[:, 7] = np.arange(len(rows)) % 251  # (byte [7] is ignored)
    return wide, strs, len(rows)


@pytest.fixture(scope="module")
def table():
    return wide_table(mixed_rows())


UNWRITTEN = 0x5A


def check_list(got, want, n):
    cnt, recs, data, status = got
    wrecs, wdata, wstatus = want
    good = int((wstatus == 0).sum())
    assert list(cnt) == [n, n, 0, good, n - good]
    assert (status[:n] == wstatus).all(), np.flatnonzero(status[:n] != wstatus)[:5]
    assert recs[:n].tobytes() == wrecs.tobytes()
    assert (data[:n] == wdata).all()  # (all 56 bytes of every record)
    # nothing beyond the records is written
    assert (recs[n:].view(np.uint8) == UNWRITTEN).all() and (data[n:] == UNWRITTEN).all() and (status[n:].view(np.uint8) == UNWRITTEN).all()


def test_lane_model_equals_the_host_function(table):
    cols, strs, rows = table
    assert rows > 1000
    G = emu().emu_msg_enc_group_records()
    assert rows > 4 * G  # (two groups of two waves: every wave loops)
    for n in (0, 1, 63, 64, 65, 257, rows):
        b = EmuEnc(3, rows, rows)
        assert b.process(cols, strs, n)
        check_list(b.read(), ec.expected_list(cols, strs, n, rows, 3, host_row_encoder()), n)
    b = EmuEnc(3, rows, rows)
    for a, p in ((1, -1), (5, -1), (24, 0), (24, -1), (27, -1)):
        assert b.process(cols, strs, 300, as_type=a, as_part=p)  # (a second call overwrites the first)
        check_list((lambda r: (r[0], r[1][:300], r[2][:300], r[3][:300]))(b.read()),
                   ec.expected_list(cols, strs, 300, rows, 3, host_row_encoder(a, p)), 300)


def test_lane_model_index_list_and_channels(table):
    cols, strs, rows = table
    rng = np.random.default_rng(9)
    nchan, max_rows = 4, 700
    idx = np.concatenate([np.arange(rows - 1, rows - 301, -1), rng.integers(0, 50, 200), [-1, rows, rows + 5, -(1 << 31), (1 << 31) - 1],
                          rng.integers(0, rows, 195)]).astype(np.int32)  # reversed, repeats, out of range
    assert len(idx) == max_rows
    by_row = rng.integers(0, nchan, rows).astype(np.int32)
    by_row[[3, 40, rows - 2]] = [nchan, -1, ec.NA]
    by_rec = rng.integers(0, nchan, max_rows).astype(np.int32)
    by_rec[[0, 64, 699]] = [nchan, -1, ec.NA]
    f = host_row_encoder()
    b = EmuEnc(nchan, max_rows, rows)
    assert b.process(cols, strs, max_rows, idx=idx)
    check_list(b.read(), ec.expected_list(cols, strs, max_rows, rows, nchan, f, idx=idx), max_rows)
    assert b.process(cols, strs, max_rows, idx=idx, chan=by_row)  # with an index list: the channel of the table row
    got = b.read()
    check_list(got, ec.expected_list(cols, strs, max_rows, rows, nchan, f, idx=idx, chan=by_row), max_rows)
    assert (got[3][:max_rows] == ec.BAD_ROW).sum() >= 5 + 3
    assert b.process(cols, strs, max_rows, chan=by_rec)  # without: the channel of the record
    got = b.read()
    check_list(got, ec.expected_list(cols, strs, max_rows, rows, nchan, f, chan=by_rec), max_rows)
    assert list(got[3][[0, 64, 699]]) == [ec.BAD_ROW] * 3 and list(got[1]["chan"][[0, 64, 699]]) == [0, 0, 0]
    # a table smaller than the list: the rows beyond it are bad rows, and the table is not read for them
    b = EmuEnc(nchan, max_rows, 100)
    assert b.process(cols, strs, 130)
    got = b.read()
    check_list((got[0], got[1][:130], got[2][:130], got[3][:130]), ec.expected_list(cols, strs, 130, 100, nchan, f), 130)
    assert (got[3][100:130] == ec.BAD_ROW).all()


def test_lane_model_bad_row_count(table):
    cols, strs, rows = table
    b = EmuEnc(2, 200, rows)
    for bad_n in (-1, 201):
        assert b.process(cols, strs, bad_n)
        cnt, recs, data, status = b.read()
        assert list(cnt) == [0, 0, 1, 0, 0]
        assert (recs.view(np.uint8) == UNWRITTEN).all() and (data == UNWRITTEN).all()  # (nothing written)
        assert b.process(cols, strs, 70)  # the next call is clean
        check_list((lambda r: (r[0], r[1][:70], r[2][:70], r[3][:70]))(b.read()),
                   ec.expected_list(cols, strs, 70, rows, 2, host_row_encoder()), 70)
        b = EmuEnc(2, 200, rows)


def _stale(exe, deps):
    return not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps)


def test_stand_alone_program_under_the_sanitizers():
    exe = os.path.join(EMUL, "enc_san")
    deps = [os.path.join(EMUL, "enc_san.cpp"), os.path.join(EMUL, "emul_msg_enc.cpp"), os.path.join(CSRC, "aisx_msg_enc.cpp"),
            os.path.join(CSRC, "aisx_msg.cpp"), os.path.join(CSRC, "aisx_msgtab.h"), os.path.join(CSRC, "k_msg_enc.h")]
    if _stale(exe, deps):
        subprocess.check_call(["make", "-C", EMUL, "-s", "-B", "enc_san"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("enc_san ok"), (r.returncode, r.stdout[-400:], r.stderr[-2000:])


def test_arguments_and_no_device():
    import ais_amd
    from ais_amd import _lib

    bad = [(0, 10, 10), (2, 0, 10), (2, 10, 0), (2, (1 << 28) + 1, 10), (-1, 10, 10)]
    for a in bad:
        assert not emu().emu_msg_enc_create(*a)
    out = (C.c_longlong * 1)()
    assert emu().emu_msg_enc_plan(2, 1000, 1000, out) == 1 and out[0] == 4
    assert emu().emu_msg_enc_plan(2, 1 << 28, 10, out) == 1 and out[0] == 4096
    L = _lib.lib()
    h = C.c_void_p()
    for a in bad:
        assert L.aisx_msg_enc_batch_create(C.byref(h), *a) == _lib.AISX_ERR_INVALID
    assert L.aisx_msg_enc_batch_create(None, 2, 10, 10) == _lib.AISX_ERR_INVALID
    assert L.aisx_msg_enc_batch_process(None, None, 0, None, None, None, None, 0, -1, None) == _lib.AISX_ERR_INVALID
    assert L.aisx_msg_enc_batch_results_device(None, None, None, None, None) == _lib.AISX_ERR_INVALID
    assert L.aisx_msg_enc_batch_read(None, None, None, 0, None, 0, None, None, None) == _lib.AISX_ERR_INVALID
    assert L.aisx_msg_enc_batch_destroy(None) == _lib.AISX_OK
    # the model's (and the C ABI's) per-call check: col_stride >= table_rows, strings aligned to 4 bytes
    cols = np.zeros((NCOL, 10), np.int32)
    strs = np.zeros(10 * 48 + 4, np.uint8)
    b = EmuEnc(1, 10, 10)
    n = np.array([0], np.int32)
    assert emu().emu_msg_enc_process(b.h, cols.ctypes.data, 9, strs.ctypes.data, None, n.ctypes.data, None, 0, -1) == 0
    assert emu().emu_msg_enc_process(b.h, cols.ctypes.data, 10, strs.ctypes.data + 1, None, n.ctypes.data, None, 0, -1) == 0
    assert emu().emu_msg_enc_process(b.h, cols.ctypes.data, 10, None, None, n.ctypes.data, None, 0, -1) == 1
    # aisx_msg_encode's pointers
    c1, s1, p1 = np.zeros(NCOL, np.int32), np.zeros(48, np.uint8), np.zeros(56, np.uint8)
    ln, st = C.c_int(), C.c_int()
    args = [c1.ctypes.data, s1.ctypes.data, 0, -1, p1.ctypes.data, 56, C.byref(ln), C.byref(st)]
    for k in (0, 4, 6, 7):
        a = list(args)
        a[k] = None
        assert L.aisx_msg_encode(*a) == _lib.AISX_ERR_INVALID, k
    a = list(args)
    a[5] = -1
    assert L.aisx_msg_encode(*a) == _lib.AISX_ERR_INVALID
    with pytest.raises(ValueError):
        ais_amd.msg_encode(ec.blank_row(TYPE=5, MMSI=1, callsign=b"TOOLONG8"))
    nd = C.c_int(-1)
    L.aisx_device_count(C.byref(nd))
    rc = L.aisx_msg_enc_batch_create(C.byref(h), 2, 10, 10)
    if nd.value <= 0:
        assert rc == _lib.AISX_ERR_NO_DEVICE
        with pytest.raises(_lib.NoDeviceError):
            ais_amd.pdu_encode_batch(2, 10, 10)
    else:
        assert rc == _lib.AISX_OK
        assert L.aisx_msg_enc_batch_destroy(h) == 0
    with pytest.raises(ValueError):
        ais_amd.pdu_encode_batch(2, 0, 10)
