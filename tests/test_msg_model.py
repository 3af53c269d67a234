"""The ITU-R M.1371 field decoder off the device: the host aisx_msg_decode (ais_amd.msg_decode) against the pure-Python
decoder of tests/msg_cases.py, the published sentences, the agreement with aisx_pdu_to_nmea's payload characters, the
kernel body (gr-ais_amd/csrc/k_msg.h) on the CPU lane model (tests/emul_msg) row for row against the host function,
the C ABI's argument checks and its refusal without a device.  -m "not gpu"."""
import ctypes as C
import os

import numpy as np
import pytest

import emul_load
from emul_load import i32, vp
import msg_cases as mc
import torch  # noqa: F401  (before libaisx.so: one HIP runtime in the process)

HERE = os.path.dirname(os.path.abspath(__file__))
NCOL = len(mc.COLUMNS)


def emu():
    return emul_load.load("emul_msg", [
        ("emu_msg_create", vp, [i32, i32, i32]),
        ("emu_msg_destroy", None, [vp]),
        ("emu_msg_process", None, [vp, vp, vp, vp, vp]),
        ("emu_msg_read", None, [vp, vp, vp, vp]),
        ("emu_msg_plan", i32, [i32, i32, i32, vp]),
    ])


@pytest.fixture(scope="module")
def payloads():
    return mc.all_payloads(np.random.default_rng(41))


@pytest.fixture(scope="module")
def host_rows(payloads):
    """aisx_msg_decode of every case, computed once"""
    import ais_amd

    return [mc.row_of(ais_amd.msg_decode(p)) for p in payloads]


def test_columns_and_dtype():
    import ais_amd

    assert tuple(ais_amd.MSG_COLUMNS) == mc.COLUMNS and ais_amd.MSG_NA == mc.NA
    assert ais_amd.MSG_DTYPE.names == tuple(c.lower() for c in mc.COLUMNS) + ("callsign", "name", "destination")
    hdr = open(os.path.join(os.path.dirname(HERE), "include", "aisx.h")).read()
    enum = hdr[hdr.index("AISX_MSG_COL_TYPE = 0"):hdr.index("AISX_MSG_NCOL")]
    names = [t.strip().split()[0] for t in enum.replace("\n", " ").split(",") if "AISX_MSG_COL_" in t]
    assert [n.replace("AISX_MSG_COL_", "") for n in names] == list(mc.COLUMNS)


def test_host_function_equals_the_python_decoder(payloads, host_rows):
    assert len(payloads) > 400
    for p, got in zip(payloads, host_rows):
        assert got == mc.row_of(mc.decode(p)), p.hex()


def test_published_sentences():
    import ais_amd

    for chars, want in mc.PUBLISHED:
        p = mc.chars_to_payload(chars)
        assert len(p) == 21
        got = ais_amd.msg_decode(p)
        for name, v in want.items():
            assert got[name] == v, (chars, name, got[name], v)
        assert got["FLAGS"] == 1 and got["callsign"] == b"" and got["name"] == b""
        assert mc.row_of(got) == mc.row_of(mc.decode(p))


def test_every_layout_is_exercised(payloads, host_rows):
    ty = mc.COLUMNS.index("TYPE")
    seen = {r[ty] for r in host_rows}
    assert seen >= set(range(64)) | {mc.NA}
    for name in mc.COLUMNS:
        k = mc.COLUMNS.index(name)
        assert any(r[k] != mc.NA for r in host_rows), name
    for s in range(3):
        assert any(r[NCOL + s] for r in host_rows)
    # type 27 in class-A units; the strings' '@' for 0 and nothing stripped
    import ais_amd

    rng = np.random.default_rng(5)
    d = ais_amd.msg_decode(mc.build("long", dict(LON=-3, LAT=54600, SOG=63, COG=359), 12, rng))
    assert (d["LON"], d["LAT"], d["SOG"], d["COG"]) == (-3000, 54600000, 1023, 3590)
    d = ais_amd.msg_decode(mc.build("long", dict(SOG=62, COG=511), 12, rng))
    assert (d["SOG"], d["COG"]) == (620, 3600)
    d = ais_amd.msg_decode(mc.build("24a", dict(name=[0, 1, 32, 63] * 5), 20, rng))
    assert d["name"] == b"@A ?" * 5 and d["PART"] == 0 and d["FLAGS"] == 1
    d = ais_amd.msg_decode(mc.build("24a", dict(name=[0, 1, 32, 63] * 5), 19, rng))
    assert d["name"] == b"" and d["FLAGS"] == 0


def test_agrees_with_the_nmea_payload_characters(payloads, host_rows):
    """decoding the payload characters of aisx_pdu_to_nmea's sentence gives what decoding the PDU gives, for the
    lengths whose bit count is a multiple of six (no padded last group)"""
    import ais_amd

    nm = ais_amd.pdu_to_nmea("A")
    n = 0
    for p, want in zip(payloads, host_rows):
        if len(p) == 0 or len(p) % 3 or len(p) > 42:  # (one fragment: 56 characters hold 42 octets)
            continue
        s = nm.msg_to_sentence(p)
        assert "\n" not in s
        bits = mc.sentence_bits(s)
        assert len(bits) == 8 * len(p)
        assert mc.row_of(mc.decode_bits(bits)) == want, s
        n += 1
    assert n > 40


class EmuMsg:
    def __init__(self, nchan, max_pdus, length_max):
        self.h = emu().emu_msg_create(nchan, max_pdus, length_max)
        assert self.h
        self.max_pdus = max_pdus

    def __del__(self):
        emu().emu_msg_destroy(self.h)

    def process(self, recs, data, npdus, nfound=None):
        n = np.array([npdus], np.int32)
        f = np.array([nfound if nfound is not None else 0], np.int32)
        emu().emu_msg_process(self.h, recs.ctypes.data, data.ctypes.data, n.ctypes.data,
                              f.ctypes.data if nfound is not None else None)

    def read(self):
        cols = np.zeros((NCOL, self.max_pdus), dtype=np.int32)
        strs = np.zeros((self.max_pdus, 48), dtype=np.uint8)
        cnt = np.zeros(3, dtype=np.int32)
        emu().emu_msg_read(self.h, cols.ctypes.data, strs.ctypes.data, cnt.ctypes.data)
        return cnt, cols, strs


def rows_of(cols, strs, n):
    """table -> [row tuples] comparable with msg_cases.row_of"""
    out = []
    for i in range(n):
        s = strs[i].tobytes()
        assert s[7:8] == b"\0"
        out.append(tuple(int(v) for v in cols[:, i]) + (s[0:7].rstrip(b"\0"), s[8:28].rstrip(b"\0"), s[28:48].rstrip(b"\0")))
    return out


UNWRITTEN = 0x5A5A5A5A


def test_lane_model_equals_the_host_function(payloads, host_rows):
    rng = np.random.default_rng(42)
    recs, data = mc.pack(payloads, rng)
    b = EmuMsg(3, len(payloads), 64)
    b.process(recs, data, len(payloads))
    cnt, cols, strs = b.read()
    assert list(cnt) == [len(payloads), len(payloads), 0]
    got = rows_of(cols, strs, len(payloads))
    for i, (g, w) in enumerate(zip(got, host_rows)):
        assert g == w, (i, payloads[i].hex())
    # absent strings are all NUL, not only empty
    nul = [i for i, w in enumerate(host_rows) if not (w[NCOL] or w[NCOL + 1] or w[NCOL + 2])]
    assert nul and not strs[nul].any()


def test_lane_model_record_counts(payloads, host_rows):
    """0, 1, 63, 64, 65 records, one workgroup's worth, one more, and max_pdus: exactly the rows counted are written"""
    rng = np.random.default_rng(43)
    G = emu().emu_msg_group_records()
    max_pdus = 2 * G + 70
    assert len(payloads) >= max_pdus
    recs, data = mc.pack(payloads[:max_pdus], rng)
    for n in (0, 1, 63, 64, 65, G, G + 1, max_pdus):
        b = EmuMsg(3, max_pdus, 64)
        b.process(recs, data, n, nfound=n + 5)
        cnt, cols, strs = b.read()
        assert list(cnt) == [n + 5, n, 0]
        assert rows_of(cols, strs, n) == host_rows[:n]
        assert (cols[:, n:].view(np.uint32) == UNWRITTEN).all() and (strs[n:] == 0x5A).all()


def test_lane_model_bad_input(payloads, host_rows):
    rng = np.random.default_rng(44)
    n = 150
    recs, data = mc.pack(payloads[:n], rng, nchan=3)
    recs["chan"][10] = 3
    recs["chan"][11] = -1
    recs["len"][70] = 64
    recs["len"][71] = -2
    recs["offset"][[10, 11, 70, 71]] = 1 << 40  # (no payload byte of a bad record is read)
    b = EmuMsg(3, n, 64)
    b.process(recs, data, n)
    cnt, cols, strs = b.read()
    assert list(cnt) == [n, n, 1]
    got = rows_of(cols, strs, n)
    fl = mc.COLUMNS.index("FLAGS")
    for i in range(n):
        if i in (10, 11, 70, 71):
            assert got[i] == tuple(4 if k == fl else mc.NA for k in range(NCOL)) + (b"", b"", b"")
            assert not strs[i].any()
        else:
            assert got[i] == host_rows[i]
    assert b.read()[0][2] == 0  # (the flag is cleared by the read)
    for bad_n in (-1, n + 1):
        b = EmuMsg(3, n, 64)
        b.process(recs, data, bad_n)
        cnt, cols, strs = b.read()
        assert list(cnt) == [0, 0, 1]
        assert (cols.view(np.uint32) == UNWRITTEN).all()  # (no rows written)


def test_arguments_and_no_device():
    import ais_amd
    from ais_amd import _lib

    bad = [(0, 10, 64), (2, 0, 64), (2, 10, 1), (2, 10, 1025)]
    for nchan, mp, lm in bad:
        assert not emu().emu_msg_create(nchan, mp, lm)
    L = _lib.lib()
    h = C.c_void_p()
    for nchan, mp, lm in bad:
        assert L.aisx_msg_batch_create(C.byref(h), nchan, mp, lm) == _lib.AISX_ERR_INVALID
    assert L.aisx_msg_batch_create(None, 2, 10, 64) == _lib.AISX_ERR_INVALID
    assert L.aisx_msg_batch_process(None, None, None, None, None, None) == _lib.AISX_ERR_INVALID
    assert L.aisx_msg_batch_results_device(None, None, None, None, None) == _lib.AISX_ERR_INVALID
    assert L.aisx_msg_batch_read(None, None, 0, None, 0, None, None, None) == _lib.AISX_ERR_INVALID
    assert L.aisx_msg_batch_destroy(None) == _lib.AISX_OK
    assert L.aisx_rx_enable_messages(None) == _lib.AISX_ERR_INVALID
    assert L.aisx_rx_pop_messages(None, 0, None, None, 0, None, None, 0, None, None, 0, None, None) == _lib.AISX_ERR_INVALID
    cols = np.zeros(NCOL, np.int32)
    strs = np.zeros(48, np.uint8)
    assert L.aisx_msg_decode(None, 1, cols.ctypes.data, strs.ctypes.data) == _lib.AISX_ERR_INVALID
    assert L.aisx_msg_decode(strs.ctypes.data, -1, cols.ctypes.data, strs.ctypes.data) == _lib.AISX_ERR_INVALID
    assert L.aisx_msg_decode(strs.ctypes.data, 1, None, strs.ctypes.data) == _lib.AISX_ERR_INVALID
    assert L.aisx_msg_decode(None, 0, cols.ctypes.data, strs.ctypes.data) == _lib.AISX_OK
    assert cols[mc.COLUMNS.index("FLAGS")] == 2 and (np.delete(cols, mc.COLUMNS.index("FLAGS")) == mc.NA).all()
    n = C.c_int(-1)
    L.aisx_device_count(C.byref(n))
    rc = L.aisx_msg_batch_create(C.byref(h), 2, 10, 1024)
    if n.value <= 0:
        assert rc == _lib.AISX_ERR_NO_DEVICE
        with pytest.raises(_lib.NoDeviceError):
            ais_amd.pdu_decode_batch(2, 10, 64)
    else:
        assert rc == _lib.AISX_OK
        assert L.aisx_msg_batch_destroy(h) == 0
    with pytest.raises(ValueError):
        ais_amd.pdu_decode_batch(2, 10, 1025)
