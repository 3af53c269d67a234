"""The batched NMEA parser's kernel bodies (gr-ais_amd/csrc/k_nmea_parse.h) on the CPU lane model
(tests/emul_nmea_parse), call by call against the host aisx_nmea_parse_work that is their specification: records,
bytes, times and every count.  Plus the refusal of a bad call, the max_pdus overflow, the C ABI's refusal without a
device and the names of the counts.  -m "not gpu"."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import emul_load
from emul_load import i32, lng, vp
import nmea_parse_cases as nc
import torch  # noqa: F401  (before libaisx.so: one HIP runtime in the process)
import ais_amd
from ais_amd import _lib

HERE = os.path.dirname(os.path.abspath(__file__))
PDU_DTYPE = np.dtype([("end_bit", "<u8"), ("offset", "<i8"), ("chan", "<i4"), ("len", "<i4")])
CASES = nc.build_cases()


def emu():
    return emul_load.load("emul_nmea_parse", [
        ("emu_nmp_create", vp, [C.POINTER(C.c_char_p), i32, i32, i32, i32, lng, i32, i32]),
        ("emu_nmp_destroy", None, [vp]),
        ("emu_nmp_reset", None, [vp]),
        ("emu_nmp_process", None, [vp, vp, vp]),
        ("emu_nmp_read", None, [vp, vp, vp, vp, vp]),
        ("emu_nmp_plan", i32, [C.POINTER(C.c_char_p), i32, i32, i32, i32, lng, i32, i32, vp]),
    ])


class EmuParser:
    def __init__(self, designators=nc.DESIGNATORS, length_max=nc.LENGTH_MAX, max_line=nc.MAX_LINE, ref_tail=False,
                 max_bytes=1 << 16, max_lines=2048, max_pdus=2048):
        d = [x.encode() if isinstance(x, str) else x for x in designators]
        self.h = emu().emu_nmp_create((C.c_char_p * len(d))(*d), len(d), length_max, max_line, int(ref_tail), max_bytes,
                                      max_lines, max_pdus)
        assert self.h
        self.max_pdus, self.length_max = max_pdus, length_max

    def __del__(self):
        emu().emu_nmp_destroy(self.h)

    def reset(self):
        emu().emu_nmp_reset(self.h)

    def work(self, piece, nbytes=None):
        # (a buffer of exactly the piece's size, at an address that is 16-byte aligned for one call in two)
        buf = np.zeros(len(piece) + 32, dtype=np.uint8)
        off = (-buf.ctypes.data) % 16 + (len(piece) % 2) * 3
        buf[off:off + len(piece)] = np.frombuffer(piece, dtype=np.uint8)
        n = np.array([len(piece) if nbytes is None else nbytes], dtype=np.int64)
        emu().emu_nmp_process(self.h, buf.ctypes.data + off, n.ctypes.data)
        recs = np.zeros(self.max_pdus, dtype=PDU_DTYPE)
        data = np.zeros(self.max_pdus * (self.length_max - 1) + 1, dtype=np.uint8)
        times = np.zeros(self.max_pdus, dtype=np.int64)
        cnt = np.zeros(_lib.AISX_NMEAP_NCNT, dtype=np.int32)
        emu().emu_nmp_read(self.h, recs.ctypes.data, data.ctypes.data, times.ctypes.data, cnt.ctypes.data)
        k = int(cnt[1])
        return nc.as_tuples(recs[:k], data, times[:k]), {n: int(v) for n, v in zip(_lib.AISX_NMEAP_NAMES, cnt)}


def host_calls(pcs, ref_tail=False, pdu_cap=None, **kw):
    h = ais_amd.nmea_to_pdu(nc.DESIGNATORS, nc.LENGTH_MAX, max_line=nc.MAX_LINE, ref_tail=ref_tail, **kw)
    out = []
    for piece in pcs:
        recs, data, times, cnt = h.work(piece, pdu_cap=pdu_cap, overflow_ok=True)
        out.append((nc.as_tuples(recs, data, times), cnt))
    return out


@pytest.mark.parametrize("name,text", CASES, ids=[c[0] for c in CASES])
@pytest.mark.parametrize("ref_tail", [False, True])
def test_cases_against_host(name, text, ref_tail):
    """every case with both flag values: whole, and under 3 seeded cuts"""
    rng = np.random.default_rng(len(text))
    e = EmuParser(ref_tail=ref_tail)
    for bounds in [[0, len(text)]] + [nc.random_cuts(rng, len(text), k) for k in (3,)]:
        pcs = nc.pieces(text, bounds)
        e.reset()
        want = host_calls(pcs, ref_tail)
        for k, piece in enumerate(pcs):
            assert e.work(piece) == want[k], (name, bounds, k)


@pytest.mark.parametrize("ref_tail", [False, True])
def test_all_cases_under_many_cuts(ref_tail):
    """A call on the lane model costs a tenth of a second, so the host test's 17 cuts per case are not repeated case
    by case here (tests/test_gpu_nmea_parse.py does that on the device): the cases one behind the other as one
    stream, under two cuts per case, which fall inside lines, groups and tag blocks alike."""
    text = b"".join(t for _, t in CASES)
    rng = np.random.default_rng(17)
    pcs = nc.pieces(text, nc.random_cuts(rng, len(text), 2 * len(CASES)))
    e = EmuParser(ref_tail=ref_tail)
    want = host_calls(pcs, ref_tail)
    for k, piece in enumerate(pcs):
        assert e.work(piece) == want[k], k
    assert sum(c["FOUND"] for _, c in want) > 150 and sum(c["REJ_FRAGMENT"] for _, c in want) > 20


def test_600_byte_text_cut_in_the_group_and_in_a_line():
    text = nc.text600()
    whole = host_calls([text])
    for cut in list(range(60, 300, 23)) + [len(text) - 1]:
        e = EmuParser()
        want = host_calls([text[:cut], text[cut:]])
        assert [e.work(text[:cut]), e.work(text[cut:])] == want, cut
        assert want[0][0] + want[1][0] == whole[0][0]


def test_bad_input_leaves_the_state_untouched():
    text = nc.text600()
    cut = text.index(b"\n", 200) + 20  # a group open and a line begun
    want = host_calls([text[:cut], text[cut:]])
    e = EmuParser(max_bytes=1024, max_lines=8)
    assert e.work(text[:cut]) == want[0]
    for piece, n in ((text[cut:], 1025), (text[cut:], -1), (b"\n" * 9, None)):
        recs, cnt = e.work(piece, n)
        assert recs == [] and cnt["BAD_INPUT"] == 1 and cnt["FOUND"] == 0 and cnt["LINES"] == 0
        assert cnt["CARRIED"] == want[0][1]["CARRIED"]
    got = e.work(text[cut:])
    assert got == want[1] and got[1]["BAD_INPUT"] == 0
    # exactly max_lines line ends are taken
    e = EmuParser(max_bytes=1024, max_lines=8)
    assert e.work(text) == host_calls([text])[0] and text.count(b"\n") == 8


def test_max_pdus_overflow_keeps_a_prefix():
    text = b"".join(c[1] for c in CASES if c[0].startswith("fill-"))
    (all_recs, all_cnt), = host_calls([text])
    assert all_cnt["FOUND"] == 6
    e = EmuParser(max_pdus=4)
    recs, cnt = e.work(text + nc.text600()[:50])
    assert recs == all_recs[:4] and cnt["FOUND"] == 6 and cnt["KEPT"] == 4
    assert (recs, cnt) == host_calls([text + nc.text600()[:50]], pdu_cap=4)[0]
    rest = nc.text600()[50:]
    assert e.work(rest) == host_calls([text + nc.text600()[:50], rest], pdu_cap=4)[1]  # the state advanced


def test_reset():
    text = nc.text600()
    e = EmuParser()
    e.work(text[:250])
    e.reset()
    assert e.work(text) == host_calls([text])[0]


def test_create_arguments():
    d = (C.c_char_p * 1)(b"A")
    ok = dict(length_max=64, max_line=128, flags=0, max_bytes=1024, max_lines=8, max_pdus=8)
    for bad in (dict(length_max=1), dict(length_max=1025), dict(max_line=63), dict(max_line=4097), dict(flags=2),
                dict(max_bytes=0), dict(max_lines=0), dict(max_pdus=0), dict(max_bytes=(1 << 30) + 1)):
        a = dict(ok, **bad)
        h = C.c_void_p()
        assert _lib.lib().aisx_nmea_parse_batch_create(C.byref(h), d, 1, a["length_max"], a["max_line"], a["flags"], a["max_bytes"],
                                                       a["max_lines"], a["max_pdus"]) == _lib.AISX_ERR_INVALID
    h = C.c_void_p()
    assert _lib.lib().aisx_nmea_parse_batch_create(C.byref(h), (C.c_char_p * 1)(b"A" * 17), 1, 64, 128, 0, 1024, 8, 8) == _lib.AISX_ERR_INVALID
    assert _lib.lib().aisx_nmea_parse_batch_create(C.byref(h), None, 1, 64, 128, 0, 1024, 8, 8) == _lib.AISX_ERR_INVALID


def test_create_without_a_device_is_an_error():
    n = C.c_int(-1)
    _lib.lib().aisx_device_count(C.byref(n))
    h = C.c_void_p()
    rc = _lib.lib().aisx_nmea_parse_batch_create(C.byref(h), (C.c_char_p * 1)(b"A"), 1, 64, 512, 0, 1 << 16, 1024, 1024)
    if n.value <= 0:
        assert rc == _lib.AISX_ERR_NO_DEVICE and not h.value
        with pytest.raises(_lib.NoDeviceError):
            ais_amd.nmea_to_pdu_batch(["A"], 64, 1 << 16, 1024, 1024)
    else:
        assert rc == _lib.AISX_OK
        assert _lib.lib().aisx_nmea_parse_batch_destroy(h) == 0


def test_count_names_match_the_header():
    txt = open(os.path.join(os.path.dirname(HERE), "include", "aisx.h")).read()
    start = txt.index("AISX_NMEAP_FOUND = 0")
    body = txt[start:txt.index("AISX_NMEAP_NCNT", start)]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = re.findall(r"AISX_NMEAP_([A-Z_]+)", body)
    assert tuple(names) == _lib.AISX_NMEAP_NAMES == nc.COUNT_NAMES
    assert "AISX_NMEA_PARSE_REF_TAIL = 1" in txt and _lib.AISX_NMEA_PARSE_REF_TAIL == 1
