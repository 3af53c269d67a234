"""The standard-form NMEA armouring's kernel bodies (gr-ais_amd/csrc/k_nmea_std.h) on the CPU lane model
(tests/emul_nmea_std), driven by the launch plan the device runs, record by record against the host
aisx_pdu_to_nmea_std that is their specification: texts, ids over calls, text_cap cuts, refusals, reset.  The model's
scan runs 128 threads, so a scan tile is 1024 records.  -m "not gpu"."""
import ctypes as C

import numpy as np
import pytest

import emul_load
from emul_load import i32, lng, vp
import nmea_std_cases as sc
import torch  # noqa: F401  (before libaisx.so: one HIP runtime in the process)

ppc = C.POINTER(C.c_char_p)


def emu():
    return emul_load.load("emul_nmea_std", [
        ("emu_nmea_std_create", vp, [ppc, ppc, i32, i32, i32, lng]),
        ("emu_nmea_std_destroy", None, [vp]),
        ("emu_nmea_std_text_cap", lng, [vp]),
        ("emu_nmea_std_scan_tile", i32, []),
        ("emu_nmea_std_set_time", i32, [vp, C.c_longlong]),
        ("emu_nmea_std_reset", None, [vp]),
        ("emu_nmea_std_next_id", i32, [vp]),
        ("emu_nmea_std_process", None, [vp, vp, vp, vp, vp]),
        ("emu_nmea_std_read", None, [vp, vp, vp, vp]),
        ("emu_nmea_std_plan", i32, [ppc, ppc, i32, i32, i32, lng, vp]),
    ])


def _strs(v):
    return (C.c_char_p * len(v))(*[d.encode("latin-1") if isinstance(d, str) else d for d in v])


class EmuNmeaStd:
    """the model behind the interface the tests share with the device handle (tests/test_gpu_nmea_std.py)"""

    def __init__(self, des, stations, max_pdus, length_max, text_cap=0):
        self.h = emu().emu_nmea_std_create(_strs(des), _strs(stations) if stations is not None else None, len(des), max_pdus,
                                           length_max, text_cap)
        assert self.h
        self.max_pdus = max_pdus
        self.text_cap = emu().emu_nmea_std_text_cap(self.h)

    def __del__(self):
        emu().emu_nmea_std_destroy(self.h)

    def set_time(self, t):
        assert emu().emu_nmea_std_set_time(self.h, t)

    def reset(self):
        emu().emu_nmea_std_reset(self.h)

    def next_id(self):
        return emu().emu_nmea_std_next_id(self.h)

    def process(self, recs, data, npdus, nfound=None):
        n = np.array([npdus], np.int32)
        f = np.array([nfound if nfound is not None else 0], np.int32)
        emu().emu_nmea_std_process(self.h, recs.ctypes.data, data.ctypes.data, n.ctypes.data,
                                   f.ctypes.data if nfound is not None else None)

    def read(self):
        recs = np.zeros(self.max_pdus, dtype=sc.REC_DTYPE)
        text = np.zeros(self.text_cap + 1, dtype=np.uint8)
        cnt = np.zeros(3, dtype=np.int32)
        emu().emu_nmea_std_read(self.h, recs.ctypes.data, text.ctypes.data, cnt.ctypes.data)
        recs = recs[: cnt[1]]
        nt = int(recs["offset"][-1] + recs["len"][-1] + (recs["len"][-1] > 0)) if len(recs) else 0
        return int(cnt[0]), int(cnt[2]), recs, text[:nt].tobytes()


def make(case):
    max_pdus = case.get("max_pdus", max(len(case["records"]), 1))
    return EmuNmeaStd(case["designators"], case["stations"], max_pdus, case["length_max"], case.get("text_cap", 0))


call = sc.check_call


def test_every_case_matches_the_host_function():
    rng = np.random.default_rng(31)
    n = 0
    for case in sc.all_cases(rng):
        n += len(call(make(case), case))
    print("%d records identical to aisx_pdu_to_nmea_std" % n)


def test_the_longest_line():
    case = sc.longest_line()
    got = call(make(case), case)
    lines = got[0][2].split("\n")
    assert len(lines) == 2 and len(lines[0]) + 1 == 135 and lines[0].startswith("\\s:%s,c:%d*" % (sc.S15, sc.T18))
    assert lines[0][43:].startswith("!AIVDM,2,1,0," + sc.D16 + ",")
    assert [len(g[2].split("\n")[0]) + 1 for g in got[:3]] == [135, 134, 134]  # (a designator, a station one byte shorter)
    assert len(got[3][2].split("\n")) == 9 and all(len(x) + 1 == 135 for x in got[3][2].split("\n")[:8])


def test_more_than_one_scan_tile():
    tile = emu().emu_nmea_std_scan_tile()
    assert tile == 1024
    case = sc.many(np.random.default_rng(32), 2 * tile + 300, tile)
    multi = [sc.is_multi(p) for _, _, p in case["records"]]
    assert multi[tile - 1] and multi[tile] and multi[2 * tile - 1] and multi[2 * tile] and multi[-1]
    b = make(case)
    call(b, case)
    assert b.next_id() == sum(multi) % 10


def test_ids_over_calls_and_reset():
    rng = np.random.default_rng(33)
    case = sc.mixed(rng)
    case["records"] = case["records"][:270]
    nm = sum(sc.is_multi(p) for _, _, p in case["records"])
    assert nm % 10 != 0
    b = make(case)
    ids = []
    for k in range(3):  # (the counter wraps 9 -> 0 inside a call and stands between calls)
        got = call(b, dict(case, time=(-1, 7, sc.T18)[k]))
        ids += [int(t.split("!")[1].split(",")[3]) for _, _, t in got if "\n" in t]
        assert b.next_id() == (k + 1) * nm % 10
    assert ids == [k % 10 for k in range(3 * nm)]
    b.reset()
    assert b.next_id() == 0
    got = call(b, case)  # (the time is back at -1 too: the case has none, and call() sets none)
    assert got[0][2].startswith("!AIVDM") or got[0][2].startswith("\\s:")
    # a single-sentence-only call leaves the counter where it is
    one = dict(case, records=[r for r in case["records"] if not sc.is_multi(r[2])])
    at = b.next_id()
    call(b, one)
    assert b.next_id() == at


def test_reset_puts_the_time_back():
    case = dict(sc.mixed(np.random.default_rng(34)), stations=[""] * 7)
    b = make(case)
    b.set_time(5)
    b.reset()
    recs, data = sc.pack(case["records"], b.max_pdus)
    b.process(recs, data, len(case["records"]))
    assert b.read()[3].startswith(b"!AIVDM")


def test_text_cap_cuts_around_a_multi_sentence_record():
    rng = np.random.default_rng(35)
    base = sc.mixed(rng, time=3)
    want, stream, _, _ = sc.expected(base)
    k = 150 + [sc.is_multi(p) for _, _, p in base["records"][150:]].index(True)  # a record of two sentences
    assert "\n" in want[k][2]
    before = sum(len(t) + 1 for _, _, t in want[:k] if t)
    whole = before + len(want[k][2]) + 1
    first = len(want[k][2].split("\n")[0]) + 1
    for cap, kept in ((before, k), (before + 1, k), (before + first, k), (whole - 1, k), (whole, k + 1), (whole + 1, k + 1)):
        case = dict(base, name="cap %d" % cap, text_cap=cap)
        b = make(case)
        for rep in range(2):  # the second call's ids follow the ones written, not the ones cut
            got = call(b, case)
            assert len(got) >= kept and sum(len(t) + 1 for _, _, t in got if t) <= cap
        assert all(not t for _, _, t in got[kept:])  # (only empty payloads fit behind the cut)
        nm = sum(sc.is_multi(p) for _, _, p in base["records"][:kept])
        assert b.next_id() == 2 * nm % 10


def test_empty_zero_and_bad_counts():
    rng = np.random.default_rng(36)
    base = sc.mixed(rng, time=1)
    call(make(base), dict(base, name="zero", records=[]))
    call(make(base), dict(base, name="zero_count", npdus=0))
    call(make(base), dict(base, name="empty only", records=[(1, 5, b""), (2, 6, b"")]))
    # a count outside [0, max_pdus]: no text, no id, INVALID once; the next call is as the first
    for n in (-1, len(base["records"]) + 1):
        b = make(base)
        call(b, dict(base, npdus=n, bad=True))
        assert b.next_id() == 0
        call(b, base)
    # a producer count above the records handed over: found says so
    b = make(base)
    got = call(b, dict(base, npdus=100, nfound=250))
    assert len(got) == 100


def test_bad_records_take_no_id():
    rng = np.random.default_rng(37)
    case = sc.bad_records(rng)
    b = make(case)
    got = call(b, case)
    assert got[10][2] == "" and got[11][2] == "" and got[40][2] == ""
    good_multi = sum(sc.is_multi(p) for i, (c, _, p) in enumerate(case["records"]) if i not in (10, 11, 40))
    assert b.next_id() == good_multi % 10


def test_create_arguments_and_plan():
    good, sta = ["A", "B"], ["x", ""]
    bad = [(["A", "x" * 17], sta, 2, 10, 64), (good, ["x", "y" * 16], 2, 10, 64), (good, ["x", "a b"], 2, 10, 64),
           (good, ["x", "a,b"], 2, 10, 64), (good, sta, 0, 10, 64), (good, sta, 2, 0, 64), (good, sta, 2, 10, 1), (good, sta, 2, 10, 380)]
    for des, st, nchan, mp, lm in bad:
        assert not emu().emu_nmea_std_create(_strs(des), _strs(st), nchan, mp, lm, 0), (des, st, nchan, mp, lm)
    h = emu().emu_nmea_std_create(_strs(["x" * 16, ""]), None, 2, 10, 379, 0)
    assert h
    emu().emu_nmea_std_destroy(h)
    b = EmuNmeaStd(good, sta, 4, 64)
    assert not emu().emu_nmea_std_set_time(b.h, 10 ** 18) and not emu().emu_nmea_std_set_time(b.h, -2)
    # text_cap = 0: the worst case of the form -- longest designator and station, 18 digits, the id digit
    from ais_amd.batch_framing import nmea_std_text_len

    out = (C.c_longlong * 2)()
    assert emu().emu_nmea_std_plan(_strs(["x" * 16, ""]), _strs(["", sc.S15]), 2, 1000, 379, 0, out)
    assert out[0] == 1000 * (nmea_std_text_len(378, 16, 15, sc.T18) + 1) == 1000 * (9 * (43 + 19 + 16) + 504 + 9)
    assert out[1] == 250
    assert emu().emu_nmea_std_plan(_strs(["A"]), None, 1, 1000, 43, 0, out) and out[0] == 1000 * (25 + 18 + 1 + 56 + 1)
    assert emu().emu_nmea_std_plan(_strs(["A"]), None, 1, 1000, 43, 500, out) and out[0] == 500
    # the library's own checks, and its refusal without a device
    from ais_amd import _lib

    L = _lib.lib()
    hh = C.c_void_p()
    for des, st, nchan, mp, lm in bad:
        assert L.aisx_nmea_batch_create_std(C.byref(hh), _strs(des), _strs(st), nchan, mp, lm, 0) == _lib.AISX_ERR_INVALID
    assert L.aisx_nmea_batch_create_std(None, _strs(good), _strs(sta), 2, 10, 64, 0) == _lib.AISX_ERR_INVALID
    n = C.c_int(-1)
    L.aisx_device_count(C.byref(n))
    rc = L.aisx_nmea_batch_create_std(C.byref(hh), _strs(good), None, 2, 10, 379, 0)
    if n.value <= 0:
        assert rc == _lib.AISX_ERR_NO_DEVICE
    else:
        assert rc == _lib.AISX_OK
        assert L.aisx_nmea_batch_destroy(hh) == 0
    for f in (L.aisx_nmea_batch_reset,):
        assert f(None) == _lib.AISX_ERR_INVALID
    assert L.aisx_nmea_batch_set_time(None, 0) == _lib.AISX_ERR_INVALID
    import ais_amd

    with pytest.raises(ValueError):
        ais_amd.pdu_to_nmea_batch(["A", "B"], 2, 10, 64, stations=["x", "y"])
    with pytest.raises(ValueError):
        ais_amd.pdu_to_nmea_batch(["A", "B"], 2, 10, 64, standard=True, stations=["x"])
