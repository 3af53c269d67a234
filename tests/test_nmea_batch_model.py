"""The batched NMEA armouring's kernel bodies (gr-ais_amd/csrc/k_nmea.h) on the CPU lane model (tests/emul_nmea),
record by record against the host aisx_pdu_to_nmea that is their specification and, on a sample, against the C
oracle's orc_pdu_to_nmea.  Plus the closed-form text length, the C ABI's argument checks and its refusal without a
device.  -m "not gpu"."""
import ctypes as C

import numpy as np
import pytest

import emul_load
from emul_load import i32, lng, vp
import nmea_cases as nc
import torch  # noqa: F401  (before libaisx.so: one HIP runtime in the process)


def emu():
    return emul_load.load("emul_nmea", [
        ("emu_nmea_create", vp, [C.POINTER(C.c_char_p), i32, i32, i32, lng]),
        ("emu_nmea_destroy", None, [vp]),
        ("emu_nmea_text_cap", lng, [vp]),
        ("emu_nmea_text_len", None, [i32, i32]),
        ("emu_nmea_process", None, [vp, vp, vp, vp, vp]),
        ("emu_nmea_read", None, [vp, vp, vp, vp]),
        ("emu_nmea_plan", i32, [C.POINTER(C.c_char_p), i32, i32, i32, lng, vp]),
    ])


def _designators(des):
    return (C.c_char_p * len(des))(*[d.encode("latin-1") if isinstance(d, str) else d for d in des])


class EmuNmea:
    def __init__(self, des, max_pdus, length_max, text_cap=0):
        self.h = emu().emu_nmea_create(_designators(des), len(des), max_pdus, length_max, text_cap)
        assert self.h
        self.max_pdus = max_pdus
        self.text_cap = emu().emu_nmea_text_cap(self.h)

    def __del__(self):
        emu().emu_nmea_destroy(self.h)

    def process(self, recs, data, npdus, nfound=None):
        n = np.array([npdus], np.int32)
        f = np.array([nfound if nfound is not None else 0], np.int32)
        emu().emu_nmea_process(self.h, recs.ctypes.data, data.ctypes.data, n.ctypes.data,
                               f.ctypes.data if nfound is not None else None)

    def read(self):
        recs = np.zeros(self.max_pdus, dtype=nc.REC_DTYPE)
        text = np.zeros(self.text_cap + 1, dtype=np.uint8)
        cnt = np.zeros(3, dtype=np.int32)
        emu().emu_nmea_read(self.h, recs.ctypes.data, text.ctypes.data, cnt.ctypes.data)
        recs = recs[: cnt[1]]
        nt = int(recs["offset"][-1] + recs["len"][-1] + (recs["len"][-1] > 0)) if len(recs) else 0
        return int(cnt[0]), int(cnt[2]), recs, text[:nt].tobytes()


def run_case(case):
    n = case.get("npdus", len(case["records"]))
    max_pdus = case.get("max_pdus", max(len(case["records"]), 1))
    b = EmuNmea(case["designators"], max_pdus, case["length_max"], case.get("text_cap", 0))
    recs, data = nc.pack(case["records"], max_pdus)
    b.process(recs, data, n, case.get("nfound"))
    return b, b.read()


def check_case(case):
    b, (found, bad, recs, text) = run_case(case)
    want, stream, kept = nc.expected(case)
    assert bad == int(bool(case.get("bad"))), case["name"]
    assert len(recs) == kept
    assert found == case.get("nfound", case.get("npdus", len(case["records"])))
    got = nc.split(recs, text)
    assert text == stream
    for g, w in zip(got, want):
        assert g == w, (case["name"], g, w)
    assert b.read()[1] == 0  # (the flag is cleared by the read)
    return got


def test_every_case_matches_the_host_function():
    rng = np.random.default_rng(11)
    n = 0
    for case in nc.all_cases(rng):
        n += len(check_case(case))
    print("%d records identical to aisx_pdu_to_nmea" % n)


def test_sample_matches_the_oracle():
    import oracle_py as orc

    rng = np.random.default_rng(12)
    case = nc.mixed(rng)
    got = check_case(case)
    for (c, e, t), (_, _, p) in list(zip(got, case["records"]))[::7]:
        if len(p):
            assert t == orc.pdu_to_nmea(case["designators"][c], p)
    case = nc.every_length(rng)
    sel = [0, 1, 2, 20, 41, 55, 83, 84, 85, 167, 168, 377, 503, 1022]
    case["records"] = [case["records"][k] for k in sel]
    got = check_case(case)
    for (c, e, t), (_, _, p) in zip(got, case["records"]):
        assert t == orc.pdu_to_nmea(case["designators"][c], p)


def test_fragment_edges():
    # payload characters per text: 56 / 58 (1 -> 2 fragments; whole octets never make 57), 112 / 114 (2 -> 3),
    # 9 -> 10 fragments, 25
    from ais_amd.batch_framing import nmea_text_len

    def frags(L):
        return ((8 * L + 5) // 6 + 55) // 56

    got = check_case(nc.every_length(np.random.default_rng(13)))
    by_len = {len(p): t for (_, _, t), p in zip(got, [r[2] for r in nc.every_length(np.random.default_rng(13))["records"]])}
    assert {(8 * L + 5) // 6 for L in by_len} >= {56, 58, 112, 114}
    assert by_len[42].count("\n") == 0 and by_len[43].count("\n") == 1 and by_len[84].count("\n") == 1
    assert by_len[85].count("\n") == 2
    L9 = max(L for L in by_len if frags(L) == 9)
    assert by_len[L9].startswith("!AIVDM,9,1,,") and by_len[L9 + 1].startswith("!AIVDM,10,1,,")
    assert by_len[L9 + 1].split("\n")[9].startswith("!AIVDM,10,10,,")
    assert by_len[1023].startswith("!AIVDM,25,1,,") and by_len[1023].count("\n") == 24
    assert all(len(t) == nmea_text_len(L, [0, 1, 16][L % 3]) for L, t in by_len.items())


def test_empty_zero_cap_and_counts():
    rng = np.random.default_rng(14)
    base = nc.mixed(rng)
    # zero records
    check_case(dict(base, name="zero", records=[]))
    check_case(dict(base, name="zero_count", npdus=0))
    # a count outside [0, max_pdus]: no text, INVALID once
    for n in (-1, len(base["records"]) + 1):
        b, (found, bad, recs, text) = run_case(dict(base, npdus=n))
        assert bad == 1 and len(recs) == 0 and text == b"" and found == 0
    # a text_cap that cuts mid-list: a prefix is written, the rest counted
    want, stream, _ = nc.expected(base)
    cap = len(stream) // 2 + 1
    case = dict(base, name="cap", text_cap=cap)
    b, (found, bad, recs, text) = run_case(case)
    _, part, kept = nc.expected(case)
    assert 0 < kept < len(base["records"]) and text == part and len(recs) == kept and found == len(base["records"])
    assert len(part) <= cap < len(part) + len(want[kept][2]) + 1
    nc.split(recs, text)
    # a producer count above the records handed over: found says so
    b, (found, bad, recs, text) = run_case(dict(base, npdus=100, nfound=250))
    assert found == 250 and len(recs) == 100 and bad == 0
    assert nc.split(recs, text) == nc.expected(dict(base, npdus=100))[0]


def test_closed_form_length():
    rng = np.random.default_rng(15)
    import ais_amd

    for D in range(17):
        nm = ais_amd.pdu_to_nmea("d" * D)
        for L in range(1, 1024):
            s = nm.msg_to_sentence(bytes(rng.integers(0, 256, L).astype(np.uint8)))
            assert emu().emu_nmea_text_len(L, D) == len(s), (L, D)
    assert emu().emu_nmea_text_len(0, 5) == 0


def test_create_arguments_and_no_device():
    from ais_amd import _lib

    good = ["A", "B"]
    bad = [(["A", "x" * 17], 2, 10, 64), (good, 0, 10, 64), (good, 2, 0, 64), (good, 2, 10, 1), (good, 2, 10, 1025)]
    for des, nchan, mp, lm in bad:
        assert not emu().emu_nmea_create(_designators(des), nchan, mp, lm, 0), (nchan, mp, lm)
    assert emu().emu_nmea_create(_designators(["x" * 16, ""]), 2, 10, 1024, 0)
    L = _lib.lib()
    h = C.c_void_p()
    for des, nchan, mp, lm in bad:
        assert L.aisx_nmea_batch_create(C.byref(h), _designators(des), nchan, mp, lm, 0) == _lib.AISX_ERR_INVALID
    assert L.aisx_nmea_batch_create(None, _designators(good), 2, 10, 64, 0) == _lib.AISX_ERR_INVALID
    assert L.aisx_nmea_batch_create(C.byref(h), None, 2, 10, 64, 0) == _lib.AISX_ERR_INVALID
    assert L.aisx_nmea_batch_create(C.byref(h), _designators(good), 2, 10, 64, -1) == _lib.AISX_ERR_INVALID
    n = C.c_int(-1)
    L.aisx_device_count(C.byref(n))
    rc = L.aisx_nmea_batch_create(C.byref(h), _designators(["x" * 16, ""]), 2, 10, 1024, 0)
    if n.value <= 0:
        assert rc == _lib.AISX_ERR_NO_DEVICE
    else:
        assert rc == _lib.AISX_OK
        assert L.aisx_nmea_batch_destroy(h) == 0
    import ais_amd

    with pytest.raises(ValueError):
        ais_amd.pdu_to_nmea_batch(["A", "B", "C"], 2, 10, 64)
    with pytest.raises(ValueError):
        ais_amd.pdu_to_nmea_batch("x" * 17, 2, 10, 64)
