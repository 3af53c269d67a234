"""The duplicate suppression off the device: the host form aisx_dedup_* (ais_amd.pdu_dedup) against the dict-based model
of tests/dedup_cases.py, and the kernel bodies (gr-ais_amd/csrc/k_dedup.h) on the CPU lane model (tests/emul_dedup), whose
lanes are free-running threads, against the host form, array for array.  -m "not gpu"."""
import ctypes as C

import numpy as np
import pytest

import dedup_cases as dc
import emul_load
from emul_load import i32, vp
import torch  # noqa: F401  (before libaisx.so: one HIP runtime in the process)

MAX_PDUS = 257  # one workgroup of 256 and one record: several waves and a ragged tail
WINDOWS = (0, 1, 3)


def emu():
    return emul_load.load("emul_dedup", [
        ("emu_dd_create", vp, [i32, i32, i32]),
        ("emu_dd_destroy", None, [vp]),
        ("emu_dd_reset", None, [vp]),
        ("emu_dd_process", i32, [vp, vp, vp, vp, vp, vp, i32]),
        ("emu_dd_read", None, [vp, vp, vp, vp, vp, vp]),
        ("emu_dd_plan", i32, [i32, i32, i32, vp]),
        ("emu_dd_home", C.c_uint, [C.c_uint64, i32]),
    ])


class HostForm:
    """ais_amd.pdu_dedup behind the interface dedup_cases.run_script drives"""

    def __init__(self, window, max_pdus=MAX_PDUS, length_max=64):
        import ais_amd

        self.t = ais_amd.pdu_dedup(window, length_max)
        self.max_pdus = max_pdus

    def reset(self):
        self.t.reset()

    def call(self, recs, data, n, stamp, marks):
        n = n if 0 <= n <= self.max_pdus else 0  # (the device form keeps nothing for such a count, as for no records)
        try:
            out, first, copies, om = self.t.work_records(recs[:n], data, stamp, marks[:n] if marks is not None else None)
        except IndexError:
            return None
        return out, first, copies, om, [self.t.counts[c] for c in dc.COUNTS]


class ModelForm(HostForm):
    def __init__(self, window, max_pdus=MAX_PDUS, length_max=64):
        self.t = dc.Model(window, length_max)
        self.max_pdus = max_pdus

    def call(self, recs, data, n, stamp, marks):
        return self.t.update(recs, data, n if 0 <= n <= self.max_pdus else 0, stamp, marks)


class LaneForm:
    """the kernel bodies on the CPU lane model"""

    def __init__(self, window, max_pdus=MAX_PDUS, length_max=64):
        self.h = emu().emu_dd_create(window, max_pdus, length_max)
        assert self.h
        self.max_pdus = max_pdus
        self.flags = []  # the bad-count flag after every call that ran
        self.found = []

    def __del__(self):
        emu().emu_dd_destroy(self.h)

    def reset(self):
        emu().emu_dd_reset(self.h)

    def call(self, recs, data, n, stamp, marks, nfound=None):
        assert len(recs) >= self.max_pdus and recs.flags.c_contiguous and data.flags.c_contiguous
        cnt = np.array([n, n if nfound is None else nfound], dtype=np.int32)
        rc = emu().emu_dd_process(self.h, recs.ctypes.data, data.ctypes.data, cnt.ctypes.data, cnt.ctypes.data + 4,
                                  marks.ctypes.data if marks is not None else None, stamp)
        if rc != 0:
            assert rc == -2
            return None
        out = np.zeros(self.max_pdus, dtype=dc.REC_DTYPE)
        first, copies, om = (np.zeros(self.max_pdus, dtype=np.int32) for _ in range(3))
        c = np.zeros(8, dtype=np.int32)
        emu().emu_dd_read(self.h, out.ctypes.data, first.ctypes.data, copies.ctypes.data, om.ctypes.data, c.ctypes.data)
        self.flags.append(int(c[2]))
        self.found.append(int(c[0]))
        k, nin = int(c[4]), int(c[3])
        assert int(c[1]) == k
        return out[:k], first[:nin], copies[:k], om[:k] if marks is not None else None, [int(v) for v in c[3:8]]


@pytest.fixture(scope="module")
def all_scripts():
    return {(w, m): dc.scripts(1000 + 10 * w + m, w, m) for w in WINDOWS for m in (MAX_PDUS, 1)}


@pytest.fixture(scope="module")
def chains():
    return {w: dc.chain_scripts(77 + w, w, MAX_PDUS) for w in WINDOWS}


NAMES = ["n0", "n1", "n64", "n65", "n257", "bad_count", "distinct", "all_same", "runs", "lengths", "bad_len", "offsets", "window",
         "no_refresh", "gaps", "extreme_stamps", "refused_stamp", "reset", "random0", "random1", "random2"]
NAMES_1 = [n for n in NAMES if n not in ("n64", "n65", "n257", "bad_len", "offsets")]


# ---- the key and the host form against the model ---------------------------------------------------------------------
def test_key_is_the_headers():
    import ais_amd

    rng = np.random.default_rng(3)
    for n in list(range(0, 20)) + [21, 63, 126, 300]:
        p = rng.integers(0, 256, size=n, dtype=np.uint8).tobytes()
        assert ais_amd.dedup_key(p) == dc.key(p) != 0
    assert len({dc.key(b"\x01"), dc.key(b"\x01\x00"), dc.key(b""), dc.key(b"\x00"), dc.key(bytes(8)), dc.key(bytes(9))}) == 6
    p = bytearray(rng.integers(0, 256, size=21, dtype=np.uint8).tobytes())
    k0 = dc.key(p)
    for i in range(21):  # every octet counts
        q = bytearray(p)
        q[i] ^= 0x40
        assert dc.key(q) != k0
    assert tuple(ais_amd.DEDUP_COUNTS) == dc.COUNTS


def test_counts_agree_with_the_header():
    import os

    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "aisx.h")).read()
    at = hdr.index("AISX_DEDUP_CNT_IN = 0")
    enum = hdr[at:hdr.index("AISX_DEDUP_NCNT", at)]
    names = [t for t in enum.replace(",", " ").split() if t.startswith("AISX_DEDUP_CNT_")]
    assert [n[len("AISX_DEDUP_CNT_"):].lower() for n in names] == list(dc.COUNTS)


def test_work_on_payloads():
    import ais_amd

    d = ais_amd.pdu_dedup(1)
    kept, first, copies = d.work([b"\x01", b"\x01\x00", b"\x01", b"x" * 70, b"", b"x" * 70], 5)
    assert list(kept) == [0, 1, 3, 4, 5] and list(first) == [0, 1, 0, 2, 3, 4] and list(copies) == [2, 1, 1, 1, 1]
    assert d.counts == {"in": 6, "kept": 5, "dup_call": 1, "dup_window": 0, "bad_len": 2}
    kept, first, copies = d.work([b"\x01", b"q", b""], 6)
    assert list(kept) == [1] and list(first) == [-2, 0, -2] and d.counts["dup_window"] == 2
    kept, first, _ = d.work([b"\x01", b"q"], 7)  # (kept at 5, suppressed at 6 without a refresh: kept again at 7)
    assert list(kept) == [0] and list(first) == [0, -2]
    with pytest.raises(IndexError):
        d.work([b"zz"], 7)
    assert list(d.work([b"zz"], 8)[0]) == [0]
    for w in (-1, 16):
        with pytest.raises(ValueError):
            ais_amd.pdu_dedup(w)


@pytest.mark.parametrize("window", WINDOWS)
def test_host_form_equals_the_model_on_the_scripts(all_scripts, chains, window):
    for m in (MAX_PDUS, 1):
        for name, ops in all_scripts[(window, m)].items():
            dc.run_script(ops, [HostForm(window, m), ModelForm(window, m)])
    for name, ops in chains[window][0].items():
        dc.run_script(ops, [HostForm(window), ModelForm(window)])


def test_the_scripts_show_what_they_are_for(all_scripts):
    s = all_scripts[(1, MAX_PDUS)]
    assert set(NAMES) <= set(s) and set(NAMES_1) <= set(all_scripts[(1, 1)])
    r = dc.run_script(s["all_same"], [ModelForm(1)])
    assert r[0][4] == [257, 1, 256, 0, 0] and list(r[0][2]) == [257]
    r = dc.run_script(s["distinct"], [ModelForm(1)])
    assert r[0][4] == [257, 257, 0, 0, 0]
    r = dc.run_script(s["bad_len"], [ModelForm(1)])
    assert r[0][4][4] == 3 and r[1][4][4] == 1
    r = dc.run_script(s["refused_stamp"], [ModelForm(1)])
    assert [x is None for x in r] == [False, True, True, True, False] and r[4][4] == [2, 1, 0, 1, 0]
    for w in WINDOWS:
        r = dc.run_script(all_scripts[(w, MAX_PDUS)]["window"], [ModelForm(w)])
        # kept at s, suppressed at s + 1 .. s + w with the age as first[], kept again at s + w + 1
        assert [int(x[1][0]) for x in r[: w + 2]] == [0] + [-1 - d for d in range(1, w + 1)] + [0]
        r = dc.run_script(all_scripts[(w, MAX_PDUS)]["no_refresh"], [ModelForm(w)])
        assert [int(x[1][0]) for x in r] == ([0, -2, 0, 0] if w else [0, 0, 0])


# ---- the kernel bodies on the lane model against the host form ----------------------------------------------------------
def test_plan():
    out = (C.c_longlong * 4)()
    assert emu().emu_dd_plan(3, MAX_PDUS, 64, out) == 1 and list(out) == [dc.hash_bits(MAX_PDUS), 2, 2, 4] and out[0] == 10
    assert emu().emu_dd_plan(0, 1, 64, out) == 1 and list(out) == [6, 1, 1, 1]
    for bad in ((-1, 4, 64), (16, 4, 64), (1, 0, 64), (1, (1 << 24) + 1, 64), (1, 4, 1), (1, 4, 1025)):
        assert emu().emu_dd_plan(*bad, out) == 0 and not emu().emu_dd_create(*bad)
    for k in (1, 0x8000000000000000, dc.M64, 0x123456789ABCDEF0):
        assert emu().emu_dd_home(k, 10) == dc.home(k, 10) and emu().emu_dd_home(k, 6) == dc.home(k, 6)


@pytest.mark.parametrize("window", WINDOWS)
@pytest.mark.parametrize("name", NAMES)
def test_lane_model_equals_the_host_form(all_scripts, window, name):
    lane = LaneForm(window)
    dc.run_script(all_scripts[(window, MAX_PDUS)][name], [HostForm(window), lane])
    assert lane.flags == ([0, 1, 1, 0] if name == "bad_count" else [0] * len(lane.flags))


@pytest.mark.parametrize("window", WINDOWS)
def test_lane_model_with_one_record_at_most(all_scripts, window):
    for name in NAMES_1:
        lane = LaneForm(window, 1)
        dc.run_script(all_scripts[(window, 1)][name], [HostForm(window, 1), lane])
        assert lane.flags == ([0, 1, 1, 0] if name == "bad_count" else [0] * len(lane.flags))


@pytest.mark.parametrize("window", WINDOWS)
def test_lane_model_on_wrapping_and_crowded_chains(chains, window):
    scripts, payloads = chains[window]
    bits = dc.hash_bits(MAX_PDUS)
    # the property the payloads were searched for, by the model's key and by the kernels' own home slot
    assert len(set(payloads["wrap"])) == 3 and all(dc.home(dc.key(p), bits) == (1 << bits) - 1 for p in payloads["wrap"])
    assert len(set(payloads["crowd"])) == 8 and all(emu().emu_dd_home(dc.key(p), bits) == 17 for p in payloads["crowd"])
    for name in ("wrap", "crowd"):
        dc.run_script(scripts[name], [HostForm(window), LaneForm(window)])


def test_lane_model_reports_what_the_producer_found_beyond_its_records():
    rng = np.random.default_rng(9)
    lane = LaneForm(1)
    P = dc.pool(rng, 4)
    recs, data, marks = dc.make_list([P[0], P[1], P[0], P[2]], rng, MAX_PDUS)
    r = lane.call(recs, data, 4, 1, marks, nfound=9)
    assert r[4] == [4, 3, 1, 0, 0] and lane.found == [3 + 5]
    r = lane.call(recs, data, 4, 2, None, nfound=4)  # (no marks: the call still works)
    assert r[4] == [4, 0, 0, 4, 0] and lane.found == [8, 0] and r[3] is None


def test_lane_model_is_the_same_from_run_to_run(all_scripts):
    ops = all_scripts[(3, MAX_PDUS)]["random0"] + [op for op in all_scripts[(3, MAX_PDUS)]["runs"]]
    ops = [op if op[0] == "reset" else op[:4] + (100 + k,) + op[5:] for k, op in enumerate(ops)]  # (rising stamps)
    runs = [dc.run_script(ops, [LaneForm(3)]) for _ in range(3)]
    for r in runs[1:]:
        for a, b in zip(r, runs[0]):
            dc.assert_same_result(a, b)
