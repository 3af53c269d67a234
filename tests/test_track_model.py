"""The vessel table off the device: the host form aisx_track_* (ais_amd.vessel_table) against the dict-based model of
tests/track_cases.py, and the kernel bodies (gr-ais_amd/csrc/k_track.h) on the CPU lane model (tests/emul_track), whose
lanes are free-running threads, against the host form, array for array.  -m "not gpu"."""
import ctypes as C
import os

import numpy as np
import pytest

import emul_load
from emul_load import i32, lng, vp
import msg_cases as mc
import track_cases as tc
import torch  # noqa: F401  (before libaisx.so: one HIP runtime in the process)

HERE = os.path.dirname(os.path.abspath(__file__))
MAX_ROWS = 257  # one workgroup of 256 and one row: several waves and a ragged tail


def emu():
    return emul_load.load("emul_track", [
        ("emu_trk_create", vp, [i32, i32]),
        ("emu_trk_destroy", None, [vp]),
        ("emu_trk_process", None, [vp, vp, lng, vp, vp, vp, i32]),
        ("emu_trk_expire", None, [vp, i32]),
        ("emu_trk_read", None, [vp, vp, vp, vp, vp]),
        ("emu_trk_gather", None, [vp, vp, vp]),
        ("emu_trk_poke", None, [vp, i32, i32, i32]),
        ("emu_trk_plan", i32, [i32, i32, vp]),
    ])


class HostForm:
    """ais_amd.vessel_table behind the interface track_cases.run_script drives"""

    def __init__(self, capacity, max_rows=MAX_ROWS):
        import ais_amd

        self.t = ais_amd.vessel_table(capacity)
        self.max_rows = max_rows

    def update(self, cols, strs, recs, n, stamp):
        n = n if 0 <= n <= self.max_rows else 0  # (the device form merges nothing for such a count)
        self.t.update(cols[:, :n], strs[:n], stamp, recs[:n] if recs is not None else None)

    def expire(self, min_stamp):
        return self.t.expire(min_stamp)

    def state(self):
        cols, strs, chg = self.t.arrays()
        return cols, strs, chg, [self.t.counts[k] for k in tc.COUNTS[:7]]


class ModelForm(HostForm):
    def __init__(self, capacity, max_rows=MAX_ROWS):
        self.t = tc.Model(capacity)
        self.max_rows = max_rows

    def update(self, cols, strs, recs, n, stamp):
        self.t.update(cols, strs, stamp, recs, n if 0 <= n <= self.max_rows else 0)

    def state(self):
        return self.t.state()


class LaneForm:
    """the kernel bodies on the CPU lane model"""

    def __init__(self, capacity, max_rows=MAX_ROWS):
        self.h = emu().emu_trk_create(capacity, max_rows)
        assert self.h
        self.capacity, self.max_rows = capacity, max_rows
        self.bad = 0

    def __del__(self):
        emu().emu_trk_destroy(self.h)

    def update(self, cols, strs, recs, n, stamp):
        assert cols.shape == (tc.NMSG, self.max_rows) and cols.flags.c_contiguous and strs.flags.c_contiguous
        cnt = np.array([n], dtype=np.int32)
        emu().emu_trk_process(self.h, cols.ctypes.data, self.max_rows, strs.ctypes.data, recs.ctypes.data if recs is not None else None,
                              cnt.ctypes.data, stamp)

    def expire(self, min_stamp):
        emu().emu_trk_expire(self.h, min_stamp)

    def read(self):
        cols = np.zeros((tc.NCOL, self.capacity), dtype=np.int32)
        strs = np.zeros((self.capacity, tc.STR), dtype=np.uint8)
        chg = np.zeros(self.max_rows, dtype=np.int32)
        cnt = np.zeros(8, dtype=np.int32)
        emu().emu_trk_read(self.h, cols.ctypes.data, strs.ctypes.data, chg.ctypes.data, cnt.ctypes.data)
        self.bad |= int(cnt[7])
        return cols, strs, chg, cnt

    def state(self):
        cols, strs, chg, cnt = self.read()
        return cols[:, :cnt[0]], strs[:cnt[0]], chg[:cnt[4]], [int(v) for v in cnt[:7]]

    def gathered(self):
        cols = np.zeros((tc.NCOL, self.max_rows), dtype=np.int32)
        strs = np.zeros((self.max_rows, tc.STR), dtype=np.uint8)
        emu().emu_trk_gather(self.h, cols.ctypes.data, strs.ctypes.data)
        return cols, strs


def feed(form, payloads, stamp, recs=None, max_rows=MAX_ROWS):
    cols, strs = tc.message_rows(payloads)
    c, s, r = tc.pad(cols, strs, recs, max_rows)
    form.update(c, s, r, len(payloads), stamp)


def both(capacity):
    return [HostForm(capacity), ModelForm(capacity)]


def vessel(form, v):
    cols, strs, _, _ = form.state()
    d = {name: int(cols[k, v]) for k, name in enumerate(tc.COLUMNS)}
    d["callsign"], d["name"] = bytes(strs[v, 0:7]), bytes(strs[v, 8:28])
    return d


# ---- the host form against the model ---------------------------------------------------------------------------------
def test_names_agree_with_the_header():
    import ais_amd

    assert tuple(ais_amd.TRACK_COLUMNS) == tc.COLUMNS and tuple(ais_amd.TRACK_COUNTS) == tc.COUNTS
    hdr = open(os.path.join(os.path.dirname(HERE), "include", "aisx.h")).read()
    enum = hdr[hdr.index("AISX_TRK_COL_COUNT"):hdr.index("AISX_TRK_NCOL")]
    assert [t for t in ("COUNT", "STAMP", "POS_STAMP", "CHAN") if "AISX_TRK_COL_" + t in enum] == list(tc.COLUMNS[tc.NMSG:])
    assert ais_amd.TRACK_DTYPE.names[: tc.NCOL] == tuple(c.lower() for c in tc.COLUMNS)


def test_static_parts_and_a_position_meet_in_one_vessel():
    rng = np.random.default_rng(1)
    forms = both(16)
    for k, p in enumerate([tc.static_a(244660123, "NOORDERLICHT", rng), tc.static_b(244660123, "PD1234", rng),
                           tc.position_b(244660123, 2893000, 31281000, rng)]):
        for f in forms:
            feed(f, [p], 10 + k)
        tc.assert_same_state(forms[0].state(), forms[1].state())
    v = vessel(forms[0], 0)
    assert forms[0].state()[3][0] == 1
    assert v["name"] == b"NOORDERLICHT@@@@@@@@" and v["callsign"] == b"PD1234@"
    assert (v["LON"], v["LAT"], v["SHIPTYPE"], v["TYPE"]) == (2893000, 31281000, 70, 18)
    assert (v["COUNT"], v["STAMP"], v["POS_STAMP"], v["CHAN"]) == (3, 12, 12, tc.NA)


def test_na_and_nul_never_overwrite_and_a_later_row_wins():
    rng = np.random.default_rng(2)
    forms = both(4)
    recs = np.zeros(4, dtype=mc.REC_DTYPE)
    recs["chan"] = [5, 6, 7, 8]
    one = [tc.position_a(211000001, 100, 200, rng, sog=11), tc.static_a(211000001, "FIRST", rng),
           tc.position_a(211000001, 300, 400, rng, sog=22), tc.static_b(211000001, "CALL", rng)]
    for f in forms:
        feed(f, one, 1, recs)
    tc.assert_same_state(forms[0].state(), forms[1].state())
    v = vessel(forms[0], 0)
    # within one call the later position wins; the static rows carry neither and leave it alone
    assert (v["LON"], v["LAT"], v["SOG"], v["NAV_STATUS"]) == (300, 400, 22, 0) and v["name"].startswith(b"FIRST@")
    assert (v["TYPE"], v["PART"], v["COUNT"], v["CHAN"], v["POS_STAMP"]) == (24, 1, 4, 8, 1)
    for f in forms:
        feed(f, [tc.static_a(211000001, "SECOND", rng)], 2, recs[:1])
    tc.assert_same_state(forms[0].state(), forms[1].state())
    v = vessel(forms[0], 0)
    # across calls: the name is replaced, the call sign (slot not carried) and the position (NA columns) stay
    assert v["name"].startswith(b"SECOND@") and v["callsign"] == b"CALL@@@" and (v["LON"], v["SOG"]) == (300, 22)
    assert (v["STAMP"], v["POS_STAMP"], v["COUNT"], v["CHAN"]) == (2, 1, 5, 5)


def test_skipped_rows_and_the_extreme_mmsis():
    rng = np.random.default_rng(3)
    forms = both(8)
    cols, strs, recs = tc.random_rows(rng, [0, (1 << 30) - 1, 7, 0, 7, (1 << 30) - 1, 9], p_skip=0.0)
    cols[tc.C["FLAGS"], 2] |= 4
    cols[tc.C["MMSI"], 4] = tc.NA
    for f in forms:
        f.update(*tc.pad(cols, strs, recs, MAX_ROWS), 7, 1)
    tc.assert_same_state(forms[0].state(), forms[1].state())
    cols_t, _, chg, cnt = forms[0].state()
    assert cnt[:5] == [3, 5, 2, 0, 3] and list(chg) == [0, 1, 2]
    assert list(cols_t[tc.C["MMSI"]]) == [0, (1 << 30) - 1, 9] and list(cols_t[tc.C["COUNT"]]) == [2, 2, 1]


def test_a_full_table_keeps_the_first_by_row_order():
    rng = np.random.default_rng(4)
    forms = both(10)
    mmsis = tc.distinct_ints(rng, 1, 1 << 30, 25)
    rows = np.concatenate([mmsis, mmsis[[3, 20, 9]]])  # later rows of kept vessels merge, of a dropped one drop
    cols, strs, recs = tc.random_rows(rng, rows, p_skip=0.0)
    for f in forms:
        f.update(*tc.pad(cols, strs, recs, MAX_ROWS), len(rows), 1)
    tc.assert_same_state(forms[0].state(), forms[1].state())
    cols_t, _, chg, cnt = forms[0].state()
    assert cnt == [10, 12, 0, 16, 10, 0, 1]
    assert list(cols_t[tc.C["MMSI"]]) == list(mmsis[:10]) and list(chg) == list(range(10))
    assert list(cols_t[tc.C["COUNT"]]) == [1, 1, 1, 2, 1, 1, 1, 1, 1, 2]
    for f in forms:  # the flag is the last update's
        f.update(*tc.pad(cols[:, :5], strs[:5], recs[:5], MAX_ROWS), 5, 2)
    assert forms[0].state()[3] == [10, 5, 0, 0, 5, 0, 0]


def test_count_saturates():
    import ais_amd

    rng = np.random.default_rng(5)
    t = ais_amd.vessel_table(2)
    cols, strs, recs = tc.random_rows(rng, [5, 5, 5], p_skip=0.0)
    t.update(cols[:, :1], strs[:1], 1)
    # (the table where it is: set the count just short of the top)
    c, stride = C.c_void_p(), C.c_long()
    from ais_amd import _lib

    _lib.lib(device=False).aisx_track_data(t._h, C.byref(c), C.byref(stride), None, None)
    np.ctypeslib.as_array(C.cast(c, C.POINTER(C.c_int32)), shape=(tc.NCOL, stride.value))[tc.C["COUNT"], 0] = tc.INT32_MAX - 1
    t.update(cols, strs, 2)
    assert t.arrays()[0][tc.C["COUNT"], 0] == tc.INT32_MAX and t.counts["merged"] == 3


def test_expire_keeps_order_and_an_expired_mmsi_comes_back_as_new():
    rng = np.random.default_rng(6)
    forms = both(6)
    a, b = tc.random_rows(rng, [11, 22, 33, 44], p_skip=0.0), tc.random_rows(rng, [22, 44], p_skip=0.0)
    for f in forms:
        f.update(*tc.pad(*a, MAX_ROWS), 4, 1)
        f.update(*tc.pad(*b, MAX_ROWS), 2, 2)
        assert f.expire(2) in (2, None)
    tc.assert_same_state(forms[0].state(), forms[1].state())
    cols_t, _, chg, cnt = forms[0].state()
    assert list(cols_t[tc.C["MMSI"]]) == [22, 44] and len(chg) == 0 and cnt == [2, 2, 0, 0, 0, 2, 0]
    c = tc.random_rows(rng, [55, 11, 44], p_skip=0.0)
    for f in forms:
        f.update(*tc.pad(*c, MAX_ROWS), 3, 3)
    tc.assert_same_state(forms[0].state(), forms[1].state())
    cols_t, _, chg, cnt = forms[0].state()
    assert list(cols_t[tc.C["MMSI"]]) == [22, 44, 55, 11] and list(chg) == [2, 3, 1]
    assert list(cols_t[tc.C["COUNT"]]) == [2, 3, 1, 1]  # 11 starts again


def test_changed_list_is_ordered_by_first_touching_row():
    forms = both(8)
    for f in forms:
        f.update(*tc.pad(*tc.random_rows(np.random.default_rng(70), [1, 2, 3, 4], p_skip=0.0), MAX_ROWS), 4, 1)
        f.update(*tc.pad(*tc.random_rows(np.random.default_rng(71), [3, 9, 1, 3, 9, 4, 1], p_skip=0.0), MAX_ROWS), 7, 2)
    tc.assert_same_state(forms[0].state(), forms[1].state())
    assert list(forms[0].state()[2]) == [2, 4, 0, 3]


@pytest.mark.parametrize("capacity", [10, 64, 300])
def test_host_form_equals_the_model_on_the_scripts(capacity):
    for name, ops in tc.scripts(100 + capacity, capacity, MAX_ROWS).items():
        tc.run_script(ops, [HostForm(capacity), ModelForm(capacity)], MAX_ROWS)


def test_host_argument_checks():
    import ais_amd

    with pytest.raises(ValueError):
        ais_amd.vessel_table(0)
    t = ais_amd.vessel_table(3)
    with pytest.raises(ValueError):
        t.update(np.zeros((tc.NMSG, 2), np.int32), np.zeros((3, tc.STR), np.uint8), 1)
    assert t.update(np.zeros((tc.NMSG, 0), np.int32), np.zeros((0, tc.STR), np.uint8), 1)["merged"] == 0


# ---- the kernel bodies on the lane model against the host form ----------------------------------------------------------
@pytest.fixture(scope="module")
def all_scripts():
    return {cap: tc.scripts(100 + cap, cap, MAX_ROWS) for cap in (10, 64, 300)}


@pytest.mark.parametrize("capacity", [10, 64, 300])
@pytest.mark.parametrize("name", ["n0", "n1", "n63", "n64", "n65", "n257", "one_mmsi", "distinct", "full_distinct", "bad_count",
                                  "sequence"])
def test_lane_model_equals_the_host_form(all_scripts, capacity, name):
    lane = LaneForm(capacity)

    def gathered(k, op):  # the gather of read_changed: row j is vessel changed[j]
        cols, strs, chg, _ = lane.state()
        g = lane.gathered()
        assert np.array_equal(g[0][:, :len(chg)], cols[:, chg]) and np.array_equal(g[1][:len(chg)], strs[chg])

    tc.run_script(all_scripts[capacity][name], [HostForm(capacity), lane], MAX_ROWS, gathered)
    assert lane.bad == (1 if name == "bad_count" else 0)


def test_lane_model_is_the_same_from_run_to_run(all_scripts):
    ops = all_scripts[64]["sequence"] + all_scripts[64]["one_mmsi"]
    runs = []
    for _ in range(3):
        lane = LaneForm(64)
        tc.run_script(ops, [lane], MAX_ROWS)
        cols, strs, chg, cnt = lane.read()
        runs.append((cols[:, :cnt[0]].copy(), strs[:cnt[0]].copy(), chg[:cnt[4]].copy(), list(cnt[:7])))
    for r in runs[1:]:
        tc.assert_same_state(r, runs[0])


def test_lane_model_count_saturates():
    rng = np.random.default_rng(8)
    lane, host = LaneForm(4), HostForm(4)
    cols, strs, recs = tc.random_rows(rng, [5] * 70 + [6], p_skip=0.0)
    p, stride = C.c_void_p(), C.c_long()
    for f in (lane, host):
        f.update(*tc.pad(cols[:, :1], strs[:1], recs[:1], MAX_ROWS), 1, 1)
    # both tables where they are: vessel 0's count just short of the top
    emu().emu_trk_poke(lane.h, tc.C["COUNT"], 0, tc.INT32_MAX - 3)
    from ais_amd import _lib

    _lib.lib(device=False).aisx_track_data(host.t._h, C.byref(p), C.byref(stride), None, None)
    np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_int32)), shape=(tc.NCOL, stride.value))[tc.C["COUNT"], 0] = tc.INT32_MAX - 3
    for f in (lane, host):
        f.update(*tc.pad(cols, strs, recs, MAX_ROWS), 71, 2)
    tc.assert_same_state(lane.state(), host.state())
    assert list(host.state()[0][tc.C["COUNT"]]) == [tc.INT32_MAX, 1]
