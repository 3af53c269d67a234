"""The vessel table on the MI355X (aisx_track_batch_*, ais_amd.vessel_table_batch) against the host form aisx_track_*
that is its specification, array for array: the scripts of tests/track_cases.py at the lane model's small shapes
(capacity 10, 64 and 300, max_rows 257), run-to-run identity, a saturating count, and the chain msg_cases.pack PDUs ->
pdu_decode_batch -> vessel_table_batch on one stream without a host synchronisation between them: read_changed against
read, its overflow return, two handles interleaved, create / destroy without a call.  -m gpu."""
import numpy as np
import pytest

import msg_cases as mc
import test_track_model as tm
import track_cases as tc

pytestmark = pytest.mark.gpu

MAX_ROWS = tm.MAX_ROWS


@pytest.fixture(scope="module")
def ais():
    import torch

    assert torch.cuda.is_available()
    import ais_amd

    return ais_amd


@pytest.fixture(scope="module")
def all_scripts():
    return {cap: tc.scripts(100 + cap, cap, MAX_ROWS) for cap in (10, 64, 300)}


class DeviceForm:
    """ais_amd.vessel_table_batch behind the interface track_cases.run_script drives"""

    def __init__(self, ais, capacity, max_rows=MAX_ROWS, stream=None):
        self.t = ais.vessel_table_batch(capacity, max_rows)
        self.max_rows, self.stream, self.bad, self.keep = max_rows, stream, 0, []

    def update(self, cols, strs, recs, n, stamp):
        import torch

        with torch.cuda.stream(self.stream or torch.cuda.current_stream()):
            d = [torch.from_numpy(cols).cuda(), torch.from_numpy(strs).cuda(),
                 torch.from_numpy(recs.view(np.uint8).copy()).cuda() if recs is not None else None,
                 torch.tensor([n], dtype=torch.int32, device="cuda")]
        self.keep.append(d)  # (the work is queued, not done)
        self.t.work_device(d[0].data_ptr(), self.max_rows, d[1].data_ptr(), d[3].data_ptr(), stamp,
                           d[2].data_ptr() if d[2] is not None else None, stream=self.stream)

    def expire(self, min_stamp):
        self.t.expire(min_stamp, stream=self.stream)

    def state(self):
        try:
            cols, strs = self.t.arrays(stream=self.stream)
        except ValueError:  # a bad count since the last read: said once, then the flag is clear
            self.bad += 1
            cols, strs = self.t.arrays(stream=self.stream)
        idx, ccols, cstrs = self.t.changed_arrays(stream=self.stream)
        cnt = self.t.get_counts(stream=self.stream)
        self.keep = []
        assert cnt["bad_input"] == 0 and cols.shape[1] == cnt["vessels"] == self.t.nvessels and len(idx) == cnt["changed"]
        # read_changed against read: row j of the gathered block is vessel idx[j]
        assert np.array_equal(ccols, cols[:, idx]) and np.array_equal(cstrs, strs[idx])
        return cols, strs, idx, [cnt[k] for k in tc.COUNTS[:7]]


@pytest.mark.parametrize("capacity", [10, 64, 300])
@pytest.mark.parametrize("name", ["n0", "n1", "n63", "n64", "n65", "n257", "one_mmsi", "distinct", "full_distinct", "bad_count",
                                  "sequence"])
def test_device_equals_the_host_form(ais, all_scripts, capacity, name):
    dev = DeviceForm(ais, capacity)
    tc.run_script(all_scripts[capacity][name], [tm.HostForm(capacity), dev], MAX_ROWS)
    assert dev.bad == (2 if name == "bad_count" else 0)  # (two bad calls, each read about once)


def test_device_is_the_same_from_run_to_run(ais, all_scripts):
    ops = all_scripts[64]["sequence"] + all_scripts[64]["one_mmsi"] + all_scripts[64]["full_distinct"]
    runs = []
    for _ in range(3):
        dev = DeviceForm(ais, 64)
        runs.append(tc.run_script(ops, [dev], MAX_ROWS))
    for r in runs[1:]:
        tc.assert_same_state(r, runs[0])


def test_count_saturates(ais):
    rng = np.random.default_rng(8)
    dev = DeviceForm(ais, 4)
    cols, strs, recs = tc.random_rows(rng, [5] * 70 + [6], p_skip=0.0)
    dev.update(*tc.pad(cols[:, :1], strs[:1], recs[:1], MAX_ROWS), 1, 1)
    assert dev.state()[0][tc.C["COUNT"], 0] == 1
    dev.t.results_device()["cols"][tc.C["COUNT"], 0] = tc.INT32_MAX - 3  # the table where it is
    dev.update(*tc.pad(cols, strs, recs, MAX_ROWS), 71, 2)
    got = dev.state()
    assert list(got[0][tc.C["COUNT"]]) == [tc.INT32_MAX, 1] and got[3][:2] == [2, 71]


def test_argument_checks_and_an_unused_handle(ais):
    for cap, rows in ((0, 10), (10, 0), (-1, 10), ((1 << 24) + 1, 10)):
        with pytest.raises(ValueError):
            ais.vessel_table_batch(cap, rows)
    t = ais.vessel_table_batch(10, 16)  # create / destroy without a call; reads of the empty table
    assert len(t.vessels()) == 0 and len(t.changed()) == 0 and t.get_counts() == dict.fromkeys(tc.COUNTS, 0)
    r = t.results_device()
    assert r["cols"].shape == (tc.NCOL, 10) and r["strs"].shape == (10, 48) and r["changed"].shape == (16,) and r["count"].shape == (8,)
    del r, t
    t = ais.vessel_table_batch(10, 16)
    del t


def _fleet(rng, nships=40):
    """static parts, positions and other traffic of a few ships, several receptions each, in a shuffled order"""
    mmsis = 200000000 + tc.distinct_ints(rng, 1, 99999999, nships)
    pl = []
    for k, m in enumerate(mmsis):
        m = int(m)
        pl += [tc.static_a(m, "SHIP %d" % k, rng), tc.static_b(m, "C%d" % k, rng), tc.position_b(m, 1000 + k, 2000 + k, rng),
               tc.position_a(m, 3000 + k, 4000 + k, rng), tc.position_a(m, 5000 + k, 6000 + k, rng)]
    pl += mc.edge_cases(rng) + mc.random_cases(rng, per_type=1)
    return [pl[i] for i in rng.permutation(len(pl))]


def test_behind_the_decoder_on_one_stream(ais):
    import torch

    rng = np.random.default_rng(9)
    batches = [_fleet(rng), _fleet(rng), _fleet(rng)]
    max_pdus = max(len(b) for b in batches) + 3
    md = ais.pdu_decode_batch(3, max_pdus, 64)
    va, vb = ais.vessel_table_batch(1000, max_pdus), ais.vessel_table_batch(30, max_pdus)  # two handles, interleaved
    ha, hb = ais.vessel_table(1000), ais.vessel_table(30)
    s = torch.cuda.Stream()
    for k, pl in enumerate(batches):
        recs, data = mc.pack(pl, rng, max_pdus=max_pdus)
        with torch.cuda.stream(s):
            d_recs, d_data = torch.from_numpy(recs.view(np.uint8).copy()).cuda(), torch.from_numpy(data).cuda()
            d_cnt = torch.tensor([len(pl), len(pl)], dtype=torch.int32, device="cuda")
        # decode and merge, queued one behind the other: the host waits for nothing in between
        md.work_device(d_recs.data_ptr(), d_data.data_ptr(), d_cnt.data_ptr(), None, stream=s)
        c, stride, sp, n = md.results_device()
        va.work_device(c, stride, sp, n + 4, k, d_recs.data_ptr(), stream=s)
        vb.work_device(c, stride, sp, n + 4, k, None, stream=s)
        if k == 1:
            va.expire(1, stream=s)
        cols, strs = tc.message_rows(pl, decode=ais.msg_decode)
        ha.update(cols, strs, k, recs[:len(pl)])
        hb.update(cols, strs, k)
        if k == 1:
            ha.expire(1)
        for dev, host in ((va, ha), (vb, hb)):
            hc, hs, hchg = host.arrays()
            dc, ds = dev.arrays(stream=s)
            assert np.array_equal(dc, hc) and np.array_equal(ds, hs), k
            cnt = dev.get_counts(stream=s)
            assert [cnt[x] for x in tc.COUNTS[:7]] == [host.counts[x] for x in tc.COUNTS[:7]]
            if len(hchg) > 1:  # too small a buffer: the count needed comes back, nothing else
                with pytest.raises(OverflowError):
                    dev.changed_arrays(cap=len(hchg) - 1, stream=s)
                assert dev.nchanged == len(hchg)
            idx, cc, cs = dev.changed_arrays(stream=s)
            assert np.array_equal(idx, hchg) and np.array_equal(cc, hc[:, hchg]) and np.array_equal(cs, hs[hchg])
        del d_recs, d_data, d_cnt
    v = va.vessels(stream=s)
    assert hb.counts["full"] == 1 and len(vb.vessels(stream=s)) == 30 and 40 < len(v) <= 1000
    ships = v[np.char.startswith(v["name"], b"SHIP ")]
    assert len(ships) >= 40 and (ships["lon"] != tc.NA).all() and (ships["callsign"] != b"").all()
    assert set(ais.TRACK_DTYPE.names) <= set(va.changed(stream=s).dtype.names)
    print("3 steps of %d PDUs: %d vessels, the tables, counts and changed lists equal the host form's" % (max_pdus - 3, len(v)))
