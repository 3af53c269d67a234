"""The duplicate suppression on the MI355X (aisx_dedup_batch_*, ais_amd.pdu_dedup_batch) against the host form
aisx_dedup_* that is its specification, array for array: the scripts of tests/dedup_cases.py at the lane model's small
shapes (max_pdus 257 and 1, windows 0, 1 and 3), two handles interleaved on two streams, and the chain text ->
nmea_to_pdu_batch -> pdu_dedup_batch -> pdu_decode_batch -> vessel_table_batch on one stream against parse, pdu_dedup, decode
of the kept payloads only and vessel_table on the host.  -m gpu."""
import numpy as np
import pytest

import dedup_cases as dc
import test_dedup_model as tm
import track_cases as tc

pytestmark = pytest.mark.gpu

MAX_PDUS = tm.MAX_PDUS


@pytest.fixture(scope="module")
def ais():
    import torch

    assert torch.cuda.is_available()
    import ais_amd

    return ais_amd


@pytest.fixture(scope="module")
def all_scripts():
    return {(w, m): dc.scripts(1000 + 10 * w + m, w, m) for w in tm.WINDOWS for m in (MAX_PDUS, 1)}


class DeviceForm:
    """ais_amd.pdu_dedup_batch behind the interface dedup_cases.run_script drives"""

    def __init__(self, ais, window, max_pdus=MAX_PDUS, stream=None):
        self.t = ais.pdu_dedup_batch(window, max_pdus, 64)
        self.max_pdus, self.stream, self.bad = max_pdus, stream, 0

    def reset(self):
        self.t.reset()

    def queue(self, recs, data, n, stamp, marks, nfound=None):
        """False when the stamp is refused; else the call is queued and nothing has waited"""
        import torch

        with torch.cuda.stream(self.stream or torch.cuda.current_stream()):
            d = [torch.from_numpy(recs.view(np.uint8).copy()).cuda(), torch.from_numpy(data).cuda(),
                 torch.tensor([n, n if nfound is None else nfound], dtype=torch.int32, device="cuda"),
                 torch.from_numpy(marks).cuda() if marks is not None else None]
        try:
            self.t.work_device(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[2].data_ptr() + 4, stamp,
                               d[3].data_ptr() if d[3] is not None else None, stream=self.stream)
        except IndexError:
            return False
        self.keep, self.with_marks, self.overflow_ok = d, marks is not None, nfound is not None  # (the work is queued, not done)
        return True

    def read(self):
        try:
            out, first, copies, om = self.t._read(self.stream, self.overflow_ok)
        except ValueError:  # a bad count: said once, then the flag is clear
            self.bad += 1
            out, first, copies, om = self.t._read(self.stream, False)
        self.keep = None
        return out.copy(), first.copy(), copies.copy(), om.copy() if self.with_marks else None, [self.t.counts[c] for c in dc.COUNTS]

    def call(self, *args, **kw):
        return self.read() if self.queue(*args, **kw) else None


@pytest.mark.parametrize("window", tm.WINDOWS)
@pytest.mark.parametrize("name", tm.NAMES)
def test_device_equals_the_host_form(ais, all_scripts, window, name):
    dev = DeviceForm(ais, window)
    dc.run_script(all_scripts[(window, MAX_PDUS)][name], [tm.HostForm(window), dev])
    assert dev.bad == (2 if name == "bad_count" else 0)


@pytest.mark.parametrize("window", tm.WINDOWS)
def test_device_with_one_record_at_most(ais, all_scripts, window):
    for name in tm.NAMES_1:
        dev = DeviceForm(ais, window, 1)
        dc.run_script(all_scripts[(window, 1)][name], [tm.HostForm(window, 1), dev])
        assert dev.bad == (2 if name == "bad_count" else 0)


@pytest.mark.parametrize("window", tm.WINDOWS)
def test_device_on_wrapping_and_crowded_chains(ais, window):
    scripts, payloads = dc.chain_scripts(77 + window, window, MAX_PDUS)
    bits = dc.hash_bits(MAX_PDUS)
    assert len(set(payloads["wrap"])) == 3 and all(dc.home(dc.key(p), bits) == (1 << bits) - 1 for p in payloads["wrap"])
    assert len(set(payloads["crowd"])) == 8 and all(dc.home(dc.key(p), bits) == 17 for p in payloads["crowd"])
    for name in ("wrap", "crowd"):
        dc.run_script(scripts[name], [tm.HostForm(window), DeviceForm(ais, window)])


def test_device_is_the_same_from_run_to_run(ais, all_scripts):
    ops = all_scripts[(3, MAX_PDUS)]["random0"] + all_scripts[(3, MAX_PDUS)]["runs"] + all_scripts[(3, MAX_PDUS)]["all_same"]
    ops = [op if op[0] == "reset" else op[:4] + (100 + k,) + op[5:] for k, op in enumerate(ops)]  # (rising stamps)
    runs = [dc.run_script(ops, [DeviceForm(ais, 3)]) for _ in range(3)]
    for r in runs[1:]:
        for a, b in zip(r, runs[0]):
            dc.assert_same_result(a, b)


def test_two_interleaved_handles(ais):
    import torch

    rng = np.random.default_rng(21)
    P = dc.pool(rng, 30)
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    da, db = DeviceForm(ais, 1, MAX_PDUS, sa), DeviceForm(ais, 3, 64, sb)
    ha, hb = tm.HostForm(1, MAX_PDUS), tm.HostForm(3, 64)
    seen = np.zeros(5, dtype=np.int64)
    for k in range(6):
        na, nb = int(rng.integers(100, MAX_PDUS + 1)), int(rng.integers(20, 65))
        opa = dc.call([P[int(j)] for j in rng.integers(0, 30, size=na)], rng, MAX_PDUS, 10 + k)
        opb = dc.call([P[int(j)] for j in rng.integers(0, 12 + 3 * k, size=nb)], rng, 64, 3 * k - 7)
        # A's call is queued on its stream and B's on its own before either is read
        assert da.queue(*opa[1:]) and db.queue(*opb[1:])
        ra, rb = da.read(), db.read()
        dc.assert_same_result(ha.call(*opa[1:]), ra, "A %d" % k)
        dc.assert_same_result(hb.call(*opb[1:]), rb, "B %d" % k)
        seen += np.array(ra[4]) + np.array(rb[4])
    assert seen[1] > 0 and seen[2] > 0 and seen[3] > 0 and da.bad == db.bad == 0


def test_what_the_producer_found_beyond_its_records_and_the_reads(ais):
    rng = np.random.default_rng(9)
    dev = DeviceForm(ais, 1)
    P = dc.pool(rng, 4)
    recs, data, marks = dc.make_list([P[0], P[1], P[0], P[2]], rng, MAX_PDUS)
    r = dev.call(recs, data, 4, 1, marks, nfound=9)
    assert r[4] == [4, 3, 1, 0, 0] and dev.t.found == 3 + 5
    with pytest.raises(OverflowError):  # (the producer's overflow shows downstream)
        dev.t.pdus()
    assert list(dev.t.first(overflow_ok=True)) == [0, 1, 0, 2] and list(dev.t.copies(overflow_ok=True)) == [2, 1, 1]
    assert np.array_equal(dev.t.marks(overflow_ok=True), marks[[0, 1, 3]]) and dev.t.get_counts()["dup_call"] == 1
    p, b, n = dev.t.results_device()
    assert p and b and n and all(dev.t.extras_device())


def test_argument_checks_and_an_unused_handle(ais):
    for bad in ((-1, 4, 64), (16, 4, 64), (1, 0, 64), (1, (1 << 24) + 1, 64), (1, 4, 1), (1, 4, 1025)):
        with pytest.raises(ValueError):
            ais.pdu_dedup_batch(*bad)
    t = ais.pdu_dedup_batch(15, 16)  # create / destroy without a call; the read of a handle that never worked
    assert len(t.pdus()) == 0 and t.get_counts() == dict.fromkeys(dc.COUNTS, 0)
    del t


def _traffic(rng, nships, repeats):
    """positions and static parts of a few ships, each heard `repeats` times, in a shuffled order"""
    pl = []
    for k, m in enumerate(200000000 + tc.distinct_ints(rng, 1, 99999999, nships)):
        m = int(m)
        pl += [tc.position_a(m, 3000 + k, 4000 + k, rng), tc.static_a(m, "SHIP %d" % k, rng), tc.position_b(m, 1000 + k, 2000 + k, rng)]
    pl = pl * repeats
    return [pl[i] for i in rng.permutation(len(pl))]


def test_chain_from_text_to_the_vessel_table(ais):
    import torch

    rng = np.random.default_rng(31)
    first = _traffic(rng, 50, 2)           # 300 sentences of which half repeat within the call
    second = first[:100] + _traffic(rng, 30, 1)  # 100 of them once more (the window's), and 90 new ones
    third = first[:40]                     # outside the window of 1 again: kept, with COUNT growing
    arm = {c: ais.pdu_to_nmea(c, standard=True) for c in "AB"}
    chunks = [("".join(arm["AB"[i % 2]].msg_to_sentence(p) + "\n" for i, p in enumerate(pl))).encode() for pl in (first, second, third)]
    max_pdus, stamps = 320, (5, 6, 8)
    ps = ais.nmea_to_pdu_batch(["A", "B"], 64, max(len(c) for c in chunks), 400, max_pdus)
    dd = ais.pdu_dedup_batch(1, max_pdus, 64)
    md = ais.pdu_decode_batch(2, max_pdus, 64)
    vt = ais.vessel_table_batch(256, max_pdus)
    hp, hd, ht = ais.nmea_to_pdu(["A", "B"], 64), ais.pdu_dedup(1), ais.vessel_table(256)
    s = torch.cuda.Stream()
    seen = np.zeros(5, dtype=np.int64)
    for chunk, stamp in zip(chunks, stamps):
        # the host path: parse, suppress, decode the kept payloads only, merge
        recs, data, _, cnt = hp.work(chunk)
        kept, first_h, copies_h, _ = hd.work_records(recs, data, stamp)
        cols, strs = tc.message_rows([data[r["offset"]:r["offset"] + r["len"]].tobytes() for r in kept], decode=ais.msg_decode)
        ht.update(cols, strs, stamp, kept)
        seen += np.array([hd.counts[c] for c in dc.COUNTS])
        # the device path, queued on one stream: the host waits for nothing in between
        ps.work(chunk, stream=s)
        dd.work(ps, stamp, stream=s)
        md.work(dd, stream=s)
        vt.work(md, stamp, stream=s, deframer=dd)
        assert np.array_equal(dd.pdus(stream=s), kept) and dd.counts == hd.counts and dd.found == len(kept)
        assert np.array_equal(dd.first(stream=s), first_h) and np.array_equal(dd.copies(stream=s), copies_h)
        hc, hs, hchg = ht.arrays()
        dcols, dstrs = vt.arrays(stream=s)
        assert np.array_equal(dcols, hc) and np.array_equal(dstrs, hs)
        idx, cc, cs = vt.changed_arrays(stream=s)
        assert np.array_equal(idx, hchg) and np.array_equal(cc, hc[:, hchg]) and np.array_equal(cs, hs[hchg])
        c = vt.get_counts(stream=s)
        assert [c[x] for x in tc.COUNTS[:7]] == [ht.counts[x] for x in tc.COUNTS[:7]]
    # the condition, which the host form alone shows: records kept, and records suppressed in each class
    assert seen[1] > 0 and seen[2] >= 100 and seen[3] >= 100 and seen[4] == 0
    v = ht.vessels()
    assert len(v) == 80 and v["count"].max() <= 3 * 2  # transmissions, not receptions: 3 kinds, at most twice kept
    print("text of %d sentences: %d kept, %d + %d suppressed; %d vessels equal the host path's"
          % (seen[0], seen[1], seen[2], seen[3], len(v)))
