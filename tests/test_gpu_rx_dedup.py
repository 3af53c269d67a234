"""-m gpu: the host-fed receiver with the duplicate suppression switched on (ais_amd.ais_rx(dedup=window),
aisx_rx_enable_dedup / aisx_rx_popped_dedup) on the stock 250 kS/s fixture, three streams of which stream 1 is a copy of
stream 0, three blocks and a flush, nmea="standard" (whose text reads back exactly): block by block the dedup receiver's
sentences, rows and repair marks are those of the plain receiver's records that ais_amd.pdu_dedup(1) keeps, its counts the
host form's, its vessel table the host table fed the kept rows; the refusals."""
import numpy as np
import pytest

import dedup_cases as dc
import test_gpu_rx as tr
import test_gpu_xlate as tx

pytestmark = pytest.mark.gpu

NBLOCKS, NSTREAMS, WINDOW = 3, 3, 1


@pytest.fixture(scope="module")
def ais():
    import torch

    assert torch.cuda.is_available(), "gpu tests need a visible MI355X"
    import ais_amd

    return ais_amd


@pytest.fixture(scope="module")
def blocks():
    xs, _ = tx._stock_inputs()
    return tr.blocks_of(np.ascontiguousarray(xs[[0, 0, 1]]), NBLOCKS)  # stream 1 hears what stream 0 hears


def _make(ais, **kw):
    return ais.ais_rx((-25e3, 25e3), tx.FS_STOCK, ("A", "B"), nstreams=NSTREAMS, block_items=tx.T * tx.DECIM,
                      preamble_symbols=tx._template(ais), max_pdus_per_block=1024, nmea="standard", **kw)


def _run(rx, blocks, dedup):
    """[(block, records, text, rows, marks, counts or None)] of every block"""
    for k, b in enumerate(blocks):
        assert rx.push(b) == k
    rx.flush()
    out = []
    while (r := rx.pop_messages(wait=True)) is not None:
        assert rx.status == 0
        out.append(r + (rx.popped_repairs(), rx.popped_dedup() if dedup else None))
    return out


@pytest.fixture(scope="module")
def both(ais, blocks):
    plain = _make(ais, repair=ais.AIS_REPAIR_RULES, decode=True)
    dd = _make(ais, repair=ais.AIS_REPAIR_RULES, dedup=WINDOW, tracks=64)
    assert dd.dedup == WINDOW and plain.dedup is None
    with pytest.raises(ValueError):
        plain.popped_dedup()
    assert dd.popped_dedup() == dict.fromkeys(dc.COUNTS, 0)  # (before the first pop)
    a, b = _run(plain, blocks, False), _run(dd, blocks, True)
    return a, b, dd.read_tracks(), dd.read_changed_tracks()


def _sentences(recs, text):
    return [text[r["offset"]:r["offset"] + r["len"]] for r in recs]


def _kept(ais, plain):
    """per block of the plain receiver: (kept indices, host counts), by pdu_dedup on the payloads its text reads back to"""
    host, parser, out = ais.pdu_dedup(WINDOW), ais.nmea_to_pdu(["A", "B"], 64), []
    for block, recs, text, rows, marks, _ in plain:
        precs, data, _, cnt = parser.work(text)
        assert len(precs) == len(recs) and cnt["SENTENCES"] == cnt["LINES"]  # (one message per record, in record order)
        kept, first, copies = host.work([data[r["offset"]:r["offset"] + r["len"]].tobytes() for r in precs], block)
        out.append((kept, dict(host.counts)))
    return out


def test_sentences_counts_rows_and_marks_are_the_kept_records(ais, both):
    plain, dd, _, _ = both
    assert [p[0] for p in plain] == [d[0] for d in dd] == list(range(NBLOCKS))
    nkept = nsupp = 0
    for (block, recs, text, rows, marks, _), (_, drecs, dtext, drows, dmarks, dcounts), (kept, counts) in zip(plain, dd, _kept(ais, plain)):
        assert _sentences(drecs, dtext) == [_sentences(recs, text)[i] for i in kept], block
        assert dcounts == counts and counts["in"] == len(recs) and counts["bad_len"] == 0, block
        assert np.array_equal(drecs["chan"], recs["chan"][kept]) and np.array_equal(drecs["end_bit"], recs["end_bit"][kept])
        assert drows.tobytes() == rows[kept].tobytes() and len(dmarks) == len(kept) and np.array_equal(dmarks, marks[kept])
        # stream 1 is a copy of stream 0, whose records come first: it contributes nothing of its own
        assert len(drecs) == 0 or not np.isin(drecs["chan"], (2, 3)).any()
        assert (recs["chan"] // 2 == 1).sum() == (recs["chan"] // 2 == 0).sum()
        nkept += len(kept)
        nsupp += len(recs) - len(kept)
    assert nkept > 0 and nsupp > 0  # the condition: some sentence is kept and some suppressed
    print("ais_rx dedup=%d: %d records kept, %d suppressed in %d blocks" % (WINDOW, nkept, nsupp, NBLOCKS))


def test_table_counts_transmissions(ais, both):
    plain, dd, (tblock, table), (cblock, changed) = both
    host = ais.vessel_table(64)
    for (block, recs, text, rows, marks, _), (kept, _) in zip(plain, _kept(ais, plain)):
        host.update(rows[kept], None, block, recs[kept])
    want = host.vessels()
    assert tblock == cblock == NBLOCKS - 1 and len(want) > 0
    assert table.dtype == want.dtype and table.tobytes() == want.tobytes()
    assert changed.tobytes() == host.changed().tobytes()
    assert table["count"].sum() == sum(len(d[1]) for d in dd) < sum(len(p[1]) for p in plain)


def test_refusals(ais, blocks):
    import torch

    def plain_rx():
        return ais.ais_rx((-25e3, 25e3), tx.FS_STOCK, ("A", "B"), nstreams=NSTREAMS, block_items=tx.T * tx.DECIM,
                          preamble_symbols=tx._template(ais))

    free0 = torch.cuda.mem_get_info()[0]
    plain = plain_rx()
    used_plain = free0 - torch.cuda.mem_get_info()[0]
    plain.push(blocks[0])
    with pytest.raises(ValueError):
        plain.enable_dedup(1)  # (only before the first block)
    assert plain.dedup is None
    with pytest.raises(ValueError):
        plain.popped_dedup()
    plain.flush()
    assert plain.pop(wait=True)[0] == 0  # (the handle goes on as before)
    del plain
    rx = plain_rx()
    rx.slot()
    with pytest.raises(ValueError):
        rx.enable_dedup(1)  # (a slot has been acquired)
    del rx
    rx = plain_rx()
    for w in (-1, 16):
        with pytest.raises(ValueError):
            rx.enable_dedup(w)
        assert rx.dedup is None
    rx.enable_dedup(15)
    with pytest.raises(ValueError):
        rx.enable_dedup(2)  # (once)
    assert rx.dedup == 15 and rx.popped_dedup() == dict.fromkeys(dc.COUNTS, 0)
    rx.push(blocks[0])
    rx.flush()
    assert rx.pop(wait=True)[0] == 0 and rx.popped_dedup()["in"] > 0 and rx.status == 0
    del rx
    torch.cuda.synchronize()
    # what a handle that never asked holds on the device has not grown by the stage's worth (16 sets of 2^17 keys and
    # the call's hash at the default max_pdus_per_block of 2^16: 20 MB and more)
    free1 = torch.cuda.mem_get_info()[0]
    again = plain_rx()
    assert free1 - torch.cuda.mem_get_info()[0] <= used_plain + (8 << 20)
    del again
