"""-m gpu: the host-fed receiver with the vessel table switched on (ais_amd.ais_rx(tracks=capacity), aisx_rx_enable_tracks
/ aisx_rx_read_tracks / aisx_rx_read_changed_tracks) on the stock 250 kS/s fixture, one stream, three blocks and a flush:
the table after the last block equals the host form fed with pop_messages()' rows block by block, stamp = the block's
number; a handle without tracks goes on as before; the refusals."""
import numpy as np
import pytest

import test_gpu_rx as tr
import test_gpu_xlate as tx
import track_cases as tc

pytestmark = pytest.mark.gpu

NBLOCKS = 3


@pytest.fixture(scope="module")
def ais():
    import torch

    assert torch.cuda.is_available(), "gpu tests need a visible MI355X"
    import ais_amd

    return ais_amd


@pytest.fixture(scope="module")
def blocks():
    xs, _ = tx._stock_inputs()
    return tr.blocks_of(np.ascontiguousarray(xs[:1]), NBLOCKS)


def _make(ais, **kw):
    return ais.ais_rx((-25e3, 25e3), tx.FS_STOCK, ("A", "B"), nstreams=1, block_items=tx.T * tx.DECIM,
                      preamble_symbols=tx._template(ais), **kw)


def _same(a, b):
    return a.dtype == b.dtype and a.tobytes() == b.tobytes()


def test_table_equals_the_host_form_fed_block_by_block(ais, blocks):
    rx = _make(ais, tracks=64)
    assert rx.decode is True and rx.tracks == 64
    assert rx.read_tracks()[0] == -1 and len(rx.read_tracks()[1]) == 0  # (before the first block)
    host = ais.vessel_table(64)
    for k, b in enumerate(blocks):
        assert rx.push(b) == k
    rx.flush()
    nrows, texts = 0, []
    while (r := rx.pop_messages(wait=True)) is not None:
        assert rx.status == 0
        host.update(r[3], None, r[0], r[1])
        nrows += len(r[1])
        texts.append(r[2])
    block, got = rx.read_tracks()
    want = host.vessels()
    assert block == NBLOCKS - 1 and nrows > 0 and len(want) > 0
    assert _same(got, want)
    assert (got["stamp"] <= NBLOCKS - 1).all() and (got["chan"] >= 0).all() and got["count"].sum() == nrows
    block, chg = rx.read_changed_tracks()
    assert block == NBLOCKS - 1 and _same(chg, host.changed())
    assert _same(rx.read_tracks(first=1, n=2)[1], want[1:3])
    # a handle without tracks: the same text, no table
    plain = _make(ais, decode=True)
    assert plain.tracks == 0
    for b in blocks:
        plain.push(b)
    plain.flush()
    base = []
    while (r := plain.pop_messages(wait=True)) is not None:
        base.append(r[2])
    assert base == texts
    with pytest.raises(ValueError):
        plain.read_tracks()
    with pytest.raises(ValueError):
        plain.read_changed_tracks()
    print("ais_rx tracks=64: %d rows in %d blocks -> %d vessels equal the host form's" % (nrows, NBLOCKS, len(want)))


def test_refusals(ais, blocks):
    import torch

    free0 = torch.cuda.mem_get_info()[0]
    plain = _make(ais)
    used_plain = free0 - torch.cuda.mem_get_info()[0]
    plain.push(blocks[0])
    with pytest.raises(ValueError):
        plain.enable_tracks(64)  # (only before the first block)
    assert plain.tracks == 0 and plain.decode is False
    plain.flush()
    assert plain.pop(wait=True)[0] == 0  # (the handle goes on as before)
    del plain
    rx = _make(ais)
    rx.slot()
    with pytest.raises(ValueError):
        rx.enable_tracks(64)  # (a slot has been acquired)
    del rx
    rx = _make(ais, decode=True)
    with pytest.raises(ValueError):
        rx.enable_tracks(0)
    assert rx.tracks == 0
    rx.enable_tracks(1 << 16)  # (after enable_messages: fine)
    with pytest.raises(ValueError):
        rx.enable_tracks(64)  # (once)
    del rx
    torch.cuda.synchronize()
    # what a handle that never asked holds on the device has not grown by a table's worth (2^16 vessels: 26 MB and more)
    free1 = torch.cuda.mem_get_info()[0]
    again = _make(ais)
    assert free1 - torch.cuda.mem_get_info()[0] <= used_plain + (8 << 20)
    del again
