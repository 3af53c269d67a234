"""-m gpu: the host-fed receiver with the field decoder switched on (ais_amd.ais_rx(decode=True), aisx_rx_enable_messages
/ aisx_rx_pop_messages) on the stock 250 kS/s fixture, one stream, three blocks and a flush: text and records byte for
byte those of a handle without it, the table row for row ais_amd.msg_decode of the PDUs that the hand-wired pipeline of
test_gpu_rx.hand_wired deframes, and the refusals."""
import numpy as np
import pytest

import msg_cases as mc
import test_gpu_rx as tr
import test_gpu_xlate as tx

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


class _Tap:
    """ais_amd as hand_wired sees it, with one addition: every sentences() read also keeps the deframer's PDUs"""

    def __init__(self, ais):
        self._ais, self.pdus = ais, []

    def __getattr__(self, name):
        return getattr(self._ais, name)

    def hdlc_deframer_batch(self, *a, **kw):
        self.hd = self._ais.hdlc_deframer_batch(*a, **kw)
        return self.hd

    def pdu_to_nmea_batch(self, *a, **kw):
        nm, tap = self._ais.pdu_to_nmea_batch(*a, **kw), self
        read = nm.sentences

        def sentences(**k):
            tap.pdus.append(tap.hd.pdus(as_list=True))
            return read(**k)

        nm.sentences = sentences
        return nm


def _rows(m):
    return [tuple(int(r[c.lower()]) for c in mc.COLUMNS) + (bytes(r["callsign"]), bytes(r["name"]), bytes(r["destination"]))
            for r in m]


def _run(rx, blocks, pop):
    for k, b in enumerate(blocks):
        assert rx.push(b) == k
    rx.flush()
    out = []
    while (r := pop(wait=True)) is not None:
        out.append(r)
        assert rx.status == 0
    return out


def test_messages_beside_unchanged_text(ais, blocks):
    tap = _Tap(ais)
    wired = tr.hand_wired(tap, [tx._dev(b) for b in blocks], 1)
    plain = tr.make_rx(ais, "cf32", 1.0, 0.0, nstreams=1)
    assert plain.decode is False
    base = _run(plain, blocks, plain.pop)
    rx = ais.ais_rx((-25e3, 25e3), tx.FS_STOCK, ("A", "B"), nstreams=1, block_items=tx.T * tx.DECIM,
                    preamble_symbols=tx._template(ais), decode=True)
    got = _run(rx, blocks, rx.pop_messages)
    assert [g[0] for g in got] == [b[0] for b in base] == list(range(NBLOCKS))
    npdu = 0
    for g, b, w, pdus in zip(got, base, wired, tap.pdus):
        assert g[2] == b[2] == w[1] and g[1].tobytes() == b[1].tobytes() == w[0].tobytes()
        assert [(c, e) for c, e, _ in pdus] == [(int(r["chan"]), int(r["end_bit"])) for r in g[1]]
        assert _rows(g[3]) == [mc.row_of(ais.msg_decode(p)) for _, _, p in pdus]
        assert all(r[mc.COLUMNS.index("FLAGS")] & 4 == 0 for r in _rows(g[3]))
        npdu += len(pdus)
    assert npdu > 0
    assert rx.pop_messages() is None and rx.pop() is None
    print("ais_rx decode=True: %d messages in %d blocks equal msg_decode of the deframed PDUs; text unchanged" % (npdu, NBLOCKS))


def test_refusals_and_overflow_keeps_the_block(ais, blocks):
    from ais_amd.batch_framing import PDU_DTYPE

    plain = tr.make_rx(ais, "cf32", 1.0, 0.0, nstreams=1)
    with pytest.raises(ValueError):
        plain.pop_messages()  # (messages were not enabled)
    plain.push(blocks[0])
    with pytest.raises(ValueError):
        plain.enable_messages()  # (only before the first block)
    assert plain.decode is False
    plain.flush()
    assert plain.pop(wait=True)[0] == 0  # (the handle goes on as before)
    rx = tr.make_rx(ais, "cf32", 1.0, 0.0, nstreams=1)
    rx.slot()
    with pytest.raises(ValueError):
        rx.enable_messages()  # (a slot has been acquired)
    del rx
    rx = tr.make_rx(ais, "cf32", 1.0, 0.0, nstreams=1)
    rx.enable_messages()
    rx.enable_messages()  # (again: nothing changes)
    for k, b in enumerate(blocks):
        rx.push(b)
    rx.flush()
    want = None
    for k in range(NBLOCKS):
        keep = rx._recs
        rx._recs = np.zeros(1, dtype=PDU_DTYPE)  # room for one record only
        try:
            r = rx.pop_messages(wait=True)  # (a block of at most one record fits)
            assert len(r[1]) <= 1
        except OverflowError:
            rx._recs = keep
            r = rx.pop_messages(wait=True)
            assert len(r[1]) > 1
            want = r
        rx._recs = keep
        assert r[0] == k and len(r[3]) == len(r[1])
    assert want is not None  # (some block had to be asked for twice, and came back whole)
    assert rx.pop_messages(wait=True) is None
