"""-m gpu: the host-fed receiver with the standard NMEA form behind it (ais_amd.ais_rx(nmea="standard", stations=, t0=),
aisx_rx_enable_standard_nmea) against a twin receiver in the reference form on the same blocks, at the small geometry
of test_gpu_rx_paths.py: 2 streams, 2 centres, 3 blocks of 4096 x 5 items.  The scene (ais_amd.gmsk_scene) carries
payloads of 21, 20 and 53 octets, of which the reference form's text keeps only the first intact.

A popped record carries text, not octets, so the twin's PDUs are found through its text: every sentence the twin pops is
the reference-form sentence of exactly one transmitted payload of its lane (the frames are CRC-checked), and that payload
is the PDU.  The standard receiver's text must then be the host aisx_pdu_to_nmea_std of those PDUs, ids taken in record
order over the blocks and the time by the block formula; its strict parse returns every one of them intact; and its
decoded messages and vessel table are the twin's."""
import math

import numpy as np
import pytest

import nmea_cases as nc
from rx_scene import BLOCK, DES, FS, NBLOCKS
from rx_scene import make_rx as _rx
from rx_scene import run as _run

pytestmark = pytest.mark.gpu

T0 = 1700000000
STATIONS = ["rx-North_1", ""]


@pytest.fixture(scope="module")
def ais():
    import torch

    assert torch.cuda.is_available(), "gpu tests need a visible MI355X"
    import ais_amd

    return ais_amd


@pytest.fixture(scope="module")
def scene(ais):
    """raw cs16 blocks [2][NBLOCKS * BLOCK][2] and the payloads per lane (= stream * 2 + centre)"""
    import rx_scene

    return rx_scene.build(ais)


@pytest.fixture(scope="module")
def twin(ais, scene):
    """the reference-form receiver's blocks, and per block the PDUs behind its records: [(chan, end_bit, payload)]"""
    rx = _rx(ais, scene, decode=True, tracks=64)
    popped = _run(rx, scene, messages=True)
    by_text = {}
    for lane, ps in scene["lanes"].items():
        for p in ps:
            by_text[(lane, ais.pdu_to_nmea(DES[lane % 2]).msg_to_sentence(p))] = p
    pdus = []
    for b, recs, text, _ in popped:
        pdus.append([(c, e, by_text[(c, t)]) for c, e, t in nc.split(recs, text)])  # (KeyError: a sentence nobody sent)
    got = {len(p) for blk in pdus for _, _, p in blk}
    print("twin: %d of %d payloads recovered" % (sum(len(b) for b in pdus), sum(len(v) for v in scene["lanes"].values())))
    assert got == {20, 21, 53}  # (the test needs every length; the clean scene gives nearly all bursts)
    return popped, pdus, rx.statuses


def _expected(ais, pdus, stations=STATIONS, t0=T0):
    """the host standard function over the twin's PDUs: per block (records [(chan, end_bit, text)], stream)"""
    nid, out = 0, []
    for b, blk in enumerate(pdus):
        t = t0 + math.floor(float(b) * BLOCK / FS) if t0 >= 0 else -1
        recs, stream = [], b""
        for c, e, p in blk:
            nm = ais.pdu_to_nmea(DES[c % 2], standard=True, station=stations[c // 2], time=t)
            nm.next_id = nid
            s = nm.msg_to_sentence(p)
            nid = nm.next_id
            recs.append((c, e, s))
            stream += (s + "\n").encode("latin-1")
        out.append((recs, stream))
    return out


def test_text_is_the_host_function_of_the_twins_pdus(ais, scene, twin):
    _, pdus, statuses = twin
    rx = _rx(ais, scene, nmea="standard", stations=STATIONS, t0=T0)
    popped = _run(rx, scene)
    assert rx.statuses == statuses
    for (b, recs, text), (wrecs, wstream) in zip(popped, _expected(ais, pdus)):
        assert text == wstream, b
        assert nc.split(recs, text) == wrecs
    # the ids ran over the blocks in record order: one per 53-octet payload
    ids = [int(t.split("!")[1].split(",")[3]) for _, recs, text in popped for _, _, t in nc.split(recs, text) if "\n" in t]
    assert len(ids) >= 2 and ids == [k % 10 for k in range(len(ids))]
    # every payload the twin recovers is in the strict parse of the standard text, intact, on its lane
    # (the parser tells channels apart by designator: A and B repeat per stream, so its chan is the centre)
    all_text = b"".join(p[2] for p in popped)
    recs, data, times, counts = ais.nmea_to_pdu(DES, 64).work(all_text)
    assert all(counts[k] == 0 for k in counts if k.startswith("REJ_")), counts
    parsed = [(int(r["chan"]), bytes(data[r["offset"]:r["offset"] + r["len"]])) for r in recs]
    assert parsed == [(c % 2, p) for blk in pdus for c, _, p in blk]
    assert (times == T0).all()  # (three blocks of 81.92 ms: all within the first second)
    # where the reference form's own text, read as strictly, loses the payloads of 20 and 53 octets
    ref_text = b"".join(p[2] for p in twin[0])
    r2, d2, _, _ = ais.nmea_to_pdu(DES, 64).work(ref_text)
    intact = {bytes(d2[r["offset"]:r["offset"] + r["len"]]) for r in r2}
    sent = [p for blk in pdus for _, _, p in blk]
    print("strict parse: standard text %d of %d intact, reference text %d" % (len(parsed), len(sent), sum(p in intact for p in sent)))
    assert all(p in intact for p in sent if len(p) == 21)


def test_decoder_and_vessel_table_behind_the_standard_form(ais, scene, twin):
    popped_twin, pdus, statuses = twin
    rx = _rx(ais, scene, nmea="standard", stations=STATIONS, t0=T0, decode=True, tracks=64)
    popped = _run(rx, scene, messages=True)
    assert rx.statuses == statuses
    want = _expected(ais, pdus)
    for (b, recs, text, msgs), (_, wrecs, _, wmsgs), (_, wstream) in zip(popped, popped_twin, want):
        assert text == wstream
        assert msgs.tobytes() == wmsgs.tobytes() and len(msgs) == len(recs) == len(wrecs)
        assert (recs["chan"] == wrecs["chan"]).all() and (recs["end_bit"] == wrecs["end_bit"]).all()
    twin_rx = _rx(ais, scene, decode=True, tracks=64)
    _run(twin_rx, scene, messages=True)
    (b1, v1), (b2, v2) = rx.read_tracks(), twin_rx.read_tracks()
    assert b1 == b2 == NBLOCKS - 1 and len(v1) > 0 and v1.tobytes() == v2.tobytes()


def test_no_stations_no_time_and_the_argument_rules(ais, scene, twin):
    _, pdus, _ = twin
    rx = _rx(ais, scene, nmea="standard")  # no tag block at all: the standard sentences alone
    popped = _run(rx, scene)
    for (b, recs, text), (wrecs, wstream) in zip(popped, _expected(ais, pdus, ["", ""], -1)):
        assert text == wstream and text.startswith(b"!AIVDM")
    with pytest.raises(ValueError):
        _rx(ais, scene, nmea="standard", stations=["a b", ""])
    with pytest.raises(ValueError):
        _rx(ais, scene, nmea="standard", stations=["a"] * 3)
    with pytest.raises(ValueError):
        _rx(ais, scene, stations=["a", "b"])
    with pytest.raises(ValueError):
        _rx(ais, scene, nmea="other")
    # only before the first block, and once
    from ais_amd import _lib

    assert _lib.lib().aisx_rx_enable_standard_nmea(rx._h, None, 0) == _lib.AISX_ERR_INVALID
    fresh = _rx(ais, scene, nmea="standard")
    assert _lib.lib().aisx_rx_enable_standard_nmea(fresh._h, None, 0) == _lib.AISX_ERR_INVALID


def test_block_times_follow_the_formula(ais):
    """48 kS/s, blocks of 65536 items: 1.365 s a block, so blocks 0..3 carry t0 + 0, 1, 2, 4"""
    fs, block, nb, t0 = 48000.0, 65536, 4, 1699999998
    rng = np.random.default_rng(62)
    pay = [bytes(rng.integers(0, 256, 21, dtype=np.uint8)) for _ in range(nb)]
    start = np.array([k * block + 20000 for k in range(nb)], np.int64)
    x = ais.gmsk_scene(pay, np.zeros(nb, np.int32), start, 5.0, 1, 0, nb * block, cfo=np.float32(100.0 / fs))
    sigma = float(np.sqrt(5.0 / 100.0 / 2.0))  # 20 dB
    x = x + (rng.normal(0, sigma, x.shape) + 1j * rng.normal(0, sigma, x.shape)).astype(np.complex64)
    rx = ais.ais_rx(0.0, fs, "A", block_items=block, max_pdus_per_block=64, nmea="standard", stations="S", t0=t0)
    seen = {}
    for k in range(nb):
        rx.push(x[:, k * block:(k + 1) * block])
    rx.flush()
    while (r := rx.pop(wait=True)) is not None:
        for _, _, t in nc.split(r[1], r[2]):
            seen.setdefault(r[0], set()).add(t.split("\\")[1].split("*")[0])
    assert len(seen) >= 3, seen
    for b, tags in seen.items():
        assert tags == {"s:S,c:%d" % (t0 + math.floor(float(b) * block / fs))}, (b, tags)
    assert {math.floor(float(b) * block / fs) for b in range(nb)} == {0, 1, 2, 4}
