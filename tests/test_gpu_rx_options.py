"""-m gpu: the receiver's options in combination (ais_amd.ais_rx.enable_*, aisx_rx_enable_*).  The other receiver tests
anchor every single option to an expectation of its own; this file anchors the combinations to them: whatever the order
in which a set of options is enabled, the receiver is the same one, a refused enable leaves it as it was, and after the
first block only enable_messages on a handle that has messages is still accepted.

The scene is test_gpu_rx_std.py's (rx_scene: 2 streams, 2 centres, cs16, 3 blocks of 4096 x 5 items, max_pdus_per_block
256) with its fourth burst of every lane left out and, in its place on lane 0, one burst sent with payload bits 77 and 78
inverted (test_gpu_hdlc_events._burst), so that with the repair of all events the marks area of a result slot carries a
mark that is not -1."""
import ctypes as C
import itertools

import numpy as np
import pytest

import rx_scene as rs

pytestmark = pytest.mark.gpu

T0 = 1700000000
STATIONS = ["rx-North_1", ""]
TRACKS = 64
FLIP = 77
OPTIONS = ("nmea", "detector", "repair", "messages", "tracks")  # ascending order
SETS = [OPTIONS] + list(itertools.combinations(OPTIONS, 2))


@pytest.fixture(scope="module")
def ais():
    import torch

    assert torch.cuda.is_available(), "gpu tests need a visible MI355X"
    import ais_amd

    return ais_amd


@pytest.fixture(scope="module")
def scene(ais):
    import test_gpu_hdlc_events as ev

    rng = np.random.default_rng(29)
    p = rng.integers(0, 2, 168).tolist()
    p[2:8] = [1, 0, 0, 0, 0, 0]  # message type 1 (pdu[0] >> 2, bits packed LSB first)
    osf = 40
    iq = ev._burst(p, (FLIP, FLIP + 1), osf)
    dur = int(iq.size / osf * rs.FS / 9600.0)
    tg = np.arange(dur) * (osf * 9600.0 / rs.FS)
    ph = np.interp(tg, np.arange(iq.size), np.unwrap(np.angle(iq)))
    env = np.interp(tg, np.arange(iq.size), np.abs(iq))
    start = 34000
    assert start + dur < 49000  # (clear of lane 0's last burst)
    x = env * np.exp(1j * (ph + 2 * np.pi * ((rs.CENTRES[0] + 120.0) / rs.FS) * (start + np.arange(dur)) + 0.7))
    sc = rs.build(ais, bursts=[b for b in rs.BURSTS if b[1] != 34000], extra=[(0, start, x)])
    sc["flipped"] = ais.pdu_to_nmea("A").msg_to_sentence(np.packbits(np.array(p, np.uint8), bitorder="little").tobytes())
    return sc


def _enable(ais, rx, name, twice=False):
    if name == "nmea":
        rx.enable_standard_nmea(STATIONS, T0)
    elif name == "detector":
        rx.enable_detector("mlse", 0.4)
    elif name == "repair":
        if twice:  # the later call wins
            rx.enable_repair(ais.AIS_REPAIR_RULES, ais.REPAIR_SINGLE)
        rx.enable_repair(ais.AIS_REPAIR_RULES, ais.AIS_REPAIR_EVENTS)
    elif name == "messages":
        rx.enable_messages()
        if twice:
            rx.enable_messages()
    else:
        rx.enable_tracks(TRACKS)


def _outcome(rx, scene):
    """everything the receiver gives for the scene, in a form that compares with =="""
    popped, repairs = [], []
    pop = rx.pop_messages if rx.decode else rx.pop
    rx.statuses = []
    for k in range(rs.NBLOCKS):
        assert rx.push(scene["raw"][:, k * rs.BLOCK:(k + 1) * rs.BLOCK]) == k
    rx.flush()
    while (r := pop(wait=True)) is not None:
        rx.statuses.append(rx.status)
        popped.append((r[0], r[1].tobytes(), r[2]) + ((r[3].tobytes(),) if rx.decode else ()))
        if rx.repair:
            fix = rx.popped_repairs()
            assert len(fix) == len(r[1])
            repairs.append(fix.tolist())
    assert [r[0] for r in popped] == list(range(rs.NBLOCKS))
    out = dict(popped=popped, statuses=rx.statuses, repairs=repairs)
    if rx.tracks:
        (b1, v1), (b2, v2) = rx.read_tracks(), rx.read_changed_tracks()
        assert b1 == b2 == rs.NBLOCKS - 1 and len(v1) > 0
        out["tracks"], out["changed"] = v1.tobytes(), v2.tobytes()
    return out


def _text_cap(rx):
    from ais_amd import _lib

    tc = C.c_long()
    assert _lib.lib().aisx_rx_geometry(rx._h, None, None, None, None, None, C.byref(tc)) == _lib.AISX_OK
    return tc.value


@pytest.mark.parametrize("names", SETS, ids=["+".join(s) for s in SETS])
def test_the_order_of_the_enables_does_not_matter(ais, scene, names):
    full = names == OPTIONS
    outs = []
    for order in (names, names[::-1]):
        rx = rs.make_rx(ais, scene)
        for name in order:
            _enable(ais, rx, name, twice=full and order is names)
        assert rx.decode == ("messages" in names or "tracks" in names) and rx.repair == ("repair" in names)
        assert rx.tracks == (TRACKS if "tracks" in names else 0) and rx.nmea == ("standard" if "nmea" in names else "reference")
        outs.append(_outcome(rx, scene))
    assert outs[0] == outs[1]
    nrec = sum(len(f) for f in outs[0]["repairs"]) if "repair" in names else None
    print("%s: %d bytes of text, repair marks %s" % ("+".join(names), sum(len(p[2]) for p in outs[0]["popped"]), nrec))
    assert sum(len(p[2]) for p in outs[0]["popped"]) > 0
    if "repair" in names:  # the marks area of the result slots is exercised: the flipped burst's mark came through it
        marks = [f for blk in outs[0]["repairs"] for f in blk if f != -1]
        assert (FLIP | 1 << 16) in marks and ais.repair_mark(FLIP | 1 << 16) == (FLIP, (1, 1))
    if "nmea" in names:
        assert _text_cap(rx) > _text_cap(rs.make_rx(ais, scene))
    if full:  # the same again through the constructor's keywords
        rx = rs.make_rx(ais, scene, nmea="standard", stations=STATIONS, t0=T0, detector="mlse", bt=0.4, repair=ais.AIS_REPAIR_RULES,
                        repair_events=ais.AIS_REPAIR_EVENTS, decode=True, tracks=TRACKS)
        assert _outcome(rx, scene) == outs[0]


def test_a_refused_enable_leaves_the_handle_as_it_was(ais, scene):
    def make():
        return rs.make_rx(ais, scene, repair=ais.AIS_REPAIR_RULES, repair_events=ais.AIS_REPAIR_EVENTS, decode=True)

    rx = make()
    cap = _text_cap(rx)
    with pytest.raises(ValueError):
        rx.enable_tracks(0)
    with pytest.raises(ValueError):
        rx.enable_detector(bt=5.0)
    with pytest.raises(ValueError):
        rx.enable_standard_nmea(["a b", ""])
    with pytest.raises(ValueError):
        rx.enable_repair(ais.AIS_REPAIR_RULES, 8)
    assert _text_cap(rx) == cap
    got, want = _outcome(rx, scene), _outcome(make(), scene)
    assert got == want
    assert any(f != -1 for blk in got["repairs"] for f in blk)  # (the repair of all events is still the one in force)
    flipped = [p for p in got["popped"] if scene["flipped"].encode("latin-1") in p[2]]
    assert len(flipped) == 1
    with pytest.raises(ValueError):
        rx.read_tracks(0, 1)


def test_after_the_first_block_only_messages_on_a_handle_that_has_them(ais, scene):
    def refused(rx, names):
        for name in names:
            with pytest.raises(ValueError):
                _enable(ais, rx, name)

    plain, decoding = rs.make_rx(ais, scene), rs.make_rx(ais, scene, decode=True)
    want = _outcome(rs.make_rx(ais, scene, decode=True), scene)
    for rx in (plain, decoding):
        assert rx.push(scene["raw"][:, :rs.BLOCK]) == 0
    refused(plain, OPTIONS)
    refused(decoding, [n for n in OPTIONS if n != "messages"])
    decoding.enable_messages()
    # neither handle changed: the blocks that follow give what they always gave
    for rx in (plain, decoding):
        for k in range(1, rs.NBLOCKS):
            assert rx.push(scene["raw"][:, k * rs.BLOCK:(k + 1) * rs.BLOCK]) == k
        rx.flush()
    got = []
    while (r := decoding.pop_messages(wait=True)) is not None:
        got.append((r[0], r[1].tobytes(), r[2], r[3].tobytes()))
    assert got == want["popped"]
    texts = []
    while (r := plain.pop(wait=True)) is not None:
        texts.append(r[2])
    assert texts == [p[2] for p in want["popped"]]
