"""The batched NMEA armouring on the MI355X (aisx_nmea_batch_*, ais_amd.pdu_to_nmea_batch) against the host
aisx_pdu_to_nmea that is its specification: the cases of tests/nmea_cases.py written straight into device PDU lists,
behind hdlc_deframer_batch at 1, 37 and 4096 channels, behind the stock pipelined chain at 4096 channels queued as
its docstring says, two handles interleaved on one stream, and the deframer's overflow surfacing here.  -m gpu."""
import numpy as np
import pytest

import hdlc_cases as hc
import nmea_cases as nc

pytestmark = pytest.mark.gpu

SPS = 4
OPTS = dict(samples_per_symbol=SPS, bits_per_sec=9600.0, clockrec_gain=0.04, omega_relative_limit=0.01, fftlen=1024)


@pytest.fixture(scope="module")
def ais():
    import torch

    assert torch.cuda.is_available()
    import ais_amd

    return ais_amd


def _device_list(case, max_pdus):
    import torch

    recs, data = nc.pack(case["records"], max_pdus)
    d_recs = torch.from_numpy(recs.view(np.uint8).copy()).cuda()
    d_data = torch.from_numpy(data).cuda()
    n = case.get("npdus", len(case["records"]))
    d_cnt = torch.tensor([n, case.get("nfound", 0)], dtype=torch.int32, device="cuda")
    return d_recs, d_data, d_cnt


def _run_case(ais, case, stream=None):
    max_pdus = case.get("max_pdus", max(len(case["records"]), 1))
    nm = ais.pdu_to_nmea_batch(case["designators"], len(case["designators"]), max_pdus, case["length_max"],
                               case.get("text_cap", 0))
    d_recs, d_data, d_cnt = _device_list(case, max_pdus)
    nm.work_device(d_recs.data_ptr(), d_data.data_ptr(), d_cnt.data_ptr(),
                   d_cnt.data_ptr() + 4 if "nfound" in case else None, stream=stream)
    return nm, (d_recs, d_data, d_cnt)


def _check_case(ais, case):
    nm, keep = _run_case(ais, case)
    want, stream, kept = nc.expected(case)
    if case.get("bad"):
        with pytest.raises(ValueError):
            nm.sentences()  # (once: the read clears the flag)
    overflow = kept < case.get("nfound", case.get("npdus", len(case["records"])))
    if overflow:
        with pytest.raises(OverflowError):
            nm.sentences()
    recs, text = nm.sentences(overflow_ok=overflow)
    assert text == stream and len(recs) == kept, case["name"]
    assert nc.split(recs, text) == want
    assert nm.found == case.get("nfound", case.get("npdus", len(case["records"])))
    return kept


def test_cases_on_device_lists(ais):
    rng = np.random.default_rng(21)
    n = 0
    for case in nc.all_cases(rng):
        n += _check_case(ais, case)
    base = nc.mixed(rng)
    _check_case(ais, dict(base, name="zero", records=[]))
    _check_case(ais, dict(base, name="zero_count", npdus=0))
    _, stream, _ = nc.expected(base)
    _check_case(ais, dict(base, name="cap", text_cap=len(stream) // 2 + 1))
    _check_case(ais, dict(base, name="producer", npdus=100, nfound=250))
    for bad_n in (-1, len(base["records"]) + 1):
        nm, _ = _run_case(ais, dict(base, npdus=bad_n))
        with pytest.raises(ValueError):
            nm.sentences()
        recs, text = nm.sentences()
        assert len(recs) == 0 and text == b""
    print("%d records identical to aisx_pdu_to_nmea" % n)


def _host_text(designators, pdus):
    """[(chan, end_bit, payload)] -> the host function's [(chan, end_bit, text)] and stream"""
    import ais_amd

    conv = {d: ais_amd.pdu_to_nmea(d) for d in set(designators)}
    out, parts = [], []
    for c, e, p in pdus:
        t = conv[designators[c]].msg_to_sentence(p) if len(p) else ""
        out.append((c, e, t))
        if t:
            parts.append(t + "\n")
    return out, "".join(parts).encode("latin-1")


def _designators(nch):
    pool = ["A", "B", "", nc.D16, "AB"]
    return [pool[c % 5] for c in range(nch)]


def _streams(rng, nch):
    base = [hc.ais_stream(rng, 6, lengths=(11, 62))[0] for _ in range(min(nch, 61))]
    return [np.roll(np.asarray(base[c % len(base)], np.uint8), 977 * c) for c in range(nch)]


@pytest.mark.parametrize("nch", [1, 37, 4096])
def test_behind_the_deframer(ais, nch):
    import torch

    rng = np.random.default_rng(200 + nch)
    streams = _streams(rng, nch)
    cuts = [sorted(rng.integers(0, len(s), 2)) for s in streams]
    calls = hc.split_calls(streams, cuts)
    stride = max(len(x) for call in calls for x in call) + 5
    des = _designators(nch)
    hd = ais.hdlc_deframer_batch(11, 64, nch, stride, 1 << 16)
    nm = ais.pdu_to_nmea_batch(des, nch, 1 << 16, 64)
    s = torch.cuda.Stream()
    tot = 0
    for call in calls:
        rows, n = hc.pack(call, stride)
        with torch.cuda.stream(s):
            b = torch.from_numpy(rows).cuda()
            nb = torch.from_numpy(n).cuda()
        hd.work(b, nb, stream=s)
        nm.work(hd, stream=s)
        pdus = hd.pdus(stream=s, as_list=True)
        got = nm.sentences(stream=s, as_list=True)
        want, stream_bytes = _host_text(des, pdus)
        assert got == want
        assert nm.sentences(stream=s)[1] == stream_bytes
        tot += len(got)
    assert tot > 0
    print("%d channels: %d PDUs armoured identically to the host" % (nch, tot))


def _replicated(base, nchan):
    import torch

    nu, T = base.shape
    reps = nchan // nu
    x = torch.as_tensor(base).cuda().repeat(reps, 1)
    rot = torch.exp(1j * torch.linspace(0, 6.0, reps, device="cuda")).to(torch.complex64)
    rot[0] = 1.0
    return (x.view(reps, nu, T) * rot.view(-1, 1, 1)).reshape(nchan, T).contiguous()


def test_stock_chain_4096_channels_to_nmea(ais):
    """The pipelined stock chain at 4096 channels x 3 steps with the deframer and the NMEA stage queued behind every
    step on one caller stream; step k - 1's PDUs and text are read while step k runs.  Every step's text equals host
    armouring of that step's PDUs and splits into exactly the records' lines."""
    import torch

    import synth

    nchan, T, steps, K = 4096, 65536, 3, 16
    tmpl = ais.modulate_vector_bc(ais.gmsk_mod(SPS, 0.4), [1, 1, 0, 0] * 7, [1])
    made = [synth.make_channel(4100 + c, T * steps, "S", SPS, amp=0.3, cfo_max=500.0) for c in range(K)]
    xs = np.stack([m[0] for m in made])
    x_dev = [_replicated(xs[:, s * T:(s + 1) * T], nchan) for s in range(steps)]
    dem = ais.ais_demod(OPTS, nchan=nchan, max_items=T, stages="stock", preamble_symbols=tmpl)
    des = ["A", "B"] * (nchan // 2)
    hd = ais.hdlc_deframer_batch(11, 64, nchan, dem.clockrec.out_capacity, 1 << 16)
    nm = ais.pdu_to_nmea_batch(des, nchan, 1 << 16, 64)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    got = []

    def collect():
        pdus = hd.pdus(stream=s, as_list=True)
        recs, text = nm.sentences(stream=s)
        got.append((pdus, recs, text))

    for k in range(steps):
        r = dem.work_pipelined(x_dev[k], x_next=x_dev[k + 1] if k + 1 < steps else None)
        if k > 0:
            collect()
        dem.wait(r["step"], stream=s)
        hd.work(r["bits"], r["produced"], stream=s)
        nm.work(hd, stream=s)
    collect()
    dem.synchronize()
    npdu = 0
    for pdus, recs, text in got:
        want, stream_bytes = _host_text(des, pdus)
        assert text == stream_bytes
        assert nc.split(recs, text) == want
        npdu += len(recs)
    assert npdu > 0
    print("chain 4096 x %d steps: %d PDUs armoured on the device, identical to the host" % (steps, npdu))


def test_two_handles_interleaved_and_deframer_overflow(ais):
    import torch

    rng = np.random.default_rng(31)
    nch = 37
    streams = _streams(rng, nch)
    stride = max(len(x) for x in streams) + 5
    rows, n = hc.pack(streams, stride)
    b, nb = torch.from_numpy(rows).cuda(), torch.from_numpy(n).cuda()
    des1, des2 = _designators(nch), ["B"] * nch
    full = ais.hdlc_deframer_batch(11, 64, nch, stride, 1 << 12)
    small = ais.hdlc_deframer_batch(11, 64, nch, stride, 5)
    nm1 = ais.pdu_to_nmea_batch(des1, nch, 1 << 12, 64)
    nm2 = ais.pdu_to_nmea_batch("B", nch, 1 << 12, 64, text_cap=1000)
    nm3 = ais.pdu_to_nmea_batch(des1, nch, 1 << 12, 64)
    full.work(b, nb)
    small.work(b, nb)
    nm1.work(full)  # two handles interleaved on one stream, over the same PDUs
    nm2.work(full)
    nm3.work(small)
    nm1.work(full)
    pdus = full.pdus(as_list=True)
    assert len(pdus) > 5
    want1, s1 = _host_text(des1, pdus)
    want2, s2 = _host_text(des2, pdus)
    assert nm1.sentences(as_list=True) == want1 and nm1.sentences()[1] == s1
    with pytest.raises(OverflowError):
        nm2.sentences()
    recs2, text2 = nm2.sentences(overflow_ok=True)
    k2 = len(recs2)
    assert nm2.found == len(pdus) and 0 < k2 < len(pdus)
    assert text2 == s2[:len(text2)] and len(text2) <= 1000 < len(text2) + len(want2[k2][2]) + 1
    # the deframer's overflow: 5 PDUs kept of all found, the NMEA read reports it
    with pytest.raises(OverflowError):
        nm3.sentences()
    got3 = nm3.sentences(as_list=True, overflow_ok=True)
    assert nm3.found == len(pdus) and got3 == want1[:5]
