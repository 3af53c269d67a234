"""-m gpu: the pipelined chain (ais_demod.work_pipelined, stock chain) with the bit tail inside the recovery kernel
against a twin chain with the switch off: bits, produced and tags equal for every step.  The fused step's outputs are
complete on the recovery's stream, not on the bit tail's: wait(step) must be all a reader of the bits needs."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

OPTS = dict(samples_per_symbol=4, bits_per_sec=9600.0, clockrec_gain=0.04, omega_relative_limit=0.01, fftlen=1024)


def test_pipelined_chain_with_the_fused_tail_equals_the_unfused_chain():
    import torch
    import ais_amd as ais
    import synth

    nchan, T, steps = 64, 4096, 4
    xs = np.stack([synth.make_channel(5200 + c, T * steps, "S", 4, amp=0.3, cfo_max=500.0)[0] for c in range(nchan)])
    a = ais.ais_demod(OPTS, nchan=nchan, max_items=T, stages="stock")
    b = ais.ais_demod(OPTS, nchan=nchan, max_items=T, stages="stock")
    b.clockrec.set_fused_tail(False)
    chunks = [torch.as_tensor(xs[:, s * T:(s + 1) * T]).cuda() for s in range(steps)]
    reader = torch.cuda.Stream()
    nbits = 0
    for s in range(steps):
        nxt = chunks[s + 1] if s + 1 < steps else None
        res = []
        for dem, fused in ((a, True), (b, False)):
            r = dem.work_pipelined(chunks[s], x_next=nxt)
            assert dem.clockrec.last_tail_fused() == fused
            # nothing but wait(step) orders this stream behind the step's outputs
            dem.wait(step=r["step"], stream=reader)
            with torch.cuda.stream(reader):
                bits, prod = r["bits"].clone(), r["produced"].clone()
            reader.synchronize()
            res.append((prod.cpu().numpy(), bits.cpu().numpy(), dem.step_tags(r["step"])))
        (pa, ba, ta), (pb, bb, tb) = res
        assert np.array_equal(pa, pb), s
        for c in range(nchan):
            assert np.array_equal(ba[c, : pa[c]], bb[c, : pb[c]]), (s, c)
        assert ta.tobytes() == tb.tobytes(), s
        nbits += int(pa.sum())
    a.synchronize()
    b.synchronize()
    assert a.clockrec.last_status() == 0 and b.clockrec.last_status() == 0
    assert nbits > nchan * (T * steps - 2048) / 4 * 0.9
