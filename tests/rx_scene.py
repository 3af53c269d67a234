"""The small receiver scene of test_gpu_rx_std.py and test_gpu_rx_options.py: 2 streams, 2 centres, cs16 input, 3 blocks
of 4096 x 5 items at 250 kS/s, max_pdus_per_block = 256.  ais_amd.gmsk_scene sends payloads of 21, 20 and 53 octets on
every lane (= stream * 2 + centre); a caller may add waveforms of its own before the noise."""
import numpy as np

FS, DECIM, ITEMS, NBLOCKS = 250e3, 5, 4096, 3
BLOCK = ITEMS * DECIM
DES = ("A", "B")
CENTRES = (-25e3, 25e3)
BURSTS = ((21, 1500), (20, 10000), (53, 19000), (53, 34000), (21, 49000))  # (octets, first item) on lane 0, + 137 items a lane


def payload(rng, n):
    """n random octets under the message type that has this length: 1 (21 octets), 24 part A (20), 5 (53)"""
    p = bytearray(rng.integers(0, 256, n, dtype=np.uint8).tobytes())
    p[0] = ({21: 1, 20: 24, 53: 5}[n] << 2) | (p[0] & 3)
    if n == 20:
        p[4] &= 0xFC  # (bits 38, 39: part number 0)
    return bytes(p)


def build(ais, bursts=BURSTS, extra=()):
    """raw cs16 blocks [2][NBLOCKS * BLOCK][2], the payloads per lane and the receiver's template.  extra: (stream, first
    item, complex items at FS) added to the stream before the noise"""
    import synth

    rng = np.random.default_rng(61)
    sps, T = FS / 9600.0, NBLOCKS * BLOCK
    pay, chan, start, cfo, lanes = [], [], [], [], {}
    for lane in range(4):
        for n, s0 in bursts:
            p = payload(rng, n)
            pay.append(p)
            chan.append(lane // 2)
            start.append(s0 + 137 * lane)
            cfo.append((CENTRES[lane % 2] + float(rng.uniform(-300, 300))) / FS)
            lanes.setdefault(lane, []).append(p)
    x = ais.gmsk_scene(pay, np.array(chan, np.int32), np.array(start, np.int64), sps, 2, 0, T, frac=rng.random(len(pay)).astype(np.float32) * 0.99,
                       cfo=np.array(cfo, np.float32), phase=rng.uniform(-3, 3, len(pay)).astype(np.float32))
    for stream, s0, iq in extra:
        x[stream, s0:s0 + len(iq)] += np.asarray(iq, np.complex64)
    sigma = float(np.sqrt(sps / 100.0 / 2.0))  # 20 dB in the channel's bandwidth, as test_gpu_tx.py's loop-back
    x = x + (rng.normal(0, sigma, x.shape) + 1j * rng.normal(0, sigma, x.shape)).astype(np.complex64)
    raw = np.rint(np.stack([x.real, x.imag], axis=-1) * 2.0 ** 13).astype(np.int16)
    tmpl = synth.resampled_template(synth.gmsk_waveform(np.array([1 if b else -1 for b in synth.sync_bits("P")], float), 40)[: 28 * 40],
                                    40, FS / DECIM / 9600.0)
    return dict(raw=raw, lanes=lanes, tmpl=tmpl)


def make_rx(ais, scene, **kw):
    return ais.ais_rx(CENTRES, FS, DES, nstreams=2, fmt="cs16", scale=2.0 ** -13, block_items=BLOCK,
                      preamble_symbols=scene["tmpl"], max_pdus_per_block=256, **kw)


def run(rx, scene, messages=False):
    """every block pushed, flushed, popped: [(block, recs, text[, messages])]; the status words are kept in rx.statuses"""
    out, rx.statuses = [], []
    pop = rx.pop_messages if messages else rx.pop
    for k in range(NBLOCKS):
        assert rx.push(scene["raw"][:, k * BLOCK:(k + 1) * BLOCK]) == k
    rx.flush()
    while (r := pop(wait=True)) is not None:
        rx.statuses.append(rx.status)
        out.append(r)
    assert [r[0] for r in out] == list(range(NBLOCKS))
    return out
