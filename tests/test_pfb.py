"""N3 (BASELINE config 5): the polyphase channelizer against the reference's
per-channel freq_xlating_fir_filter_ccf (oracle restatement), and every lane of
every frame against a float64 polyphase reference (pfb_ref64), with several streams,
strided rows and history carried across calls.  CPU lane model here; the -m gpu
tests at the bottom run the same comparisons on the device."""
import numpy as np
import pytest

import oracle_py as orc

FS = 25e6


def _wideband(rng, n):
    # a few narrow-band tones/carriers on lane centres and between them, plus noise
    t = np.arange(n)
    x = 0.05 * (rng.normal(size=n) + 1j * rng.normal(size=n))
    for lane, amp, off in [(3, 1.0, 0.0), (200, 0.7, 3000.0), (777, 0.5, -5000.0), (1023, 0.9, 1000.0)]:
        f = lane * FS / 1024 + off
        x = x + amp * np.exp(2j * np.pi * f / FS * t + 1j * rng.uniform(-3, 3))
    return x.astype(np.complex64)


def _check(out, x, taps, decim, lanes, k_list):
    for m in lanes:
        for k in k_list:
            want = orc.freq_xlating_fir(taps, decim, m * FS / 1024, FS, x, k, 1)[0]
            got = out[m, k]
            assert abs(got - want) < 2e-4 * max(1.0, abs(want)), (m, k, got, want)


@pytest.mark.parametrize("decim", [1024, 512])
def test_emul_pfb_matches_freq_xlating_filter(decim):
    import emul_py as emu

    rng = np.random.default_rng(decim)
    taps = orc.firdes_low_pass(1.0, FS, 11e3, 1e3)
    assert taps.size == 60227 and abs(taps.sum() - 1.0) < 1e-3
    nframes = [6, 2, 5]
    x = _wideband(rng, sum(nframes) * decim)
    p = emu.Pfb(taps, decim)
    outs, k = [], 0
    for nf in nframes:  # state (history, frame counter) carries across calls
        outs.append(p.work(x[k:k + nf * decim]))
        k += nf * decim
    out = np.concatenate(outs, axis=1)
    _check(out, x, taps, decim, [0, 3, 200, 511, 777, 1023], [0, 1, 5, 7, 12])
    # the tone sitting on lane 3 shows up on that lane and not on a far one (the 60227-tap
    # prototype is 59 frames long, so by frame 12 it is still filling)
    assert abs(out[3, 12]) > 20 * abs(out[100, 12])


def pfb_ref64(taps, decim, x, k0=0, nf=None):
    """float64 channelizer, all 1024 lanes of frames k0 .. k0 + nf - 1 of stream x (zero before it), from the
    identity in k_pfb.h's header: u_k[p] = sum_q h[p + qM] x[kD - p - qM], an M-point inverse DFT across p,
    times e^{-j 2 pi m k D / M}.  Returns [1024][nf] complex128."""
    M = 1024
    K = (taps.size + M - 1) // M
    h = np.zeros(K * M)
    h[:taps.size] = np.asarray(taps, np.float32)
    h = h.reshape(K, M)
    xp = np.concatenate([np.zeros(K * M), np.asarray(x, np.complex128)])
    nf = (x.size // decim - k0) if nf is None else nf
    out = np.empty((M, nf), np.complex128)
    m = np.arange(M)
    for b in range(0, nf, 32):
        ks = np.arange(k0 + b, k0 + min(nf, b + 32))
        # r[f, q, p] = x[kD - qM - p]: the window ending at kD, reversed
        win = np.stack([xp[K * M + k * decim - K * M + 1:K * M + k * decim + 1][::-1] for k in ks]).reshape(-1, K, M)
        u = np.einsum("qp,fqp->fp", h, win)
        y = M * np.fft.ifft(u, axis=1)
        rot = np.exp(-2j * np.pi * ((m[None, :] * ((ks[:, None] * decim) % M)) % M) / M)
        out[:, b:b + ks.size] = (y * rot).T
    return out


def _direct64(taps, decim, lane, x, k0, nout):
    # freq_xlating_fir_filter_ccf's direct form for one channel in float64 (what orc_freq_xlating_fir computes
    # before it rounds its output to float32)
    t = np.asarray(taps, np.float32).astype(np.float64)
    # (f_m n / fs = m n / 1024: the phase reduced exactly, so that a large argument does not cost digits)
    hr = t * np.exp(2j * np.pi * ((lane * np.arange(t.size)) % 1024) / 1024)
    xp = np.concatenate([np.zeros(t.size), np.asarray(x, np.complex128)])
    out = np.empty(nout, np.complex128)
    for i in range(nout):
        k = k0 + i
        w = xp[t.size + k * decim - t.size + 1:t.size + k * decim + 1][::-1]
        out[i] = np.dot(hr, w) * np.exp(-2j * np.pi * ((lane * decim * k) % 1024) / 1024)
    return out


def _frame_err(got, ref):
    """per frame: the largest lane error over the frame's RMS across all lanes"""
    rms = np.sqrt(np.mean(np.abs(ref) ** 2, axis=0))
    return np.max(np.abs(got - ref), axis=0) / rms


@pytest.mark.parametrize("decim", [1024, 512])
def test_pfb_ref64_matches_direct_form(decim):
    # the float64 polyphase reference against the per-channel direct form on 10 lanes: the oracle's
    # freq_xlating_fir, whose double sums are rounded to float32 on output (measured at most 5.7e-8 of the value,
    # gate 2^-23), and the same direct form kept in float64 with its phases reduced exactly (measured at most
    # 6e-15 of the frame's RMS over all lanes, gate 1e-12)
    rng = np.random.default_rng(5 + decim)
    taps = orc.firdes_low_pass(1.0, FS, 11e3, 1e3)
    nf = 70
    x = _wideband(rng, nf * decim)
    ref = pfb_ref64(taps, decim, x)
    rms = np.sqrt(np.mean(np.abs(ref) ** 2, axis=0))
    ks = [0, 1, 2, 30, 58, 59, 60, 69]
    for m in [0, 1, 3, 200, 511, 512, 513, 777, 1000, 1023]:
        want = orc.freq_xlating_fir(taps, decim, m * FS / 1024, FS, x, 0, nf).astype(np.complex128)
        e32 = np.abs(ref[m] - want) / (np.abs(want) + 1e-9 * rms)
        assert e32.max() <= 2.0 ** -23, (m, e32.max())
        d = _direct64(taps, decim, m, x, ks[0], ks[-1] + 1)[ks]
        e64 = np.abs(ref[m, ks] - d) / rms[ks]
        assert e64.max() <= 1e-12, (m, e64.max())


def _pfb_streams(decim, nframes, seed):
    # three different seeded wideband streams and a fourth equal to the first
    rng = np.random.default_rng(seed)
    xs = [_wideband(rng, nframes * decim) for _ in range(3)]
    return np.stack(xs + [xs[0]])


# per-frame error over the frame's RMS against pfb_ref64: measured at most 2.5e-6 on one MI355X (both
# decimations, tests below) and under the lane model; 4x headroom
PFB_GATE = 1e-5

# frames per call: one frame, calls shorter than the history (59 frames at D = 1024, 118 at D = 512), calls of
# max_frames (67), odd counts so that (-1)^(m k) at D = 512 changes parity between calls
PFB_CALLS = [1, 7, 67, 3, 33, 67, 1, 5, 67]
PFB_MAX_FRAMES = 67


@pytest.mark.parametrize("decim", [1024, 512])
def test_emul_pfb_streams_match_ref64(decim):
    # nstreams = 3 under the lane model (stream offsets into history, input and output) against the float64
    # reference on every lane of every frame; per-frame error over the frame's RMS, measured at most 2.5e-6
    # (D = 1024) and 1.7e-6 (D = 512), gate PFB_GATE
    import emul_py as emu

    calls = [1, 7, 3, 9, 1, 5]
    taps = orc.firdes_low_pass(1.0, FS, 11e3, 1e3)
    xs = _pfb_streams(decim, sum(calls), 40 + decim)[:3]
    p = emu.Pfb(taps, decim, nstreams=3)
    outs, k = [], 0
    for nf in calls:
        outs.append(p.work(xs[:, k:k + nf * decim]))
        k += nf * decim
    out = np.concatenate(outs, axis=1)
    worst = 0.0
    for s in range(3):
        e = _frame_err(out[s * 1024:(s + 1) * 1024], pfb_ref64(taps, decim, xs[s]))
        worst = max(worst, float(e.max()))
    assert worst < PFB_GATE


def test_host_firdes_matches_oracle():
    import ais_amd

    a = ais_amd.firdes_low_pass(1.0, 250e3, 11e3, 1e3)
    b = orc.firdes_low_pass(1.0, 250e3, 11e3, 1e3)
    assert a.size == b.size == 603
    assert np.max(np.abs(a - b)) < 1e-7


@pytest.mark.gpu
@pytest.mark.parametrize("decim", [1024, 512])
def test_gpu_pfb_matches_freq_xlating_filter(decim):
    import torch

    import ais_amd

    rng = np.random.default_rng(decim + 1)
    taps = ais_amd.firdes_low_pass(1.0, FS, 11e3, 1e3)
    nframes = [64, 3, 40]
    x = _wideband(rng, sum(nframes) * decim)
    p = ais_amd.pfb_channelizer_ccf(1024, taps, decim=decim, max_frames=128)
    outs, k = [], 0
    for nf in nframes:
        outs.append(p.work(torch.as_tensor(x[k:k + nf * decim]).cuda()).cpu().numpy())
        k += nf * decim
    out = np.concatenate(outs, axis=1)
    _check(out, x, taps, decim, [0, 3, 200, 511, 777, 1023], [0, 1, 60, 65, 70, 106])
    with pytest.raises(ValueError):
        ais_amd.pfb_channelizer_ccf(512, taps)


@pytest.mark.gpu
@pytest.mark.parametrize("decim", [1024, 512])
def test_gpu_pfb_streams_match_ref64(decim):
    # four streams (three seeded, the fourth a copy of the first) in strided input rows, into an output whose
    # row stride exceeds the call's frames, called with PFB_CALLS frames (history through both buffers many
    # times); every lane of every frame against the float64 reference, per-frame error over the frame's RMS
    # (measured on one MI355X: 2.46e-6 at D = 1024, 2.50e-6 at D = 512), and the copy's lanes equal to stream 0's
    # bit for bit
    import ctypes as C

    import torch

    import ais_amd
    from ais_amd import _lib

    taps = ais_amd.firdes_low_pass(1.0, FS, 11e3, 1e3)
    total = sum(PFB_CALLS)
    xs = _pfb_streams(decim, total, 90 + decim)
    p = ais_amd.pfb_channelizer_ccf(1024, taps, decim=decim, nstreams=4, max_frames=PFB_MAX_FRAMES)
    ostride = PFB_MAX_FRAMES + 5
    outs, k = [], 0
    for nf in PFB_CALLS:
        n = nf * decim
        ibuf = torch.full((4, n + 7), 3e9, dtype=torch.complex64, device="cuda")
        xin = ibuf[:, 1:n + 1]
        xin.copy_(torch.as_tensor(xs[:, k:k + n]).cuda())
        out = torch.full((4 * 1024, ostride), -3e9, dtype=torch.complex64, device="cuda")
        got = C.c_int(0)
        rc = _lib.lib().aisx_pfb_process(p._h, xin.data_ptr(), xin.stride(0), n, out.data_ptr(), out.stride(0),
                                         C.byref(got), C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0 and got.value == nf
        oh = out.cpu().numpy()
        assert np.all(oh[:, nf:] == np.complex64(-3e9))  # nothing written past the call's frames
        outs.append(oh[:, :nf])
        k += n
    out = np.concatenate(outs, axis=1)
    assert np.array_equal(out[3 * 1024:].view(np.uint64), out[:1024].view(np.uint64))
    worst = 0.0
    for s in range(3):
        e = _frame_err(out[s * 1024:(s + 1) * 1024], pfb_ref64(taps, decim, xs[s]))
        worst = max(worst, float(e.max()))
    print("pfb device vs float64 (D = %d): %.3g" % (decim, worst))
    assert worst < PFB_GATE
