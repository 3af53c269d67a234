"""The sequence detector's kernel body (gr-ais_amd/csrc/k_mlse.h) on the CPU lane model (tests/emul_mlse: one OS thread
per lane, driven as aisx_mlse.hip drives the device) against the host form (ais_amd.mlse_detector), bit for bit: the
1 000-symbol stream of test_mlse_host.py in every split, ragged multi-channel input over several calls, flush and
reset, a bad count.  And the same comparison once in a stand-alone program built with AddressSanitizer and
UndefinedBehaviorSanitizer (tests/emul_mlse/mlse_san.cpp: nothing of it is loaded into this process).  -m "not gpu"."""
import ctypes as C
import glob
import os
import subprocess

import numpy as np
import pytest

import emul_load
from emul_load import i32, lng, vp
import mlse_cases as mc

HERE = os.path.dirname(os.path.abspath(__file__))
EMUL = os.path.join(HERE, "emul_mlse")
CSRC = os.path.join(os.path.dirname(HERE), "gr-ais_amd", "csrc")


def _stale(target, extra=()):
    deps = glob.glob(os.path.join(CSRC, "*.h")) + [os.path.join(EMUL, "emul_mlse.cpp"), os.path.join(HERE, "emul", "emul.cpp")] + list(extra)
    return not os.path.exists(target) or any(os.path.getmtime(d) > os.path.getmtime(target) for d in deps)


def emu():
    return emul_load.load("emul_mlse", [
        ("emu_mlse_create", vp, [vp, i32, i32]),
        ("emu_mlse_destroy", None, [vp]),
        ("emu_mlse_reset", None, [vp]),
        ("emu_mlse_process", None, [vp, vp, lng, vp, vp, lng, vp]),
        ("emu_mlse_flush", None, [vp, vp, lng, vp]),
        ("emu_mlse_status", None, [vp]),
        ("emu_mlse_plan", i32, [i32, i32, vp]),
    ])


class LaneForm:
    """the kernel body on the CPU lane model, behind the interface of ais_amd.mlse_detector_batch (numpy arrays)"""

    def __init__(self, ais, nchan, max_syms, bt=0.4):
        rot = np.ascontiguousarray(ais.mlse_detector(bt).model()[2])
        self.h = emu().emu_mlse_create(rot.ctypes.data, nchan, max_syms)
        assert self.h
        self.nchan, self.max_syms = nchan, max_syms
        self.bits = np.full((nchan, max_syms + 79), 0x5a, np.uint8)
        self.nbits = np.full(nchan, -7, np.int32)

    def __del__(self):
        emu().emu_mlse_destroy(self.h)

    def process(self, syms, nsyms):
        assert syms.dtype == np.complex64 and syms.flags.c_contiguous and syms.shape[0] == self.nchan and syms.shape[1] >= self.max_syms
        n = np.ascontiguousarray(nsyms, np.int32)
        emu().emu_mlse_process(self.h, syms.ctypes.data, syms.shape[1], n.ctypes.data, self.bits.ctypes.data, self.bits.shape[1],
                               self.nbits.ctypes.data)
        return self.bits, self.nbits

    def flush(self):
        emu().emu_mlse_flush(self.h, self.bits.ctypes.data, self.bits.shape[1], self.nbits.ctypes.data)
        return self.bits, self.nbits

    def reset(self):
        emu().emu_mlse_reset(self.h)

    def status(self):
        return emu().emu_mlse_status(self.h)


@pytest.fixture(scope="module")
def ais():
    import ais_amd

    return ais_amd


def test_lane_model_equals_the_host_form_on_every_split(ais):
    rng = np.random.default_rng(4)
    N = 1000
    s = (rng.normal(size=N) + 1j * rng.normal(size=N)).astype(np.complex64)
    ref = np.concatenate(mc.host_run(ais, [s])).tobytes()
    cuts = sorted(rng.integers(0, N + 1, 16).tolist() + [300, 300, 301, 640])
    edges = [0] + cuts + [N]
    for sizes in ([N], [b - a for a, b in zip(edges[:-1], edges[1:])], [100] * 10):
        lane = LaneForm(ais, 1, N)
        got, o = [], 0
        buf = np.zeros((1, N + 5), np.complex64)
        for n in sizes:
            buf[0, :n] = s[o:o + n]
            bits, nb = lane.process(buf, [n])
            got.append(bits[0, :nb[0]].copy())
            o += n
        bits, nb = lane.flush()
        got.append(bits[0, :nb[0]].copy())
        assert b"".join(g.tobytes() for g in got) == ref, sizes
        assert sum(g.size for g in got[:-1]) == 960 and lane.status() == 0


def test_lane_model_equals_the_host_form_on_ragged_channels(ais):
    """5 channels, counts drawn from the sizes at which a window, a block or a wave's tile begins or ends, four calls,
    flush, reset, one call more; clean symbols in one channel, noise in the others"""
    rng = np.random.default_rng(9)
    nchan, max_syms = 5, 5000
    lane = LaneForm(ais, nchan, max_syms)
    host = [ais.mlse_detector() for _ in range(nchan)]
    buf = np.zeros((nchan, max_syms + 3), np.complex64)
    plan = [[5000, 0, 79, 80, 145], [1, 5000, 1, 64, 15], [143, 16, 5000, 17, 0], [63, 81, 144, 5000, 64]]
    for rnd in range(2):
        for counts in (plan if rnd == 0 else plan[:1]):
            for c, n in enumerate(counts):
                buf[c, :n] = mc.clean_symbols(rng.integers(0, 2, n + 2)) if c == 0 else (rng.normal(size=n) + 1j * rng.normal(size=n))
            bits, nb = lane.process(buf, counts)
            for c, n in enumerate(counts):
                want = host[c].work(buf[c, :n])
                assert nb[c] == want.size and bits[c, :nb[c]].tobytes() == want.tobytes(), (rnd, counts, c)
        bits, nb = lane.flush()
        for c in range(nchan):
            want = host[c].flush()
            assert nb[c] == want.size and bits[c, :nb[c]].tobytes() == want.tobytes(), (rnd, c)
        lane.reset()
    assert lane.status() == 0


def test_lane_model_bad_counts(ais):
    rng = np.random.default_rng(10)
    nchan, max_syms = 3, 200
    lane = LaneForm(ais, nchan, max_syms)
    host = [ais.mlse_detector() for _ in range(nchan)]
    buf = (rng.normal(size=(nchan, max_syms)) + 1j * rng.normal(size=(nchan, max_syms))).astype(np.complex64)
    for counts in ([200, 150, 200], [-1, 200, max_syms + 1], [200, 200, 200]):
        bits, nb = lane.process(buf, counts)
        bad = [n < 0 or n > max_syms for n in counts]
        assert lane.status() == (1 if any(bad) else 0) and lane.status() == 0
        for c, n in enumerate(counts):
            want = host[c].work(buf[c, :0 if bad[c] else n])
            assert nb[c] == want.size and bits[c, :nb[c]].tobytes() == want.tobytes(), (counts, c)
            assert not (bad[c] and nb[c])


def test_stand_alone_program_under_the_sanitizers():
    exe = os.path.join(EMUL, "mlse_san")
    if _stale(exe, [os.path.join(EMUL, "mlse_san.cpp"), os.path.join(CSRC, "aisx_mlse.cpp"), os.path.join(CSRC, "aisx_tx.cpp")]):
        subprocess.check_call(["make", "-C", EMUL, "-s", "-B", "mlse_san"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("mlse_san ok"), (r.returncode, r.stdout[-400:], r.stderr[-2000:])
