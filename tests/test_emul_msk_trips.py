"""The plain lock-step pair loop of k_msk.h under the CPU lane model at 8 channels per wave, where a run's pairs go in
straight-line trips of MSK_TRIP pairs and the remainder by the bits of the count (msk_run_trips): every run length from 1
to 16, forced by set_max_noutput_items(Q) (a general_work call of Q symbols starts with a run of Q - 1 pairs) and free
(Q = 0: runs of 16 and the short ones before landings), with the symbol of a pair staged while the next pair loads (the
rotated scheme of the hand-scheduled device build and of the lane model) and at the end of its own pair (the device's
compiler-scheduled builds) -- symbols, bits, counts against the oracle bit for bit over calls that carry the state on, and
the model's counters of runs per length say that every length was in fact taken.

The model libraries here are tests/emul's source built with those counters and trips of 8, once per staging scheme
(tests/emul_msk_trips, tests/emul_msk_trips_end)."""
import ctypes as C

import numpy as np
import pytest

import emul_load
import oracle_py as orc
import synth
from emul_load import f32, i32, lng, vp

TAG_DTYPE = np.dtype([("offset", "<u8"), ("value", "<f8"), ("key", "<i4"), ("chan", "<i4")])
LENS = [700, 37, 1, 300]
TOTAL = sum(LENS)
NCHAN = 9  # a full wave of eight channels and a ragged one with a single live channel
PAIRS_MAX = 16
_XS = []


def lib(end_stage):
    name = "emul_msk_trips_end" if end_stage else "emul_msk_trips"
    L = emul_load.load(name, [
        ("emu_msk_create", vp, [f32, f32, f32, i32, i32]),
        ("emu_msk_destroy", None, [vp]),
        ("emu_msk_set_lpw", None, [vp, i32]),
        ("emu_msk_set_time_parallel", None, [vp, i32, i32, i32]),
        ("emu_msk_process_stream", i32, [vp, vp, lng, i32, vp, vp, i32, vp, vp, vp, vp, lng, vp, vp]),
        ("emu_msk_run_stats", C.POINTER(C.c_long), []),
        ("emu_msk_run_stats_reset", None, []),
        ("emu_msk_end_stage", i32, []),
    ], extra_deps=("../../tests/emul_msk_trips/emul_msk_trips.cpp",))
    assert L.emu_msk_end_stage() == end_stage
    return L


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _signal():
    if not _XS:
        _XS.append(np.stack([synth.make_channel(520 + c, TOTAL, "P", 4, amp=1.0, cfo_max=50.0)[0] for c in range(NCHAN)])
                   .astype(np.complex64))
    return _XS[0]


_ORACLE = {}


def _oracle(q):
    """per call and channel (symbols, bits, consumed) of the reference at max_noutput q, computed once"""
    if q not in _ORACLE:
        xs = _signal()
        res = []
        o = [orc.MskStream(4.0, 0.04, 0.01, 1, max_noutput=q) for _ in range(NCHAN)]
        bt = [orc.BitTail() for _ in range(NCHAN)]
        k = 0
        for L in LENS:
            row = []
            for c in range(NCHAN):
                out, _, _, cons = o[c].step(xs[c, k:k + L], np.zeros(0, orc.TAG_DTYPE))
                row.append((out, bt[c].process(out), cons))
            res.append(row)
            k += L
        _ORACLE[q] = res
    return _ORACLE[q]


def _run(q, end_stage):
    """the model over LENS -> the counters of plain runs per length"""
    L_ = lib(end_stage)
    xs = _signal()
    ref = _oracle(q)
    L_.emu_msk_run_stats_reset()
    h = L_.emu_msk_create(4.0, 0.04, 0.01, 1, NCHAN)
    try:
        L_.emu_msk_set_lpw(h, 8)
        L_.emu_msk_set_time_parallel(h, -1, 256, q)
        k = nsym = 0
        for i, n in enumerate(LENS):
            x = np.ascontiguousarray(xs[:, k:k + n])
            cap = n // 2 + 300
            syms = np.zeros((NCHAN, cap), np.complex64)
            bits = np.zeros((NCHAN, cap), np.uint8)
            prod = np.zeros(NCHAN, np.int32)
            cons = np.zeros(NCHAN, np.int32)
            st = L_.emu_msk_process_stream(h, _p(x), n, n, None, None, 0, _p(syms), None, None, _p(bits), cap, _p(prod), _p(cons))
            assert st == 0
            for c in range(NCHAN):
                out, rbits, rcons = ref[i][c]
                p = prod[c]
                assert p == len(out) and cons[c] == rcons, (i, c)
                assert np.array_equal(syms[c, :p].view(np.uint32), out.view(np.uint32)), (i, c)
                assert np.array_equal(bits[c, :p], rbits), (i, c)
                nsym += int(p)
            k += n
        assert nsym > NCHAN * TOTAL / 4 * 0.9
        st = L_.emu_msk_run_stats()
        return [int(st[j]) for j in range(PAIRS_MAX + 1)]
    finally:
        L_.emu_msk_destroy(h)


@pytest.mark.parametrize("end_stage", [0, 1])
@pytest.mark.parametrize("q", list(range(2, 18)) + [0])
def test_emul_msk_trips_every_run_length(q, end_stage):
    runs = _run(q, end_stage)
    assert runs[0] == 0
    if q:
        assert runs[q - 1] > 0, runs                  # the run a general_work call of q symbols starts with
        assert not any(runs[q:]), runs                # and none longer
    else:
        assert runs[PAIRS_MAX] > 0, runs              # free runs
        assert sum(runs[1:PAIRS_MAX]) > 0, runs       # and the short ones before a landing or the end of the call

