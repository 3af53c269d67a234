"""-m gpu: the plain lock-step pair loop of the timing recovery in straight-line trips (k_msk.h: msk_run_trips), on the
device: the hand-scheduled build (aisx_msk_set_pair_core mode 1, trips of MSK_TRIP pairs) against the compiler-scheduled one
(mode 0, trips of MSK_TRIP_CXX) on twin handles fed identically, the scheme and the shapes of tests/test_gpu_msk_pair_core.py
(9 channels: a full wave and a ragged one with a single live channel, or 70; calls of 4133, 64, 1, 2309 and 600 items) --
symbols, whole bit rows, produced counts and the status word as bit patterns, call by call, the last call of a stream being
the "one further call" that shows the carried state; the sps 4 cases are also held to oracle_py.MskStream.

set_max_noutput_items(q) gives runs of q - 1 pairs: q here takes the lengths that file leaves out, so that between the two
every run length 1 .. 16, that is every remainder of every trip length, is executed on the device."""
import numpy as np
import pytest

import test_gpu_msk_pair_core as pc
from test_gpu_msk_pair_core import LENS, TOTAL, ais  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

_TWIN = {}


def _twin(ais, key, xs, **kw):
    """the mode 0 run of a configuration, computed once"""
    if key not in _TWIN:
        _TWIN[key] = pc._run(ais, xs, [0] * len(LENS), **kw)
    return _TWIN[key]


@pytest.mark.parametrize("q", [6, 7, 9, 10, 11, 12, 13, 14, 15, 16, 17, 0])
def test_run_lengths(ais, q):
    xs = pc._signal(9)
    got = pc._run(ais, xs, [1] * len(LENS), q=q)
    nsym = pc._same(got, _twin(ais, ("q", q), xs, q=q))
    assert got[-1][3] == 0 and nsym > 9 * TOTAL / 4 * 0.95
    pc._oracle(got, xs, 4.0, 0.04, 0.01, q, None, range(9))


@pytest.mark.parametrize("q", [0, 7])  # (7: runs of 6 pairs, a multiple of no trip length above 2)
def test_tags(ais, q):
    xs = pc._signal(70)
    tags = pc._tag_cases(70, ais.TAG_DTYPE)
    got = pc._run(ais, xs, [1] * len(LENS), q=q, tags=tags)
    pc._same(got, _twin(ais, ("tags", q), xs, q=q, tags=tags))
    assert got[-1][3] == 0
    pc._oracle(got, xs, 4.0, 0.04, 0.01, q, tags, range(0, 70, 3))


@pytest.mark.parametrize("sps", [3.0, 5.2083])
def test_loop_parameters(ais, sps):
    # (0.2, 0.05): the error clip at 3 and the omega clip at `limit` both engage
    xs = pc._signal(9)
    kw = dict(sps=sps, gain=0.2, limit=0.05)
    got = pc._run(ais, xs, [1] * len(LENS), **kw)
    nsym = pc._same(got, _twin(ais, ("par", sps), xs, **kw))
    assert nsym > 9 * TOTAL / sps * 0.9
