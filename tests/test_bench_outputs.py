"""bench.py --dump-outputs on the CPU: the sample of channels is fixed, the files are float32 / float64 and stay under
64 MB at the benchmark's shapes, a row holds only the bits the channel produced, and the same outputs give the same files
whatever order the tags come in.  --full is off unless asked for."""
import os

import numpy as np
import torch

import bench
from ais_amd.blocks import TAG_DTYPE


def _outputs(nchan, cap, ntags, seed):
    g = torch.Generator().manual_seed(seed)
    bits = torch.randint(0, 2, (nchan, cap), generator=g, dtype=torch.uint8)
    prod = torch.randint(cap - 400, cap - 15, (nchan,), generator=g, dtype=torch.int32)
    rng = np.random.default_rng(seed)
    tags = np.zeros(ntags, TAG_DTYPE)
    tags["chan"] = rng.integers(0, nchan, ntags)
    tags["offset"] = rng.integers(0, 1 << 40, ntags)
    tags["key"] = rng.integers(0, 3, ntags)
    tags["value"] = rng.random(ntags)
    return bits, prod, tags


def _load(d):
    return {n[:-4]: np.load(os.path.join(d, n)) for n in sorted(os.listdir(d))}


def test_dump_is_fixed_bounded_and_masked(tmp_path):
    nchan, cap = 4096, 16400  # the default workload: 4096 channels, 65536 / 4 bits each and some room
    bits, prod, tags = _outputs(nchan, cap, 40000, 0)
    bench.dump_outputs(str(tmp_path / "a"), nchan, tags, bits=bits, produced=prod)
    bench.dump_outputs(str(tmp_path / "b"), nchan, tags[np.random.default_rng(1).permutation(len(tags))], bits=bits, produced=prod)
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert sorted(a) == ["bits", "channels", "produced", "tags"]
    for k in a:
        assert a[k].dtype in (np.float32, np.float64) and np.array_equal(a[k], b[k]), k
    assert sum(os.path.getsize(tmp_path / "a" / (k + ".npy")) for k in a) < 64 << 20
    ch = a["channels"].astype(np.int64)
    assert 1 < len(ch) < nchan and np.all(np.diff(ch) > 0)
    assert np.array_equal(a["produced"], prod.numpy())
    for i, c in enumerate(ch):
        p = int(prod[c])
        assert np.array_equal(a["bits"][i, :p], bits[c, :p].numpy()) and np.all(a["bits"][i, p:] == -1)
    t = a["tags"]
    assert set(t[:, 0].astype(np.int64)) <= set(ch)
    assert len(t) == int(np.isin(tags["chan"], ch).sum())
    assert np.all(np.diff(t[:, 0]) >= 0)


def test_dump_of_the_correlator_chain(tmp_path):
    y = torch.randn(100, 65536, generator=torch.Generator().manual_seed(2), dtype=torch.complex64)
    bench.dump_outputs(str(tmp_path), 100, np.zeros(0, TAG_DTYPE), y=y)
    d = _load(tmp_path)
    ch = d["channels"].astype(np.int64)
    assert d["y"].dtype == np.float32 and d["y"].shape == (len(ch), 65536, 2) and d["y"].nbytes <= bench.DUMP_ROWS_BYTES
    assert np.array_equal(d["y"][..., 0] + 1j * d["y"][..., 1], y[torch.as_tensor(ch)].numpy())
    assert d["tags"].shape == (0, 4)


def test_plain_run_is_the_default():
    a = bench.parse_args(["--steps", "7"])
    assert a.steps == 7 and not a.full and a.dump_outputs is None
    assert bench.parse_args(["--full", "--dump-outputs", "x"]).full
