"""bench.py --dump-outputs on the CPU: the dump's files, their dtype, the 64 MB bound
and the seeded sample of the batch elements (no GPU, no solve)."""
import os

import numpy as np
import torch

import bench


def _arrays(B, rng):
    return {"xs": torch.from_numpy(rng.standard_normal((B, 5, 7))),
            "us": torch.from_numpy(rng.standard_normal((B, 4, 3))),
            "results": torch.from_numpy(rng.standard_normal((B, 7)))}


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_whole_output_below_the_limit(tmp_path):
    arr = _arrays(6, np.random.default_rng(0))
    bench.dump_outputs(str(tmp_path / "o"), arr)
    got = _load(str(tmp_path / "o"))
    assert sorted(got) == ["elements", "results", "us", "xs"]
    assert all(a.dtype == np.float64 for a in got.values())
    np.testing.assert_array_equal(got["elements"], np.arange(6))
    for k, a in arr.items():
        np.testing.assert_array_equal(got[k], a.numpy())


def test_dump_samples_the_same_elements_within_the_limit(tmp_path):
    B = 301  # odd, and many times what the limit below holds
    arr = _arrays(B, np.random.default_rng(1))
    limit = 40 * 1024
    for name in ("a", "b"):
        bench.dump_outputs(str(tmp_path / name), arr, limit=limit)
    a, b = _load(str(tmp_path / "a")), _load(str(tmp_path / "b"))
    size = sum(os.path.getsize(str(tmp_path / "a" / f)) for f in os.listdir(str(tmp_path / "a")))
    assert size <= limit
    el = a["elements"].astype(int)
    assert 0 < el.size < B and (np.diff(el) > 0).all() and el[0] >= 0 and el[-1] < B
    for k in a:  # two dumps of one output: the same sample, the same numbers
        np.testing.assert_array_equal(a[k], b[k])
    for k, t in arr.items():
        np.testing.assert_array_equal(a[k], t.numpy()[el])


def test_dump_limit_is_64_mb():
    assert bench.DUMP_LIMIT_BYTES <= 64 * 10 ** 6
