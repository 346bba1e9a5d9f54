"""`bench.py --dump-outputs` on the host: which arrays `dump_outputs` writes, in which dtype, and the fixed sample it takes of
a fidelity slab above its size bound.  No GPU: the outputs of a step are handed over as CPU tensors.  (The GPU run itself:
tests/test_gpu_bench.py::test_bench_plain_run_and_dump_outputs.)"""
import importlib
import os

import numpy as np
import pytest
import torch


@pytest.fixture
def bench(monkeypatch):
    # bench.py sets HSA_ENABLE_IPC_MODE_LEGACY at import, for its own GPU processes: set here first, undone after the test
    monkeypatch.setenv("HSA_ENABLE_IPC_MODE_LEGACY", os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    return importlib.import_module("bench")


@pytest.fixture
def be():
    return importlib.import_module("code-robchar_amd.backend")


def _step_outputs(R, K, group=3):
    """A fidelity slab whose values name their position, and the last step's columns of a group's packed (15, group x R) metric
    table - a non-contiguous view, as `run_pipeline` hands it over."""
    fid = torch.arange(R, dtype=torch.float64)[:, None] * 1e6 + torch.arange(K, dtype=torch.float64)[None, :]
    packed = torch.arange(15 * group * R, dtype=torch.float64).reshape(15, group * R)
    return {"fidelity": fid, "metric_table": packed[:, (group - 1) * R:]}


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_writes_the_step_outputs(tmp_path, bench, be):
    out = _step_outputs(4, 50)
    bench.dump_outputs(str(tmp_path / "d"), out, be)
    got = _load(tmp_path / "d")
    assert sorted(got) == ["fidelity", "min", "q", "rim1", "std"]
    assert all(a.dtype == np.float64 for a in got.values())
    assert np.array_equal(got["fidelity"], out["fidelity"].numpy())
    table = out["metric_table"].numpy()
    assert np.array_equal(got["rim1"], table[0:3]) and np.array_equal(got["std"], table[3:6])
    assert np.array_equal(got["min"], table[6:9]) and np.array_equal(got["q"], table[9:15].reshape(3, 2, 4))


def test_dump_samples_a_large_slab_the_same_way_every_time(tmp_path, bench, be, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_MAX_VALUES", 60)
    R, K = 4, 50
    for run in ("a", "b"):
        bench.dump_outputs(str(tmp_path / run), _step_outputs(R, K), be)
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert sorted(a) == ["fidelity_sample", "min", "q", "rim1", "std"]
    assert all(np.array_equal(a[k], b[k]) for k in a)
    s = a["fidelity_sample"]
    assert s.dtype == np.float64 and s.shape == (R, 60 // R)
    cols = s[0]                                              # the same columns for every controller, in order, no repeats
    assert np.all(np.diff(cols) > 0) and cols[0] >= 0 and cols[-1] < K
    assert np.array_equal(s, np.arange(R)[:, None] * 1e6 + cols[None, :])


def test_dump_bound(bench):
    """The largest slab written whole (or the sample of a larger one) leaves room under the 64 MB the outputs may take for
    the metric arrays (120 bytes per controller)."""
    assert bench.DUMP_MAX_VALUES * 8 <= 48 << 20
