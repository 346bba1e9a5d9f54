"""`noise_model_base.optimize_controllers(bounds=...)` around a NumPy stand-in of the device entries (CPU tensors, the boxed
`lbfgs.py` behind `lbfgs_init` / `lbfgs_advance` / `lbfgs_result`, an analytic "gradient launch"), in the pattern of
test_lbfgs_driver_host.py: the bounds are broadcast from a scalar, (N+1,) and (C, N+1), NumPy or torch, handed to init and - the
same two tensors - to every advance, and the results equal a direct run of `lbfgs.py` - runs without a GPU."""
import importlib

import numpy as np
import pytest

import lbfgs_checks as lc

lbfgs = lc.lbfgs


@pytest.fixture
def stand_in(monkeypatch):
    torch = pytest.importorskip("torch")
    be = importlib.import_module("code-robchar_amd.backend")
    noise = importlib.import_module("code-robchar_amd.noise")
    log = {"grad_calls": 0, "machine": None, "init_bounds": None, "advance_bounds": [], "kinds": []}
    rows = lc.sample_rows(6, 9)

    def grad_philox(controllers, n_draws, nspin, inspin, outspin, seed, offset=0, sigma=0.05, shared=False, h0_diag=None,
                    h0_offdiag=None, want=()):
        log["grad_calls"] += 1
        mean, moment = rows(controllers.numpy())
        return {k: torch.from_numpy(v) for k, v in (("mean", mean), ("moment", moment)) if k in want}

    def init(x0, mask=None, m=5, bounds=None):
        assert bounds is not None, "optimize_controllers(bounds=...) started the unbounded machine"
        lo, hi = bounds
        assert tuple(lo.shape) == tuple(hi.shape) == tuple(x0.shape) and lo.dtype == hi.dtype == torch.float64
        assert lo.is_contiguous() and hi.is_contiguous()
        log["init_bounds"] = bounds
        mc = lbfgs.LBFGS(m=m, **log.get("params", {})).init(x0.numpy(), None if mask is None else mask.numpy(), lo.numpy(), hi.numpy())
        log["machine"] = mc
        return torch.from_numpy(mc.state_array()), torch.from_numpy(mc.trial.copy())

    def advance(state, trial, row_a, row_b=None, *, m=5, kind="one_minus", lam=0.0, bounds=None, **params):
        mc = log["machine"]
        assert np.array_equal(trial.numpy(), mc.trial, equal_nan=True) and params == log.get("params", {})
        log["advance_bounds"].append(bounds)
        log["kinds"].append((kind, lam))
        mc.advance(*lbfgs.objective(kind, row_a.numpy(), None if row_b is None else row_b.numpy(), lam))
        state.copy_(torch.from_numpy(mc.state_array()))
        trial.copy_(torch.from_numpy(mc.trial))

    def result(state, trial, *, m=5, want=be.LBFGS_RESULT_OUTPUTS):
        return {k: torch.from_numpy(np.asarray(v)) for k, v in log["machine"].result().items()}

    monkeypatch.setattr(be, "mc_fidelity_grad_philox", grad_philox)
    monkeypatch.setattr(be, "lbfgs_init", init)
    monkeypatch.setattr(be, "lbfgs_advance", advance)
    monkeypatch.setattr(be, "lbfgs_result", result)
    monkeypatch.setattr(be, "compute_device", lambda: torch.device("cpu"))
    nm = noise.structured_perturbation(Nspin=5, inspin=0, outspin=4, noise=0.05)
    return nm, log, rows, torch


def direct(rows, x0, evals, kind, lam, lo, hi, mask=None, **params):
    mc = lbfgs.LBFGS(**params).init(x0, mask, lo, hi)
    for _ in range(evals):
        mean, moment = rows(mc.trial)
        mc.advance(*lbfgs.objective(kind, mean, moment, lam))
    return mc


X0 = 0.5 * np.random.default_rng(0).standard_normal((9, 6))
ROW_LO = np.array([-0.3, -0.2, -np.inf, -0.4, -0.1, 0.0])
ROW_HI = np.array([0.3, np.inf, 0.25, 0.4, 0.1, 0.6])
FULL_LO = np.broadcast_to(ROW_LO, (9, 6)) - 0.05 * np.arange(9)[:, None]
FULL_HI = np.broadcast_to(ROW_HI, (9, 6)) + 0.05 * np.arange(9)[:, None]


def as_given(kind, torch):
    if kind == "scalar":
        return (-0.25, 0.3), (np.full((9, 6), -0.25), np.full((9, 6), 0.3))
    if kind == "row":
        return (ROW_LO, ROW_HI), (np.broadcast_to(ROW_LO, (9, 6)), np.broadcast_to(ROW_HI, (9, 6)))
    if kind == "full":
        return (FULL_LO, FULL_HI), (FULL_LO, FULL_HI)
    if kind == "torch_mixed":                                                   # a torch row and a NumPy scalar
        return (torch.from_numpy(ROW_LO.copy()), np.float64(0.7)), (np.broadcast_to(ROW_LO, (9, 6)), np.full((9, 6), 0.7))
    raise ValueError(kind)


@pytest.mark.parametrize("shape", ("scalar", "row", "full", "torch_mixed"))
def test_bounds_are_broadcast_and_passed_to_every_call(stand_in, shape):
    nm, log, rows, torch = stand_in
    given, (lo, hi) = as_given(shape, torch)
    got = nm.optimize_controllers(X0, 16, 3, max_evals=14, poll=4, bounds=given, m=3)
    n = log["grad_calls"]
    assert 1 <= n <= 14 and len(log["advance_bounds"]) == n
    ilo, ihi = log["init_bounds"]
    assert np.array_equal(ilo.numpy(), lo) and np.array_equal(ihi.numpy(), hi)
    for b in log["advance_bounds"]:                                             # the same two tensors at every call
        assert b is not None and b[0].data_ptr() == ilo.data_ptr() and b[1].data_ptr() == ihi.data_ptr()
    mc = direct(rows, X0, n, "one_minus", 0.0, lo, hi, m=3)
    for k, v in mc.result().items():
        assert np.array_equal(got[k], v, equal_nan=True), k
    assert (got["x"] >= lo).all() and (got["x"] <= hi).all()
    assert ((got["x"] == lo) | (got["x"] == hi)).any() and (got["iters"] >= 1).any()


def test_std_objective_mask_and_bounds(stand_in):
    nm, log, rows, torch = stand_in
    mask = np.ones(6)
    mask[5] = 0.0                                                               # T fixed, and outside the box: it is projected
    got = nm.optimize_controllers(X0, 16, 3, objective=("std", 0.5), mask=mask, max_evals=12, poll=5, bounds=(ROW_LO, ROW_HI))
    assert set(log["kinds"]) == {("one_minus_plus_std", 0.5)}
    want_T = np.clip(X0[:, 5], ROW_LO[5], ROW_HI[5])
    assert np.array_equal(got["x"][:, 5], want_T) and not np.array_equal(want_T, X0[:, 5])
    mc = direct(rows, X0, log["grad_calls"], "one_minus_plus_std", 0.5, ROW_LO, ROW_HI, mask=np.broadcast_to(mask, X0.shape))
    assert np.array_equal(got["x"], mc.x) and np.array_equal(got["f"], mc.f) and np.array_equal(got["status"], mc.status)


def test_no_bounds_is_todays_call(stand_in, monkeypatch):
    """without bounds neither entry sees a `bounds` keyword (the stand-in of test_lbfgs_driver_host.py has none)"""
    nm, log, rows, torch = stand_in
    be = importlib.import_module("code-robchar_amd.backend")
    seen = []

    def init(x0, mask=None, m=5, **kw):
        seen.append(kw)
        mc = lbfgs.LBFGS(m=m).init(x0.numpy(), None)
        log["machine"] = mc
        return torch.from_numpy(mc.state_array()), torch.from_numpy(mc.trial.copy())

    def advance(state, trial, row_a, row_b=None, *, m=5, kind="one_minus", lam=0.0, **kw):
        seen.append(kw)
        mc = log["machine"]
        mc.advance(*lbfgs.objective(kind, row_a.numpy(), None, lam))
        trial.copy_(torch.from_numpy(mc.trial))
    monkeypatch.setattr(be, "lbfgs_init", init)
    monkeypatch.setattr(be, "lbfgs_advance", advance)
    nm.optimize_controllers(X0, 16, 3, max_evals=3)
    assert seen == [{}, {}, {}, {}]
