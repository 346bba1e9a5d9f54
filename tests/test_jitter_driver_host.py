"""`noise_model_base.optimize_controllers(jitter=...)` and `fidelity_jitter_moments_philox` around a NumPy stand-in of the device
entries (CPU tensors, `lbfgs.py` behind the L-BFGS entries, an analytic "gradient launch"): with `jitter` the driver evaluates
through `mc_fidelity_grad_times_philox` and the right grid reaches it, ("cvar", alpha) with jitter raises, and jitter=None calls
the single-time entry as before - runs without a GPU."""
import importlib

import numpy as np
import pytest

import lbfgs_checks as lc

lbfgs = lc.lbfgs
X0 = 0.5 * np.random.default_rng(0).standard_normal((9, 6))


@pytest.fixture
def stand_in(monkeypatch):
    torch = pytest.importorskip("torch")
    be = importlib.import_module("code-robchar_amd.backend")
    noise = importlib.import_module("code-robchar_amd.noise")
    log = {"single": [], "grid": [], "kinds": [], "machine": None}
    rows = lc.sample_rows(6, 9)

    def answer(controllers, want):
        c = controllers.numpy() if hasattr(controllers, "numpy") else np.asarray(controllers)
        mean, moment = rows(c)
        return {k: torch.from_numpy(v) for k, v in (("mean", mean), ("moment", moment)) if k in want}

    def grad_philox(controllers, n_draws, nspin, inspin, outspin, seed, offset=0, sigma=0.05, shared=False, h0_diag=None,
                    h0_offdiag=None, want=()):
        log["single"].append(dict(K=n_draws, seed=seed, shared=shared, want=tuple(want)))
        return answer(controllers, want)

    def grad_times_philox(controllers, n_draws, nspin, inspin, outspin, seed, offset=0, sigma=0.05, shared=False, tscale=None,
                          tshift=None, weights=None, h0_diag=None, h0_offdiag=None, want=()):
        log["grid"].append(dict(K=n_draws, seed=seed, shared=shared, want=tuple(want), tscale=tscale, tshift=tshift, weights=weights,
                                offset=offset, sigma=sigma))
        return answer(controllers, want)

    def init(x0, mask=None, m=5):
        mc = lbfgs.LBFGS(m=m).init(x0.numpy(), None if mask is None else mask.numpy())
        log["machine"] = mc
        return torch.from_numpy(mc.state_array()), torch.from_numpy(mc.trial.copy())

    def advance(state, trial, row_a, row_b=None, *, m=5, kind="one_minus", lam=0.0, **params):
        mc = log["machine"]
        log["kinds"].append((kind, lam))
        mc.advance(*lbfgs.objective(kind, row_a.numpy(), None if row_b is None else row_b.numpy(), lam))
        state.copy_(torch.from_numpy(mc.state_array()))
        trial.copy_(torch.from_numpy(mc.trial))

    def result(state, trial, *, m=5, want=be.LBFGS_RESULT_OUTPUTS):
        return {k: torch.from_numpy(np.asarray(v)) for k, v in log["machine"].result().items()}

    monkeypatch.setattr(be, "mc_fidelity_grad_philox", grad_philox)
    monkeypatch.setattr(be, "mc_fidelity_grad_times_philox", grad_times_philox)
    monkeypatch.setattr(be, "lbfgs_init", init)
    monkeypatch.setattr(be, "lbfgs_advance", advance)
    monkeypatch.setattr(be, "lbfgs_result", result)
    monkeypatch.setattr(be, "compute_device", lambda: torch.device("cpu"))
    nm = noise.structured_perturbation(Nspin=5, inspin=0, outspin=4, noise=0.05)
    return nm, log, noise


def same_grid(call, tscale, tshift, weights):
    eq = lambda a, b: (a is None and b is None) or (a is not None and b is not None and np.array_equal(np.asarray(a), np.asarray(b)))
    return eq(call["tscale"], tscale) and eq(call["tshift"], tshift) and eq(call["weights"], weights)


def test_sigma_t_reaches_the_entry_as_the_gauss_hermite_grid(stand_in):
    nm, log, noise = stand_in
    got = nm.optimize_controllers(X0, 16, 3, max_evals=5, jitter=0.1)
    tshift, weights = noise.readout_jitter_nodes(0.1, 8)
    assert len(log["grid"]) == 5 and not log["single"]
    assert all(same_grid(c, None, tshift, weights) and c["want"] == ("mean",) and c["shared"] and c["K"] == 16 and c["seed"] == 3
               for c in log["grid"])
    assert set(log["kinds"]) == {("one_minus", 0.0)} and got["x"].shape == X0.shape


def test_order_and_the_std_objective(stand_in):
    nm, log, noise = stand_in
    nm.optimize_controllers(X0, 16, 3, objective=("std", 0.5), max_evals=3, jitter=(0.2, 5))
    tshift, weights = noise.readout_jitter_nodes(0.2, 5)
    assert len(log["grid"]) == 3 and not log["single"] and len(weights) == 5
    assert all(same_grid(c, None, tshift, weights) and c["want"] == ("mean", "moment") for c in log["grid"])
    assert set(log["kinds"]) == {("one_minus_plus_std", 0.5)}


def test_an_explicit_grid_is_taken_as_it_is(stand_in):
    nm, log, _ = stand_in
    grid = dict(tscale=np.array([0.9, 1.0, 1.1]), tshift=np.array([0.0, 0.1, -0.1]), weights=np.array([0.25, 0.5, 0.25]))
    nm.optimize_controllers(X0, 16, 3, max_evals=2, jitter=grid)
    assert len(log["grid"]) == 2 and all(same_grid(c, grid["tscale"], grid["tshift"], grid["weights"]) for c in log["grid"])
    with pytest.raises(ValueError, match="weights"):
        nm.optimize_controllers(X0, 16, 3, max_evals=2, jitter=dict(tshift=np.zeros(3)))
    with pytest.raises(ValueError, match="weights"):
        nm.optimize_controllers(X0, 16, 3, max_evals=2, jitter=dict(weights=np.ones(3), nodes=np.zeros(3)))


def test_cvar_with_jitter_raises(stand_in):
    nm, log, _ = stand_in
    with pytest.raises(NotImplementedError, match="jitter"):
        nm.optimize_controllers(X0, 16, 3, objective=("cvar", 0.2), max_evals=2, jitter=0.1)
    assert not log["grid"] and not log["single"]


def test_without_jitter_the_single_time_entry_is_called(stand_in):
    nm, log, _ = stand_in
    nm.optimize_controllers(X0, 16, 3, max_evals=4)
    nm.optimize_controllers(X0, 16, 3, max_evals=4, jitter=None, objective=("std", 1.0))
    assert len(log["single"]) == 8 and not log["grid"]
    assert [c["want"] for c in log["single"]] == [("mean",)] * 4 + [("mean", "moment")] * 4


def test_jitter_moments_are_moments_from_sums_of_one_launch(stand_in):
    nm, log, noise = stand_in
    got = nm.fidelity_jitter_moments_philox(X0, 32, 9, sigma_t=0.15, order=6, offset=11, shared=True)
    assert len(log["grid"]) == 1 and not log["single"]
    call = log["grid"][0]
    tshift, weights = noise.readout_jitter_nodes(0.15, 6)
    assert same_grid(call, None, tshift, weights) and call["want"] == ("mean", "moment") and call["offset"] == 11 and call["shared"]
    assert call["K"] == 32 and call["seed"] == 9 and call["sigma"] == 0.05
    mean, moment = lc.sample_rows(6, 9)(X0)
    want = noise.moments_from_sums(mean, moment)
    assert sorted(got) == sorted(want) == sorted(nm_keys())
    for k in want:
        assert np.array_equal(got[k], want[k], equal_nan=True), k


def nm_keys():
    return ("fav", "grad_fav", "var", "grad_var", "std", "grad_std")
