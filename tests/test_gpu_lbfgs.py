"""The batched L-BFGS state machine on the device (lbfgs_init_kernel / lbfgs_advance_kernel behind `backend.lbfgs_init`,
`lbfgs_advance`, `lbfgs_result`) and `noise_model_base.optimize_controllers` on top of it: the kernels against lbfgs.py (the
definition) bit for bit, the device loop against the same definition driven from the host by the same gradient entry, the
properties the line search guarantees, the known answer of the 3-chain and the batched script."""
import importlib
import os
import sys

import numpy as np
import pytest

import chain_checks as cc
import lbfgs_checks as lc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
lbfgs = lc.lbfgs
KINDS = ("raw", "one_minus", "one_minus_plus_std")


@pytest.fixture(scope="module")
def noise():
    return importlib.import_module("code-robchar_amd.noise")


def same(got, want):
    return np.array_equal(got, want, equal_nan=True)                 # (a NaN is a NaN: sign and payload are not defined)


@pytest.mark.parametrize("kind", (0, 1, 2), ids=KINDS)
@pytest.mark.parametrize("n, m", [(3, 1), (8, 5), (13, 8), (3, 8), (13, 1), (8, 8), (3, 5), (13, 5), (8, 1)])
def test_kernel_equals_definition(be, n, m, kind):
    """25 calls on host-made rows: every state field and the trial points after every call, and the result entry at the end"""
    import torch
    dev = be.compute_device()
    for C in (1, 63, 64, 65, 130):
        case = lc.identity_case(n, m, kind, C)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        state, trial = be.lbfgs_init(up(case["x0"]), up(case["mask"]), m=m)
        assert same(state.cpu().numpy(), case["init"][0]) and same(trial.cpu().numpy(), case["init"][1]), (C, "init")
        for call, (a, b, want_state, want_trial) in enumerate(case["calls"], 1):
            be.lbfgs_advance(state, trial, up(a), up(b) if kind == 2 else None, m=m, kind=KINDS[kind], lam=case["lam"], **case["params"])
            got = state.cpu().numpy()
            if not same(got, want_state):
                field = np.nonzero(~((got == want_state) | (np.isnan(got) & np.isnan(want_state))).all(axis=1))[0]
                raise AssertionError(f"C = {C}, call {call}: state fields {field} differ ({lbfgs.field_offsets(n, m)})")
            assert same(trial.cpu().numpy(), want_trial), (C, call, "trial")
        off = lbfgs.field_offsets(n, m)
        res = {k: v.cpu().numpy() for k, v in be.lbfgs_result(state, trial, m=m).items()}
        assert same(res["x"], want_state[off["x"]:off["x"] + n].T) and same(res["grad"], want_state[off["g"]:off["g"] + n].T)
        assert same(res["f"], want_state[off["f"]]) and np.array_equal(res["status"], case["status"])
        assert np.array_equal(res["iters"], want_state[off["iters"]]) and np.array_equal(res["evals"], want_state[off["evals"]])
        assert res["status"].dtype == np.int32 and len(set(case["status"])) >= min(3, C)
        only = be.lbfgs_result(state, trial, m=m, want=("f",))
        assert list(only) == ["f"] and same(only["f"].cpu().numpy(), res["f"])
        if C == 65 and kind == 1:                                     # no mask given: all free
            s2, t2 = be.lbfgs_init(up(case["x0"]), None, m=m)
            assert (s2.cpu().numpy()[off["mask"]:] == 1.0).all() and same(t2.cpu().numpy(), case["init"][1])


class DeviceMachine:
    """the device kernels behind the machine interface of lbfgs_checks (objective kind raw, state downloaded after every call)"""

    def __init__(self, be, x0, mask, **params):
        import torch
        self.be, self.dev, self.torch = be, be.compute_device(), torch
        self.m = params.pop("m", 5)
        self.params = params
        x0 = np.ascontiguousarray(x0, dtype=np.float64)
        self.n = x0.shape[1]
        mask = None if mask is None else torch.from_numpy(np.array(np.broadcast_to(mask, x0.shape), dtype=np.float64)).to(self.dev)
        self.dstate, self.dtrial = be.lbfgs_init(torch.from_numpy(x0).to(self.dev), mask, m=self.m)
        self.refresh()

    def refresh(self):
        arr = self.dstate.cpu().numpy()
        self.arr = arr
        off, n, m = lbfgs.field_offsets(self.n, self.m), self.n, self.m
        self.x, self.g = arr[off["x"]:off["x"] + n].T.copy(), arr[off["g"]:off["g"] + n].T.copy()
        self.f, self.sy = arr[off["f"]].copy(), arr[off["sy"]:off["sy"] + m].T.copy()
        for k in ("count", "head", "nback", "iters", "evals", "status"):
            setattr(self, k, arr[off[k]].astype(np.int64))
        self.trial = self.dtrial.cpu().numpy()

    def state_array(self):
        return self.arr

    def advance(self, ft, gt):
        a = np.concatenate([np.asarray(ft, dtype=np.float64)[:, None], np.asarray(gt, dtype=np.float64)], axis=1)
        self.be.lbfgs_advance(self.dstate, self.dtrial, self.torch.from_numpy(np.ascontiguousarray(a)).to(self.dev), None, m=self.m,
                              kind="raw", **self.params)
        self.refresh()


@pytest.mark.parametrize("name", lc.ALL_CHECKS)
def test_checks_on_the_device(be, name):
    lc.run_check(name, lambda x0, mask=None, **params: DeviceMachine(be, x0, mask, **params))


def test_known_answer_host_objective(be):
    lc.check_known_answer(lambda x0, mask=None, **params: DeviceMachine(be, x0, mask, **params))


# ---- the device loop of optimize_controllers -----------------------------------------------------------------------------------------
def host_driven(be, nm, x0, K, seed, objective, sigma, shared, evals, **params):
    """`lbfgs.py` driven from the host by the same gradient entries: one upload and one download per evaluation"""
    import torch
    dev = be.compute_device()
    diag, off, _, _ = nm._static_terms()
    N = nm.Nspin
    mc = lbfgs.LBFGS(**params).init(x0, None)
    values = []
    for _ in range(evals):
        trial = torch.from_numpy(mc.trial.copy()).to(dev)
        if objective == "mean" or objective[0] == "std":
            want = ("mean",) if objective == "mean" else ("mean", "moment")
            res = be.mc_fidelity_grad_philox(trial, K, N, nm.inspin, nm.outspin, seed, sigma=sigma, shared=shared, h0_diag=diag,
                                             h0_offdiag=off, want=want)
            a = res["mean"].cpu().numpy()
            b = res["moment"].cpu().numpy() if "moment" in res else None
            ft, gt = lbfgs.objective("one_minus" if b is None else "one_minus_plus_std", a, b, 0.0 if b is None else objective[1])
        else:
            total, _ = nm._cvar_device(trial, K, seed, objective[1], sigma, 0, shared, diag, off)
            ft, gt = lbfgs.objective("one_minus", total.cpu().numpy())
        mc.advance(ft, gt)
        values.append((mc.f.copy(), mc.accepted.copy(), mc.status.copy(), mc.trial.copy()))
    return mc, values


LOOP_CASES = [(5, 130, 128, "mean"), (5, 130, 128, ("std", 1.0)), (5, 130, 128, ("cvar", 0.25)), (10, 65, 64, "mean"),
              (10, 65, 64, ("std", 1.0))]


@pytest.mark.parametrize("shared", (True, False), ids=("shared", "per_controller"))
@pytest.mark.parametrize("N, C, K, objective", LOOP_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_device_loop_equals_host_driven_loop(be, noise, N, C, K, objective, shared):
    """15 evaluations at sigma = 0.05.  A row's `mean` depends on its own controller row only (a tile belongs to one controller,
    the row mean has a fixed order), so the two loops see the same bits."""
    nm = noise.structured_perturbation(Nspin=N, inspin=0, outspin=N - 1, noise=0.05)
    x0 = cc.deloc_ctrl(np.random.default_rng(N), C, N, 0.5)
    got = nm.optimize_controllers(x0, K, 77, objective=objective, shared=shared, max_evals=15, poll=8, m=5)
    mc, _ = host_driven(be, nm, x0, K, 77, objective, 0.05, shared, 15, m=5)
    assert same(got["x"], mc.x) and same(got["f"], mc.f) and np.array_equal(got["status"], mc.status)
    assert np.array_equal(got["iters"], mc.iters) and np.array_equal(got["evals"], mc.evals) and same(got["grad"], mc.g)
    assert (mc.iters >= 1).any()


def test_guaranteed_properties(be, noise):
    """on the delocalised N = 5 rows of highfid.npz: every accepted value is at most its predecessor, every row that starts with
    |g|_inf > 1e-3 ends strictly below its start, a done row's trial row is NaN, and no tile left the gradient kernel's fast path"""
    from conftest import highfid_workload
    N, a, b, x0, _ = highfid_workload(2)
    nm = noise.structured_perturbation(Nspin=N, inspin=a, outspin=b, noise=0.05)
    be.grad_general_tiles(reset=True)
    mc, values = host_driven(be, nm, x0, 256, 5, "mean", 0.05, True, 30, m=5, gtol=1e-4)
    f = None
    first = None
    for fv, acc, status, trial in values:
        if f is None:
            first = fv.copy()
        else:
            assert (fv[acc] <= f[acc]).all()
            assert same(fv[~acc], f[~acc])
        f = fv
        assert np.isnan(trial[status != 0]).all() and not np.isnan(trial[status == 0]).any()
    got = nm.optimize_controllers(x0, 256, 5, objective="mean", shared=True, max_evals=30, m=5, gtol=1e-4)
    assert same(got["f"], mc.f) and np.array_equal(got["status"], mc.status)
    g0 = np.abs(nm.fidelity_moments_philox(x0, 256, 5, shared=True)["grad_fav"]).max(axis=1)
    assert (g0 > 1e-3).sum() >= 50
    assert (got["f"][g0 > 1e-3] < first[g0 > 1e-3]).all()
    assert be.grad_general_tiles() == 0


def test_known_answer_through_optimize_controllers(be, noise):
    """N = 3, 0 -> 2, sigma = 0, K = 1: every row reaches 1 - F <= 1e-10 with status 1 within 12 evaluations at gtol = 1e-7"""
    nm = noise.structured_perturbation(Nspin=3, inspin=0, outspin=2, noise=0.0)
    got = nm.optimize_controllers(lc.known_answer_start(), 1, 1, objective="mean", sigma=0.0, max_evals=12, poll=4, gtol=1e-7)
    print("evals", got["evals"], "max 1 - F", got["f"].max())
    assert (got["status"] == 1).all(), got["status"]
    assert (got["evals"] <= 12).all() and (got["f"] <= 1e-10).all(), (got["evals"], got["f"])


def test_batched_script(be):
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        script = importlib.import_module("robust_lbfgs_batched")
    finally:
        sys.path.pop(0)
    out = script.run(rows=8, evals=20, verbose=True)
    assert out["x"].shape == (8, 8) and (out["evals"] <= 20).all() and (out["iters"] >= 1).all()
    assert (out["f"][out["iters"] >= 1] < out["start"][out["iters"] >= 1]).all() and (out["f"] <= out["start"]).all()
    assert out["test_final"].mean() < out["test_start"].mean()        # (other draws than the objective's: the set, not every row)
