"""The BOXED batched L-BFGS state machine on the device (lbfgs_init_box_kernel / lbfgs_advance_box_kernel behind
`backend.lbfgs_init / lbfgs_advance(bounds=...)`) and `noise_model_base.optimize_controllers(bounds=...)` on top of it: the kernels
against lbfgs.py (the definition) bit for bit, the checks of lbfgs_box_checks through the kernels, the device loop against the same
definition driven from the host by the same gradient entry, the product property on the shipped 0 -> 3 controllers (with a guard:
the unbounded run leaves the box) and the batched script."""
import importlib
import os
import sys

import numpy as np
import pytest

import chain_checks as cc
import lbfgs_box_checks as bc
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
@pytest.mark.parametrize("n, m", [(3, 1), (6, 5), (8, 3), (13, 8)])
def test_kernel_equals_definition(be, n, m, kind):
    """25 calls on host-made rows in per-row boxes: every state field and the trial points after every call, and the result"""
    import torch
    dev = be.compute_device()
    for C in (1, 63, 64, 65, 130):
        case = bc.identity_case(n, m, kind, C)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        bounds = (up(case["lo"]), up(case["hi"]))
        state, trial = be.lbfgs_init(up(case["x0"]), up(case["mask"]), m=m, bounds=bounds)
        assert same(state.cpu().numpy(), case["init"][0]) and same(trial.cpu().numpy(), case["init"][1]), (C, "init")
        for call, (a, b, want_state, want_trial) in enumerate(case["calls"], 1):
            be.lbfgs_advance(state, trial, up(a), up(b) if kind == 2 else None, m=m, kind=KINDS[kind], lam=case["lam"], bounds=bounds,
                             **case["params"])
            got = state.cpu().numpy()
            if not same(got, want_state):
                field = np.nonzero(~((got == want_state) | (np.isnan(got) & np.isnan(want_state))).all(axis=1))[0]
                raise AssertionError(f"C = {C}, call {call}: state fields {field} differ ({lbfgs.field_offsets(n, m)})")
            assert same(trial.cpu().numpy(), want_trial), (C, call, "trial")
        off = lbfgs.field_offsets(n, m)
        res = {k: v.cpu().numpy() for k, v in be.lbfgs_result(state, trial, m=m).items()}
        assert same(res["x"], want_state[off["x"]:off["x"] + n].T) and same(res["grad"], want_state[off["g"]:off["g"] + n].T)
        assert same(res["f"], want_state[off["f"]]) and np.array_equal(res["status"], case["status"])
        if C >= 63:                                                   # the inputs hit bounds, reject and finish in several ways
            assert case["counters"]["on_bound"] > 0 and case["counters"]["rejected"] > 0 and len(set(case["status"])) >= 3


def test_identity_inputs_reset(be):
    """(among the cases above, rows also drop their history once: the one-time reset)"""
    assert sum(bc.identity_case(n, m, kind, 65)["counters"]["reset"] for n, m in ((6, 5), (8, 3), (13, 8)) for kind in (0, 1, 2)) > 0


class DeviceMachine:
    """the boxed device kernels behind the machine interface of lbfgs_box_checks (objective kind raw, state downloaded per call)"""

    def __init__(self, be, x0, mask, lo, hi, **params):
        import torch
        self.be, self.dev, self.torch = be, be.compute_device(), torch
        self.m = params.pop("m", 5)
        self.params = params
        x0 = np.ascontiguousarray(x0, dtype=np.float64)
        self.n = x0.shape[1]
        full = lambda v: torch.from_numpy(np.array(np.broadcast_to(np.asarray(v, dtype=np.float64), x0.shape))).to(self.dev)
        self.bounds = (full(lo), full(hi))
        self.dstate, self.dtrial = be.lbfgs_init(torch.from_numpy(x0).to(self.dev), None if mask is None else full(mask), m=self.m,
                                                 bounds=self.bounds)
        self.refresh()

    def refresh(self):
        arr = self.dstate.cpu().numpy()
        self.arr = arr
        off, n, m = lbfgs.field_offsets(self.n, self.m), self.n, self.m
        self.x, self.g = arr[off["x"]:off["x"] + n].T.copy(), arr[off["g"]:off["g"] + n].T.copy()
        self.f = arr[off["f"]].copy()
        for k in ("count", "head", "nback", "iters", "evals", "status"):
            setattr(self, k, arr[off[k]].astype(np.int64))
        self.trial = self.dtrial.cpu().numpy()

    def state_array(self):
        return self.arr

    def advance(self, ft, gt):
        a = np.concatenate([np.asarray(ft, dtype=np.float64)[:, None], np.asarray(gt, dtype=np.float64)], axis=1)
        self.be.lbfgs_advance(self.dstate, self.dtrial, self.torch.from_numpy(np.ascontiguousarray(a)).to(self.dev), None, m=self.m,
                              kind="raw", bounds=self.bounds, **self.params)
        self.refresh()


@pytest.mark.parametrize("name", bc.ALL_CHECKS)
def test_checks_on_the_device(be, name):
    bc.run_check(name, lambda x0, mask=None, lo=None, hi=None, **params: DeviceMachine(be, x0, mask, lo, hi, **params))


# ---- the device loop of optimize_controllers(bounds=...) ------------------------------------------------------------------------------
def host_driven(be, nm, x0, K, seed, objective, sigma, shared, evals, lo, hi, **params):
    """the boxed `lbfgs.py` driven from the host by the same gradient entry: one upload and one download per evaluation"""
    import torch
    dev = be.compute_device()
    diag, off, _, _ = nm._static_terms()
    mc = lbfgs.LBFGS(**params).init(x0, None, lo, hi)
    values = []
    for _ in range(evals):
        trial = torch.from_numpy(mc.trial.copy()).to(dev)
        want = ("mean",) if objective == "mean" else ("mean", "moment")
        res = be.mc_fidelity_grad_philox(trial, K, nm.Nspin, nm.inspin, nm.outspin, seed, sigma=sigma, shared=shared, h0_diag=diag,
                                         h0_offdiag=off, want=want)
        a = res["mean"].cpu().numpy()
        b = res["moment"].cpu().numpy() if "moment" in res else None
        mc.advance(*lbfgs.objective("one_minus" if b is None else "one_minus_plus_std", a, b, 0.0 if b is None else objective[1]))
        values.append((mc.f.copy(), mc.x.copy(), mc.trial.copy(), mc.status.copy()))
    return mc, values


@pytest.mark.parametrize("shared", (True, False), ids=("shared", "per_controller"))
@pytest.mark.parametrize("N, C, objective", [(5, 130, "mean"), (5, 130, ("std", 1.0)), (10, 65, "mean")],
                         ids=lambda v: str(v).replace(" ", ""))
def test_device_loop_equals_host_driven_loop(be, noise, N, C, objective, shared):
    """K = 64, 12 evaluations at sigma = 0.05 in the box [-0.35, 0.35]^N x [T0 - 1, T0 + 0.5] around the delocalised rows (biases
    U(-0.5, 0.5): three in ten start outside and are projected onto a bound)"""
    nm = noise.structured_perturbation(Nspin=N, inspin=0, outspin=N - 1, noise=0.05)
    x0 = cc.deloc_ctrl(np.random.default_rng(N), C, N, 0.5)
    lo, hi = np.full((C, N + 1), -0.35), np.full((C, N + 1), 0.35)
    lo[:, N], hi[:, N] = x0[:, N] - 1.0, x0[:, N] + 0.5
    got = nm.optimize_controllers(x0, 64, 77, objective=objective, shared=shared, max_evals=12, poll=8, m=5, bounds=(lo, hi))
    mc, _ = host_driven(be, nm, x0, 64, 77, objective, 0.05, shared, 12, lo, hi, m=5)
    assert same(got["x"], mc.x) and same(got["f"], mc.f) and np.array_equal(got["status"], mc.status)
    assert np.array_equal(got["iters"], mc.iters) and np.array_equal(got["evals"], mc.evals) and same(got["grad"], mc.g)
    assert (mc.iters >= 1).any() and (got["x"] >= lo).all() and (got["x"] <= hi).all()
    assert ((got["x"] == lo) | (got["x"] == hi)).any() and (x0 < lo).any()


def n7_box():
    lo, hi = np.full(8, -10.0), np.full(8, 10.0)
    lo[7], hi[7] = 0.0, 30.0
    return lo, hi


def violation(x, lo, hi):
    return np.maximum(np.maximum(lo - x, x - hi), 0.0).max(axis=1)


def test_product_property_with_guard(be, noise, lbfgs_n7):
    """the first 16 shipped 0 -> 3 controllers of N = 7, K = 64 shared draws, sigma = 0.05, 30 evaluations, box [-10, 10]^7 x
    [0, 30]: the boxed run keeps every row inside the box (violation exactly 0) and no row's value is above its start; the guard:
    the UNBOUNDED run from the same rows leaves the box by more than 1e-3 on at least 8 rows (CPU reference: 13 of 16, worst
    68.8; 14 of the 16 rows start on a bound; all 16 improved in the boxed run)"""
    x0 = np.array(lbfgs_n7["ctrl_0-3"][:16], dtype=np.float64)
    lo, hi = n7_box()
    assert violation(x0, lo, hi).max() == 0.0
    print("rows that start on a bound:", int(((x0 == lo) | (x0 == hi)).any(axis=1).sum()))
    nm = noise.structured_perturbation(Nspin=7, inspin=0, outspin=3, noise=0.05)
    start = nm.optimize_controllers(x0, 64, 0x5EED0010, objective="mean", sigma=0.05, shared=True, max_evals=1, bounds=(lo, hi))["f"]
    boxed = nm.optimize_controllers(x0, 64, 0x5EED0010, objective="mean", sigma=0.05, shared=True, max_evals=30, bounds=(lo, hi))
    free = nm.optimize_controllers(x0, 64, 0x5EED0010, objective="mean", sigma=0.05, shared=True, max_evals=30)
    vb, vf = violation(boxed["x"], lo, hi), violation(free["x"], lo, hi)
    print("boxed: violation", vb.max(), "improved rows", int((boxed["f"] < start).sum()), "mean", start.mean(), "->", boxed["f"].mean())
    print("unbounded: rows outside by > 1e-3:", int((vf > 1e-3).sum()), "worst", vf.max(), "mean ->", free["f"].mean())
    assert (vb == 0.0).all(), vb
    assert (boxed["f"] <= start).all(), (boxed["f"], start)
    assert (vf > 1e-3).sum() >= 8, vf


def test_batched_script_with_a_box(be):
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        script = importlib.import_module("robust_lbfgs_batched")
    finally:
        sys.path.pop(0)
    out = script.run(rows=8, evals=12, train=64, pair="0-3", box=(10, 30), verbose=True)
    assert out["x"].shape == (8, 8) and (out["violation"] == 0.0).all(), out["violation"]
    assert (out["on_bound"] >= 0).all() and out["on_bound"].sum() > 0 and (out["f"] <= out["start"]).all()
