#!/usr/bin/env python
"""Robust re-optimisation of a shipped controller on the GPU: L-BFGS-B on 1 - fidelity_ss_av over the training set of
`randHset_constructor`, value AND analytic gradient from one kernel launch per evaluation
(`noise_model_base.fidelity_ss_av_grad`) - what the reference's qnewton.py does on the CPU with its block-expm gradient.

    python scripts/robust_lbfgs.py [--row 0] [--sigma 0.05] [--maxiter 30] [--train 1000] [--draws set|philox] [--risk 0.0 | --cvar ALPHA]

--draws philox: no training set is materialised - the gradient kernel generates `train` counter-based draws per evaluation itself
(`noise_model_base.fidelity_moments_philox`, shared draws at a fixed seed and offset: common random numbers, so the objective is
a deterministic smooth function of the controller, as L-BFGS-B needs) and the objective is the risk-averse
1 - mean F + risk * std F, value and gradient still from one launch.  The test figure then comes from 10 000 draws of the same
stream behind the training draws.
--cvar ALPHA (with --draws philox; exclusive with --risk): the tail objective 1 - CVaR_ALPHA F - one minus the mean of the worst
ALPHA * train draws - from `noise_model_base.fidelity_cvar_philox` (a fidelity launch over all draws, the selection on the
device, a gradient launch over the selected draws only), same shared draws.  Piecewise smooth: the gradient is exact wherever
the tail set is locally constant.

Prints value, gradient norm and launches per iteration; `run()` returns the trace for callers (tests)."""
import argparse
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def run(row=0, sigma=0.05, maxiter=30, train=1000, pair="0-6", verbose=True, draws="set", risk=0.0, seed=0x5EED0010, cvar=None):
    from scipy.optimize import minimize
    if draws not in ("set", "philox"):
        raise ValueError("draws must be 'set' or 'philox'")
    if draws == "set" and risk != 0.0:
        raise ValueError("a risk term needs the moment sums of the kernel that generates its draws: draws='philox'")
    if cvar is not None and risk != 0.0:
        raise ValueError("cvar and risk are two objectives: give one of them")
    if cvar is not None and draws != "philox":
        raise ValueError("the CVaR objective needs the kernels that generate their draws: draws='philox'")
    if cvar is not None and not (0.0 < cvar <= 1.0):
        raise ValueError("cvar: alpha in (0, 1]")
    noise = importlib.import_module("code-robchar_amd.noise")
    z = np.load(os.path.join(ROOT, "tests", "golden", "lbfgs_n7.npz"))
    x0 = np.array(z["ctrl_" + pair][row], dtype=np.float64)
    a, b = (int(v) for v in pair.split("-"))
    nm = noise.structured_perturbation(Nspin=7, inspin=a, outspin=b, noise=sigma)
    philox = draws == "philox"
    train_set, test_set = (None, None) if philox else nm.randHset_constructor(train_size=train, test_size=10000)

    def risk_objective(x, n_draws, offset):
        """(1 - fav + risk std, its gradient, fav, std) over `n_draws` shared draws of stream `seed` from element `offset` on"""
        if cvar is not None:                        # (1 - CVaR, its gradient, CVaR, value at risk)
            t = nm.fidelity_cvar_philox(np.asarray(x, dtype=np.float64)[None], n_draws, seed, cvar, sigma=sigma, offset=offset, shared=True)
            return 1.0 - float(t["cvar"][0]), -t["grad_cvar"][0], float(t["cvar"][0]), float(t["var"][0])
        m = nm.fidelity_moments_philox(np.asarray(x, dtype=np.float64)[None], n_draws, seed, sigma=sigma, offset=offset, shared=True)
        return (1.0 - float(m["fav"][0]) + risk * float(m["std"][0]), -m["grad_fav"][0] + risk * m["grad_std"][0],
                float(m["fav"][0]), float(m["std"][0]))

    launches = [0]
    trace = []                                      # (objective, |gradient|, launches so far) per accepted iterate

    seen = {}                                       # evaluations so far: the callback looks its iterate up here

    def objective(x):
        key = np.asarray(x, dtype=np.float64).tobytes()
        if key not in seen and philox:
            seen[key] = risk_objective(x, train, 0)[:2]
            launches[0] += 1
        elif key not in seen:
            fav, grad = nm.fidelity_ss_av_grad(np.asarray(x)[None], train_set)
            launches[0] += 1
            seen[key] = (1.0 - float(fav[0]), -grad[0])
        return seen[key]

    def callback(xk):
        val, g = objective(xk)
        trace.append((val, float(np.linalg.norm(g)), launches[0]))
        if verbose:
            print(f"iter {len(trace):3d}  1 - F = {val:.10f}  |grad| = {trace[-1][1]:.3e}  launches = {launches[0]}")

    start = objective(x0)
    if verbose:
        print(f"start     1 - F = {start[0]:.10f}  |grad| = {np.linalg.norm(start[1]):.3e}")
    res = minimize(objective, x0, jac=True, method="L-BFGS-B", callback=callback, options={"maxiter": maxiter})
    final = objective(res.x)
    if philox:                                      # 10 000 draws of the same stream behind the `train` x N x 3 training elements
        test_final, _, test_fav, test_std = risk_objective(res.x, 10000, train * 7 * 3)
    else:
        test_fav, _ = nm.fidelity_ss_av_grad(res.x[None], test_set)
        test_final = 1.0 - float(test_fav[0])
    out = {"x0": x0, "x": res.x, "start": start[0], "final": final[0], "final_grad": final[1], "trace": trace,
           "launches": launches[0], "test_final": test_final, "model": nm, "train_set": train_set}
    if philox:
        out.update(test_fav=test_fav, test_std=test_std, seed=seed, risk=risk, cvar=cvar)       # (cvar: test_fav = CVaR, test_std = VaR)
    if verbose:
        print(f"final     {'1 - CVaR' if cvar is not None else '1 - F + risk std' if philox else '1 - F'} = {final[0]:.10f} (train)  {out['test_final']:.10f} (test)  after {launches[0]} launches, "
              f"{len(trace)} iterations")
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--row", type=int, default=0)
    ap.add_argument("--sigma", type=float, default=0.05)
    ap.add_argument("--maxiter", type=int, default=30)
    ap.add_argument("--train", type=int, default=1000)
    ap.add_argument("--pair", default="0-6", choices=("0-6", "0-3"))
    ap.add_argument("--draws", default="set", choices=("set", "philox"))
    goal = ap.add_mutually_exclusive_group()
    goal.add_argument("--risk", type=float, default=0.0)
    goal.add_argument("--cvar", type=float, default=None, metavar="ALPHA")
    args = ap.parse_args()
    run(args.row, args.sigma, args.maxiter, args.train, args.pair, draws=args.draws, risk=args.risk, cvar=args.cvar)
