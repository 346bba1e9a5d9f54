#!/usr/bin/env python
"""Robust re-optimisation of the shipped N = 7 controllers ALL AT ONCE on the GPU: the batched L-BFGS state machine on the device
(`noise_model_base.optimize_controllers`) - one gradient launch over all rows and one advance launch per evaluation, nothing
but the status column ever returns to the host.  scripts/robust_lbfgs.py does one row through SciPy.

    python scripts/robust_lbfgs_batched.py [--rows 57] [--sigma 0.05] [--evals 60] [--train 1000] [--pair 0-6] [--risk LAM | --cvar ALPHA]
                                            [--box BMAX TMAX] [--jitter SIGMA_T]

The objective is 1 - mean F (--risk LAM: + LAM std F; --cvar ALPHA: 1 - CVaR_ALPHA F) over `train` shared counter-based draws
(common random numbers); the test figure of a row is 1 - mean F over 10 000 draws of the same stream behind the training draws.
--box BMAX TMAX: the boxed machine with |bias| <= BMAX and 0 <= T <= TMAX (the shipped controllers are box-constrained results: 10
and 30); per row the largest bound violation of the result (which must be 0) and the number of variables that end on a bound are
printed too.  --jitter SIGMA_T: the fidelity of every sample is averaged over a Gaussian readout-time jitter of standard deviation
SIGMA_T (8-point Gauss-Hermite rule; `optimize_controllers(jitter=SIGMA_T)`: one launch of the gradient kernel on the grid of
readout times per evaluation), for the mean and --risk objectives; start, final and test values are then jitter-averaged too.
Prints start / final / test value per row; `run()` returns them for callers (tests)."""
import argparse
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def run(rows=None, sigma=0.05, evals=60, train=1000, pair="0-6", verbose=True, risk=0.0, cvar=None, seed=0x5EED0010, box=None,
        jitter=None, **lbfgs_params):
    if cvar is not None and risk != 0.0:
        raise ValueError("cvar and risk are two objectives: give one of them")
    if cvar is not None and jitter is not None:
        raise ValueError("the CVaR objective has no readout-jitter variant")
    noise = importlib.import_module("code-robchar_amd.noise")
    z = np.load(os.path.join(ROOT, "tests", "golden", "lbfgs_n7.npz"))
    x0 = np.array(z["ctrl_" + pair], dtype=np.float64)
    x0 = x0[: x0.shape[0] if rows is None else int(rows)]
    a, b = (int(v) for v in pair.split("-"))
    nm = noise.structured_perturbation(Nspin=7, inspin=a, outspin=b, noise=sigma)
    objective = ("cvar", cvar) if cvar is not None else ("std", risk) if risk != 0.0 else "mean"

    def moments(x, n_draws, offset):
        if jitter is not None:
            return nm.fidelity_jitter_moments_philox(x, n_draws, seed, jitter, sigma=sigma, offset=offset, shared=True)
        return nm.fidelity_moments_philox(x, n_draws, seed, sigma=sigma, offset=offset, shared=True)

    def value(x, n_draws, offset):
        if cvar is not None:
            return 1.0 - nm.fidelity_cvar_philox(x, n_draws, seed, cvar, sigma=sigma, offset=offset, shared=True)["cvar"]
        mo = moments(x, n_draws, offset)
        return 1.0 - mo["fav"] + risk * mo["std"]
    if box is not None:
        bmax, tmax = (float(v) for v in box)
        lo, hi = np.full(8, -bmax), np.full(8, bmax)
        lo[7], hi[7] = 0.0, tmax
        lbfgs_params["bounds"] = (lo, hi)
        x0 = np.clip(x0, lo, hi)                          # (what the boxed machine starts from: `start` is its value)
    start = value(x0, train, 0)
    if jitter is not None:
        lbfgs_params["jitter"] = float(jitter)
    res = nm.optimize_controllers(x0, train, seed, objective=objective, sigma=sigma, shared=True, max_evals=evals, **lbfgs_params)
    if box is not None:
        res["violation"] = np.maximum(np.maximum(lo - res["x"], res["x"] - hi), 0.0).max(axis=1)
        res["on_bound"] = ((res["x"] == lo) | (res["x"] == hi)).sum(axis=1)
    test_start, test_final = (1.0 - moments(x, 10000, train * 7 * 3)["fav"] for x in (x0, res["x"]))
    if verbose:
        print(f"# objective {objective}{'' if jitter is None else f', readout jitter sigma_t = {jitter}'}, sigma = {sigma}, {train} shared draws, at most {evals} evaluations; test: 1 - mean F over 10 000 draws")
        print("# row      start        final   test start   test final  status iters evals" + ("  violation on_bound" if box else ""))
        for c in range(x0.shape[0]):
            print(f"{c:5d} {start[c]:12.8f} {res['f'][c]:12.8f} {test_start[c]:12.8f} {test_final[c]:12.8f} {res['status'][c]:7d} "
                  f"{res['iters'][c]:5d} {res['evals'][c]:5d}" + (f" {res['violation'][c]:10.3g} {res['on_bound'][c]:8d}" if box else ""))
        print(f"# mean   {start.mean():12.8f} {res['f'].mean():12.8f} {test_start.mean():12.8f} {test_final.mean():12.8f}")
    return {"x0": x0, "start": start, "test_start": test_start, "test_final": test_final, "model": nm, "objective": objective, **res}


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, default=None)
    ap.add_argument("--sigma", type=float, default=0.05)
    ap.add_argument("--evals", type=int, default=60)
    ap.add_argument("--train", type=int, default=1000)
    ap.add_argument("--pair", default="0-6", choices=("0-6", "0-3"))
    goal = ap.add_mutually_exclusive_group()
    goal.add_argument("--risk", type=float, default=0.0)
    goal.add_argument("--cvar", type=float, default=None, metavar="ALPHA")
    ap.add_argument("--box", type=float, nargs=2, default=None, metavar=("BMAX", "TMAX"))
    ap.add_argument("--jitter", type=float, default=None, metavar="SIGMA_T")
    args = ap.parse_args()
    run(args.rows, args.sigma, args.evals, args.train, args.pair, risk=args.risk, cvar=args.cvar, box=args.box, jitter=args.jitter)
