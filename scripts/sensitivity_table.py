#!/usr/bin/env python
"""Differential sensitivity of the shipped N = 7 L-BFGS controllers to the structured noise, next to their RIM: per controller
and sigma level the RIM_1 (mean infidelity), its slope along the RIM(sigma) curve d(1 - F)/d ln(sigma) - read from the SAME
samples, no second Monte-Carlo run - and the structured direction the mean fidelity is most sensitive to; first the nominal
(sigma = 0) sensitivity.  One `noise_sensitivity` launch per sigma level.

    python scripts/sensitivity_table.py [--pair 0-6] [--rows 8] [--draws 10000]"""
import argparse
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SIGMAS = (0.01, 0.02, 0.05, 0.1)          # from the paper's noise grid np.linspace(0, 0.1, 11); sigma = 0 is the nominal table
KIND = ("site energy", "real coupling", "imag coupling")


def direction_name(i, c):
    return f"{KIND[c]} {i}" if c == 0 else f"{KIND[c]} {i - 1}-{i}"


def run(pair="0-6", rows=8, draws=10000, seed=1, sigmas=SIGMAS):
    noise = importlib.import_module("code-robchar_amd.noise")
    z = np.load(os.path.join(ROOT, "tests", "golden", "lbfgs_n7.npz"), allow_pickle=False)
    ctrl = np.ascontiguousarray(z["ctrl_" + pair][:rows])
    a, b = (int(t) for t in pair.split("-"))
    N = 7
    nm = noise.structured_perturbation(Nspin=N, inspin=a, outspin=b, noise=sigmas[0])
    unit = np.random.default_rng(seed).standard_normal((1, draws, N, 3))       # one z for every level: g = sigma z
    out = {"nominal": nm.nominal_sensitivity(ctrl), "levels": {}}
    for sigma in sigmas:
        out["levels"][sigma] = nm.noise_sensitivity(ctrl, sigma * unit)
    return ctrl, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pair", default="0-6", choices=("0-6", "0-3"))
    ap.add_argument("--rows", type=int, default=8)
    ap.add_argument("--draws", type=int, default=10000)
    args = ap.parse_args()
    ctrl, out = run(args.pair, args.rows, args.draws)
    nom = out["nominal"]
    print(f"# shipped N = 7 L-BFGS controllers, transfer {args.pair}, {args.draws} draws per level")
    print("# nominal (sigma = 0): largest |dF/d direction|")
    for c in range(ctrl.shape[0]):
        i, k = np.unravel_index(np.abs(nom[c]).argmax(), nom[c].shape)
        print(f"ctrl {c:2d}  T = {abs(ctrl[c, -1]):6.2f}   {nom[c, i, k]:+.3e}  ({direction_name(i, k)})")
    for sigma, res in out["levels"].items():
        print(f"# sigma = {sigma}:  RIM_1 = 1 - mean F | d RIM_1 / d ln(sigma) | most sensitive direction (mean dF/dg)")
        for c in range(ctrl.shape[0]):
            d = res["direction"][c]
            i, k = np.unravel_index(np.abs(d).argmax(), d.shape)
            print(f"ctrl {c:2d}  {1.0 - res['fav'][c]:.6f} | {-res['dfav_dlogsigma'][c]:+.6f} | {d[i, k]:+.3e}  ({direction_name(i, k)})")


if __name__ == "__main__":
    main()
