#!/usr/bin/env python3
"""Which noise source limits a controller: the variance of the fidelity over the structured noise and the first- / total-order
variance indices of groups of noise coordinates (`noise_model_base.noise_variance_indices_philox`, the pick-freeze kernel) for the
first rows of a shipped controller set.

    python scripts/variance_table.py [--rows 2] [--samples 2048] [--sigma 0.05] [--replicates 4] [--pair 0-6]

prints, per row, F mean and Var F and, per group - the three kinds, then the single site energies -, "first / total" with the
standard error over the replicates.  The controllers are the shipped N = 7 L-BFGS rows of tests/golden/lbfgs_n7.npz."""
import argparse
import importlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

noise = importlib.import_module("code-robchar_amd.noise")
vi = importlib.import_module("code-robchar_amd.variance_indices")

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=2)
ap.add_argument("--samples", type=int, default=2048)
ap.add_argument("--sigma", type=float, default=0.05)
ap.add_argument("--replicates", type=int, default=4)
ap.add_argument("--pair", default="0-6", choices=("0-6", "0-3"))
ap.add_argument("--seed", type=int, default=1)
args = ap.parse_args()

N = 7
a, b = (int(v) for v in args.pair.split("-"))
ctrl = np.ascontiguousarray(np.load(os.path.join(ROOT, "tests", "golden", "lbfgs_n7.npz"))[f"ctrl_{args.pair}"][:args.rows])
model = noise.structured_perturbation(Nspin=N, inspin=a, outspin=b, noise=args.sigma)
kinds, kl = vi.kind_groups(N)
masks = np.concatenate([kinds, np.array([1 << vi.coordinate(i, 0) for i in range(N)], dtype=np.uint64)])
labels = ["all site energies", "all real couplings", "all imaginary couplings"] + [f"site energy {i} alone" for i in range(N)]
res = model.noise_variance_indices_philox(ctrl, args.samples, args.seed, groups=masks, sigma=args.sigma, replicates=args.replicates)
R = args.replicates
print(f"# N = {N}, {a} -> {b}, sigma = {args.sigma}, K = {args.samples}, {R} replicate(s); first / total"
      + (" (standard error over the replicates)" if R > 1 else ""))
head = " | ".join(f"row {c} (F = {res['fav'][c]:.3f}, Var {res['var'][c]:.2e})" for c in range(len(ctrl)))
print(f"| group | {head} |")
print("|---|" + "---|" * len(ctrl))
for g, label in enumerate(labels):
    cells = []
    for c in range(len(ctrl)):
        cell = f"{res['first'][c, g]:.3f} / {res['total'][c, g]:.3f}"
        if R > 1:
            cell += f" ({res['first_se'][c, g]:.3f} / {res['total_se'][c, g]:.3f})"
        cells.append(cell)
    print(f"| {label} | " + " | ".join(cells) + " |")
