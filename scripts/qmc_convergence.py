#!/usr/bin/env python3
"""Standard error of RIM_1 against the number of evaluations K, plain Monte Carlo (the counter-based Philox stream) against
randomised quasi-Monte Carlo (R = 16 scrambled Sobol replicates of K / 16 points): the table a user reads to choose K.  The
delocalised controller sets of the test suite - shipped N = 5 (0 -> 4) and N = 7 (0 -> 6), constructed N = 10 (0 -> 9) -, the first 8
rows of each, sigma = 0.01 / 0.05 / 0.1; per cell the median over the rows of SE_MC, SE_RQMC and their ratio.
SE_MC = std(F) / sqrt(K) from 2^18 Philox draws; SE_RQMC = `noise_model.fidelity_rqmc`'s.

    python scripts/qmc_convergence.py > profiles/qmc_convergence.txt"""
import importlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

be = importlib.import_module("code-robchar_amd.backend")
nm = importlib.import_module("code-robchar_amd.noise")
dev = torch.device("cuda", 0)
R, ROWS = 16, 8

print(f"# median over {ROWS} controllers; R = {R} replicates; SE of the mean fidelity (= SE of RIM_1)")
print("#  N  sigma       K     SE_MC    SE_RQMC   ratio")
GOLDEN = os.path.join(ROOT, "tests", "golden")
highfid, lbfgs_n7 = np.load(os.path.join(GOLDEN, "highfid.npz")), np.load(os.path.join(GOLDEN, "lbfgs_n7.npz"))
SETS = ((5, 0, 4, highfid["c2_ctrl"], None), (7, 0, 6, lbfgs_n7["ctrl_0-6"], None), (10, 0, 9, highfid["c5_ctrl"], highfid["c5_h0_diag"]))
for N, a, b, rows, h0 in SETS:
    ctrl = np.ascontiguousarray(rows[:ROWS], dtype=np.float64)
    model = nm.structured_perturbation(Nspin=N, inspin=a, outspin=b)
    if h0 is not None:
        model.HH = model.HH + np.diag(h0)
    diag, off, _, _ = model._static_terms()
    ct = torch.from_numpy(ctrl).to(dev)
    for sigma in (0.01, 0.05, 0.1):
        std = be.mc_fidelity_philox(ct, 2 ** 18, N, a, b, seed=7, sigma=sigma, h0_diag=diag, h0_offdiag=off).std(dim=1).cpu().numpy()
        for K in (1024, 4096, 16384, 65536):
            se_q = model.fidelity_rqmc(ctrl, replicates=R, points=K // R, seed=11, sigma=sigma)["se"]
            se_mc = std / np.sqrt(K)
            print(f"  {N:2d}  {sigma:5.2f}  {K:6d}  {np.median(se_mc):.3e}  {np.median(se_q):.3e}  {np.median(se_mc / se_q):6.1f}")
