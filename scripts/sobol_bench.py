#!/usr/bin/env python3
"""The fused Sobol fidelity kernel against the fused Philox kernel of the same build and against its own two-kernel route
(sobol_draws_kernel + mc_fid_chain_kernel): 100 controllers x 10 240 samples (R = 10 replicates of P = 1024 points), N = 5, 7, 10,
13, end-to-end pair.  One process, the three routes interleaved launch by launch, HIP events, 200 timed launches after 20, three
repeats; prints the median time per launch of each route and repeat, the ratios with their spread over the repeats, and whether the
two Sobol routes gave the same bits.

    python scripts/sobol_bench.py > profiles/sobol_bench.txt"""
import importlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

be = importlib.import_module("code-robchar_amd.backend")
sobol = importlib.import_module("code-robchar_amd.sobol")
dev = torch.device("cuda", 0)
C, R, P, WARM, TIMED, REPEATS = 100, 10, 1024, 20, 200, 3
K = R * P


def interleaved(routes):
    """median microseconds per launch of every route, the routes taking turns launch by launch"""
    for _ in range(WARM):
        for f in routes.values():
            f()
    ev = {k: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(TIMED)] for k in routes}
    for i in range(TIMED):
        for k, f in routes.items():
            a, b = ev[k][i]
            a.record()
            f()
            b.record()
    torch.cuda.synchronize()
    return {k: float(np.median([a.elapsed_time(b) for a, b in ev[k]])) * 1e3 for k in routes}


print(f"# {C} x {K} (R = {R}, P = {P}), sigma = 0.05, end-to-end pair; us per launch, median of {TIMED} after {WARM}, routes interleaved")
for N in (5, 7, 10, 13):
    rng = np.random.default_rng(N)
    x = np.empty((C, N + 1))
    x[:, :N] = rng.uniform(-1, 1, (C, N))
    x[:, N] = rng.uniform(0.5 * N, 0.7 * N, C)
    ct = torch.from_numpy(x).to(dev)
    dirnum, shift = sobol.scramble(3 * N, R, seed=N)
    dn, sh = (torch.from_numpy(a.view(np.int32)).to(dev) for a in (dirnum, shift))
    o_sobol, o_philox, o_two = (torch.empty((C, K), dtype=torch.float64, device=dev) for _ in range(3))

    def two():
        d = be.sobol_normal(dn, sh, P, K, sigma=0.05, C=C)
        be.mc_fidelity(ct, d.view(C, K, N, 3), N, 0, N - 1, out=o_two)

    routes = {"sobol fused": lambda: be.mc_fidelity_sobol(ct, K, N, 0, N - 1, dn, sh, P, sigma=0.05, out=o_sobol),
              "philox fused": lambda: be.mc_fidelity_philox(ct, K, N, 0, N - 1, 99, sigma=0.05, out=o_philox),
              "sobol two kernels": two}
    runs = [interleaved(routes) for _ in range(REPEATS)]
    for k in routes:
        print(f"N={N:2d} {k:18s} " + "  ".join(f"{r[k]:8.1f}" for r in runs))
    for num, den in (("sobol fused", "philox fused"), ("sobol fused", "sobol two kernels")):
        q = [r[num] / r[den] for r in runs]
        print(f"N={N:2d} {num} / {den}: {np.median(q):.3f}  (repeats {min(q):.3f} .. {max(q):.3f})")
    print(f"N={N:2d} fused and two-kernel Sobol routes identical: {bool(torch.equal(o_sobol, o_two))}")
