#!/usr/bin/env python3
"""The pick-freeze kernel of the variance indices against the routes a user had before it: 100 controllers x 10 000 samples,
N = 5, 7, 10, 13, end-to-end pair, the kind groups (G = 3) and the direction groups (G = 3 N - 2), row means only.

    fused         one `mc_fidelity_pickfreeze_philox` launch (want = ("mean",))
    tensor route  two `philox_normal` launches, G `torch.where` passes, G + 2 `mc_fidelity` launches and the elementwise
                  reductions to the same 3 + 2 G row means - the line to beat
    G + 2 philox  G + 2 `mc_fidelity_philox` launches: the evaluation work alone, the draws regenerated for every slab

One process, the routes interleaved launch by launch, HIP events, 200 timed launches after 20, three repeats; prints the median
time per launch of each route and repeat, the ratios with their spread over the repeats, the time per evaluation, and the
largest difference between the fused and the tensor route's row means.

    python scripts/variance_bench.py > profiles/variance_bench.txt"""
import importlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

be = importlib.import_module("code-robchar_amd.backend")
vi = importlib.import_module("code-robchar_amd.variance_indices")
dev = torch.device("cuda", 0)
C, K, WARM, TIMED, REPEATS, SEED = 100, 10000, 20, 200, 3, 99


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


print(f"# {C} x {K}, sigma = 0.05, end-to-end pair, row means only; us per launch, median of {TIMED} after {WARM}, routes interleaved")
for N in (5, 7, 10, 13):
    rng = np.random.default_rng(N)
    x = np.empty((C, N + 1))
    x[:, :N] = rng.uniform(-1, 1, (C, N))
    x[:, N] = rng.uniform(0.5 * N, 0.7 * N, C)
    ct = torch.from_numpy(x).to(dev)
    block = C * K * 3 * N
    for name, (masks, _) in (("kind", vi.kind_groups(N)), ("direction", vi.direction_groups(N))):
        G = len(masks)
        bits = torch.as_tensor(vi.mask_bits(masks, N), device=dev)
        A, B, H = (torch.empty((C, K, N, 3), dtype=torch.float64, device=dev) for _ in range(3))
        f = torch.empty((G + 2, C, K), dtype=torch.float64, device=dev)
        keep = {}

        def tensor_route():
            be.philox_normal((C, K, N, 3), SEED, scale=0.05, offset=0, out=A)
            be.philox_normal((C, K, N, 3), SEED, scale=0.05, offset=block, out=B)
            be.mc_fidelity(ct, A, N, 0, N - 1, out=f[0])
            be.mc_fidelity(ct, B, N, 0, N - 1, out=f[1])
            cols = [f[0].mean(dim=1), f[1].mean(dim=1), ((f[0] - f[1]) ** 2).mean(dim=1)]
            for g in range(G):
                torch.where(bits[g][None, None], B, A, out=H)
                be.mc_fidelity(ct, H, N, 0, N - 1, out=f[2 + g])
                cols += [((f[0] - f[2 + g]) ** 2).mean(dim=1), ((f[1] - f[2 + g]) ** 2).mean(dim=1)]
            keep["tensor"] = torch.stack(cols, dim=1)

        def philox_route():
            for e in range(G + 2):
                be.mc_fidelity_philox(ct, K, N, 0, N - 1, SEED, offset=e * block, sigma=0.05, out=f[e])

        def fused():
            keep["fused"] = be.mc_fidelity_pickfreeze_philox(ct, K, N, 0, N - 1, SEED, masks, offset=0, offset_b=block, sigma=0.05)["mean"]

        routes = {"fused": fused, "tensor route": tensor_route, "G + 2 philox": philox_route}
        runs = [interleaved(routes) for _ in range(REPEATS)]
        for k in routes:
            print(f"N={N:2d} {name:9s} G={G:2d} {k:13s} " + "  ".join(f"{r[k]:9.1f}" for r in runs))
        for den in ("tensor route", "G + 2 philox"):
            q = [r["fused"] / r[den] for r in runs]
            print(f"N={N:2d} {name:9s} G={G:2d} fused / {den}: {np.median(q):.3f}  (repeats {min(q):.3f} .. {max(q):.3f})")
        per = lambda k: np.median([r[k] for r in runs]) * 1e3 / ((G + 2) * C * K)
        print(f"N={N:2d} {name:9s} G={G:2d} ns per evaluation: fused {per('fused'):.3f}, mc_fid_chain_philox_kernel {per('G + 2 philox'):.3f}")
        print(f"N={N:2d} {name:9s} G={G:2d} fused - tensor route, row means: max |diff| {float((keep['fused'] - keep['tensor']).abs().max()):.2e}")
