#!/usr/bin/env python
"""Time of the noise-sensitivity kernel next to the two kernels it is measured against: the fidelity kernel (finite
differences over the 3 N - 2 structured directions cost 3 N - 1 fidelity launches; the kernel earns its place below that)
and the controller-gradient kernel, whose eigensystem it shares.

HIP events around `--launches` launches after `--warmup`, draw tensors rotated through more than the 256 MiB Infinity
Cache, 100 x 10 000 samples at sigma = 0.05: N = 5, 7, 10 on the delocalised controller sets of the benchmark, and
N = 9, 11, 12 (the largest single-pass size and the two with the most QL passes) on chain_checks.deloc_ctrl rows.

    python scripts/sens_bench.py [--out profiles/sens_bench.txt]"""
import argparse
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import chain_checks as cc
    from conftest import highfid_workload
    be = importlib.import_module("code-robchar_amd.backend")
    dev = be.compute_device()
    C, K = 100, 10000
    lines = [f"# noise-sensitivity kernel vs fidelity and controller-gradient kernels, {C} x {K} samples, sigma = 0.05, "
             f"{args.launches} launches after {args.warmup}, HIP events, draws rotated past the Infinity Cache",
             f"# device: {torch.cuda.get_device_name(dev)}",
             "# N  in out | fidelity us | grad (all) us | sens (fid+sens+mean) us  /fid  /grad | sens (mean only) us  /fid  /grad | 3N - 1"]
    work = [highfid_workload(cid, C=C) for cid in (2, 3, 5)]
    rng = np.random.default_rng(12)
    work += [(N, 0, N - 1, cc.deloc_ctrl(rng, C, N, 0.5), None) for N in (9, 11, 12)]
    for N, a, b, ctrl, h0 in work:
        nbuf = int(np.ceil(300 * 2 ** 20 / (C * K * N * 24))) + 1
        gen = torch.Generator(device=dev).manual_seed(N)
        bufs = [0.05 * torch.randn((C, K, N, 3), dtype=torch.float64, device=dev, generator=gen) for _ in range(nbuf)]
        ct = torch.from_numpy(ctrl).to(dev)
        fid = torch.empty((C, K), dtype=torch.float64, device=dev)

        def timed(fn):
            for i in range(args.warmup):
                fn(bufs[i % nbuf])
            torch.cuda.synchronize(dev)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for i in range(args.launches):
                fn(bufs[i % nbuf])
            e1.record()
            torch.cuda.synchronize(dev)
            return e0.elapsed_time(e1) * 1e3 / args.launches

        t_f = timed(lambda d: be.mc_fidelity(ct, d, N, a, b, h0_diag=h0, out=fid))
        t_g = timed(lambda d: be.mc_fidelity_grad(ct, d, N, a, b, h0_diag=h0))
        t_all = timed(lambda d: be.mc_fidelity_sens(ct, d, N, a, b, h0_diag=h0))
        t_mean = timed(lambda d: be.mc_fidelity_sens(ct, d, N, a, b, h0_diag=h0, want=("mean",)))
        lines.append(f"{N:3d} {a:3d} {b:3d} | {t_f:9.1f} | {t_g:9.1f} | {t_all:9.1f} {t_all / t_f:6.2f} {t_all / t_g:6.2f} | "
                     f"{t_mean:9.1f} {t_mean / t_f:6.2f} {t_mean / t_g:6.2f} | {3 * N - 1}")
        print(lines[-1], flush=True)
        del bufs
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
