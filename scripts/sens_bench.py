#!/usr/bin/env python
"""Time of the noise-sensitivity kernel next to the two kernels it is measured against: the fidelity kernel (finite
differences over the 3 N - 2 structured directions cost 3 N - 1 fidelity launches; the kernel earns its place below that)
and the controller-gradient kernel, whose eigensystem it shares.

HIP events around `--launches` launches after `--warmup`, draw tensors rotated through more than the 256 MiB Infinity
Cache, 100 x 10 000 samples at sigma = 0.05: N = 5, 7, 10 on the delocalised controller sets of the benchmark, and
N = 9, 11, 12 (the largest single-pass size and the two with the most QL passes) on chain_checks.deloc_ctrl rows.

Then the kernel that generates its own draws (`mc_fidelity_sens_philox`) against the two-kernel route it replaces
(`philox_normal` into one reused buffer + `mc_fidelity_sens`), mean only, `--fused-launches` launches after `--fused-warmup`,
the two routes alternated in one process and repeated `--repeats` times so that the spread is known:
  leg (a)  100 x 10 000 at N = 5 / 7 / 10 / 12, the fidelity kernel (on the generated buffer) timed beside them;
  leg (b)  the product shape - 11 sigma levels x 100 controllers x K = 1000 and K = 100: ONE fused launch over the 1100 rows
           with a sigma per row against 11 x (generator + sensitivity kernel), at N = 7.

    python scripts/sens_bench.py [--out profiles/sens_bench.txt] [--skip-kernels]"""
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
    ap.add_argument("--fused-launches", type=int, default=200)
    ap.add_argument("--fused-warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--skip-kernels", action="store_true", help="only the fused-against-two-kernel legs")
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
    for N, a, b, ctrl, h0 in ([] if args.skip_kernels else work):
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

    # ---- the kernel that generates its own draws against generator + sensitivity kernel
    def timed_calls(fn, launches, warmup):
        for _ in range(warmup):
            fn()
        torch.cuda.synchronize(dev)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(launches):
            fn()
        e1.record()
        torch.cuda.synchronize(dev)
        return e0.elapsed_time(e1) * 1e3 / launches

    def spread(v):
        return f"{min(v):9.1f} .. {max(v):9.1f}"

    sigma, seed = 0.05, 7
    FL, FW = args.fused_launches, args.fused_warmup
    lines += [f"# (a) fused draws (mc_fidelity_sens_philox) against philox_normal + mc_fidelity_sens, mean only, {C} x {K}, sigma = {sigma}, "
              f"{FL} launches after {FW}, routes alternated, {args.repeats} repeats (min .. max, us per launch)",
              "# N  in out | two kernels us | fused us | fused / two (of the minima) | fidelity kernel us | draw tensor not allocated, MB | 3N - 1"]
    byN = {w[0]: w for w in work}
    for N in (5, 7, 10, 12):
        _, a, b, ctrl, h0 = byN[N]
        ct = torch.from_numpy(ctrl).to(dev)
        buf = torch.empty((C, K, N, 3), dtype=torch.float64, device=dev)
        fid = torch.empty((C, K), dtype=torch.float64, device=dev)

        def two():
            be.philox_normal(buf.shape, seed, scale=sigma, out=buf)
            be.mc_fidelity_sens(ct, buf, N, a, b, h0_diag=h0, want=("mean",))

        t2, t1, tf = [], [], []
        for _ in range(args.repeats):
            t2.append(timed_calls(two, FL, FW))
            t1.append(timed_calls(lambda: be.mc_fidelity_sens_philox(ct, K, N, a, b, seed, sigma=sigma, h0_diag=h0, want=("mean",)), FL, FW))
            tf.append(timed_calls(lambda: be.mc_fidelity(ct, buf, N, a, b, h0_diag=h0, out=fid), FL, FW))
        lines.append(f"{N:3d} {a:3d} {b:3d} | {spread(t2)} | {spread(t1)} | {min(t1) / min(t2):5.2f} | {spread(tf)} | "
                     f"{buf.numel() * 8 / 1e6:8.1f} | {3 * N - 1}")
        print(lines[-1], flush=True)
        del buf
    L, Cp, N = 11, 100, 7
    _, a, b, ctrl, h0 = byN[N]
    levels = np.linspace(0.0, 0.1, L)
    lines += [f"# (b) the product shape at N = {N}: {L} levels x {Cp} controllers x K; one fused launch over {L * Cp} rows (sigma per row) "
              f"against {L} x (generator + sensitivity kernel); {FL} repetitions of the whole algorithm after {FW}",
              "#     K | 11 x two kernels us | one fused launch us | fused / two (of the minima) | draw tensors not allocated, MB"]
    for Kp in (1000, 100):
        ct = torch.from_numpy(ctrl[:Cp]).to(dev)
        tiled = ct.repeat(L, 1)
        rows = torch.from_numpy(np.repeat(levels, Cp)).to(dev)
        buf = torch.empty((Cp, Kp, N, 3), dtype=torch.float64, device=dev)
        per = Cp * Kp * N * 3

        def eleven():
            for j in range(L):
                be.philox_normal(buf.shape, seed, scale=float(levels[j]), offset=j * per, out=buf)
                be.mc_fidelity_sens(ct, buf, N, a, b, h0_diag=h0, want=("mean",))

        t2, t1 = [], []
        for _ in range(args.repeats):
            t2.append(timed_calls(eleven, FL, FW))
            t1.append(timed_calls(lambda: be.mc_fidelity_sens_philox(tiled, Kp, N, a, b, seed, sigma=rows, h0_diag=h0, want=("mean",)), FL, FW))
        lines.append(f"{Kp:7d} | {spread(t2)} | {spread(t1)} | {min(t1) / min(t2):5.2f} | {L * per * 8 / 1e6:8.1f}")
        print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
