#!/usr/bin/env python
"""Time of the fidelity on a grid of M readout times from one eigen decomposition per sample (`mc_fidelity_times`) next to what
it replaces: M launches of the fidelity kernel on controllers with the time entry replaced.

100 x 10 000 samples, sigma = 0.05, the delocalised controller sets, N = 5, 7, 10, M = 1, 4, 16.  HIP events around `--launches`
launches after `--warmup`, draw tensors rotated through more than the 256 MiB Infinity Cache, the routes alternated in one
process, `--repeats` repeats (min .. max).  Routes:

    (a) M launches of mc_fidelity(kernel="auto")         (the product's fidelity kernel: the line to beat)
    (b) M launches of mc_fidelity(kernel="tridiag_ql")   (the rows kernel: the same arithmetic as the new one, M times over)
    (c) one launch of mc_fidelity_times writing the M slabs
    (d) the same writing "wsum" and "min" only

    python scripts/times_bench.py [--out profiles/times_bench.txt]"""
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
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--sizes", default="5,7,10")
    ap.add_argument("--grids", default="1,4,16")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from conftest import highfid_workload
    be = importlib.import_module("code-robchar_amd.backend")
    dev = be.compute_device()
    C, K = 100, 10000
    sizes = [int(v) for v in args.sizes.split(",")]
    grids = [int(v) for v in args.grids.split(",")]
    lines = [f"# fidelity on a grid of M readout times, {C} x {K} samples, sigma = 0.05, {args.launches} launches after {args.warmup}, "
             f"HIP events, draws rotated past the Infinity Cache, routes alternated, {args.repeats} repeats (min .. max, us per "
             "evaluation of the whole grid)",
             f"# device: {torch.cuda.get_device_name(dev)}",
             "# (a) M x mc_fidelity(auto) | (b) M x mc_fidelity(tridiag_ql) | (c) mc_fidelity_times, M slabs | (d) mc_fidelity_times, "
             "wsum + min only",
             "# N  in out   M | (a) us | (b) us | (c) us | (d) us | (c)/(a) | (d)/(a) (of the minima) | (a) - (c) over 3 x the larger "
             "spread of the two"]
    work = {w[0]: w for w in (highfid_workload(cid, C=C) for cid in (2, 3, 5))}

    def spread(v):
        return f"{min(v):9.1f} .. {max(v):9.1f}"

    for N in sizes:
        _, a, b, ctrl, h0 = work[N]
        nbuf = int(np.ceil(300 * 2 ** 20 / (C * K * N * 24))) + 1
        gen = torch.Generator(device=dev).manual_seed(N)
        bufs = [0.05 * torch.randn((C, K, N, 3), dtype=torch.float64, device=dev, generator=gen) for _ in range(nbuf)]
        for M in grids:
            tscale = np.linspace(0.9, 1.1, M) if M > 1 else np.ones(1)
            weights = np.full(M, 1.0 / M)
            t = be.readout_times(ctrl[:, N], tscale, None)
            rows = []
            for j in range(M):                                          # the M controller sets of routes (a) and (b)
                cj = ctrl.copy()
                cj[:, N] = t[:, j]
                rows.append(torch.from_numpy(cj).to(dev))
            ct = torch.from_numpy(ctrl).to(dev)
            fid = torch.empty((M, C, K), dtype=torch.float64, device=dev)
            state = {"i": 0}

            def draws():
                state["i"] += 1
                return bufs[state["i"] % nbuf]

            def launches_of(kernel):
                d = draws()                                             # the M launches of one evaluation read the same draws
                for j in range(M):
                    be.mc_fidelity(rows[j], d, N, a, b, h0_diag=h0, kernel=kernel, out=fid[j])

            def timed(fn):
                for _ in range(args.warmup):
                    fn()
                torch.cuda.synchronize(dev)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.launches):
                    fn()
                e1.record()
                torch.cuda.synchronize(dev)
                return e0.elapsed_time(e1) * 1e3 / args.launches

            ta, tb, tc, td = [], [], [], []
            for _ in range(args.repeats):
                ta.append(timed(lambda: launches_of("auto")))
                tb.append(timed(lambda: launches_of("tridiag_ql")))
                tc.append(timed(lambda: be.mc_fidelity_times(ct, draws(), N, a, b, tscale=tscale, h0_diag=h0, want=("fid",))))
                td.append(timed(lambda: be.mc_fidelity_times(ct, draws(), N, a, b, tscale=tscale, weights=weights, h0_diag=h0,
                                                             want=("wsum", "min"))))
            margin = (min(ta) - min(tc)) / (3.0 * max(max(ta) - min(ta), max(tc) - min(tc), 1e-9))
            lines.append(f"{N:3d} {a:3d} {b:3d} {M:3d} | {spread(ta)} | {spread(tb)} | {spread(tc)} | {spread(td)} | "
                         f"{min(tc) / min(ta):5.2f} | {min(td) / min(ta):5.2f} | {margin:7.1f}")
            print(lines[-1], flush=True)
            del fid
        del bufs
    text = "\n".join(lines) + "\n"
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
