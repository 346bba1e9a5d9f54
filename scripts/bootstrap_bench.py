#!/usr/bin/env python
"""Time of the on-device bootstrap of the metrics (`backend.bootstrap_metrics`: bootstrap_replicates_kernel, and with the summary
the row sort + bootstrap_summary_kernel) next to the same result written as chunked `torch` operations (`randint`, `gather`,
reductions; with the summary: `sort` + picks) in the same process.

HIP events around `--launches` launches after `--warmup`; the fidelity slabs (Beta(8, 2) values) are rotated through more than the
256 MiB Infinity Cache.  Shapes C x K with B replicates: 100 x 10^4, B = 1000 (LDS route, 10^9 draws); 1000 x 10^4, B = 100;
100 x 10^5, B = 100 (global route).  The torch formulation is timed over `--torch-launches` launches after two (it is chunked to at
most 2^27 gathered values at a time, and slow).

Its floor: index written and read (int64), gathered value written and read = 32 B through HBM per resampled value, i.e. 4.0 ms
per 10^9 values at 8 TB/s.

    python scripts/bootstrap_bench.py [--out profiles/bootstrap_bench.txt]"""
import argparse
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SHAPES = ((100, 10_000, 1000), (1000, 10_000, 100), (100, 100_000, 100))
CHUNK = 1 << 27


def torch_bootstrap(torch, fid, B, thr, summary, ranks):
    C, K = fid.shape
    step = max(1, CHUNK // (C * K))
    parts = []
    for b0 in range(0, B, step):
        nb = min(step, B - b0)
        idx = torch.randint(K, (C, nb, K), device=fid.device)
        g = fid[:, None, :].expand(C, nb, K).gather(2, idx)
        parts.append(torch.stack([1.0 - g.mean(2), g.std(2, unbiased=False), g.amin(2)]
                                 + [(g >= t).to(torch.float64).mean(2) for t in thr]))
    rep = torch.cat(parts, dim=2)                                   # (M, C, B)
    if not summary:
        return rep
    srt = torch.sort(rep, dim=2).values
    return torch.stack([rep.mean(2), rep.std(2, unbiased=True), srt[:, :, ranks[0]], srt[:, :, ranks[1]]], dim=1)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--torch-launches", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    be = importlib.import_module("code-robchar_amd.backend")
    boot = importlib.import_module("code-robchar_amd.bootstrap")
    dev = be.compute_device()
    thr = be.Q_THRESHOLDS

    def timed(fn, launches, warmup):
        for i in range(warmup):
            fn(i)
        torch.cuda.synchronize(dev)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(launches):
            fn(warmup + i)
        e1.record()
        torch.cuda.synchronize(dev)
        return e0.elapsed_time(e1) / launches                        # ms per launch

    lines = [f"# bootstrap of the metrics on the device against chunked torch operations, {args.launches} launches after {args.warmup} "
             f"(torch: {args.torch_launches} after 2), HIP events, fidelity slabs rotated past the Infinity Cache",
             f"# device: {torch.cuda.get_device_name(dev)}",
             "# C x K, B | route | draws | replicates ms | + summary ms | ns per 10^3 draws | torch replicates ms | torch + summary ms | "
             "torch floor ms (32 B per draw at 8 TB/s)"]
    for C, K, B in SHAPES:
        nslab = (300 * 2 ** 20) // (C * K * 8) + 2
        rng = np.random.default_rng(C + K)
        slabs = [torch.from_numpy(rng.beta(8.0, 2.0, (C, K))).to(dev) for _ in range(nslab)]
        ranks = boot.ranks(B, 0.95)
        rep_ms = timed(lambda i: be.bootstrap_metrics(slabs[i % nslab], B, 7, offset=i, want=("replicates",)), args.launches, args.warmup)
        sum_ms = timed(lambda i: be.bootstrap_metrics(slabs[i % nslab], B, 7, offset=i, want=("summary",)), args.launches, args.warmup)
        t_rep = timed(lambda i: torch_bootstrap(torch, slabs[i % nslab], B, thr, False, ranks), args.torch_launches, 2)
        t_sum = timed(lambda i: torch_bootstrap(torch, slabs[i % nslab], B, thr, True, ranks), args.torch_launches, 2)
        draws = C * K * B
        lines.append(f"{C} x {K}, B = {B} | {'lds' if K <= boot.LDS_MAX_K else 'global'} | {draws:.1e} | {rep_ms:.3f} | {sum_ms:.3f} | "
                     f"{rep_ms * 1e9 / draws:.2f} | {t_rep:.1f} | {t_sum:.1f} | {draws * 32 / 8e12 * 1e3:.2f}")
        print(lines[-1], flush=True)
        del slabs
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
