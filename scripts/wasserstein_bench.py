#!/usr/bin/env python
"""Time of the pairwise Wasserstein matrix on the device (`backend.wasserstein_matrix` on sorted rows: wasserstein_tile_kernel and,
where K is split, wasserstein_finish_kernel) next to three yardsticks, in the same process:

  (a) the chunked `torch` formulation a user would write today, `(A[i0:i1, None, :] - B[None]).abs().mean(-1)` (p = 2: `.square()`,
      `.sqrt()`) with temporaries of at most 1 GiB; it streams at least 2 x 8 CA CB K bytes through HBM;
  (b) the VALU floor: the fp64 VALU instructions per term counted in the built kernel's own listing (`--listing`, the inner loop of
      wasserstein_tile_kernel; 2 by design when no listing is at hand), 4 issue cycles per wave64 instruction, every SIMD busy, at
      the shader clock read while the kernel runs (`rocm-smi --showclocks`; the nominal 2.4 GHz when it cannot be read);
  (c) `scipy.stats.wasserstein_distance` per pair on this host's CPU, for scale only (p = 1).

HIP events around `--launches` launches after `--warmup`, the routes in turn, `--repeats` times (the best and the median of the
repeats are printed); the sorted inputs (Beta(5, 1.5) rows) are rotated through more than the 256 MiB Infinity Cache.  Shapes:
100 x 100 and 1000 x 1000 (symmetric mode) at K = 10^3 and 10^4, and the rectangular 1000 x 100 x 10^4; p = 1 and 2.

    python scripts/wasserstein_bench.py [--out profiles/wasserstein_bench.txt] [--listing code-robchar_amd/csrc/robchar_hip.gfx950.s]"""
import argparse
import importlib
import os
import re
import subprocess
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SHAPES = ((100, None, 1_000), (100, None, 10_000), (1000, None, 1_000), (1000, None, 10_000), (1000, 100, 10_000))
TEMP_BYTES = 1 << 30
NOMINAL_HZ = 2.4e9


def torch_matrix(torch, A, B, p):
    CA, K = A.shape
    step = max(1, TEMP_BYTES // (B.shape[0] * K * 8))
    out = torch.empty((CA, B.shape[0]), dtype=torch.float64, device=A.device)
    for i0 in range(0, CA, step):
        d = A[i0:i0 + step, None, :] - B[None]
        out[i0:i0 + step] = d.abs().mean(-1) if p == 1 else d.square().mean(-1).sqrt()
    return out


def valu_per_term(listing):
    """fp64 VALU instructions per term of wasserstein_tile_kernel<1> and <2>, counted in the basic block of the listing that holds
    the ds_read_b128 (the unrolled inner loop: four reads and 16 terms per lane and value of k).  None when there is no listing."""
    if not listing or not os.path.exists(listing):
        return None
    text = open(listing).read()
    out = {}
    for p in (1, 2):
        m = re.search(r"^_ZN\S*wasserstein_tile_kernelILi%dE\S*:.*?\n(.*?)\n\s*s_endpgm" % p, text, re.S | re.M)
        if not m:
            return None
        blocks = re.split(r"^(?:\.LBB\S*:|\s+s_c?branch\S*\s).*$", m.group(1), flags=re.M)
        ops = lambda blk: [l.split()[0] for l in blk.splitlines() if l.split()]
        loop = max(blocks, key=lambda blk: ops(blk).count("ds_read_b128"))
        reads = ops(loop).count("ds_read_b128")
        if not reads:
            return None
        out[p] = sum(1 for op in ops(loop) if re.match(r"v_\w+_f64", op)) / (reads // 4 * 16)
    return out


class ClockSampler(threading.Thread):
    """shader clock (Hz) read from `rocm-smi --showclocks` while the timed launches run"""

    def __init__(self):
        super().__init__(daemon=True)
        self.samples, self.stop = [], False

    def run(self):
        while not self.stop:
            try:
                txt = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=20).stdout
                mhz = [int(v) for v in re.findall(r"sclk clock level:.*?\((\d+)Mhz\)", txt)]
                if mhz:
                    self.samples.append(max(mhz) * 1e6)
            except Exception:
                return
            time.sleep(0.05)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--torch-launches", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--listing", default=os.path.join(ROOT, "code-robchar_amd", "csrc", "robchar_hip.gfx950.s"))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    be = importlib.import_module("code-robchar_amd.backend")
    dev = be.compute_device()
    simds = 4 * torch.cuda.get_device_properties(dev).multi_processor_count
    per_term = valu_per_term(args.listing)
    counted = per_term is not None and all(per_term.values())
    if not counted:
        per_term = {1: 2.0, 2: 2.0}

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

    lines = [f"# pairwise Wasserstein matrix on the device against (a) chunked torch, (b) the VALU floor, (c) scipy per pair; "
             f"{args.launches} launches after {args.warmup} (torch: {args.torch_launches} after 1), routes in turn, {args.repeats} repeats "
             f"(best / median), HIP events, inputs rotated past the Infinity Cache",
             f"# device: {torch.cuda.get_device_name(dev)}, {simds} SIMDs",
             f"# fp64 VALU instructions per term: p=1 {per_term[1]:.3f}, p=2 {per_term[2]:.3f} "
             f"({'counted in the listing' if counted else 'by design: no listing at hand'})"]
    try:
        from scipy import stats
        rng = np.random.default_rng(1)
        for K in (1_000, 10_000):
            x, y = rng.beta(5.0, 1.5, (20, K)), rng.beta(2.0, 2.0, (20, K))
            t0 = time.perf_counter()
            for a, b in zip(x, y):
                stats.wasserstein_distance(a, b)
            lines.append(f"# (c) scipy.stats.wasserstein_distance on this host: {(time.perf_counter() - t0) / 20 * 1e3:.3f} ms per pair at K = {K}")
    except ImportError:
        lines.append("# (c) scipy not installed: not measured")
    lines.append("# CA x CB x K | p | kernel ms best / median | (b) floor ms @ clock GHz | kernel / floor | (a) torch ms | torch / kernel | "
                 "torch's HBM floor ms (16 B per term at 8 TB/s)")
    print("\n".join(lines), flush=True)
    for CA, CB, K in SHAPES:
        rows_b = CA if CB is None else CB
        nslab = (300 * 2 ** 20) // ((CA + (CB or 0)) * K * 8) + 2
        rng = np.random.default_rng(CA + K)
        mk = lambda C, ab: torch.from_numpy(np.sort(rng.beta(ab[0], ab[1], (C, K)), axis=1)).to(dev)
        slabs = [(mk(CA, (5.0, 1.5)), None if CB is None else mk(CB, (2.0, 2.0))) for _ in range(nslab)]
        out = torch.empty((CA, rows_b), dtype=torch.float64, device=dev)
        terms = (CA * (CA + 1) // 2 if CB is None else CA * CB) * K       # what the launch computes: symmetric mode, half
        t_kernel, t_torch, clocks = {1: [], 2: []}, {1: [], 2: []}, []
        for _ in range(args.repeats):
            for p in (1, 2):
                sampler = ClockSampler()
                sampler.start()
                t_kernel[p].append(timed(lambda i: be.wasserstein_matrix(*slabs[i % nslab], p=p, assume_sorted=True, out=out),
                                         args.launches, args.warmup))
                sampler.stop = True
                sampler.join(timeout=30)
                clocks += sampler.samples
                t_torch[p].append(timed(lambda i: torch_matrix(torch, slabs[i % nslab][0], slabs[i % nslab][1] if CB else slabs[i % nslab][0], p),
                                        args.torch_launches, 1))
        hz = float(np.median(clocks)) if clocks else NOMINAL_HZ
        for p in (1, 2):
            best, med = min(t_kernel[p]), float(np.median(t_kernel[p]))
            floor = terms * per_term[p] / 64 * 4 / (simds * hz) * 1e3
            tt = float(np.median(t_torch[p]))
            lines.append(f"{CA} x {rows_b}{' (symmetric)' if CB is None else ''} x {K} | {p} | {best:.4f} / {med:.4f} | {floor:.4f} @ "
                         f"{hz / 1e9:.2f}{'' if clocks else ' (nominal, not read)'} | {best / floor:.2f} | {tt:.2f} | {tt / best:.0f} | "
                         f"{CA * rows_b * K * 16 / 8e12 * 1e3:.3f}")
            print(lines[-1], flush=True)
        del slabs
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
