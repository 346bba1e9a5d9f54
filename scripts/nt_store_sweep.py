#!/usr/bin/env python3
"""Where the non-temporal store of the fidelities pays (the store rule of launch_chain, robchar_hip.hip): the chain kernel on
C = 25 ... 10 000 controllers x 10 000 draws per launch (3 925 ... 1 570 000 tiles), every size with the rule forced ON and OFF
through the hook rc_debug_nt_store_tiles, the two interleaved rep by rep, back-to-back launches inside one pair of HIP events
(as scripts/launch_size_sweep.py).  Prints us per launch for both, their ratio and each side's spread (max - min over the reps).

usage: python3 scripts/nt_store_sweep.py [--N 7] [--out end|mid] [--sizes 25,100,...] [--reps 5] [--total 4e8]
"""
import argparse, ctypes, importlib, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
be = importlib.import_module("code-robchar_amd.backend")
lib = importlib.import_module("code-robchar_amd._lib").load()
hook = lib.rc_debug_nt_store_tiles
hook.argtypes, hook.restype = [ctypes.c_longlong], ctypes.c_longlong

ap = argparse.ArgumentParser()
ap.add_argument("--N", type=int, default=7)
ap.add_argument("--K", type=int, default=10000)
ap.add_argument("--out", default="end")
ap.add_argument("--sizes", default="25,100,400,1000,2000,4000,10000")
ap.add_argument("--total", type=float, default=4e8)
ap.add_argument("--reps", type=int, default=5)
args = ap.parse_args()
N, K = args.N, args.K
o = N - 1 if args.out == "end" else N // 2
sizes = [int(v) for v in args.sizes.split(",")]
Cmax = max(sizes)
rng = np.random.default_rng(20220714 + N)
ctrl = np.empty((Cmax, N + 1)); ctrl[:, :N] = rng.uniform(-10, 10, (Cmax, N)); ctrl[:, N] = rng.uniform(2, 30, Cmax)
ct = torch.from_numpy(ctrl).cuda()
draws = be.philox_normal((Cmax, K, N, 3), seed=N, scale=0.05, as_torch=True)
out = torch.empty((Cmax, K), dtype=torch.float64, device="cuda")
st = torch.cuda.current_stream()
print(f"# N={N} 0->{o} K={K}; built-in rule: fewer than {hook(-1)} tiles")
try:
    for C in sizes:
        nl = max(20, int(args.total / (C * K)))
        nwin = max(1, Cmax // C)

        def run(n):
            for j in range(n):
                w = (j % nwin) * C
                be.mc_fidelity(ct[w:w + C], draws[w:w + C], N, 0, o, out=out[w:w + C])
        res = {0: [], 1: []}
        run(max(10, nl // 4))
        torch.cuda.synchronize()
        for r in range(args.reps):
            for on in (1, 0):
                hook(1 << 62 if on else 0)
                run(max(5, nl // 10))
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(st); run(nl); e1.record(st)
                torch.cuda.synchronize()
                res[on].append(e0.elapsed_time(e1) / nl * 1e3)
        m1, m0 = float(np.median(res[1])), float(np.median(res[0]))
        print(f"C={C:6d} tiles={C * ((K + 63) // 64):8d} launches={nl:5d}: nt {m1:10.2f} us (spread {np.ptp(res[1]) / m1 * 100:.2f} %)   "
              f"plain {m0:10.2f} us (spread {np.ptp(res[0]) / m0 * 100:.2f} %)   nt / plain {m1 / m0:.4f}", flush=True)
finally:
    hook(-1)
