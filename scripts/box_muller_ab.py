#!/usr/bin/env python3
"""What the nudge in box_muller_pair's radicand costs: the two kernels that spend most of their time in that routine - the
draw generator (philox_normal_kernel) and the N = 7 fidelity kernel that generates its own draws (mc_fid_chain_philox_kernel) - on
two builds of the library loaded side by side in ONE process (ctypes), the same device buffers, launches interleaved build by
build and rep by rep inside one pair of HIP events each (the method of scripts/ab_rounds.py's kernel part and
scripts/nt_store_sweep.py).  Prints every figure, the medians, each side's spread (max - min over the reps) and whether the two
builds wrote the same bits.

usage: python3 scripts/box_muller_ab.py --libs parent=/path/to/librobchar_hip.so,branch=code-robchar_amd/csrc/librobchar_hip.so
                                        [--reps 7] [--launches 400] [--out FILE]
"""
import argparse
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--libs", required=True, help="name=path,name=path (last = reference)")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--launches", type=int, default=400)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    fh = open(args.out, "w") if args.out else None

    def log(s):
        print(s, flush=True)
        if fh:
            fh.write(s + "\n")
            fh.flush()

    import torch
    dev = torch.device("cuda", 0)
    vp, ll, ull, i, d = ctypes.c_void_p, ctypes.c_longlong, ctypes.c_ulonglong, ctypes.c_int, ctypes.c_double
    libs = []
    for item in args.libs.split(","):
        name, path = item.split("=", 1)
        lib = ctypes.CDLL(os.path.abspath(path))
        lib.rc_draws_philox_f64_async.argtypes = [i, vp, ull, ull, ll, d, vp]
        lib.rc_draws_philox_f64_async.restype = i
        lib.rc_mc_fidelity_philox_f64_async.argtypes = [i, vp, i, i, i, i, vp, vp, vp, ull, ull, d, vp, ll, ll, vp]
        lib.rc_mc_fidelity_philox_f64_async.restype = i
        lib.rc_version.restype = i
        libs.append((name, lib))
    log("libraries: " + ", ".join(f"{n} (ABI {l.rc_version()})" for n, l in libs))
    st = torch.cuda.current_stream(dev)
    sp = ctypes.c_void_p(st.cuda_stream)
    N, C, K = 7, 100, 10000
    rng = np.random.default_rng(20220714 + 3)
    ctrl_np = np.empty((C, N + 1))
    ctrl_np[:, :N] = rng.uniform(-10, 10, (C, N))
    ctrl_np[:, N] = rng.uniform(2, 30, C)
    ctrl = torch.from_numpy(ctrl_np).to(dev)
    nd = C * K * N * 3
    draws = {n: torch.empty(nd, dtype=torch.float64, device=dev) for n, _ in libs}
    fid = {n: torch.empty((C, K), dtype=torch.float64, device=dev) for n, _ in libs}

    def gen(lib, name, n):
        for j in range(n):
            assert lib.rc_draws_philox_f64_async(0, sp, 1234, 0, nd, 0.05, vp(draws[name].data_ptr())) == 0

    def fused(lib, name, n):
        for j in range(n):
            assert lib.rc_mc_fidelity_philox_f64_async(0, sp, 0, N, 0, N - 1, None, None, vp(ctrl.data_ptr()), 1234, 0, 0.05, None, C, K,
                                                       vp(fid[name].data_ptr())) == 0

    for label, run, unit, per in (("generator: philox_normal_kernel, 2.1e7 normals per launch", gen, "us per launch", 1.0),
                                  (f"fused fidelity: mc_fid_chain_philox_kernel<{N}, ends>, {C} x {K}", fused, "us per 1e6 evaluations", 1e6 / (C * K))):
        for n, lib in libs:
            run(lib, n, 30)
        run(libs[0][1], libs[0][0], 300)                               # clock pre-roll
        torch.cuda.synchronize(dev)
        res = {n: [] for n, _ in libs}
        for r in range(args.reps):
            for n, lib in libs:
                run(lib, n, 40)                                        # the build's own short lead-in
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(st)
                run(lib, n, args.launches)
                e1.record(st)
                torch.cuda.synchronize(dev)
                res[n].append(e0.elapsed_time(e1) / args.launches * 1e3 * per)
        ref = libs[-1][0]
        buf = draws if run is gen else fid
        log(f"{label}  ({unit}, {args.launches} launches per figure)")
        for n, _ in libs:
            v = res[n]
            same = bool(torch.equal(buf[n].view(torch.int64), buf[ref].view(torch.int64)))
            log(f"    {n:>7s}: " + "  ".join(f"{x:8.2f}" for x in v) + f"   median {np.median(v):8.2f}  spread {np.ptp(v) / np.median(v) * 100:.2f} %"
                f"   vs {ref} {np.median(v) / np.median(res[ref]):.4f}   bits equal to {ref}: {same}")
        log(f"    NaN in the output: {bool(torch.isnan(buf[ref]).any())}")


if __name__ == "__main__":
    main()
