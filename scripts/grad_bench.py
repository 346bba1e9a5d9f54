#!/usr/bin/env python
"""Time of the fidelity-gradient kernel next to the fidelity kernel it competes with (central differences through
`mc_fidelity` cost 2 (N + 1) launches per gradient; the kernel earns its place below N + 1).

HIP events around `--launches` launches after `--warmup`, draw tensors rotated through more than the 256 MiB Infinity
Cache, N = 5, 7, 10 at 100 x 10 000 on the delocalised controller sets; per-sample output and mean-only output separately.

    python scripts/grad_bench.py [--out profiles/grad_bench.txt]

--philox runs ANOTHER leg instead (the output above is unchanged without it): the gradient kernel that generates its own draws
(`mc_fidelity_grad_philox`) against the two-kernel route it replaces, N = 5, 7, 10, 12 at 100 x 10 000, sigma = 0.05,
delocalised sets: (a) `philox_normal` + `mc_fidelity_grad`, mean only; (b) the fused kernel, mean only; (c) the fused kernel,
mean + moment.  The routes alternate in one process, `--launches` launches after `--warmup`, HIP events, `--repeats` repeats.

    python scripts/grad_bench.py --philox [--out profiles/grad_philox_bench.txt]

--listed runs the CVaR leg: (a) the full launch, `mc_fidelity_grad_philox` mean only, against (b) the fidelity launch over all K
draws (`mc_fidelity_philox`) + the selection on the device (`noise.tail_weights`) + the listed launch over the selected alpha K
(`mc_fidelity_grad_listed`, sum only), alpha = 0.1 and 0.01, N = 5, 7, 10, 12 at 100 x 10 000, sigma = 0.05, same alternation.

    python scripts/grad_bench.py --listed [--out profiles/grad_listed_bench.txt]

Its last three columns split (b) at alpha = 0.1 into its launches: fidelity, selection (`backend.tail_select`), listed.

--select times the selection alone on a table of fidelities (N = 7, sigma = 0.05): (a) the torch route it replaces
(`noise._tail_weights_torch` + the gather / max of the value at risk), (b) `backend.tail_select`, (c) `reduce_metrics` through its
standalone route on the same table - the floor: it reads each row once.  100 x 10 000 and 1000 x 10 000 at alpha = 0.1 and 0.01,
11 000 x 100 at alpha = 0.1, 1000 x 100 000 at alpha = 0.01 (a tenth of the launches: its torch sort takes ~0.1 s).

    python scripts/grad_bench.py --select [--out profiles/tail_select_bench.txt]

--times runs the readout-jitter leg: the gradient on a grid of M readout times, M = 1, 4, 8, 16 (the Gauss-Hermite rule of
`noise.readout_jitter_nodes(0.1, M)`), N = 5, 7, 10 at 100 x 10 000, sigma = 0.05, same alternation: (a) M launches of
`mc_fidelity_grad_philox`, mean only, on copies of the controllers with the time entry moved to each grid time (what a
jitter-averaged gradient took before; the combination of the M rows is not even counted), (b) ONE launch of
`mc_fidelity_grad_times_philox`, mean only, (c) the same with the moment sums.

    python scripts/grad_bench.py --times [--out profiles/grad_times_bench.txt]"""
import argparse
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def philox_leg(args, be, dev, C, K):
    import torch
    import chain_checks as cc
    from conftest import highfid_workload
    sigma, seed = 0.05, 7
    lines = [f"# gradient kernel with its own draws (mc_fidelity_grad_philox) against philox_normal + mc_fidelity_grad, {C} x {K}, "
             f"sigma = {sigma}, {args.launches} launches after {args.warmup}, routes alternated, {args.repeats} repeats "
             "(min .. max, us per launch), HIP events",
             f"# device: {torch.cuda.get_device_name(dev)}",
             "# N  in out | (a) two kernels, mean us | (b) fused, mean us | (c) fused, mean + moment us | (b)/(a) | (c)/(b) "
             "(of the minima) | draw tensor not allocated, MB"]
    work = {w[0]: w for w in (highfid_workload(cid, C=C) for cid in (2, 3, 5))}
    work[12] = (12, 0, 11, cc.deloc_ctrl(np.random.default_rng(12), C, 12, 0.5), None)

    def timed_calls(fn):
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

    def spread(v):
        return f"{min(v):9.1f} .. {max(v):9.1f}"

    for N in (5, 7, 10, 12):
        _, a, b, ctrl, h0 = work[N]
        ct = torch.from_numpy(ctrl).to(dev)
        buf = torch.empty((C, K, N, 3), dtype=torch.float64, device=dev)

        def two():
            be.philox_normal(buf.shape, seed, scale=sigma, out=buf)
            be.mc_fidelity_grad(ct, buf, N, a, b, h0_diag=h0, want=("mean",))

        ta, tb, tc = [], [], []
        for _ in range(args.repeats):
            ta.append(timed_calls(two))
            tb.append(timed_calls(lambda: be.mc_fidelity_grad_philox(ct, K, N, a, b, seed, sigma=sigma, h0_diag=h0, want=("mean",))))
            tc.append(timed_calls(lambda: be.mc_fidelity_grad_philox(ct, K, N, a, b, seed, sigma=sigma, h0_diag=h0,
                                                                     want=("mean", "moment"))))
        lines.append(f"{N:3d} {a:3d} {b:3d} | {spread(ta)} | {spread(tb)} | {spread(tc)} | {min(tb) / min(ta):5.2f} | "
                     f"{min(tc) / min(tb):5.2f} | {buf.numel() * 8 / 1e6:8.1f}")
        print(lines[-1], flush=True)
        del buf
    return "\n".join(lines) + "\n"


def times_leg(args, be, dev, C, K):
    import torch
    from conftest import highfid_workload
    noise = importlib.import_module("code-robchar_amd.noise")
    sigma, seed, sigma_t = 0.05, 7, 0.1
    lines = [f"# gradient on a grid of M readout times: (a) M launches of mc_fidelity_grad_philox (mean only) against (b) one launch of "
             f"mc_fidelity_grad_times_philox (mean only) and (c) the same with the moment sums, {C} x {K}, sigma = {sigma}, grid = "
             f"readout_jitter_nodes({sigma_t}, M), {args.launches} launches after {args.warmup}, routes alternated, {args.repeats} "
             "repeats (min .. max, us per evaluation), HIP events",
             f"# device: {torch.cuda.get_device_name(dev)}",
             "# N  in out   M | (a) M launches us | (b) one launch us | (c) with moments us | (b)/(a) | (c)/(b) (of the minima) | "
             "(a) - (b) us (of the minima) | 3 x the larger spread us | (a) - (b) > 3 x spread"]
    work = {w[0]: w for w in (highfid_workload(cid, C=C) for cid in (2, 3, 5))}

    def timed_calls(fn):
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

    def spread(v):
        return f"{min(v):9.1f} .. {max(v):9.1f}"

    for N in (5, 7, 10):
        _, a, b, ctrl, h0 = work[N]
        ct = torch.from_numpy(ctrl).to(dev)
        for M in (1, 4, 8, 16):
            tshift, weights = noise.readout_jitter_nodes(sigma_t, M)
            moved = []
            for j in range(M):
                cj = ctrl.copy()
                cj[:, N] = ctrl[:, N] + tshift[j]
                moved.append(torch.from_numpy(cj).to(dev))

            def single():
                for cj in moved:
                    be.mc_fidelity_grad_philox(cj, K, N, a, b, seed, sigma=sigma, h0_diag=h0, want=("mean",))

            def grid(want):
                be.mc_fidelity_grad_times_philox(ct, K, N, a, b, seed, sigma=sigma, tshift=tshift, weights=weights, h0_diag=h0, want=want)

            ta, tb, tc = [], [], []
            for _ in range(args.repeats):
                ta.append(timed_calls(single))
                tb.append(timed_calls(lambda: grid(("mean",))))
                tc.append(timed_calls(lambda: grid(("mean", "moment"))))
            gain, noise_us = min(ta) - min(tb), 3.0 * max(max(ta) - min(ta), max(tb) - min(tb))
            lines.append(f"{N:3d} {a:3d} {b:3d} {M:3d} | {spread(ta)} | {spread(tb)} | {spread(tc)} | {min(tb) / min(ta):5.2f} | "
                         f"{min(tc) / min(tb):5.2f} | {gain:9.1f} | {noise_us:9.1f} | {'yes' if gain > noise_us else 'no'}")
            print(lines[-1], flush=True)
    return "\n".join(lines) + "\n"


def listed_leg(args, be, dev, C, K):
    import torch
    import chain_checks as cc
    from conftest import highfid_workload
    noise = importlib.import_module("code-robchar_amd.noise")
    sigma, seed, alphas = 0.05, 7, (0.1, 0.01)
    lines = [f"# CVaR route (mc_fidelity_philox + tail_weights + mc_fidelity_grad_listed, sum only) against the full launch "
             f"(mc_fidelity_grad_philox, mean only), {C} x {K}, sigma = {sigma}, {args.launches} launches after {args.warmup}, routes "
             f"alternated, {args.repeats} repeats (min .. max, us per evaluation), HIP events",
             f"# device: {torch.cuda.get_device_name(dev)}",
             "# N  in out | (a) full launch us | " + " | ".join(f"(b) alpha = {al} us | (b)/(a)" for al in alphas) + " (of the minima)"
             f" | the launches of (b) at alpha = {alphas[0]} alone: fidelity us | selection us | listed us (minima)"]
    work = {w[0]: w for w in (highfid_workload(cid, C=C) for cid in (2, 3, 5))}
    work[12] = (12, 0, 11, cc.deloc_ctrl(np.random.default_rng(12), C, 12, 0.5), None)

    def timed_calls(fn):
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

    def spread(v):
        return f"{min(v):9.1f} .. {max(v):9.1f}"

    for N in (5, 7, 10, 12):
        _, a, b, ctrl, h0 = work[N]
        ct = torch.from_numpy(ctrl).to(dev)
        fid = torch.empty((C, K), dtype=torch.float64, device=dev)

        def tail(alpha):
            be.mc_fidelity_philox(ct, K, N, a, b, seed, sigma=sigma, h0_diag=h0, out=fid)
            listed, weights = noise.tail_weights(fid, alpha)
            be.mc_fidelity_grad_listed(ct, K, listed, weights, nspin=N, inspin=a, outspin=b, seed=seed, sigma=sigma, h0_diag=h0,
                                       want=("sum",))

        ta, tb, tf, ts, tl = [], {al: [] for al in alphas}, [], [], []
        be.mc_fidelity_philox(ct, K, N, a, b, seed, sigma=sigma, h0_diag=h0, out=fid)
        sel = be.tail_select(fid, alphas[0], want=("list", "weight"))
        for _ in range(args.repeats):
            ta.append(timed_calls(lambda: be.mc_fidelity_grad_philox(ct, K, N, a, b, seed, sigma=sigma, h0_diag=h0, want=("mean",))))
            for al in alphas:
                tb[al].append(timed_calls(lambda: tail(al)))
            tf.append(timed_calls(lambda: be.mc_fidelity_philox(ct, K, N, a, b, seed, sigma=sigma, h0_diag=h0, out=fid)))
            ts.append(timed_calls(lambda: be.tail_select(fid, alphas[0], want=("list", "weight"))))
            tl.append(timed_calls(lambda: be.mc_fidelity_grad_listed(ct, K, sel["list"], sel["weight"], nspin=N, inspin=a, outspin=b,
                                                                     seed=seed, sigma=sigma, h0_diag=h0, want=("sum",))))
        lines.append(f"{N:3d} {a:3d} {b:3d} | {spread(ta)} | " + " | ".join(f"{spread(tb[al])} | {min(tb[al]) / min(ta):5.2f}" for al in alphas)
                     + f" | {min(tf):9.1f} | {min(ts):9.1f} | {min(tl):9.1f}")
        print(lines[-1], flush=True)
    return "\n".join(lines) + "\n"


def select_leg(args, be, dev):
    import torch
    from conftest import highfid_workload
    noise = importlib.import_module("code-robchar_amd.noise")
    sigma, seed = 0.05, 7
    shapes = ((100, 10_000, (0.1, 0.01), 1), (1000, 10_000, (0.1, 0.01), 1), (11_000, 100, (0.1,), 1), (1000, 100_000, (0.01,), 10))
    lines = [f"# tail selection of a (C, K) fidelity table (N = 7, sigma = {sigma}): (a) torch route (stable argsort + sort + masks + gather / "
             f"max), (b) backend.tail_select, (c) reduce_metrics, standalone route, no thresholds (the floor: one read of every row); "
             f"{args.launches} launches after {args.warmup} (the last shape: a tenth of both), routes alternated, {args.repeats} repeats "
             "(min .. max, us per call), HIP events",
             f"# device: {torch.cuda.get_device_name(dev)}",
             "#     C       K  alpha | (a) torch us | (b) tail_select us | (c) reduce us | (b)/(a) | (b)/(c) (of the minima) | table MB"]

    def spread(v):
        return f"{min(v):10.1f} .. {max(v):10.1f}"

    for C, K, alphas, fewer in shapes:
        N, a, b, ctrl, h0 = highfid_workload(3, C=C)
        ct = torch.from_numpy(ctrl).to(dev)
        try:
            fid = be.mc_fidelity_philox(ct, K, N, a, b, seed, sigma=sigma, h0_diag=h0)
            noise._tail_weights_torch(fid, alphas[0])                # (does the sort's workspace fit?)
            torch.cuda.synchronize(dev)
        except (RuntimeError, MemoryError) as exc:
            lines.append(f"{C:7d} {K:7d}: the table and the torch sort's temporaries do not fit: {type(exc).__name__}")
            print(lines[-1], flush=True)
            continue
        warmup, launches = max(1, args.warmup // fewer), max(1, args.launches // fewer)

        def timed_calls(fn):
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

        def old(alpha):
            listed, weights = noise._tail_weights_torch(fid, alpha)
            return torch.gather(fid, 1, listed.clamp(min=0).long()).max(dim=1).values

        for alpha in alphas:
            ta, tb, tc = [], [], []
            for _ in range(args.repeats):
                ta.append(timed_calls(lambda: old(alpha)))
                tb.append(timed_calls(lambda: be.tail_select(fid, alpha)))
                tc.append(timed_calls(lambda: be.reduce_metrics(fid, q_thresholds=(), overlapped=False)))
            lines.append(f"{C:7d} {K:7d} {alpha:6.2f} | {spread(ta)} | {spread(tb)} | {spread(tc)} | {min(tb) / min(ta):7.4f} | "
                         f"{min(tb) / min(tc):6.2f} | {fid.numel() * 8 / 1e6:8.1f}")
            print(lines[-1], flush=True)
        del fid
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--philox", action="store_true", help="the fused-against-two-kernel leg instead of the kernel table")
    ap.add_argument("--listed", action="store_true", help="the CVaR route against the full gradient launch instead of the kernel table")
    ap.add_argument("--select", action="store_true", help="the tail selection against the torch route and the reduction instead of the kernel table")
    ap.add_argument("--times", action="store_true", help="the gradient on a grid of readout times against M single-time launches instead of the kernel table")
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    import torch
    from conftest import highfid_workload
    be = importlib.import_module("code-robchar_amd.backend")
    dev = be.compute_device()
    C, K = 100, 10000
    if args.philox or args.listed or args.select or args.times:
        text = (select_leg(args, be, dev) if args.select else
                (times_leg if args.times else (listed_leg if args.listed else philox_leg))(args, be, dev, C, K))
        print(text, end="")
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as fh:
                fh.write(text)
        return
    lines = [f"# fidelity + gradient kernel vs fidelity kernel, {C} x {K} samples, sigma = 0.05, {args.launches} launches after "
             f"{args.warmup}, HIP events, draws rotated past the Infinity Cache",
             f"# device: {torch.cuda.get_device_name(dev)}",
             "# N  in out | fidelity us | grad (fid+grad+mean) us  ratio | grad (mean only) us  ratio | N + 1"]
    for cid in (2, 3, 5):
        N, a, b, ctrl, h0 = highfid_workload(cid, C=C)
        nbuf = int(np.ceil(300 * 2 ** 20 / (C * K * N * 24))) + 1
        gen = torch.Generator(device=dev).manual_seed(cid)
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
        t_all = timed(lambda d: be.mc_fidelity_grad(ct, d, N, a, b, h0_diag=h0))
        t_mean = timed(lambda d: be.mc_fidelity_grad(ct, d, N, a, b, h0_diag=h0, want=("mean",)))
        lines.append(f"{N:3d} {a:3d} {b:3d} | {t_f:9.1f} | {t_all:9.1f} {t_all / t_f:6.2f} | {t_mean:9.1f} {t_mean / t_f:6.2f} | {N + 1}")
        del bufs
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
