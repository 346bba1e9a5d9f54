#!/usr/bin/env python
"""What the batched L-BFGS step costs beside the gradient launch it consumes (MI355X; objective "mean", sigma = 0.05, shared draws):

  (a) the gradient launch alone (`mc_fidelity_grad_philox`, want = ("mean",)): the floor of an evaluation;
  (b) gradient launch + `backend.lbfgs_advance` (one kernel over all rows);
  (c) gradient launch + the same state machine as `torch` operations on the device (a transcription of lbfgs.py's `advance`).

Shapes 1000 x 1000 and 100 x 10 000 at N = 5 / 7 / 10.  Method: the three routes alternated in one process, 200 evaluations after
20, HIP events around the 200, three repeats (min .. max, us per evaluation).  The state machines run on live states: every route
restarts from the same start rows before its timed stretch, with gtol = 0 and a large maxiter, so that rows keep stepping.
Beside it: the value scripts/robust_lbfgs.py (SciPy L-BFGS-B, one row) reaches on the first shipped 0 -> 6 controller with the
evaluation budget the batched loop gives every row (printed, not asserted).

--box: instead of (c), the BOXED machine under the same protocol, alternated with (a) and (b) in the same process:

  (d) gradient launch + `backend.lbfgs_advance(bounds=...)` in the box [-W, W]^N x [T0 - 1, T0 + 0.5] around the start rows
      (--box-width W, default 0.35; biases U(-0.5, 0.5): at 0.35 three in ten start outside and are projected, so rows sit on bounds
      while they step; at 1.0 the bounds are touched rarely),

reported against (b) of the same run, with the number of rows still running at the end of (b) and of (d): a row that has ended is a
NaN row, which the gradient kernel skips, so a route with fewer running rows does less gradient work.

    python scripts/lbfgs_bench.py [--out profiles/lbfgs_bench.txt] [--evals 200] [--warm 20] [--repeats 3]
    python scripts/lbfgs_bench.py --box --out profiles/lbfgs_box_bench.txt"""
import argparse
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "scripts")):
    if p not in sys.path:
        sys.path.insert(0, p)


class TorchLBFGS:
    """lbfgs.py's `advance` on torch tensors (kind one_minus): the same selects and the same sequential sums, one torch operation
    each - the route a Python client without the kernel would take."""

    def __init__(self, x0, m=5, c1=1e-4, gtol=0.0, maxiter=10 ** 9, maxback=20):
        import torch
        self.t_ = torch
        C, n = x0.shape
        z = lambda *s: torch.zeros(s, dtype=torch.float64, device=x0.device)
        zi = lambda *s: torch.zeros(s, dtype=torch.int64, device=x0.device)
        self.m, self.c1, self.gtol, self.maxiter, self.maxback = m, c1, gtol, maxiter, maxback
        self.x, self.f, self.g, self.d, self.t, self.gd = x0.clone(), z(C), z(C, n), z(C, n), z(C), z(C)
        self.S, self.Y, self.sy = z(C, m, n), z(C, m, n), z(C, m)
        self.count, self.head, self.nback, self.iters, self.status = zi(C), zi(C), zi(C), zi(C), zi(C)
        self.first = torch.ones(C, dtype=torch.bool, device=x0.device)
        self.trial = x0.clone()
        self.ar = torch.arange(C, device=x0.device)

    @staticmethod
    def dot(a, b):
        acc = a[:, 0] * b[:, 0]
        for i in range(1, a.shape[1]):
            acc = acc + a[:, i] * b[:, i]
        return acc

    def first_step(self, g):
        r = 1.0 / self.t_.sqrt(self.dot(g, g))
        return self.t_.where(r < 1.0, r, self.t_.ones_like(r))

    def advance(self, mean):
        torch, m, ar = self.t_, self.m, self.ar
        ft, gt = 1.0 - mean[:, 0], -mean[:, 1:]
        run = self.status == 0
        first = run & self.first
        later = run & ~self.first
        self.first = self.first & ~first
        finite = torch.isfinite(ft) & torch.isfinite(gt).all(dim=1)
        start = first & finite
        self.status = torch.where(first & ~finite, 5, self.status)
        accept = later & torch.isfinite(ft) & (ft <= self.f + (self.c1 * self.t) * self.gd)
        reject = later & ~accept
        s, y = self.trial - self.x, gt - self.g
        ss, yy, sy = self.dot(s, s), self.dot(y, y), self.dot(s, y)
        store = accept & (sy > 0.0) & (sy >= (1e-10 * torch.sqrt(ss)) * torch.sqrt(yy))
        slot = self.head
        sel = store[:, None]
        self.S[ar, slot] = torch.where(sel, s, self.S[ar, slot])
        self.Y[ar, slot] = torch.where(sel, y, self.Y[ar, slot])
        self.sy[ar, slot] = torch.where(store, sy, self.sy[ar, slot])
        self.head = torch.where(store, (self.head + 1) % m, self.head)
        self.count = torch.where(store, torch.clamp(self.count + 1, max=m), self.count)
        moved = start | accept
        self.x = torch.where(moved[:, None], self.trial, self.x)
        self.f = torch.where(moved, ft, self.f)
        self.g = torch.where(moved[:, None], gt, self.g)
        self.iters = self.iters + accept
        gmax = self.g.abs().max(dim=1).values
        st1 = moved & (gmax <= self.gtol)
        st3 = accept & ~st1 & (self.iters >= self.maxiter)
        self.status = torch.where(st1, 1, torch.where(st3, 3, self.status))
        newdir = moved & (self.status == 0)
        q = self.g.clone()
        alpha = []
        for j in range(m):
            act = (newdir & (j < self.count))[:, None]
            slot = (self.head - 1 - j) % m
            a = (1.0 / self.sy[ar, slot]) * self.dot(self.S[ar, slot], q)
            q = torch.where(act, q - a[:, None] * self.Y[ar, slot], q)
            alpha.append(a)
        newest = (self.head - 1) % m
        h0 = self.sy[ar, newest] / self.dot(self.Y[ar, newest], self.Y[ar, newest])
        q = torch.where((newdir & (self.count > 0))[:, None], h0[:, None] * q, q)
        for j in range(m - 1, -1, -1):
            act = (newdir & (j < self.count))[:, None]
            slot = (self.head - 1 - j) % m
            b = (1.0 / self.sy[ar, slot]) * self.dot(self.Y[ar, slot], q)
            q = torch.where(act, q + (alpha[j] - b)[:, None] * self.S[ar, slot], q)
        dq = -q
        gdq = self.dot(self.g, dq)
        self.nback = torch.where(reject, self.nback + 1, self.nback)
        over = reject & (self.nback > self.maxback)
        reset = over & (self.count > 0)
        self.status = torch.where(over & (self.count == 0), 4, self.status)
        self.t = torch.where(reject & ~over, self.t * 0.5, self.t)
        quasi = newdir & (self.count > 0) & ~(gdq >= 0.0)
        steep = (newdir & ~quasi) | reset
        self.count = torch.where(steep, 0, self.count)
        self.head = torch.where(steep, 0, self.head)
        ds = -self.g
        self.d = torch.where(quasi[:, None], dq, torch.where(steep[:, None], ds, self.d))
        self.gd = torch.where(quasi, gdq, torch.where(steep, self.dot(self.g, ds), self.gd))
        self.t = torch.where(quasi, torch.ones_like(self.t), torch.where(steep, self.first_step(self.g), self.t))
        self.nback = torch.where(newdir | reset, 0, self.nback)
        going = run & (self.status == 0)
        self.trial = torch.where(going[:, None], self.x + self.t[:, None] * self.d, torch.full_like(self.x, float("nan")))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None)
    ap.add_argument("--evals", type=int, default=200)
    ap.add_argument("--warm", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--no-scipy", action="store_true")
    ap.add_argument("--box", action="store_true", help="time the boxed advance (d) beside (a) and (b) instead of the torch route (c)")
    ap.add_argument("--box-width", type=float, default=0.35)
    args = ap.parse_args()
    import torch
    import chain_checks as cc
    be = importlib.import_module("code-robchar_amd.backend")
    dev = be.compute_device()
    lines = [f"# per evaluation, us: (a) gradient launch alone, (b) + backend.lbfgs_advance, (c) + the state machine as torch operations; "
             f"objective mean, sigma = 0.05, shared draws, m = 5; {args.evals} evaluations after {args.warm}, routes alternated, "
             f"{args.repeats} repeats (min .. max), HIP events",
             "#  N      C       K | (a) grad us | (b) grad + advance us | (c) grad + torch us | (b)/(a) | (b)/(c) (of the minima) | (c) check"]
    if args.box:
        lines = [f"# per evaluation, us: (a) gradient launch alone, (b) + backend.lbfgs_advance, (d) + backend.lbfgs_advance(bounds=...), box "
                 f"[-{args.box_width}, {args.box_width}]^N x [T0 - 1, T0 + 0.5]; objective mean, sigma = 0.05, shared draws, m = 5; {args.evals} evaluations after "
                 f"{args.warm}, routes alternated, {args.repeats} repeats (min .. max), HIP events",
                 "#  N      C       K | (a) grad us | (b) grad + advance us | (d) grad + boxed advance us | (b)/(a) | (d)/(b) (of the minima) | "
                 "(d) entries on a bound; rows running at the end of (b), of (d)"]
    params = dict(gtol=0.0, maxiter=10 ** 9)

    def timed(step, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            step()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / n

    for N in (5, 7, 10):
        for C, K in ((1000, 1000), (100, 10000)):
            x0 = torch.from_numpy(cc.deloc_ctrl(np.random.default_rng(N), C, N, 0.5)).to(dev)
            grad = lambda ctrl: be.mc_fidelity_grad_philox(ctrl, K, N, 0, N - 1, 77, sigma=0.05, shared=True, want=("mean",))["mean"]
            ta, tb, tc = [], [], []
            check = ""
            for rep in range(args.repeats):
                timed(lambda: grad(x0), args.warm)
                ta.append(timed(lambda: grad(x0), args.evals))
                state, trial = be.lbfgs_init(x0, None, m=5)
                step_b = lambda: be.lbfgs_advance(state, trial, grad(trial), None, m=5, kind="one_minus", **params)
                timed(step_b, args.warm)
                tb.append(timed(step_b, args.evals))
                if args.box:
                    lo, hi = torch.full_like(x0, -args.box_width), torch.full_like(x0, args.box_width)
                    lo[:, N], hi[:, N] = x0[:, N] - 1.0, x0[:, N] + 0.5
                    bstate, btrial = be.lbfgs_init(x0, None, m=5, bounds=(lo, hi))
                    step_d = lambda: be.lbfgs_advance(bstate, btrial, grad(btrial), None, m=5, kind="one_minus", bounds=(lo, hi), **params)
                    timed(step_d, args.warm)
                    tc.append(timed(step_d, args.evals))
                    if rep == 0:
                        res = be.lbfgs_result(bstate, btrial, m=5, want=("x", "status"))
                        run_b = int((be.lbfgs_result(state, trial, m=5, want=("status",))["status"] == 0).sum())
                        check = (f"{int(((res['x'] == lo) | (res['x'] == hi)).sum())} of {res['x'].numel()}; "
                                 f"{run_b}, {int((res['status'] == 0).sum())} of {C}")
                    continue
                tm = TorchLBFGS(x0, m=5)
                step_c = lambda: tm.advance(grad(tm.trial))
                timed(step_c, args.warm)
                tc.append(timed(step_c, args.evals))
                if rep == 0:                      # the transcription follows the kernel (it sums in the same order)
                    fb = be.lbfgs_result(state, trial, m=5, want=("f",))["f"]
                    check = f"max |f_b - f_c| = {float((fb - tm.f).abs().max()):.1e}"
            fmt = lambda t: f"{min(t):8.1f} .. {max(t):8.1f}"
            last = min(tc) / min(tb) if args.box else min(tb) / min(tc)
            lines.append(f"  {N:2d} {C:6d} {K:7d} | {fmt(ta)} | {fmt(tb)} | {fmt(tc)} | {min(tb) / min(ta):6.3f} | {last:6.3f} | {check}")
            print(lines[-1], flush=True)
    if not args.no_scipy and not args.box:
        try:
            batched = importlib.import_module("robust_lbfgs_batched").run(rows=1, evals=60, verbose=False)
            scipy_run = importlib.import_module("robust_lbfgs").run(row=0, maxiter=60, train=1000, verbose=False, draws="philox")
            lines.append(f"# first shipped 0 -> 6 controller, 1 - mean F over 1000 shared draws: start {batched['start'][0]:.8f}; batched loop, "
                         f"60 evaluations: {batched['f'][0]:.8f} ({int(batched['evals'][0])} used); scripts/robust_lbfgs.py (SciPy L-BFGS-B, one "
                         f"row): {scipy_run['final']:.8f} after {scipy_run['launches']} launches")
        except ImportError as exc:
            lines.append(f"# SciPy comparison not run: {exc}")
        print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
