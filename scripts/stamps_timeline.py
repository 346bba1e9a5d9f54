#!/usr/bin/env python3
"""Timeline of ONE launch of the fidelity kernel, per compute unit, from the per-wave stamps of a diagnostic build
(`scripts/build_variant.sh stamps -DRC_STAMPS -DRC_DEV_FEW_N`, then scripts/stamps.py with DUMP=...): how long the pipeline takes to
fill (the first round of waves all ask for their draws at once), how long a wave lives alone and in a crowd, how long the drain is.
s_memtime counts per CU (the 256 counters are not synchronised), so tiles are grouped by counter base: a group of 58 ... 64 tiles
(15 700 / 256 = 61.3) is ONE compute unit; groups whose bases happen to lie close together are skipped.  Host-only: reads the .npy.

usage: python3 scripts/stamps_timeline.py gpurun_out/<label>/stamps_n7.npy [--ghz 1.95]
columns of the dump (per tile): 0 begin, 1 staged, 2 end (s_memtime ticks), 3 realtime ticks of the wave (100 MHz), 4 ctrl row read,
5 first staging phase landed, 6 QL starts, 7 QL done, 8 HW_ID (wave slot [3:0], SIMD [5:4], CU [11:8], SH [12], SE [15:13]),
9 XCC_ID (XCD [3:0]), 10 / 11 begin / end on the chip-wide 100 MHz clock (comparable between units and between launches)

With columns 8 .. 11 (records indexed by tile) a second part follows - the DRAIN per SIMD: waves of a compute unit are told apart
by the hardware ids instead of by counter base, and for every unit the resident and computing waves of each of its four SIMDs over
the last 12 us, the end time of each SIMD, the spread of the units' end times over the chip and, from a dump of two back-to-back
launches, the gap between the last unit's end and the next launch's first wave.
"""
import sys
import numpy as np

raw = np.load(sys.argv[1]).astype(np.int64)
both = raw if raw.ndim == 3 else raw[None]             # (launches, tiles, slots): scripts/stamps.py dumps two back-to-back launches
s = both[0]
life_us = s[:, 3] / 100.0
tick = float(np.median((s[:, 2] - s[:, 0]) / np.maximum(life_us, 1e-9)))          # ticks per us, from the waves' own realtime
if "--ghz" in sys.argv:
    tick = float(sys.argv[sys.argv.index("--ghz") + 1]) * 1e3
idx = np.argsort(s[:, 0])
cut = np.where(np.diff(s[idx, 0]) > 300000)[0]
bounds = np.concatenate([[0], cut + 1, [len(idx)]])
cus = [idx[bounds[i]:bounds[i + 1]] for i in range(len(bounds) - 1) if 58 <= bounds[i + 1] - bounds[i] <= 64]
print(f"{len(s)} tiles, {len(bounds) - 1} counter groups, {len(cus)} of them single compute units; {tick / 1e3:.3f} GHz tick rate")
agg = []
for seg in cus:
    t0 = s[seg, 0].min()
    seg = seg[np.argsort(s[seg, 0])]
    agg.append(((s[seg, 0] - t0) / tick, (s[seg, 1] - t0) / tick, (s[seg, 2] - t0) / tick))
med = lambda f: float(np.median([f(a) for a in agg]))
print(f"per compute unit (medians over the {len(agg)}): {med(lambda a: len(a[0])):.0f} tiles, launch span {med(lambda a: a[2].max()):.1f} us")
print(f"  fill : the first 16 waves begin within {med(lambda a: a[0][15]):.2f} us; their draws are staged after {med(lambda a: np.median(a[1][:16] - a[0][:16])):.2f} us "
      f"(slowest {med(lambda a: (a[1][:16] - a[0][:16]).max()):.2f}); later waves: {med(lambda a: np.median((a[1] - a[0])[20:])):.2f} us")
print(f"  first wave computing at {med(lambda a: a[1].min()):.2f} us, 8 of 16 at {med(lambda a: np.sort(a[1][:16])[7]):.2f} us, all 16 at {med(lambda a: np.sort(a[1][:16])[15]):.2f} us")
print(f"  compute phase of a wave: first four staged (alone on their SIMDs) {med(lambda a: np.median((a[2] - a[1])[np.argsort(a[1][:16])[:4]])):.2f} us, "
      f"steady state (4 per SIMD) {med(lambda a: np.median((a[2] - a[1])[20:45])):.2f} us, last ten {med(lambda a: np.median((a[2] - a[1])[-10:])):.2f} us")
print(f"  drain: the last wave begins at {med(lambda a: a[0].max()):.1f} us, the unit ends at {med(lambda a: a[2].max()):.1f} us")
tgrid = np.arange(0.0, max(a[2].max() for a in agg) + 2.0, 2.0)
print("  t_us   resident  staging  computing   (waves per compute unit, mean over the units)")
for t in tgrid:
    res = np.mean([((a[0] <= t) & (a[2] > t)).sum() for a in agg])
    stg = np.mean([((a[0] <= t) & (a[1] > t)).sum() for a in agg])
    print(f"  {t:5.1f}  {res:8.1f}  {stg:7.1f}  {res - stg:9.1f}")
steady = np.mean([np.mean([((a[1] <= t) & (a[2] > t)).sum() for t in np.arange(14.0, 34.0, 1.0)]) for a in agg])
area = np.mean([(a[2] - a[1]).sum() for a in agg])
span = med(lambda a: a[2].max())
print(f"  computing waves in steady state {steady:.1f} per unit; compute-time integral / (span x steady) = {area / (span * steady):.3f} "
      f"-> {span * (1 - area / (span * steady)):.1f} us of the {span:.1f} us span are fill + drain")

# ------------------------------------------------------------------------------------------------------------------------
# the drain per SIMD (columns 8 .. 11)
# ------------------------------------------------------------------------------------------------------------------------
if s.shape[1] < 12:
    sys.exit(0)


def units_of(rec):
    """{(xcd, se, sh, cu): rows of that compute unit}, times in us: within a unit from its own s_memtime counter"""
    hw, xcc = rec[:, 8], rec[:, 9] & 0xf
    key = (xcc << 8) | (((hw >> 13) & 7) << 5) | (((hw >> 12) & 1) << 4) | ((hw >> 8) & 0xf)
    out = {}
    for k in np.unique(key):
        rows = np.where(key == k)[0]
        out[int(k)] = rows
    return out


hw = s[:, 8]
simd = (hw >> 4) & 3
units = units_of(s)
r0 = s[:, 10].min()
print(f"\ndrain per SIMD: {len(units)} compute units by hardware id, {np.mean([len(v) for v in units.values()]):.1f} tiles each "
      f"(min {min(len(v) for v in units.values())}, max {max(len(v) for v in units.values())})")
rel = np.arange(-12.0, 0.01, 1.0)
res_rank, cmp_rank, res_simd = [], [], []
simd_end, lone, last_begin, tiles_simd = [], [], [], []
unit_end_rt = []
for rows in units.values():
    t0 = s[rows, 0].min()
    b, l, e = ((s[rows, c] - t0) / tick for c in (0, 1, 2))
    sd = simd[rows]
    end = e.max()
    unit_end_rt.append((s[rows, 11].max() - r0) / 100.0)
    res = np.array([[((b <= end + t) & (e > end + t) & (sd == q)).sum() for q in range(4)] for t in rel])
    cmp_ = np.array([[((l <= end + t) & (e > end + t) & (sd == q)).sum() for q in range(4)] for t in rel])
    res_simd.append(res)
    res_rank.append(-np.sort(-res, axis=1))
    cmp_rank.append(-np.sort(-cmp_, axis=1))
    ends = np.array([e[sd == q].max() if (sd == q).any() else 0.0 for q in range(4)])
    simd_end.append(np.sort(ends) - end)                # <= 0: how long before the unit's end each SIMD (by rank) went idle
    tiles_simd.append(np.sort([(sd == q).sum() for q in range(4)]))
    last_begin.append(end - b.max())
    # time a SIMD spends with exactly ONE resident wave before its own end (a lone wave runs at the dependent-issue rate)
    lo = []
    for q in range(4):
        bq, eq = np.sort(b[sd == q]), np.sort(e[sd == q])
        if len(eq) >= 2:
            lo.append(eq[-1] - max(eq[-2], bq[-1]))
    lone.append(np.mean(lo) if lo else 0.0)
res_rank, cmp_rank, res_simd = np.mean(res_rank, axis=0), np.mean(cmp_rank, axis=0), np.mean(res_simd, axis=0)
print("  waves per SIMD over the last 12 us of a unit (mean over the units; SIMDs of a unit ordered busiest first at each time)")
print("  t - end   resident: busiest .. idlest      computing: busiest .. idlest      resident by SIMD id 0 .. 3")
for i, t in enumerate(rel):
    print(f"  {t:6.1f}    " + " ".join(f"{v:5.2f}" for v in res_rank[i]) + "        " + " ".join(f"{v:5.2f}" for v in cmp_rank[i])
          + "        " + " ".join(f"{v:5.2f}" for v in res_simd[i]))
simd_end = np.array(simd_end)
spread = -simd_end[:, 0]
print("  end of each SIMD before the end of its unit, us (SIMDs ordered first-idle .. last; median / p90 over the units): "
      + "  ".join(f"{np.median(simd_end[:, q]):.2f} / {np.percentile(simd_end[:, q], 10):.2f}" for q in range(4)))
print(f"  spread of the four SIMD end times of a unit: median {np.median(spread):.2f} us, p90 {np.percentile(spread, 90):.2f}, max {spread.max():.2f}; "
      f"mean idle SIMD time before the unit's end {np.median(-simd_end.mean(axis=1)):.2f} us (median unit)")
ts = np.array(tiles_simd)
print(f"  tiles per SIMD of a unit (fewest .. most, mean over the units): " + " ".join(f"{v:.1f}" for v in ts.mean(axis=0)))
print(f"  last wave of a unit begins {np.median(last_begin):.2f} us before the unit ends (median); a SIMD's final wave is alone on it "
      f"for {np.median(lone):.2f} us (median unit, mean of its SIMDs; p90 {np.percentile(lone, 90):.2f})")
ue = np.array(unit_end_rt)
print(f"  unit end times over the chip (us after the launch's first wave, 100 MHz clock): min {ue.min():.2f}  p10 {np.percentile(ue, 10):.2f}  "
      f"median {np.median(ue):.2f}  p90 {np.percentile(ue, 90):.2f}  max {ue.max():.2f}   -> last - median {ue.max() - np.median(ue):.2f} us, "
      f"last - first {ue.max() - ue.min():.2f} us")
first_begin = np.array([(s[rows, 10].min() - r0) / 100.0 for rows in units.values()])
print(f"  first wave of a unit begins (us after the launch's first wave): median {np.median(first_begin):.2f}  p90 {np.percentile(first_begin, 90):.2f}  "
      f"max {first_begin.max():.2f}")
if both.shape[0] >= 2:
    s2 = both[1]
    gap = (s2[:, 10].min() - s[:, 11].max()) / 100.0
    idle_from_median = (s2[:, 10].min() - r0) / 100.0 - np.median(ue)
    print(f"  next launch: its first wave begins {gap:.2f} us after this launch's last wave ended (kernel end + dispatch), "
          f"{idle_from_median:.2f} us after the median unit ended; launch period {(s2[:, 10].min() - r0) / 100.0:.2f} us")
