"""Bootstrap of the per-controller metrics: the DEFINITION of the device kernels behind `rc_bootstrap_metrics_f64_async`
(csrc/bootstrap_core.h, csrc/k_bootstrap.inc.h), in plain NumPy.  The product never runs this file on its hot path; it is what the
kernel is built to and what the tests' stand-in runs.

Input: `fid` (C, K) float64, `n_boot` = B >= 1 replicates, a 64-bit `seed`, `offset` (in Philox counters), thresholds thr[nq].

Index stream.  Philox4x32-10 (Salmon et al., SC'11) keyed by the seed, counter high words 0.  With Q = ceil(K / 4), draw t
(0 <= t < K) of replicate b of row c is output word `t & 3` of counter `offset + (c B + b) Q + (t >> 2)`, and
`idx = (word * K) >> 32`.  No rejection step: the bias, below K / 2^32, is part of the definition.  Row c of a C-row call equals
row 0 of a one-row call with `offset + c B Q`.

Replicate statistics.  m = the row's mean; over the K gathered values f and g = f - m:  S1 = sum g,  S2 = sum g^2,
    rim1 = 1 - (m + S1 / K),   std = sqrt(max(0, S2 / K - (S1 / K)^2))   (population),   min = min f,   q[i] = #{f >= thr[i]} / K.
Signs are those of `backend.reduce_metrics`: q and min positive.  A row holding any NaN gives NaN in every output.  The device
fixes a summation order (one wave per replicate); this file uses NumPy's, so sums agree to rounding and min and q K exactly.

Summary.  Per metric and row over the B replicates: mean, standard error (std with ddof = 1, NaN for B = 1) and the order
statistics of ranks `rank_lo`, `rank_hi` (0-based, ascending).  `ranks(n_boot, conf)` gives a = (1 - conf) / 2,
rank_lo = floor(a (B - 1)), rank_hi = ceil((1 - a) (B - 1)): NumPy's quantile methods "lower" and "higher".

Layouts: replicates (M, C, B), summary (M, 4, C), M = 3 + nq in the order rim1, std, min, q[0 .. nq)."""
from __future__ import annotations

import math

import numpy as np

FIXED_METRICS = ("rim1", "std", "min")
SUMMARY_FIELDS = ("mean", "se", "lower", "upper")
MAX_N_BOOT = 16384          # the row sort behind the summary (one launch)
LDS_MAX_K = 18432           # longest row of the LDS route

_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
_LOW = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def metric_names(nq: int):
    return FIXED_METRICS + tuple(f"q{i}" for i in range(int(nq)))


def philox4x32_10(ctr, seed: int):
    """The four output words, shape (4,) + ctr.shape uint32, of the uint64 counters `ctr` (counter high words 0) under key `seed`."""
    ctr = np.asarray(ctr, dtype=np.uint64)
    c0, c1 = ctr & _LOW, ctr >> _S32
    c2 = np.zeros_like(c0)
    c3 = np.zeros_like(c0)
    k0, k1 = int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = _M0 * c0, _M1 * c2                     # 32 x 32 -> 64 bits: no overflow
        c0, c1, c2, c3 = (p1 >> _S32) ^ c1 ^ np.uint64(k0), p1 & _LOW, (p0 >> _S32) ^ c3 ^ np.uint64(k1), p0 & _LOW
        k0, k1 = (k0 + _W0) & 0xFFFFFFFF, (k1 + _W1) & 0xFFFFFFFF
    return np.stack([c0, c1, c2, c3]).astype(np.uint32)


def quads(K: int) -> int:
    return (int(K) + 3) // 4


def indices(C: int, K: int, n_boot: int, seed: int, offset: int = 0):
    """(C, B, K) int64: the resampling indices of every replicate of every row."""
    C, K, B = int(C), int(K), int(n_boot)
    Q = quads(K)
    if int(offset) + C * B * Q > 2 ** 64:
        raise ValueError("offset + C * B * ceil(K / 4) wraps 2^64")
    start = [(int(offset) + r * Q) & (2 ** 64 - 1) for r in range(C * B)]
    with np.errstate(over="ignore"):
        ctr = np.array(start, dtype=np.uint64).reshape(C * B, 1) + np.arange(Q, dtype=np.uint64)[None, :]
    words = philox4x32_10(ctr, seed)                                                 # (4, C B, Q)
    words = np.moveaxis(words, 0, -1).reshape(C * B, 4 * Q)[:, :K]                   # draw t = 4 (t >> 2) + (t & 3)
    idx = (words.astype(np.uint64) * np.uint64(K)) >> _S32
    return idx.astype(np.int64).reshape(C, B, K)


def replicates(fid, n_boot: int, seed: int, offset: int = 0, q_thresholds=()):
    """(M, C, B) float64: every metric of every replicate."""
    fid = np.asarray(fid, dtype=np.float64)
    if fid.ndim != 2 or fid.shape[1] < 1:
        raise ValueError("fid: expected (C, K) with K >= 1")
    C, K = fid.shape
    B = int(n_boot)
    if B < 1:
        raise ValueError("n_boot must be positive")
    thr = np.asarray(q_thresholds, dtype=np.float64).reshape(-1)
    out = np.full((3 + thr.size, C, B), np.nan)
    if int(offset) + C * B * quads(K) > 2 ** 64:
        raise ValueError("offset + C * B * ceil(K / 4) wraps 2^64")
    for c in range(C):
        row = fid[c]
        if np.isnan(row).any():
            continue
        m = row.sum() / K
        f = row[indices(1, K, B, seed, int(offset) + c * B * quads(K))[0]]          # (B, K); a row's counters start at c B Q
        g = f - m
        mg = g.sum(axis=1) / K
        out[0, c] = 1.0 - (m + mg)
        out[1, c] = np.sqrt(np.maximum(0.0, (g * g).sum(axis=1) / K - mg * mg))
        out[2, c] = f.min(axis=1)
        for i, t in enumerate(thr):
            out[3 + i, c] = (f >= t).sum(axis=1) / K
    return out


def ranks(n_boot: int, conf: float):
    """(rank_lo, rank_hi) of the two-sided interval at level `conf`: np.quantile's "lower" at a and "higher" at 1 - a."""
    B, conf = int(n_boot), float(conf)
    if not 0.0 < conf < 1.0:
        raise ValueError("conf must be in (0, 1)")
    a = (1.0 - conf) / 2.0
    lo, hi = int(math.floor(a * (B - 1))), int(math.ceil((1.0 - a) * (B - 1)))
    return max(0, min(lo, B - 1)), max(0, min(hi, B - 1))


def summary(rep, rank_lo: int, rank_hi: int):
    """(M, 4, C) float64 from the replicates (M, C, B): mean, standard error, the two order statistics."""
    rep = np.asarray(rep, dtype=np.float64)
    M, C, B = rep.shape
    if not 0 <= rank_lo <= rank_hi < B:
        raise ValueError("ranks must satisfy 0 <= rank_lo <= rank_hi < B")
    out = np.empty((M, 4, C))
    out[:, 0] = rep.sum(axis=2) / B
    with np.errstate(invalid="ignore", divide="ignore"):
        out[:, 1] = np.sqrt(((rep - out[:, 0][:, :, None]) ** 2).sum(axis=2) / (B - 1)) if B > 1 else np.nan
    srt = np.sort(rep, axis=2)                           # (NaN rows are all NaN)
    out[:, 2] = srt[:, :, rank_lo]
    out[:, 3] = srt[:, :, rank_hi]
    return out


def bootstrap_metrics(fid, n_boot: int, seed: int, offset: int = 0, q_thresholds=(), conf: float = 0.95):
    """The whole definition: {"replicates" (M, C, B), "summary" (M, 4, C), "names"}."""
    thr = np.asarray(q_thresholds, dtype=np.float64).reshape(-1)
    rep = replicates(fid, n_boot, seed, offset, thr)
    lo, hi = ranks(n_boot, conf)
    return {"replicates": rep, "summary": summary(rep, lo, hi), "names": metric_names(thr.size)}
