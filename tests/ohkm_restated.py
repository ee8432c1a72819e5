"""numpy float64 restatement of the joint MSE with online hard keypoint mining (TEST INFRASTRUCTURE), written from the definition
in include/mindpose_hip.h / DESIGN.md 4.17 and from nothing else:

  S[n,k]   = sum_i (pred_i - target_i)^2 * w[n,k]                                 (w absent = 1)
  order    : a NaN before every number (NaNs among themselves by index), then the larger S, then the lower joint index
  rank(k)  = #{j : S_j before S_k},   sel[n,k] = rank(k) < topk
  L        = sum_n sum_{k selected} S[n,k] / (N * topk * HW)
  dL/dpred = g * sel * w * 2 (pred - target) / (N * topk * HW)

The inputs are taken as they are (fp32 arrays are widened exactly); every sum and product is float64.
"""
import numpy as np


def row_sums(pred, target, weight=None):
    """S [N, K] float64."""
    d = np.asarray(pred, dtype=np.float64) - np.asarray(target, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        s = (d * d).reshape(d.shape[0], d.shape[1], -1)
        if weight is not None:
            s = s * np.asarray(weight, dtype=np.float64).reshape(d.shape[0], d.shape[1], 1)
        return s.sum(axis=2)


def before(sj, j, sk, k):
    """Does joint j with sum sj come before joint k with sum sk (j != k)?"""
    nj, nk = sj != sj, sk != sk
    if nj or nk:
        return bool(nj and (not nk or j < k))
    return bool(sj > sk or (sj == sk and j < k))


def select(s, topk):
    """sel [N, K] uint8 from row sums of any float type, by the rank statement (quadratic on purpose: no sort whose tie or NaN
    behaviour would have to be trusted)."""
    s = np.asarray(s)
    n, k = s.shape
    sel = np.zeros((n, k), dtype=np.uint8)
    for a in range(n):
        for i in range(k):
            rank = sum(1 for j in range(k) if j != i and before(s[a, j], j, s[a, i], i))
            sel[a, i] = rank < topk
    return sel


def select_fast(s, topk):
    """The same selection through a stable sort on (not NaN, -S), for the large-K cases; tests/test_ohkm_cpu.py holds it equal to
    ``select``."""
    s = np.asarray(s, dtype=np.float64)
    n, k = s.shape
    sel = np.zeros((n, k), dtype=np.uint8)
    for a in range(n):
        nan = np.isnan(s[a])
        key = np.where(nan, 0.0, -(s[a] + 0.0))  # + 0.0: -0.0 and +0.0 get one key
        order = np.lexsort((np.arange(k), key, ~nan))  # last key first: NaNs, then descending S, then index
        sel[a, order[:topk]] = 1
    return sel


def loss(s, sel, topk, hw):
    """L as float64 (the kernel's result is this, rounded to fp32); a selected non-finite sum makes it non-finite."""
    s = np.asarray(s, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        return float(np.where(sel.astype(bool), s, 0.0).sum() / (float(s.shape[0]) * topk * hw))


def grad(pred, target, weight, sel, topk, g=1.0):
    """dL/dpred [N, K, H, W] float64; rows that are not selected are exact zeros whatever they hold."""
    pred, target = np.asarray(pred, dtype=np.float64), np.asarray(target, dtype=np.float64)
    n, k = pred.shape[:2]
    hw = pred[0, 0].size
    c = np.full((n, k), 2.0 * g / (float(n) * topk * hw))
    if weight is not None:
        c = c * np.asarray(weight, dtype=np.float64).reshape(n, k)
    out = np.zeros(pred.shape, dtype=np.float64)
    on = sel.astype(bool)
    with np.errstate(invalid="ignore", over="ignore"):
        out[on] = (pred[on] - target[on]) * c[on][:, None, None]
    return out


def ohkm(pred, target, weight, topk, g=1.0):
    """(loss, S, sel, grad) of the definition."""
    s = row_sums(pred, target, weight)
    sel = select(s, topk) if s.shape[1] <= 160 else select_fast(s, topk)
    hw = np.asarray(pred)[0, 0].size
    return loss(s, sel, topk, hw), s, sel, grad(pred, target, weight, sel, topk, g)
