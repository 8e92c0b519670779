"""Recommendation-list metrics on the device: the expensive parts of the
reference's metrics/accurate.py and metrics/diversity.py as HIP kernels (csrc/metrics.hip).

hit_flags           `item in items` labels (accurate.py:24-31, :69-76)   lg_rec_hits
accuracy            P / R / NDCG, fp64 on the device (accurate.py:11-102)
pair_overlap        sum_{u != v} |R_u & R_v|, exact (diversity.py:15-63)  lg_rec_pair_overlap
hamming             calHammingDistance's value, unrounded
intra_similarity    calInternalSimilarity's value, unrounded             lg_rec_intra_similarity_f64
                    (diversity.py:66-115)
rank_metrics        MRR, mean rank, AUC and P / R / NDCG at any cut-offs from full-catalog ranks
                    (ops.score_rank, lg_score_rank_f32; ops.spread_rank, lg_rows_rank_f64, with
                    n_pool= for rankings that drop exclusions); plain torch on the ranks' device

The reference-signature wrappers (dicts, numpy matrices, 5-decimal rounding, float32 torch
reductions) are metrics/accurate.py and metrics/diversity.py of this package.
No CPU fallback: GPU tensors only (rank_metrics, a few reductions over [nnz] integers, runs where
its ranks are).
"""
from __future__ import annotations

import torch

from . import _native as N
from .graph import RowSets


def _recs(recs: torch.Tensor) -> torch.Tensor:
    N.require_gpu(recs, "recs")
    if recs.dim() != 2:
        raise ValueError(f"recs must be [n_users, k], got shape {tuple(recs.shape)}")
    return recs.to(torch.int64).contiguous()


def hit_flags(recs: torch.Tensor, eval_rows: torch.Tensor, pos: RowSets) -> torch.Tensor:
    """uint8 [n_eval, k]: recs[eval_rows[q]][p] in row q of ``pos`` (one row per evaluated
    user, in eval_rows order)."""
    recs = _recs(recs)
    eval_rows = eval_rows.to(recs.device, torch.int64).contiguous()
    n_eval, k = int(eval_rows.numel()), recs.shape[1]
    if pos.n_rows != n_eval:
        raise ValueError(f"pos has {pos.n_rows} rows for {n_eval} evaluated users")
    if n_eval and (int(eval_rows.min()) < 0 or int(eval_rows.max()) >= recs.shape[0]):
        raise IndexError("evaluated user outside the recommendation matrix")
    hit = torch.empty((n_eval, k), dtype=torch.uint8, device=recs.device)
    N.check(N.lib().lg_rec_hits(N.ptr(recs), recs.shape[0], k, N.ptr(eval_rows), n_eval,
                                N.ptr(pos.rowptr), N.ptr(pos.col), N.ptr(hit),
                                N.stream_handle(recs.device)), "lg_rec_hits")
    return hit


def accuracy(recs: torch.Tensor, test: RowSets, k: int | None = None) -> dict:
    """Precision, recall and NDCG over the users with at least one test item (``test``: one
    sorted row per user of recs), in fp64 (the reference computes them in fp32 torch).
    NDCG keeps the reference's ideal DCG of k ones (accurate.py:80-89)."""
    recs = _recs(recs)
    k = recs.shape[1] if k is None else int(k)
    deg = test.degrees()
    eval_rows = torch.nonzero(deg > 0).flatten()
    # the non-empty rows ascending: their compacted row pointers are rowptr[eval_rows] + end
    pos = RowSets(torch.cat([test.rowptr[eval_rows], test.rowptr[-1:]]), test.col,
                  int(eval_rows.numel()), test.n_cols)
    hit = hit_flags(recs, eval_rows, pos).to(torch.float64)
    w = 1.0 / torch.log2(torch.arange(2, recs.shape[1] + 2, dtype=torch.float64,
                                      device=recs.device))
    n = hit.sum(1)
    idcg = float(w[:min(k, recs.shape[1])].sum())  # ones in the first min(len, k) slots
    return {"precision": float(n.mean()) / k, "recall": float((n / deg[eval_rows]).mean()),
            "ndcg": float(((hit * w).sum(1) / (idcg if idcg else 1.0)).mean()),
            "n_eval": int(eval_rows.numel())}


def pair_overlap(recs: torch.Tensor, n_items: int | None = None) -> int:
    """sum over ordered user pairs u != v of |set(R_u) & set(R_v)| (exact integer)."""
    recs = _recs(recs)
    if n_items is None:
        n_items = int(recs.max()) + 1 if recs.numel() else 0
    counts = torch.empty(max(1, n_items), dtype=torch.int32, device=recs.device)
    total = torch.zeros(1, dtype=torch.int64, device=recs.device)
    N.check(N.lib().lg_rec_pair_overlap(N.ptr(recs), recs.shape[0], recs.shape[1], n_items,
                                        N.ptr(counts), N.ptr(total),
                                        N.stream_handle(recs.device)), "lg_rec_pair_overlap")
    return int(total.item())


def hamming(recs: torch.Tensor, k: int, n_items: int | None = None) -> float:
    """calHammingDistance's mean over ordered user pairs of 1 - overlap / k (unrounded)."""
    U = recs.shape[0]
    pairs = U * (U - 1)
    s = pair_overlap(recs, n_items)
    return (pairs - s / k) / pairs  # ZeroDivisionError for one user, as the reference


def intra_similarity_parts(recs: torch.Tensor, by_item: RowSets,
                           item_degree: torch.Tensor) -> torch.Tensor:
    """fp64 [n_users * k]: per (user, position p) the sum over later positions of the
    item-pair similarity co(a, b) / sqrt(k_a k_b)."""
    recs = _recs(recs)
    item_degree = item_degree.to(recs.device, torch.int64).contiguous()
    if item_degree.numel() != by_item.n_rows:
        raise ValueError("item_degree must have one entry per item column")
    part = torch.empty(recs.numel(), dtype=torch.float64, device=recs.device)
    N.check(N.lib().lg_rec_intra_similarity_f64(
        N.ptr(recs), recs.shape[0], recs.shape[1], N.ptr(by_item.rowptr), N.ptr(by_item.col),
        N.ptr(item_degree), by_item.n_rows, N.ptr(part), N.stream_handle(recs.device)),
        "lg_rec_intra_similarity_f64")
    return part


def intra_similarity(recs: torch.Tensor, by_item: RowSets, item_degree: torch.Tensor,
                     k: int) -> float:
    """calInternalSimilarity (unrounded): every unordered pair counted twice, as the
    reference's ordered double loop does."""
    total = 2.0 * float(intra_similarity_parts(recs, by_item, item_degree).sum())
    return total / (recs.shape[0] * k * (k - 1))



def rank_metrics(rank: torch.Tensor, targets: RowSets, n_items: int, ks=(20,),
                 n_pool: torch.Tensor | None = None) -> dict:
    """Ranking metrics from the full-catalog ranks of held-out items (ops.score_rank,
    ops.rows_rank, ops.spread_rank, or ops.spread_rank_tiled where the dense spreading
    matrices do not fit): `rank`
    int64 [nnz] aligned with targets.col (0 = first, -1 = not ranked), one row of `targets` per
    user. Plain torch on rank's device, fp64. Targets with rank -1 are left out and counted in
    n_skipped; users left with no target are not averaged. With n_t a user's evaluated targets:

    mrr           mean over users of 1 / (1 + the user's best rank)
    mean_rank     mean over all evaluated targets of rank
    auc           mean over users of 1 - mean_i((rank_i - a_i) / (n_items - n_t)), a_i the number of
                  the user's own targets ranked above i: the share of (target, other item) pairs
                  the model orders correctly. n_pool (an int64 / fp64 [rows] tensor: the columns
                  that rank for each user) replaces n_items in the denominator, n_pool - n_t: a
                  ranking that DROPS a user's exclusions (ops.rows_rank, ops.spread_rank,
                  ops.spread_rank_tiled with drop=True) ranks n_items - |excl row| columns, and n_items would count the
                  dropped ones as correctly ordered pairs. None: n_items, bit for bit as before.
    precision@k, recall@k, ndcg@k for every k in ks, from rank < k with metrics.accuracy's
                  definitions (hits / k, hits / n_t, DCG over the ideal DCG of k ones)
    n_eval        the users averaged over."""
    n_items = int(n_items)
    rank = rank.reshape(-1).to(torch.int64)
    dev = rank.device
    rp = targets.rowptr.to(dev)
    R = targets.n_rows
    if int(rank.numel()) != int(targets.col.numel()):
        raise ValueError(f"{int(rank.numel())} ranks for {int(targets.col.numel())} targets")
    if n_pool is not None:
        if not isinstance(n_pool, torch.Tensor) or n_pool.dtype not in (torch.int64,
                                                                        torch.float64):
            raise TypeError("n_pool must be an int64 or float64 tensor")
        if tuple(n_pool.shape) != (R,):
            raise ValueError(f"n_pool must have shape ({R},), got {tuple(n_pool.shape)}")
        n_pool = n_pool.to(dev, torch.float64)
    pos = torch.arange(rank.numel(), dtype=torch.int64, device=dev)
    row = torch.searchsorted(rp, pos, right=True) - 1
    inside = (row >= 0) & (row < R)
    ok = inside & (rank >= 0)
    out = {"n_skipped": int((inside & (rank < 0)).sum())}
    row, rk = row[ok], rank[ok]
    n_t = torch.bincount(row, minlength=R).to(torch.float64)
    ev = n_t > 0
    n_eval = int(ev.sum())
    out["n_eval"] = n_eval
    names = ["mrr", "mean_rank", "auc"] + [f"{m}@{int(k)}" for k in ks
                                           for m in ("precision", "recall", "ndcg")]
    if n_eval == 0:
        out.update({n: float("nan") for n in names})
        return out
    f64 = rk.to(torch.float64)
    zeros = torch.zeros(R, dtype=torch.float64, device=dev)

    def user_mean(per_user):
        return float(per_user[ev].mean())

    best = torch.full((R,), n_items, dtype=torch.int64, device=dev)
    best.scatter_reduce_(0, row, rk, "amin")
    out["mrr"] = user_mean(1.0 / (1.0 + best.to(torch.float64)))
    out["mean_rank"] = float(f64.mean())
    # a_i: the position of i among its user's targets by rank
    order = torch.argsort(row * (n_items + 1) + rk)
    first = torch.cumsum(n_t, 0) - n_t  # the first sorted position of every user
    a = torch.empty_like(f64)
    a[order] = torch.arange(rk.numel(), dtype=torch.float64, device=dev) - first[row[order]]
    others = ((n_items if n_pool is None else n_pool) - n_t).clamp(min=1.0)
    out["auc"] = user_mean(1.0 - zeros.index_add(0, row, (f64 - a) / others[row])
                           / n_t.clamp(min=1.0))
    gain = 1.0 / torch.log2(f64 + 2.0)
    for k in ks:
        k = int(k)
        hit = (rk < k).to(torch.float64)
        n = zeros.index_add(0, row, hit)
        idcg = float((1.0 / torch.log2(torch.arange(2, k + 2, dtype=torch.float64))).sum())
        out[f"precision@{k}"] = user_mean(n) / k
        out[f"recall@{k}"] = user_mean(n / n_t.clamp(min=1.0))
        out[f"ndcg@{k}"] = user_mean(zeros.index_add(0, row, hit * gain) / (idcg if idcg else 1.0))
    return out
