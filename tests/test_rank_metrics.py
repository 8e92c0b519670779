"""lgcnhs.metrics.rank_metrics on hand-made ranks (CPU tensors: the function is plain torch on
its ranks' device): MRR, mean rank, AUC with its own-targets correction, and precision / recall /
NDCG at several cut-offs against metrics.accuracy's formulas restated in numpy on recommendation
lists built from the same ranks."""
import math

import numpy as np
import pytest
import torch


def _targets(lists, n_items):
    from lgcnhs.graph import RowSets
    rp = np.zeros(len(lists) + 1, np.int64)
    rp[1:] = np.cumsum([len(x) for x in lists])
    col = np.concatenate([np.asarray(x, np.int64) for x in lists] + [np.zeros(0, np.int64)])
    return RowSets(torch.as_tensor(rp), torch.as_tensor(col.astype(np.int32)), len(lists),
                   n_items)


def _metrics(ranks, lists, n_items, ks):
    from lgcnhs.metrics import rank_metrics
    flat = [r for row in ranks for r in row]
    return rank_metrics(torch.tensor(flat, dtype=torch.int64), _targets(lists, n_items), n_items,
                        ks)


def test_one_user_by_hand():
    """Targets at ranks {0, 3, 10} over 100 items (given out of order): every number worked out
    here. AUC: the three targets have 0, 1 and 2 own targets above them, so 0, 2 and 8 of the 97
    other items are above them."""
    m = _metrics([[3, 10, 0]], [[7, 20, 55]], 100, (5, 20, 1))
    assert m["n_eval"] == 1 and m["n_skipped"] == 0
    assert m["mrr"] == 1.0
    assert m["mean_rank"] == pytest.approx(13 / 3, abs=1e-12)
    assert m["auc"] == pytest.approx(1 - (0 + 2 + 8) / 3 / 97, abs=1e-12)
    idcg5 = sum(1 / math.log2(p + 2) for p in range(5))
    idcg20 = sum(1 / math.log2(p + 2) for p in range(20))
    assert m["precision@5"] == pytest.approx(2 / 5, abs=1e-12)
    assert m["recall@5"] == pytest.approx(2 / 3, abs=1e-12)
    assert m["ndcg@5"] == pytest.approx((1 + 1 / math.log2(5)) / idcg5, abs=1e-12)
    assert m["precision@20"] == pytest.approx(3 / 20, abs=1e-12)
    assert m["recall@20"] == pytest.approx(1.0, abs=1e-12)
    assert m["ndcg@20"] == pytest.approx(
        (1 + 1 / math.log2(5) + 1 / math.log2(12)) / idcg20, abs=1e-12)
    assert m["precision@1"] == 1.0 and m["ndcg@1"] == 1.0
    assert m["recall@1"] == pytest.approx(1 / 3, abs=1e-12)


def test_auc_counts_own_targets_out():
    """A user whose n_t targets hold the first n_t ranks has AUC 1, the last n_t ranks AUC 0 --
    without a_i neither would be exact; one target at rank r of n items: 1 - r / (n - 1)."""
    n = 50
    assert _metrics([[2, 0, 1]], [[4, 5, 6]], n, ())["auc"] == 1.0
    assert _metrics([[n - 1, n - 3, n - 2]], [[4, 5, 6]], n, ())["auc"] == pytest.approx(0.0,
                                                                                       abs=1e-15)
    assert _metrics([[7]], [[9]], n, ())["auc"] == pytest.approx(1 - 7 / 49, abs=1e-15)
    # two users: the mean of their AUCs, not of their targets'
    m = _metrics([[0, 1], [10]], [[1, 2], [3]], n, ())
    assert m["auc"] == pytest.approx((1.0 + (1 - 10 / 49)) / 2, abs=1e-15)
    assert m["mrr"] == pytest.approx((1.0 + 1 / 11) / 2, abs=1e-15)
    assert m["mean_rank"] == pytest.approx(11 / 3, abs=1e-15)


def test_skipped_targets_and_empty_users():
    """rank -1 is left out (and counted); a user without targets, or with skipped ones only, is
    not averaged: the numbers are those of the remaining users alone."""
    lists = [[], [3, 8], [5], [], [1, 2, 9]]
    ranks = [[], [4, -1], [-1], [], [0, 30, 2]]
    m = _metrics(ranks, lists, 40, (3, 10))
    ref = _metrics([[4], [0, 30, 2]], [[3], [1, 2, 9]], 40, (3, 10))
    assert m["n_skipped"] == 2 and ref["n_skipped"] == 0
    assert m["n_eval"] == ref["n_eval"] == 2
    for key, v in ref.items():
        if key != "n_skipped":
            assert m[key] == pytest.approx(v, abs=1e-15), key
    assert m["mrr"] == pytest.approx((1 / 5 + 1.0) / 2, abs=1e-15)
    # nothing to evaluate: counts, and NaN for every mean
    e = _metrics([[-1], []], [[2], []], 40, (3,))
    assert e["n_eval"] == 0 and e["n_skipped"] == 1
    assert all(math.isnan(e[key]) for key in ("mrr", "mean_rank", "auc", "recall@3"))
    from lgcnhs.metrics import rank_metrics
    with pytest.raises(ValueError, match="ranks"):
        rank_metrics(torch.zeros(3, dtype=torch.int64), _targets([[1]], 40), 40)


def _accuracy_numpy(recs, lists, k):
    """metrics.accuracy's formulas on a [U, k] list: users with a test item; hits / k, hits /
    degree, DCG over the ideal DCG of k ones."""
    w = 1.0 / np.log2(np.arange(2, k + 2, dtype=np.float64))
    idcg = w.sum()
    p, r, g = [], [], []
    for row, items in zip(recs, lists):
        if len(items) == 0:
            continue
        hit = np.isin(row, items).astype(np.float64)
        p.append(hit.sum())
        r.append(hit.sum() / len(items))
        g.append((hit * w).sum() / idcg)
    return np.mean(p) / k, np.mean(r), np.mean(g)


@pytest.mark.parametrize("k", [1, 5, 20, 64])
def test_cutoff_metrics_are_accuracys(k):
    """Random distinct ranks per user over 300 items: the list a top-k run would give holds a
    user's target at position rank for every rank < k; accuracy's formulas on that list equal
    rank_metrics' from the ranks alone."""
    rng = np.random.default_rng(5)
    n_items, U = 300, 40
    lists, ranks, recs = [], [], []
    for u in range(U):
        n = int(rng.integers(0, 9)) if u % 7 else 0
        items = np.sort(rng.permutation(n_items)[:n])
        rk = rng.permutation(min(n_items, 3 * k + 10))[:n]  # distinct; about a third below k
        others = np.setdiff1d(np.arange(n_items), items)
        row = others[:k].copy()  # non-targets everywhere ...
        for it, r in zip(items, rk):
            if r < k:
                row[r] = it      # ... but at the targets' ranks
        lists.append(items)
        ranks.append(rk.tolist())
        recs.append(row)
    m = _metrics(ranks, lists, n_items, (k,))
    p, r, g = _accuracy_numpy(recs, lists, k)
    assert m["n_eval"] == sum(1 for x in lists if len(x))
    assert m[f"precision@{k}"] == pytest.approx(p, abs=1e-12)
    assert m[f"recall@{k}"] == pytest.approx(r, abs=1e-12)
    assert m[f"ndcg@{k}"] == pytest.approx(g, abs=1e-12)
