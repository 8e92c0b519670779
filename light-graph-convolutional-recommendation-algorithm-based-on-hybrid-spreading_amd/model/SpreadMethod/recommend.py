"""Spreading recommenders with the reference's interface
(reference model/SpreadMethod/recommend.py:18-115).

recommendSpreadMethod runs entirely on the GPU from the DataFrames: sparse A, general_W,
W (with the reference's per-method lambda / transpose overrides), then F = A @ W block by
block fused into the filtered top-k — F is never brought to the host. Ties are ordered
(value desc, item asc) where the reference's np.argsort leaves them unspecified.
"""
from collections import defaultdict

import numpy as np
import pandas as pd
import torch

from const import cfg
from lgcnhs import ops
from lgcnhs.graph import RowSets
from lgcnhs.recs import topk_to_dict, exclusion_from_dfs, gpu_device, save_recs


def _save(recs: dict) -> None:
    save_recs(recs, cfg.RECOMMEND["save_path"] + "all_user_recommend_dict_" + cfg.MODEL["name"]
              + "_" + str(cfg.RECOMMEND["k"]) + ".npy")


def _unfiltered() -> bool:
    # reference :49-50: movielens + ProbS returns sorted_items[:k] without the filter
    return cfg.DATA_SET == "movielens" and cfg.MODEL["name"] == "ProbS"


def _to_dict(idx: torch.Tensor, user_num: int) -> dict:
    return topk_to_dict(idx, user_num, defaultdict)


def recommendForAllUser(F_new: np.ndarray, user_num: int, train_data_df: pd.DataFrame,
                        val_data_df: pd.DataFrame, k: int) -> dict:
    """Per user: the k best items by F_new not in train|val (reference :18-56). k in
    [1, 1024]: lg_rows_topk_f64 up to 128, lg_rows_topk_wide_f64 above (the reference's [:k]
    takes any k; larger k raises ValueError)."""
    dev = gpu_device()
    F = torch.as_tensor(np.ascontiguousarray(F_new[:user_num]), dtype=torch.float64).to(dev)
    excl = exclusion_from_dfs(user_num, F.shape[1], train_data_df, val_data_df, device=dev)
    _, idx = ops.rows_topk(F, k, excl, drop=not _unfiltered())
    recs = _to_dict(idx, user_num)
    _save(recs)
    return recs


def spread_method_topk(user_num: int, item_num: int, train_data_df: pd.DataFrame,
                       val_data_df: pd.DataFrame, method: str, lambda_val: float,
                       dataset: str, k: int, unfiltered: bool = False, device=None,
                       tiled: bool | None = None, users=None, items=None):
    """Device (values, items) of the whole spreading recommendation. k in [1, 1024]; above
    128 the dense path takes lg_rows_topk_wide_f64 and the tiled path peels ceil(k / 128)
    walks (ops.spread_topk_tiled). ``users`` (ids, tensor or list): only those users' rows,
    in that order (ops.spread_recommend). ``items`` (ids, a bool mask or an ascending device
    tensor: ops.item_candidates): rank only those items -- the spreading still runs over the
    whole graph -- with real item ids in the lists (ops.spread_recommend)."""
    dev = device or gpu_device()
    both = pd.concat([train_data_df, val_data_df])
    inter = ops.Interactions.from_pairs(
        torch.from_numpy(both["user_id"].to_numpy(np.int64)),
        torch.from_numpy(both["item_id"].to_numpy(np.int64)), user_num, item_num, dev)
    transpose = False
    if method == "ProbS" and dataset == "movielens":  # reference :87-91
        lambda_val, transpose = 0.01, True
    elif method == "HeatS" and dataset == "douban":  # reference :97-101
        lambda_val, transpose = 0.99, True
    excl = inter.by_user  # train|val positives == the nonzeros of A
    # dense I x I general_W / W when they fit, else the factored tile path (same values within a few ulp)
    return ops.spread_recommend(inter, lambda_val, k, excl, drop=not unfiltered,
                                transpose=transpose, tiled=tiled, users=users,
                                items=items)


def recommendForBaskets(baskets: dict, user_num: int, item_num: int,
                        train_data_df: pd.DataFrame, val_data_df: pd.DataFrame, method: str,
                        lambda_val: float, dataset: str, k: int, items=None,
                        device=None) -> dict:
    """{key: [items]} for item baskets {key: item ids} that need not belong to any user of the
    DataFrames -- a new visitor's cart, a session, one item: per basket the k best items of
    B @ HybridS(A, general_W, lambda) not in the basket (the reference's scores and filter,
    :31-50, for the user such a basket would be), by ops.spread_rows_recommend: two sweeps of
    the interactions, no I x I matrix at any catalog size. ``method`` / ``dataset`` resolve as
    in spread_method_topk (general_W is exactly symmetric: the transposes change nothing).
    ``items``: rank only those items (ops.item_candidates' forms). Lists hold real item ids;
    a basket with fewer than k rankable items gets a shorter list. Nothing is written."""
    dev = device or gpu_device()
    both = pd.concat([train_data_df, val_data_df])
    inter = ops.Interactions.from_pairs(
        torch.from_numpy(both["user_id"].to_numpy(np.int64)),
        torch.from_numpy(both["item_id"].to_numpy(np.int64)), user_num, item_num, dev)
    if method == "ProbS" and dataset == "movielens":  # reference :87-91
        lambda_val = 0.01
    elif method == "HeatS" and dataset == "douban":  # reference :97-101
        lambda_val = 0.99
    keys = list(baskets)
    _, idx = ops.spread_rows_recommend(inter, [baskets[key] for key in keys], lambda_val, k,
                                       items=items)
    lists = topk_to_dict(idx)
    return {key: lists[r] for r, key in enumerate(keys)}


def held_out_rows(held_df: pd.DataFrame, user_num: int, item_num: int, dev, users=None):
    """The held-out positives of a DataFrame (user_id, item_id) as target rows: one sorted
    row per user, or per entry of ``users`` in that order."""
    held = RowSets.from_pairs(torch.from_numpy(held_df["user_id"].to_numpy(np.int64)),
                              torch.from_numpy(held_df["item_id"].to_numpy(np.int64)),
                              user_num, item_num, dev)
    if users is None:
        return held
    return held.take(torch.as_tensor(users).to(dev, torch.int64).reshape(-1))


def spread_method_ranks(user_num: int, item_num: int, train_data_df: pd.DataFrame,
                        val_data_df: pd.DataFrame, held_df: pd.DataFrame, method: str,
                        lambda_val: float, dataset: str, unfiltered: bool = False, device=None,
                        users=None, tiled: bool | None = None, tile: int | None = None):
    """(targets RowSets, rank int64 [nnz]): where every held-out (user, item) of ``held_df``
    stands among ALL items for its user under spread_method_topk's scores -- the same
    interactions, per-method overrides, exclusions and drop -- so rank < k iff
    spread_method_topk(..., k) lists the item at that position of the user's row (k <= 1024;
    the rank itself has no depth limit). rank is aligned with targets.col, 0 = first, -1 for an
    item that does not rank (it is in train|val and those are dropped). ``users``: only those
    users' rows, in that order. ``tiled``: False the dense path (ops.spread_rank), True the
    factored tile walk (ops.spread_rank_tiled, ``tile`` its tile width; general_W is exactly
    symmetric, so the transpose overrides are served unchanged), None the dense path when the
    I x I matrices fit (ops.dense_spread_fits), else the walk -- as spread_method_topk."""
    dev = device or gpu_device()
    both = pd.concat([train_data_df, val_data_df])
    inter = ops.Interactions.from_pairs(
        torch.from_numpy(both["user_id"].to_numpy(np.int64)),
        torch.from_numpy(both["item_id"].to_numpy(np.int64)), user_num, item_num, dev)
    transpose = False
    if method == "ProbS" and dataset == "movielens":  # reference :87-91
        lambda_val, transpose = 0.01, True
    elif method == "HeatS" and dataset == "douban":  # reference :97-101
        lambda_val, transpose = 0.99, True
    targets = held_out_rows(held_df, user_num, item_num, dev, users)
    if tiled is None:
        tiled = not ops.dense_spread_fits(item_num, dev)
    if tiled:
        kw = {} if tile is None else {"tile": int(tile)}
        rank, _ = ops.spread_rank_tiled(inter, lambda_val, targets, inter.by_user,
                                        drop=not unfiltered, users=users, **kw)
        return targets, rank
    rank, _ = ops.spread_rank(inter, lambda_val, targets, inter.by_user, drop=not unfiltered,
                              transpose=transpose, users=users, tiled=False)
    return targets, rank


def recommendSpreadMethod(user_num: int, item_num: int, train_data_df: pd.DataFrame,
                          val_data_df: pd.DataFrame, method: str,
                          lambda_val: float = 0) -> dict:
    """Reference :59-115 (lambda from cfg, as the reference reads it at :74)."""
    k = cfg.RECOMMEND["k"]
    lambda_val = cfg.MODEL["HyperParameter"]["lambda"]
    if method not in ["ProbS", "HeatS", "HybridS"]:
        raise ValueError(f"Invalid parameter: method={method}，必须为 ProbS | HeatS | HybridS")
    _, idx = spread_method_topk(user_num, item_num, train_data_df, val_data_df, method,
                                lambda_val, cfg.DATA_SET, k, unfiltered=_unfiltered())
    recs = _to_dict(idx, user_num)
    _save(recs)
    return recs
