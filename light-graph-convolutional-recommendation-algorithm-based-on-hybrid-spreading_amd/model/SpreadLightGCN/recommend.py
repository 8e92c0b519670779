"""LGCNHS-e recommendation with the reference's interface
(reference model/SpreadLightGCN/recommend.py:18-75).

recommendSpreadLightGCN runs fused on the GPU: F = A @ W per user block, multiplied by the
fp32 e0 score (promoted to fp64 as numpy's G * F does) inside the top-k kernel, train|val
items dropped. Neither G nor F is materialised for all users.
"""
from collections import defaultdict

import numpy as np
import pandas as pd
import torch

from const import cfg
from lgcnhs import ops
from lgcnhs.recs import topk_to_dict, exclusion_from_dfs, gpu_device, save_recs


def _to_dict(idx: torch.Tensor, user_num: int) -> dict:
    return topk_to_dict(idx, user_num, defaultdict)


def _save(recs: dict) -> None:
    save_recs(recs, cfg.RECOMMEND["save_path"] + "all_user_recommend_dict_" + cfg.MODEL["name"]
              + "_" + str(cfg.RECOMMEND["k"]) + ".npy")


def recommendForAllUser(F_new: np.ndarray, user_num: int, train_data_df: pd.DataFrame,
                        val_data_df: pd.DataFrame, k: int) -> dict:
    """Top-k by F_new without train|val items (reference :18-52). k in [1, 1024]:
    lg_rows_topk_f64 up to 128, lg_rows_topk_wide_f64 above (the reference's [:k] takes any
    k; larger k raises ValueError)."""
    dev = gpu_device()
    F = torch.as_tensor(np.ascontiguousarray(F_new[:user_num]), dtype=torch.float64).to(dev)
    excl = exclusion_from_dfs(user_num, F.shape[1], train_data_df, val_data_df, device=dev)
    _, idx = ops.rows_topk(F, k, excl, drop=True)
    recs = _to_dict(idx, user_num)
    _save(recs)
    return recs


def spread_lightgcn_topk(model, user_num: int, item_num: int, train_data_df: pd.DataFrame,
                         val_data_df: pd.DataFrame, lambda_val: float, k: int, device=None,
                         tiled: bool | None = None, users=None, items=None):
    """Device (values fp64, items int64) of the whole LGCNHS recommendation. k in [1, 1024];
    above 128 the dense path takes lg_rows_topk_wide_f64 and the tiled path peels
    ceil(k / 128) walks (ops.spread_topk_tiled). ``users`` (ids, tensor or list): only those
    users' rows, in that order (ops.spread_recommend). ``items`` (ids, a bool mask or an
    ascending device tensor: ops.item_candidates): rank only those items -- the spreading and
    the embeddings stay the whole graph's -- with real item ids in the lists."""
    dev = device or gpu_device(model.users_emb.weight)
    both = pd.concat([train_data_df, val_data_df])
    inter = ops.Interactions.from_pairs(
        torch.from_numpy(both["user_id"].to_numpy(np.int64)),
        torch.from_numpy(both["item_id"].to_numpy(np.int64)), user_num, item_num, dev)
    eu = model.users_emb.weight.detach().to(dev, torch.float32).contiguous()
    ei = model.items_emb.weight.detach().to(dev, torch.float32).contiguous()
    # dense I x I general_W / W when they fit, else the factored tile path (same values within a few ulp)
    return ops.spread_recommend(inter, lambda_val, k, inter.by_user, drop=True, eu=eu, ei=ei,
                                tiled=tiled, users=users, items=items)


def spread_lightgcn_baskets(model, baskets: dict, basket_emb, user_num: int, item_num: int,
                            train_data_df: pd.DataFrame, val_data_df: pd.DataFrame,
                            lambda_val: float, k: int, device=None, items=None) -> dict:
    """{key: [items]} of the LGCNHS scores G * F for item baskets {key: item ids} outside the
    graph: F by ops.spread_rows_recommend (two sweeps of the interactions), G from the
    caller's ``basket_emb`` -- one float32 row per basket, in the dict's order: an unseen user
    has no learned e0, the caller decides what stands for it -- and model.items_emb.weight.
    The basket's own items are dropped; lists hold real item ids and come out shorter when
    fewer than k items rank. ``items``: rank only those items. Nothing is written."""
    dev = device or gpu_device(model.items_emb.weight)
    both = pd.concat([train_data_df, val_data_df])
    inter = ops.Interactions.from_pairs(
        torch.from_numpy(both["user_id"].to_numpy(np.int64)),
        torch.from_numpy(both["item_id"].to_numpy(np.int64)), user_num, item_num, dev)
    eu = torch.as_tensor(basket_emb).detach().to(dev, torch.float32).contiguous()
    ei = model.items_emb.weight.detach().to(dev, torch.float32).contiguous()
    keys = list(baskets)
    _, idx = ops.spread_rows_recommend(inter, [baskets[key] for key in keys], lambda_val, k,
                                       eu=eu, ei=ei, items=items)
    lists = topk_to_dict(idx)
    return {key: lists[r] for r, key in enumerate(keys)}


def spread_lightgcn_ranks(model, user_num: int, item_num: int, train_data_df: pd.DataFrame,
                          val_data_df: pd.DataFrame, held_df: pd.DataFrame, lambda_val: float,
                          device=None, users=None, tiled: bool | None = None,
                          tile: int | None = None):
    """(targets RowSets, rank int64 [nnz]): where every held-out (user, item) of ``held_df``
    stands among ALL items for its user under spread_lightgcn_topk's scores G * F -- the same
    interactions, embeddings and dropped train|val items -- so rank < k iff
    spread_lightgcn_topk(..., k) lists the item at that position of the user's row (k <= 1024;
    the rank itself has no depth limit). rank is aligned with targets.col, 0 = first, -1 for an
    item that does not rank. ``users``: only those users' rows, in that order. ``tiled``: False
    the dense path (ops.spread_rank), True the factored tile walk (ops.spread_rank_tiled,
    ``tile`` its tile width), None the dense path when the I x I matrices fit
    (ops.dense_spread_fits), else the walk -- as spread_lightgcn_topk."""
    from model.SpreadMethod.recommend import held_out_rows

    dev = device or gpu_device(model.users_emb.weight)
    both = pd.concat([train_data_df, val_data_df])
    inter = ops.Interactions.from_pairs(
        torch.from_numpy(both["user_id"].to_numpy(np.int64)),
        torch.from_numpy(both["item_id"].to_numpy(np.int64)), user_num, item_num, dev)
    eu = model.users_emb.weight.detach().to(dev, torch.float32).contiguous()
    ei = model.items_emb.weight.detach().to(dev, torch.float32).contiguous()
    targets = held_out_rows(held_df, user_num, item_num, dev, users)
    if tiled is None:
        tiled = not ops.dense_spread_fits(item_num, dev)
    if tiled:
        kw = {} if tile is None else {"tile": int(tile)}
        rank, _ = ops.spread_rank_tiled(inter, lambda_val, targets, inter.by_user, drop=True,
                                        eu=eu, ei=ei, users=users, **kw)
        return targets, rank
    rank, _ = ops.spread_rank(inter, lambda_val, targets, inter.by_user, drop=True, eu=eu,
                              ei=ei, users=users, tiled=False)
    return targets, rank


def recommendSpreadLightGCN(user_num: int, item_num: int, rating_df: pd.DataFrame,
                            train_data_df: pd.DataFrame, val_data_df: pd.DataFrame,
                            test_data_df: pd.DataFrame) -> dict:
    """Reference :55-75."""
    from model.SpreadLightGCN.model import getLightGCNModel

    k = cfg.RECOMMEND["k"]
    model = getLightGCNModel(user_num, item_num, rating_df, train_data_df, val_data_df,
                             test_data_df, k)[0]
    _, idx = spread_lightgcn_topk(model, user_num, item_num, train_data_df, val_data_df,
                                  cfg.MODEL["HyperParameter"]["lambda"], k)
    recs = _to_dict(idx, user_num)
    _save(recs)
    return recs
