"""LightGCN recommendation with the reference's interface
(reference model/LightGCN/recommend.py:22-159).

recommendForAllUser scores with the layer-0 embeddings, masks train and val positives with
-1024 and takes the top-k — in one HIP kernel that never holds the U x I score matrix,
chosen by ops.score_topk's dispatch: above ops.screen_pays' size crossover
lg_score_topk_screened_f32 (a bf16 MFMA screen, the exact fp32 chain of lg_score_topk_f32 on
the tiles it cannot rule out), below it lg_score_topk_f32 itself; the lists are the same bit
for bit, ties ordered (score desc, item asc). RECOMMEND["k"] up to 128 takes those kernels;
128 < k <= 1024 takes lg_score_topk_wide_f32 (the same scores and order, lists in global
slabs); larger k raises.

recommendForUsers is the request form: the same lists for a few user ids only, through
ops.score_topk_users (lg_score_topk_batch_f32 for short lists: no rows gathered, no other
user's scores computed). With items= it ranks a candidate item set only (the in-stock items,
one category, a retrieval stage's output): lg_score_topk_batch_items_f32 for short lists, which
gathers nothing and reads only the candidates' rows. recommendFromCandidates ranks every user
over its OWN candidate list (a per-user retrieval stage's output, sampled negatives) in one
launch of lg_score_topk_cand_f32. recommendForAllUser keeps the reference's signature.
"""
import numpy as np
import pandas as pd
import torch

from const import cfg
from lgcnhs import ops
from lgcnhs.recs import exclusion_from_coo, gpu_device, save_recs, topk_to_dict
from utils.graph import convertEdgeIndexToAdjMatrix
from utils.log import logger
from utils.wrapper import calTimes


def _edge_index(df: pd.DataFrame) -> torch.Tensor:
    return torch.stack([torch.tensor(df["user_id"].values, dtype=torch.long),
                        torch.tensor(df["item_id"].values, dtype=torch.long)])


@calTimes(logger, "LightGCN图建立完成")
def buildGraph(user_num: int, item_num: int, rating_df: pd.DataFrame,
               train_data_df: pd.DataFrame, val_data_df: pd.DataFrame,
               test_data_df: pd.DataFrame) -> tuple:
    """-> (edge_index of all ratings [2, E], train/val/test symmetric COO adjacencies)
    (reference :22-66)."""
    edge_index = _edge_index(rating_df)
    return (edge_index,
            convertEdgeIndexToAdjMatrix(user_num, item_num, _edge_index(train_data_df)),
            convertEdgeIndexToAdjMatrix(user_num, item_num, _edge_index(val_data_df)),
            convertEdgeIndexToAdjMatrix(user_num, item_num, _edge_index(test_data_df)))


def topk_for_all_users(model, user_num: int, item_num: int, train_edge_index,
                       val_edge_index, k: int, items=None):
    """Device result of recommendForAllUser: (scores [U,k] fp32, items [U,k] int64). items:
    rank only a candidate item set (ops.item_candidates' forms; real item ids come back)."""
    w_u = model.users_emb.weight.detach()
    dev = gpu_device(w_u)
    eu = w_u.to(dev, torch.float32).contiguous()
    ei = model.items_emb.weight.detach().to(dev, torch.float32).contiguous()
    excl = exclusion_from_coo(user_num, item_num, train_edge_index, val_edge_index, device=dev)
    return ops.score_topk(eu, ei, k, excl, mask_value=float(-(1 << 10)), items=items)


def recommendForAllUser(model, user_num: int, item_num: int,
                        train_edge_index: torch.Tensor, val_edge_index: torch.Tensor,
                        test_edge_index: torch.Tensor, k: int) -> dict:
    """{uid: top-k items} (reference :68-125)."""
    _, idx = topk_for_all_users(model, user_num, item_num, train_edge_index, val_edge_index, k)
    recs = topk_to_dict(idx)
    save_recs(recs, cfg.RECOMMEND["save_path"] + "all_user_recommend_dict_" + cfg.MODEL["name"]
              + "_" + str(cfg.RECOMMEND["k"]) + ".npy")
    return recs


def topk_for_users(model, user_ids, user_num: int, item_num: int, train_edge_index,
                   val_edge_index, k: int, items=None):
    """Device result of recommendForUsers: (scores [B,k] fp32, items [B,k] int64), row j =
    topk_for_all_users' row user_ids[j] (ops.score_topk_users: no score row of any other
    user is computed). items: rank only a candidate item set (ops.item_candidates' forms;
    short lists run lg_score_topk_batch_items_f32, which reads the candidates' rows only)."""
    w_u = model.users_emb.weight.detach()
    dev = gpu_device(w_u)
    eu = w_u.to(dev, torch.float32).contiguous()
    ei = model.items_emb.weight.detach().to(dev, torch.float32).contiguous()
    excl = exclusion_from_coo(user_num, item_num, train_edge_index, val_edge_index, device=dev)
    return ops.score_topk_users(eu, ei, user_ids, k, excl, mask_value=float(-(1 << 10)),
                                items=items)


def recommendForUsers(model, user_ids, user_num: int, item_num: int,
                      train_edge_index: torch.Tensor, val_edge_index: torch.Tensor,
                      test_edge_index: torch.Tensor, k: int, items=None) -> dict:
    """{uid: top-k items} for the given user ids only: the matching entries of
    recommendForAllUser (same -1024 mask, same lists). Writes no file. An id outside
    [0, user_num) raises ValueError. items: recommend only from a candidate item set (ids, a
    bool mask over the items, or a strictly ascending device tensor: ops.item_candidates); a
    user with fewer than k candidates that can rank gets a shorter list."""
    ids = [int(u) for u in torch.as_tensor(user_ids).reshape(-1).tolist()]
    _, idx = topk_for_users(model, ids, user_num, item_num, train_edge_index, val_edge_index, k,
                            items=items)
    rows = topk_to_dict(idx)
    return {u: rows[j] for j, u in enumerate(ids)}


def topk_for_candidates(model, candidates, user_num: int, item_num: int, train_edge_index,
                        val_edge_index, k: int, user_ids=None):
    """Device result of recommendFromCandidates: (scores [R,k] fp32, items [R,k] int64), row r
    the top-k of row r's OWN candidate list for user user_ids[r] (None: user r), with
    topk_for_users' mask and exclusions (ops.score_topk_cand: lg_score_topk_cand_f32, one
    launch for every row, no row gathered). candidates: ops.candidate_rows' forms (a RowSets,
    {row: ids}, a list of id lists, or a (rows, items) pair)."""
    w_u = model.users_emb.weight.detach()
    dev = gpu_device(w_u)
    eu = w_u.to(dev, torch.float32).contiguous()
    ei = model.items_emb.weight.detach().to(dev, torch.float32).contiguous()
    n_rows = user_num if user_ids is None else int(torch.as_tensor(user_ids).numel())
    cand = ops.candidate_rows(candidates, n_rows, item_num, dev)
    excl = exclusion_from_coo(user_num, item_num, train_edge_index, val_edge_index, device=dev)
    return ops.score_topk_cand(eu, ei, cand, k, excl, mask_value=float(-(1 << 10)),
                               users=user_ids)


def recommendFromCandidates(model, candidates, user_num: int, item_num: int,
                            train_edge_index: torch.Tensor, val_edge_index: torch.Tensor,
                            test_edge_index: torch.Tensor, k: int, user_ids=None) -> dict:
    """{uid: top-k items} where every user is ranked over its own candidate list (a per-user
    retrieval stage's output; the sampled-negative evaluation protocol): per user the list of
    recommendForUsers(..., items=that user's candidates), in one launch. candidates row r
    belongs to user user_ids[r] (None: user r, every user; ids should not repeat: the dict
    keeps one list per id). Writes no file. A user or item id outside its table raises
    ValueError. A user with fewer than k candidates that can rank gets a shorter list."""
    ids = (list(range(user_num)) if user_ids is None
           else [int(u) for u in torch.as_tensor(user_ids).reshape(-1).tolist()])
    _, idx = topk_for_candidates(model, candidates, user_num, item_num, train_edge_index,
                                 val_edge_index, k, user_ids=None if user_ids is None else ids)
    rows = topk_to_dict(idx)
    return {u: rows[j] for j, u in enumerate(ids)}


def recommendLightGCN(user_num: int, item_num: int, rating_df: pd.DataFrame,
                      train_data_df: pd.DataFrame, val_data_df: pd.DataFrame,
                      test_data_df: pd.DataFrame) -> dict:
    """Reference :127-159. A cached model is a state_dict loaded with weights_only=True
    (the reference's whole-model pickle cannot load on torch>=2.6)."""
    from model.LightGCN.model import LightGCN
    from model.LightGCN.train import trainLightGCN

    k = cfg.RECOMMEND["k"]
    edge_index, train_ei, val_ei, test_ei = buildGraph(user_num, item_num, rating_df,
                                                       train_data_df, val_data_df, test_data_df)
    path = cfg.MODEL["save_path"] + str(k) + "_LightGCN.pth"
    try:
        hp = cfg.MODEL["HyperParameter"]
        model = LightGCN(user_num, item_num, hp["embedding_dim"], hp["layers"])
        model.load_state_dict(torch.load(path, weights_only=True))
        model = model.to(gpu_device())
        logger.info("模型加载完毕")
    except Exception:
        logger.info("模型加载失败，正在重新训练模型")
        model = trainLightGCN(user_num, item_num, edge_index, train_ei, val_ei)
    return recommendForAllUser(model, user_num, item_num, train_ei, val_ei, test_ei, k)
