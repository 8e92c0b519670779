"""Host side of the spreading ranks, with CPU tensors: ops.rows_rank / ops.spread_rank refuse a
wrong dtype (TypeError) or shape (ValueError) and the tiled path before the native library is
touched (N.lib is replaced by a function that fails the test), and
lgcnhs.metrics.rank_metrics(n_pool=...) against a numpy restatement."""
import numpy as np
import pytest
import torch

from lgcnhs import _native as N
from lgcnhs import metrics as M
from lgcnhs import ops
from lgcnhs.graph import RowSets


@pytest.fixture(autouse=True)
def no_library(monkeypatch):
    def boom():
        raise AssertionError("the native library was reached before the argument check")
    monkeypatch.setattr(N, "lib", boom)
    monkeypatch.setattr(N, "load_library", boom)


def _rs(n_rows=4, n_cols=9, per_row=2):
    rp = torch.arange(n_rows + 1, dtype=torch.int64) * per_row
    col = torch.arange(n_rows * per_row, dtype=torch.int32) % n_cols
    return RowSets(rp, col, n_rows, n_cols)


F64 = torch.zeros(4, 9, dtype=torch.float64)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.int64])
def test_rows_rank_F_of_another_dtype(dtype):
    with pytest.raises(TypeError, match="F must be float64"):
        ops.rows_rank(F64.to(dtype), _rs())


@pytest.mark.parametrize("dtype", [torch.float64, torch.float16, torch.bfloat16])
@pytest.mark.parametrize("side", ["eu", "ei"])
def test_rows_rank_embeddings_of_another_dtype(dtype, side):
    eu, ei = torch.zeros(4, 8), torch.zeros(9, 8)
    eu, ei = (eu.to(dtype), ei) if side == "eu" else (eu, ei.to(dtype))
    with pytest.raises(TypeError, match=f"{side} must be float32"):
        ops.rows_rank(F64, _rs(), None, True, eu, ei)


def test_rows_rank_half_set_embeddings():
    with pytest.raises(TypeError, match="ei must be a tensor"):
        ops.rows_rank(F64, _rs(), None, True, torch.zeros(4, 8), None)
    with pytest.raises(TypeError, match="eu must be a tensor"):
        ops.rows_rank(F64, _rs(), None, True, None, torch.zeros(9, 8))


def test_rows_rank_shapes():
    with pytest.raises(ValueError, match="F must have 2 dimensions"):
        ops.rows_rank(torch.zeros(36, dtype=torch.float64), _rs())
    with pytest.raises(ValueError, match="eu must have 2 dimensions"):
        ops.rows_rank(F64, _rs(), None, True, torch.zeros(32), torch.zeros(9, 8))
    for eu, ei in ((torch.zeros(5, 8), torch.zeros(9, 8)),     # a row too many
                   (torch.zeros(4, 8), torch.zeros(10, 8)),    # an item too many
                   (torch.zeros(4, 8), torch.zeros(9, 16))):   # another width
        with pytest.raises(ValueError, match="eu must be"):
            ops.rows_rank(F64, _rs(), None, True, eu, ei)
    with pytest.raises(ValueError, match="exclusion rows 5 != rows of F 4"):
        ops.rows_rank(F64, _rs(), _rs(5))
    with pytest.raises(ValueError, match="target rows 3 != rows of F 4"):
        ops.rows_rank(F64, _rs(3))
    with pytest.raises(ValueError, match="requires drop=True"):
        ops.rows_rank(F64, _rs(), _rs(), False, torch.zeros(4, 8), torch.zeros(9, 8))


def test_rows_rank_right_types_on_the_cpu_meet_the_device_check():
    with pytest.raises(RuntimeError, match="F must be a GPU tensor"):
        ops.rows_rank(F64, _rs())


def _inter(n_users=4, n_items=9):
    """What spread_rank reads of an Interactions before it reaches the library (building a real
    one runs a kernel)."""
    from types import SimpleNamespace
    return SimpleNamespace(by_user=_rs(n_users, n_items), n_users=n_users, n_items=n_items,
                           k_item=torch.zeros(n_items, dtype=torch.float64))


def test_spread_rank_refuses_the_tiled_path():
    """The factored walk keeps bounded lists and has no rank: tiled=True says so."""
    with pytest.raises(ValueError, match="bounded lists.*no rank"):
        ops.spread_rank(_inter(), 0.5, _rs(), None, tiled=True)
    with pytest.raises(ValueError, match="bounded lists.*no rank"):
        ops.spread_rank(_inter(), 0.5, _rs(), None, W=torch.zeros(9, 9, dtype=torch.float64),
                        tiled=True)


def test_spread_rank_refuses_when_the_dense_path_does_not_fit(monkeypatch):
    monkeypatch.setattr(ops, "dense_spread_fits", lambda n_items, device: False)
    with pytest.raises(ValueError, match="bounded lists.*no rank"):
        ops.spread_rank(_inter(), 0.5, _rs(), None)


def test_spread_rank_dtypes_and_shapes():
    A = _inter()
    W = torch.zeros(9, 9, dtype=torch.float64)
    with pytest.raises(TypeError, match="W must be float64"):
        ops.spread_rank(A, 0.5, _rs(), None, W=W.float())
    with pytest.raises(ValueError, match="W has shape"):
        ops.spread_rank(A, 0.5, _rs(), None, W=torch.zeros(9, 8, dtype=torch.float64))
    with pytest.raises(TypeError, match="eu must be float32"):
        ops.spread_rank(A, 0.5, _rs(), None, True, torch.zeros(4, 8).double(),
                        torch.zeros(9, 8), W=W)
    with pytest.raises(TypeError, match="ei must be float32"):
        ops.spread_rank(A, 0.5, _rs(), None, True, torch.zeros(4, 8), torch.zeros(9, 8).half(),
                        W=W)
    with pytest.raises(ValueError, match="eu must be"):
        ops.spread_rank(A, 0.5, _rs(), None, True, torch.zeros(3, 8), torch.zeros(9, 8), W=W)
    with pytest.raises(ValueError, match="exclusion rows 5 != users 4"):
        ops.spread_rank(A, 0.5, _rs(), _rs(5), W=W)
    with pytest.raises(ValueError, match="target rows 3 != 4 users"):
        ops.spread_rank(A, 0.5, _rs(3), None, W=W)
    with pytest.raises(ValueError, match="target rows 4 != 2 users"):
        ops.spread_rank(A, 0.5, _rs(), None, W=W, users=[1, 3])


# ------------------------------------------------------------------------------ rank_metrics
def _auc_numpy(rank, rowptr, denom_base):
    """Ten lines of numpy: per user 1 - mean_i((rank_i - a_i) / (base_u - n_t)), a_i the number
    of the user's own evaluated targets ranked above i; the mean over users with a target."""
    per_user = []
    for u in range(len(rowptr) - 1):
        r = np.asarray([x for x in rank[rowptr[u]:rowptr[u + 1]] if x >= 0], np.float64)
        if len(r) == 0:
            continue
        a = np.argsort(np.argsort(r, kind="stable"), kind="stable").astype(np.float64)
        per_user.append(1.0 - np.mean((r - a) / max(denom_base[u] - len(r), 1.0)))
    return float(np.mean(per_user))


RANKS = np.array([0, 7, 3, -1, 12, 49, 5, 1, 2, -1, 30], np.int64)
ROWPTR = np.array([0, 3, 3, 6, 9, 10, 11], np.int64)  # user 1 empty, user 4 only unranked
N_ITEMS = 50
N_POOL = np.array([45, 50, 20, 50, 10, 31], np.int64)   # n_items - |excl row|


def _targets():
    return RowSets(torch.as_tensor(ROWPTR), torch.arange(len(RANKS), dtype=torch.int32),
                   len(ROWPTR) - 1, N_ITEMS)


@pytest.mark.parametrize("dtype", [torch.int64, torch.float64])
def test_rank_metrics_n_pool_replaces_n_items_in_the_auc(dtype):
    rk = torch.as_tensor(RANKS)
    got = M.rank_metrics(rk, _targets(), N_ITEMS, ks=(5,), n_pool=torch.as_tensor(N_POOL).to(dtype))
    want = _auc_numpy(RANKS, ROWPTR, N_POOL.astype(np.float64))
    assert abs(got["auc"] - want) < 1e-12
    base = M.rank_metrics(rk, _targets(), N_ITEMS, ks=(5,))
    assert abs(base["auc"] - _auc_numpy(RANKS, ROWPTR, np.full(6, float(N_ITEMS)))) < 1e-12
    assert got["auc"] < base["auc"]  # (a smaller pool: the same ranks are a larger share)
    # nothing else reads the pool
    for name in base:
        if name != "auc":
            assert got[name] == base[name], name


def test_rank_metrics_n_pool_none_is_the_present_result():
    rk = torch.as_tensor(RANKS)
    a = M.rank_metrics(rk, _targets(), N_ITEMS, ks=(5, 20))
    b = M.rank_metrics(rk, _targets(), N_ITEMS, ks=(5, 20), n_pool=None)
    assert a == b
    # ... and the pool of all items is that result too
    c = M.rank_metrics(rk, _targets(), N_ITEMS, ks=(5, 20),
                       n_pool=torch.full((6,), N_ITEMS, dtype=torch.int64))
    assert a == c


def test_rank_metrics_n_pool_guards():
    rk = torch.as_tensor(RANKS)
    with pytest.raises(TypeError, match="n_pool"):
        M.rank_metrics(rk, _targets(), N_ITEMS, n_pool=torch.zeros(6, dtype=torch.int32))
    with pytest.raises(TypeError, match="n_pool"):
        M.rank_metrics(rk, _targets(), N_ITEMS, n_pool=[50] * 6)
    with pytest.raises(ValueError, match="n_pool"):
        M.rank_metrics(rk, _targets(), N_ITEMS, n_pool=torch.zeros(5, dtype=torch.int64))
