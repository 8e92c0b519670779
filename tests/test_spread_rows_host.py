"""Host side of the basket spreading (ops.spread_rows_resource / spread_rows_recommend /
spread_rows_rank / spread_related_items), with CPU tensors: a wrong dtype (TypeError) or shape
(ValueError) is refused before the native library is touched (N.lib is replaced by a function
that fails the test), and the baskets' host forms collapse duplicate items."""
from types import SimpleNamespace

import pytest
import torch

from lgcnhs import _native as N
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


def _inter(n_users=5, n_items=9):
    """What the spread_rows_* calls read of an Interactions before they reach the library
    (building a real one runs a kernel)."""
    return SimpleNamespace(by_user=_rs(n_users, n_items), n_users=n_users, n_items=n_items,
                           k_item=torch.zeros(n_items, dtype=torch.float64))


A = _inter()
ROWS = [[0, 1], [2], [3, 4, 5], []]   # 4 baskets
W = torch.zeros(9, 9, dtype=torch.float64)


def recommend(**kw):
    args = dict(A=A, rows=ROWS, lam=0.5, k=3)
    args.update(kw)
    return ops.spread_rows_recommend(**args)


def test_constants_are_visible():
    assert ops.SPREAD_ROWS_BLOCK == N.LG_SPREAD_ROWS_BLOCK
    assert ops.SPREAD_ROWS_SEG == N.LG_SPREAD_ROWS_SEG


@pytest.mark.parametrize("dtype", [torch.float64, torch.float16, torch.bfloat16])
@pytest.mark.parametrize("side", ["eu", "ei"])
def test_embeddings_of_another_dtype(dtype, side):
    eu, ei = torch.zeros(4, 8), torch.zeros(9, 8)
    eu, ei = (eu.to(dtype), ei) if side == "eu" else (eu, ei.to(dtype))
    with pytest.raises(TypeError, match=f"{side} must be float32"):
        recommend(eu=eu, ei=ei)
    with pytest.raises(TypeError, match=f"{side} must be float32"):
        ops.spread_rows_rank(A, ROWS, 0.5, [[1], [2], [3], [4]], eu=eu, ei=ei)


def test_half_set_embeddings():
    with pytest.raises(TypeError, match="ei must be a tensor"):
        recommend(eu=torch.zeros(4, 8))
    with pytest.raises(TypeError, match="eu must be a tensor"):
        recommend(ei=torch.zeros(9, 8))
    with pytest.raises(TypeError, match="ei must be a tensor"):
        ops.spread_rows_rank(A, ROWS, 0.5, [[1], [2], [3], [4]], eu=torch.zeros(4, 8))


def test_embedding_shapes():
    with pytest.raises(ValueError, match="eu must have 2 dimensions"):
        recommend(eu=torch.zeros(32), ei=torch.zeros(9, 8))
    # one eu row per BASKET (not per user of A: 5), the full item table, one width
    for eu, ei in ((torch.zeros(5, 8), torch.zeros(9, 8)),
                   (torch.zeros(3, 8), torch.zeros(9, 8)),
                   (torch.zeros(4, 8), torch.zeros(10, 8)),
                   (torch.zeros(4, 8), torch.zeros(9, 16))):
        with pytest.raises(ValueError, match="eu must be"):
            recommend(eu=eu, ei=ei)
        with pytest.raises(ValueError, match="eu must be"):
            ops.spread_rows_rank(A, ROWS, 0.5, [[1], [2], [3], [4]], eu=eu, ei=ei)


def test_exclusion_rows():
    with pytest.raises(ValueError, match="exclusion rows 5 != baskets 4"):
        recommend(excl=_rs(5))
    with pytest.raises(ValueError, match="exclusion rows 3 != baskets 4"):
        ops.spread_rows_rank(A, ROWS, 0.5, [[1], [2], [3], [4]], excl=_rs(3))
    with pytest.raises(TypeError, match="excl must be a RowSets"):
        recommend(excl=[[0], [1], [2], [3]])
    with pytest.raises(ValueError, match="requires drop=True"):
        recommend(excl=_rs(4), drop=False, eu=torch.zeros(4, 8), ei=torch.zeros(9, 8))


def test_item_ids_outside_the_catalog():
    for bad in ([[0, 9], [1], [2], [3]], [[-1], [1], [2], [3]]):
        with pytest.raises(ValueError, match=r"item id outside \[0, 9\)"):
            recommend(rows=bad)
        with pytest.raises(ValueError, match=r"item id outside \[0, 9\)"):
            ops.spread_rows_resource(A, bad, 0.5)
    with pytest.raises(ValueError, match="item ids must be integers"):
        recommend(rows=[[0.5], [1], [2], [3]])
    with pytest.raises(ValueError, match=r"item id outside \[0, 9\)"):
        ops.spread_related_items(A, [3, 9], 0.5, 3)
    with pytest.raises(ValueError, match="item ids must be integers"):
        ops.spread_related_items(A, [1.0], 0.5, 3)
    with pytest.raises(ValueError, match=r"item id outside \[0, 9\)"):
        ops.spread_rows_rank(A, ROWS, 0.5, [[1], [2], [9], [4]])
    with pytest.raises(ValueError, match="baskets over 8 items, A has 9"):
        recommend(rows=_rs(4, 8))


def test_W_of_the_wrong_type_or_shape():
    with pytest.raises(TypeError, match="W must be float64"):
        recommend(W=W.float())
    with pytest.raises(ValueError, match="W has shape"):
        recommend(W=torch.zeros(9, 8, dtype=torch.float64))
    with pytest.raises(ValueError, match="W has shape"):
        recommend(W=torch.zeros(8, 8, dtype=torch.float64))


def test_items_as_a_slice():
    with pytest.raises(ValueError, match="items= is a candidate set"):
        recommend(items=slice(0, 4))
    with pytest.raises(ValueError, match="items= is a candidate set"):
        ops.spread_related_items(A, [1], 0.5, 3, items=slice(0, 4))
    with pytest.raises(ValueError, match=r"item id outside \[0, 9\)"):
        recommend(items=[1, 2, 11])


def test_k_range():
    for k in (0, -1, 1025):
        with pytest.raises(ValueError, match="not in \\[1, 1024\\]"):
            recommend(k=k)


def test_targets_and_out():
    with pytest.raises(ValueError, match="target rows 3 != 4 baskets"):
        ops.spread_rows_rank(A, ROWS, 0.5, _rs(3))
    with pytest.raises(TypeError, match="out must be float64"):
        ops.spread_rows_resource(A, ROWS, 0.5, out=torch.zeros(4, 9))
    for out in (torch.zeros(3, 9, dtype=torch.float64), torch.zeros(4, 8, dtype=torch.float64),
                torch.zeros(9, 4, dtype=torch.float64).t()):
        with pytest.raises(ValueError, match="out has shape"):
            ops.spread_rows_resource(A, ROWS, 0.5, out=out)


def test_right_types_on_the_cpu_meet_the_device_check():
    with pytest.raises(RuntimeError, match="A must be a GPU tensor"):
        ops.spread_rows_resource(A, ROWS, 0.5)
    with pytest.raises(RuntimeError, match="A must be a GPU tensor"):
        recommend()


def test_duplicate_items_collapse():
    """A is 0/1: an item named twice counts once -- every host form of the baskets comes out
    as sorted, de-duplicated rows."""
    B = ops._basket_rows([[5, 1, 5, 1, 1], [], [7], [2, 2]], 9, "cpu")
    assert B.n_rows == 4 and B.n_cols == 9
    assert B.rowptr.tolist() == [0, 2, 2, 3, 4] and B.col.tolist() == [1, 5, 7, 2]
    D = ops._basket_rows({0: [5, 1, 5], 3: [2, 2]}, 9, "cpu")   # rows 1, 2 are empty
    assert D.n_rows == 4 and D.rowptr.tolist() == [0, 2, 2, 2, 3] and D.col.tolist() == [1, 5, 2]
    P = ops._basket_rows(([1, 0, 0, 1], [4, 3, 3, 4]), 9, "cpu")
    assert P.n_rows == 2 and P.rowptr.tolist() == [0, 1, 2] and P.col.tolist() == [3, 4]
    assert ops._basket_rows(B, 9, "cpu") is B
    assert ops._basket_rows([], 9, "cpu").n_rows == 0
