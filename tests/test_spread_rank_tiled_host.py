"""Host side of ops.spread_rank_tiled, with CPU tensors: a wrong dtype (TypeError), shape or
device (ValueError) is refused, and no user / no target returns, before the native library is
touched (N.lib is replaced by a function that fails the test)."""
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


def _inter(n_users=4, n_items=9):
    """What spread_rank_tiled reads of an Interactions before it reaches the library (building
    a real one runs a kernel)."""
    return SimpleNamespace(by_user=_rs(n_users, n_items), n_users=n_users, n_items=n_items,
                           k_item=torch.zeros(n_items, dtype=torch.float64))


EU, EI = torch.zeros(4, 32), torch.zeros(9, 32)


def test_embeddings_of_another_dtype():
    A = _inter()
    with pytest.raises(TypeError, match="eu must be float32"):
        ops.spread_rank_tiled(A, 0.5, _rs(), None, True, EU.double(), EI)
    with pytest.raises(TypeError, match="ei must be float32"):
        ops.spread_rank_tiled(A, 0.5, _rs(), None, True, EU, EI.half())
    with pytest.raises(TypeError, match="ei must be a tensor"):
        ops.spread_rank_tiled(A, 0.5, _rs(), None, True, EU, None)
    with pytest.raises(TypeError, match="eu must be a tensor"):
        ops.spread_rank_tiled(A, 0.5, _rs(), None, True, None, EI)


def test_shapes():
    A = _inter()
    for eu, ei in ((torch.zeros(5, 32), EI), (EU, torch.zeros(10, 32)),
                   (EU, torch.zeros(9, 64))):
        with pytest.raises(ValueError, match="eu must be"):
            ops.spread_rank_tiled(A, 0.5, _rs(), None, True, eu, ei)
    with pytest.raises(ValueError, match="embedding width 48"):
        ops.spread_rank_tiled(A, 0.5, _rs(), None, True, torch.zeros(4, 48), torch.zeros(9, 48))
    with pytest.raises(ValueError, match="exclusion rows 5 != users 4"):
        ops.spread_rank_tiled(A, 0.5, _rs(), _rs(5))
    with pytest.raises(ValueError, match="target rows 3 != 4 users"):
        ops.spread_rank_tiled(A, 0.5, _rs(3), None)
    with pytest.raises(ValueError, match="target rows 4 != 2 users"):
        ops.spread_rank_tiled(A, 0.5, _rs(), None, users=[1, 3])
    with pytest.raises(ValueError, match="requires drop=True"):
        ops.spread_rank_tiled(A, 0.5, _rs(), _rs(), False, EU, EI)
    with pytest.raises(ValueError, match="tile 0"):
        ops.spread_rank_tiled(A, 0.5, _rs(), None, tile=0)


def test_devices():
    A = _inter()
    meta = torch.device("meta")
    tg = _rs()
    with pytest.raises(ValueError, match="eu is on meta"):
        ops.spread_rank_tiled(A, 0.5, tg, None, True, EU.to(meta), EI)
    with pytest.raises(ValueError, match="ei is on meta"):
        ops.spread_rank_tiled(A, 0.5, tg, None, True, EU, EI.to(meta))
    ex = RowSets(tg.rowptr.to(meta), tg.col.to(meta), 4, 9)
    with pytest.raises(ValueError, match="excl is on meta"):
        ops.spread_rank_tiled(A, 0.5, tg, ex)


def test_right_types_on_the_cpu_meet_the_device_check():
    with pytest.raises(RuntimeError, match="A must be a GPU tensor"):
        ops.spread_rank_tiled(_inter(), 0.5, _rs(), None)


def test_no_user_and_no_target_return_without_the_library():
    A = _inter()
    rk, val = ops.spread_rank_tiled(A, 0.5, _rs(per_row=0), None)
    assert rk.shape == (0,) and rk.dtype == torch.int64
    assert val.shape == (0,) and val.dtype == torch.float64
    rk, val = ops.spread_rank_tiled(A, 0.5, _rs(0), None, users=[])
    assert rk.numel() == 0 and val.numel() == 0
    A0 = _inter(0)
    rk, val = ops.spread_rank_tiled(A0, 0.5, _rs(0), None, True, torch.zeros(0, 32), EI)
    assert rk.numel() == 0 and val.numel() == 0
