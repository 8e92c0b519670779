"""Argument refusals of the torch-facing wrappers, with CPU tensors: a wrong dtype is a
TypeError and a wrong shape a ValueError, both raised before the native library is touched
(N.lib is replaced by a function that fails the test). The kernels reinterpret what they are
handed -- a float32 W read as fp64 runs past its end, an int64 col is read as int32 pairs --
so these are the only line of defence."""
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


WRONG = [torch.float64, torch.float16, torch.bfloat16]


def _embedding_entries(eu, ei):
    """Every entry that takes fp32 embeddings, as thunks on the given tables."""
    return {
        "score_topk": lambda: ops.score_topk(eu, ei, 3),
        "score_topk_screened": lambda: ops.score_topk(eu, ei, 3, screen=True),
        "score_topk_wide": lambda: ops.score_topk(eu, ei, 256),
        "score_topk_items": lambda: ops.score_topk(eu, ei, 3, items=[0, 1]),
        "score_topk_users": lambda: ops.score_topk_users(eu, ei, [0, 1], 3),
        "score_topk_cand": lambda: ops.score_topk_cand(eu, ei, _rs(4, 9), 3),
        "score_cand": lambda: ops.score_cand(eu, ei, _rs(4, 9)),
        "score_rank": lambda: ops.score_rank(eu, ei, _rs(4, 9)),
        "score_dense": lambda: ops.score_dense(eu, ei),
        "rows_topk": lambda: ops.rows_topk(torch.zeros(4, 9, dtype=torch.float64), 3, None, True,
                                           eu, ei),
    }


@pytest.mark.parametrize("dtype", WRONG)
@pytest.mark.parametrize("side", ["eu", "ei"])
def test_embeddings_of_another_dtype_are_type_errors(dtype, side):
    good_u, good_i = torch.zeros(4, 8), torch.zeros(9, 8)
    eu = good_u.to(dtype) if side == "eu" else good_u
    ei = good_i.to(dtype) if side == "ei" else good_i
    for name, call in _embedding_entries(eu, ei).items():
        with pytest.raises(TypeError, match=f"{side} must be float32"):
            call()


def test_embeddings_of_another_rank_are_value_errors():
    for name, call in _embedding_entries(torch.zeros(32), torch.zeros(9, 8)).items():
        with pytest.raises(ValueError, match="eu must have 2 dimensions"):
            call()
    for name, call in _embedding_entries(torch.zeros(4, 8), torch.zeros(9, 8, 1)).items():
        with pytest.raises(ValueError, match="ei must have 2 dimensions"):
            call()


def test_cpu_tensors_of_the_right_type_still_meet_the_device_check():
    for name, call in _embedding_entries(torch.zeros(4, 8), torch.zeros(9, 8)).items():
        with pytest.raises(RuntimeError, match="must be a GPU tensor"):
            call()


@pytest.mark.parametrize("dtype", WRONG)
def test_propagation_and_conversion_refuse_other_dtypes(dtype):
    e0 = torch.zeros(10, 64, dtype=dtype)
    nodes = torch.tensor([1, 2])
    for call in (lambda: ops.propagate_mean(None, e0, 2),
                 lambda: ops.propagate(None, e0, 2),
                 lambda: ops.propagate(None, e0, 2, store=torch.float16),
                 lambda: ops.propagate_rows_mean(None, e0, 2, nodes),
                 lambda: ops.propagate_rows(None, e0, 2, nodes)):
        with pytest.raises(TypeError, match="e0 must be float32"):
            call()
    with pytest.raises(TypeError, match="x must be float32"):
        ops.rows_to_f16(e0)
    with pytest.raises(TypeError, match="x must be float32"):
        ops.bound_operands(e0)
    with pytest.raises(ValueError, match="2 dimensions"):
        ops.propagate_mean(None, torch.zeros(640), 2)


def test_rows_to_f16_out():
    x = torch.zeros(10, 64)
    with pytest.raises(TypeError, match="out must be float16"):
        ops.rows_to_f16(x, out=torch.zeros(10, 64))
    with pytest.raises(ValueError, match="out must be contiguous of x's shape"):
        ops.rows_to_f16(x, out=torch.zeros(9, 64, dtype=torch.float16))
    with pytest.raises(ValueError, match="out must be contiguous of x's shape"):
        ops.rows_to_f16(x, out=torch.zeros(64, 10, dtype=torch.float16).t())
    with pytest.raises(RuntimeError, match="GPU tensor"):  # (a good pair: the device check)
        ops.rows_to_f16(x, out=torch.zeros(10, 64, dtype=torch.float16))


def _interactions(U=5, I=6):
    return SimpleNamespace(n_users=U, n_items=I, by_user=_rs(U, I))


def test_spread_resource():
    A = _interactions()
    W = torch.zeros(6, 6, dtype=torch.float64)
    with pytest.raises(TypeError, match="W must be float64"):  # (read as fp64 past its end)
        ops.spread_resource(A, W.float())
    with pytest.raises(ValueError, match=r"W has shape \(6, 5\)"):
        ops.spread_resource(A, W[:, :5])
    with pytest.raises(ValueError, match=r"W has shape \(5, 6\)"):
        ops.spread_resource(A, W[:5])
    with pytest.raises(ValueError, match="W must have 2 dimensions"):
        ops.spread_resource(A, W.reshape(-1))
    with pytest.raises(TypeError, match="out must be float64"):
        ops.spread_resource(A, W, out=torch.zeros(5, 6))
    with pytest.raises(ValueError, match="expected at least"):
        ops.spread_resource(A, W, out=torch.zeros(4, 6, dtype=torch.float64))
    with pytest.raises(ValueError, match="expected at least"):
        ops.spread_resource(A, W, out=torch.zeros(5, 5, dtype=torch.float64))
    with pytest.raises(ValueError, match="unit column stride"):
        ops.spread_resource(A, W, out=torch.zeros(6, 5, dtype=torch.float64).t())
    with pytest.raises(ValueError, match="users"):
        ops.spread_resource(A, W, users=slice(2, 9))
    # a user block needs only its own rows of out
    with pytest.raises(RuntimeError, match="GPU tensor"):
        ops.spread_resource(A, W, users=slice(1, 3), out=torch.zeros(2, 6, dtype=torch.float64))


def test_rows_topk():
    F = torch.zeros(4, 9, dtype=torch.float64)
    eu, ei = torch.zeros(4, 8), torch.zeros(9, 8)
    with pytest.raises(TypeError, match="F must be float64"):
        ops.rows_topk(F.float(), 3)
    with pytest.raises(ValueError, match="F must have 2 dimensions"):
        ops.rows_topk(F.reshape(-1), 3)
    with pytest.raises(ValueError, match=r"eu must be \[4, d\]"):
        ops.rows_topk(F, 3, None, True, eu[:3], ei)
    with pytest.raises(ValueError, match=r"ei \[9, d\]"):
        ops.rows_topk(F, 3, None, True, eu, ei[:8])
    with pytest.raises(ValueError, match=r"ei \[9, d\]"):
        ops.rows_topk(F, 3, None, True, eu, torch.zeros(9, 16))
    with pytest.raises(ValueError, match="exclusion rows 5 != rows of F 4"):
        ops.rows_topk(F, 3, _rs(5, 9))
    with pytest.raises(ValueError, match="k=0"):
        ops.rows_topk(F, 0)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        ops.rows_topk(F, 3, _rs(4, 9), True, eu, ei)


def test_run_layer_and_spmm_layer():
    n, d = 10, 64
    x = torch.zeros(n, d)
    rp, src, dis = torch.zeros(n + 1, dtype=torch.int64), torch.zeros(0, dtype=torch.int32), \
        torch.zeros(n)

    def run(x=x, y=None, x0=None, acc=None, out=None, n_rows=n, off=0, **kw):
        ops.run_layer(rp, src, dis, None, x, y, x0, acc, out, n_rows, off, N.LG_ACC_NONE, 1.0,
                      **kw)

    for bad in (x.double(), x.bfloat16(), x.to(torch.int32)):
        with pytest.raises(TypeError, match="x must be a float32 or float16"):
            run(x=bad)
    with pytest.raises(ValueError, match="x must be contiguous"):
        run(x=torch.zeros(d, n).t())
    with pytest.raises(ValueError, match="x must be contiguous"):
        run(x=torch.zeros(n, 2 * d)[:, :d])
    with pytest.raises(ValueError, match="x must be contiguous"):
        run(x=torch.zeros(n * d))
    with pytest.raises(ValueError, match="outside x's 10 rows"):
        run(n_rows=6, off=5)
    with pytest.raises(ValueError, match="16-byte aligned"):
        run(x=torch.zeros(n * d + 1)[1:].view(n, d))
    with pytest.raises(TypeError, match="y must be float32"):
        run(y=torch.zeros(n, d, dtype=torch.float64))
    with pytest.raises(ValueError, match="a float16 x needs a float16 y"):
        run(x=x.half(), y=torch.zeros(n, d))
    for name in ("x0", "acc", "out"):
        with pytest.raises(TypeError, match=f"{name} must be float32"):
            run(**{name: torch.zeros(n, d, dtype=torch.float16)})
        with pytest.raises(TypeError, match=f"{name} must be float32"):  # (also with f16 storage)
            run(x=x.half(), **{name: torch.zeros(n, d, dtype=torch.float16)})
        with pytest.raises(ValueError, match=f"{name} must be contiguous of x's shape"):
            run(**{name: torch.zeros(n - 1, d)})
        with pytest.raises(ValueError, match=f"{name} must be contiguous of x's shape"):
            run(**{name: torch.zeros(d, n).t()})
    with pytest.raises(ValueError, match="y must be contiguous of x's shape"):
        run(y=torch.zeros(n, 32))
    with pytest.raises(ValueError, match="live must be a uint8 mask"):
        run(live=torch.zeros(n, dtype=torch.int32))
    with pytest.raises(ValueError, match="live must be a uint8 mask"):
        run(live=torch.zeros(n - 1, dtype=torch.uint8))
    with pytest.raises(ValueError, match="row_mask must be a uint8 mask"):
        run(row_mask=torch.zeros(n, dtype=torch.bool))
    with pytest.raises(ValueError, match="row_mask must be a uint8 mask"):
        run(row_mask=torch.zeros(n + 1, dtype=torch.uint8))
    adj = SimpleNamespace(n_nodes=n + 1)
    with pytest.raises(ValueError, match="x has 10 rows, graph has 11 nodes"):
        ops.spmm_layer(adj, x, None, None, None, None, N.LG_ACC_NONE, 1.0)


def test_chunk_bounds():
    d = 64
    ub, un = torch.zeros(5, d, dtype=torch.int16), torch.zeros(5)
    ib, inorm = torch.zeros(300, d, dtype=torch.int16), torch.zeros(300)
    with pytest.raises(TypeError, match="ub must be int16"):
        ops.chunk_bounds(ub.to(torch.bfloat16), un, ib, inorm, d, 0, 256)
    with pytest.raises(TypeError, match="ib must be int16"):
        ops.chunk_bounds(ub, un, ib.float(), inorm, d, 0, 256)
    with pytest.raises(TypeError, match="un must be float32"):
        ops.chunk_bounds(ub, un.double(), ib, inorm, d, 0, 256)
    with pytest.raises(TypeError, match="inorm must be float32"):
        ops.chunk_bounds(ub, un, ib, inorm.half(), d, 0, 256)
    with pytest.raises(ValueError, match="are not"):
        ops.chunk_bounds(ub, un, ib, inorm, 32, 0, 256)
    with pytest.raises(ValueError, match="norms for"):
        ops.chunk_bounds(ub, un[:4], ib, inorm, d, 0, 256)
    with pytest.raises(ValueError, match="norms for"):
        ops.chunk_bounds(ub, un, ib, inorm[:299], d, 0, 256)
    with pytest.raises(ValueError, match=r"items \[100, 356\) outside"):
        ops.chunk_bounds(ub, un, ib, inorm, d, 100, 256)
    with pytest.raises(TypeError, match="out must be float32"):
        ops.chunk_bounds(ub, un, ib, inorm, d, 0, 256, out=torch.zeros(20, dtype=torch.float64))
    with pytest.raises(TypeError, match="qout must be uint8"):
        ops.chunk_bounds(ub, un, ib, inorm, d, 0, 256,
                         qout=torch.zeros(5, 256, dtype=torch.int8))
    with pytest.raises(ValueError, match="qout must be contiguous"):
        ops.chunk_bounds(ub, un, ib, inorm, d, 0, 257,
                         qout=torch.zeros(5, 256, dtype=torch.uint8))
    with pytest.raises(ValueError, match="qout must be contiguous"):
        ops.chunk_bounds(ub, un, ib, inorm, d, 0, 256,
                         qout=torch.zeros(4, 256, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="GPU tensor"):
        ops.chunk_bounds(ub, un, ib, inorm, d, 0, 256,
                         qout=torch.zeros(5, 256, dtype=torch.uint8))


def test_rowsets_constructor():
    rp = torch.tensor([0, 2, 3, 3], dtype=torch.int64)
    col = torch.tensor([1, 4, 0], dtype=torch.int32)
    s = RowSets(rp, col, 3, 5)
    assert s.n_rows == 3 and s.col.dtype == torch.int32 and s.rowptr.dtype == torch.int64
    with pytest.raises(TypeError, match="col must be int32"):  # (read as int32 pairs)
        RowSets(rp, col.to(torch.int64), 3, 5)
    with pytest.raises(TypeError, match="col must be int32"):
        RowSets(rp, col.float(), 3, 5)
    with pytest.raises(TypeError, match="rowptr must be int64"):
        RowSets(rp.to(torch.int32), col, 3, 5)
    with pytest.raises(TypeError, match="rowptr must be a tensor"):
        RowSets(rp.tolist(), col, 3, 5)
    with pytest.raises(ValueError, match="rowptr has 4 entries for 4 rows"):
        RowSets(rp, col, 4, 5)
    with pytest.raises(ValueError, match="rowptr has 4 entries for 2 rows"):
        RowSets(rp, col, 2, 5)
    with pytest.raises(ValueError, match="col must be 1-D"):
        RowSets(rp, col.reshape(1, 3), 3, 5)
    with pytest.raises(ValueError, match="rowptr must be 1-D"):
        RowSets(rp.reshape(4, 1), col, 3, 5)
    # strided views are made contiguous, values kept
    wide_rp = torch.stack([rp, rp + 100], 1)[:, 0]
    wide_col = torch.stack([col, col + 100], 1)[:, 0]
    assert not wide_rp.is_contiguous() and not wide_col.is_contiguous()
    s = RowSets(wide_rp, wide_col, 3, 5)
    assert s.rowptr.is_contiguous() and s.col.is_contiguous()
    assert torch.equal(s.rowptr, rp) and torch.equal(s.col, col)
    # the views the library itself makes still pass
    assert s.slice_rows(1, 3).n_rows == 2 and s.slice_rows(1, 3).rowptr.tolist() == [2, 3, 3]
    assert s.take([2, 0]).rowptr.tolist() == [0, 0, 2]
    assert s.restrict_cols(torch.tensor([0, 4], dtype=torch.int32)).col.tolist() == [1, 0]
    e = RowSets(torch.zeros(4, dtype=torch.int64), torch.zeros(0, dtype=torch.int32), 3, 5)
    assert e.col.numel() == 0 and e.col.dtype == torch.int32


def test_aligned_copies_only_what_is_misaligned():
    n, d = 6, 8
    base = torch.arange(n * d + 4, dtype=torch.float32)
    assert base.data_ptr() % 16 == 0
    odd = base[1:1 + n * d].view(n, d)          # contiguous, 4 bytes off
    assert odd.is_contiguous() and odd.data_ptr() % 16 == 4
    got = ops._aligned(odd)
    assert got.data_ptr() % 16 == 0 and torch.equal(got, odd) and got.is_contiguous()
    even = base[4:4 + n * d].view(n, d)         # contiguous, 16 bytes off: taken as it is
    assert ops._aligned(even).data_ptr() == even.data_ptr()
    for view in (base[:n * d].view(n, d)[:, :4],            # a column slice
                 base[:n * d].view(d, n).t(),                # a transposed table
                 base[:d].expand(n, d)):                     # a stride-0 gradient
        got = ops._aligned(view)
        assert got.is_contiguous() and got.data_ptr() % 16 == 0 and torch.equal(got, view)
    ids = torch.arange(9, dtype=torch.int64)[1:]             # 8 bytes off
    assert ops._aligned(ids).data_ptr() % 16 == 0 and torch.equal(ops._aligned(ids), ids)
    empty = base[1:1]
    assert ops._aligned(empty).numel() == 0
