"""No result may depend on how the caller's tensors lie in memory, or on the stream.

Every entry is called on views of its inputs -- row slices of one concatenated table, a
contiguous view at an odd float offset of a larger buffer (4 bytes off 16-byte alignment), a
column slice of a wider table, a transposed table, a RowSets.slice_rows view whose rowptr starts
8 bytes off and whose columns start past the beginning of col, the stride-0 gradient of
``out.sum().backward()`` -- and must return, bit for bit, what it returns on fresh contiguous
copies. The wrappers make such inputs contiguous and 16-byte aligned before a kernel sees them
(lgcnhs.ops._aligned); outputs the caller hands in are checked instead (tests/test_arg_guards.py).
The stream tests run an entry under torch.cuda.stream(s) and expect the default stream's bits.

One small shape per family: 70 users, 3000 items, d = 64.
"""
import numpy as np
import pytest
import torch

import _poison as P
from oracle import lgcn_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
U, I, D = 70, 3000, 64


def _emb(n, d, seed, scale=0.1):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(n, d, generator=g) * scale).float()


def _rowsets(rp, col, n_rows, n_cols):
    from lgcnhs.graph import RowSets
    return RowSets(torch.as_tensor(np.asarray(rp, np.int64)).to(DEV),
                   torch.as_tensor(np.asarray(col, np.int32)).to(DEV), n_rows, n_cols)


# -------------------------------------------------------------------------------- the layouts
def _row_slices(t):
    """t as rows [3, 3 + n) of one concatenated table."""
    pad = torch.full((3, t.shape[1]), 7.0, dtype=t.dtype, device=t.device)
    v = torch.cat([pad, t, pad])[3:3 + t.shape[0]]
    assert v.is_contiguous()
    return v


def _split(t):
    """t as the second piece of torch.split."""
    return torch.split(torch.cat([t * 2.0, t]), t.shape[0])[1]


def _odd_offset(t):
    """t as a contiguous view one element into a larger buffer: 4 (fp32) or 8 (fp64) bytes off
    16-byte alignment."""
    buf = torch.full((t.numel() + 3,), 7.0, dtype=t.dtype, device=t.device)
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == t.element_size()
    return v


def _column_slice(t):
    """t as the first d columns of a table twice as wide."""
    wide = torch.cat([t, t * 3.0], dim=1)
    v = wide[:, :t.shape[1]]
    assert not v.is_contiguous()
    return v


def _transposed(t):
    """t stored column-major."""
    v = t.t().contiguous().t()
    assert v.stride() == (1, t.shape[0]) and not v.is_contiguous()
    return v


LAYOUTS = {"row_slices": _row_slices, "split": _split, "odd_offset": _odd_offset,
           "column_slice": _column_slice, "transposed": _transposed}


def _fresh(t):
    c = t.clone(memory_format=torch.contiguous_format)
    assert c.is_contiguous() and c.data_ptr() % 16 == 0
    return c


_T = {}


def _tables():
    if not _T:
        from lgcnhs import ops
        from lgcnhs.graph import Adjacency
        from lgcnhs.synth import synth_interactions
        eu, ei = _emb(U, D, 1).to(DEV), _emb(I, D, 2).to(DEV)
        rng = np.random.default_rng(3)
        n = int(U * I * 0.03)
        rp, col = O.exclusion_csr(U, I, (rng.integers(0, U, n), rng.integers(0, I, n)))
        # the same rows behind a 3-entry dummy row: slice_rows(1, U + 1) starts its rowptr 8
        # bytes off and points 3 entries into col
        big = _rowsets(np.concatenate([[0], rp + 3]), np.concatenate([[0, 1, 2], col]), U + 1, I)
        users, items = synth_interactions(U, I, 4000, seed=4)
        adj = Adjacency.from_interactions(torch.as_tensor(users), torch.as_tensor(items), U, I,
                                          DEV)
        A = ops.Interactions.from_pairs(torch.as_tensor(users), torch.as_tensor(items), U, I, DEV)
        _T.update(eu=eu, ei=ei, ex=_rowsets(rp, col, U, I), ex_view=big.slice_rows(1, U + 1),
                  adj=adj, e0=torch.cat([eu, ei]), A=A)
    return _T


def _check_layouts(call, eu, ei, layouts=LAYOUTS):
    """call(eu, ei) on every layout of both tables == call on fresh contiguous copies."""
    want = call(_fresh(eu), _fresh(ei))
    for name, view in layouts.items():
        vu, vi = view(eu), view(ei)
        assert torch.equal(vu, eu) and torch.equal(vi, ei)
        assert P.bit_equal(call(vu, vi), want), name
    return want


# ------------------------------------------------------------------------------- the entries
def test_exclusion_view_is_a_real_view():
    t = _tables()
    v = t["ex_view"]
    assert v.rowptr.data_ptr() % 16 == 8 and int(v.rowptr[0]) == 3
    assert v.rowptr.data_ptr() != t["ex"].rowptr.data_ptr()
    assert torch.equal(v.rowptr - 3, t["ex"].rowptr) and torch.equal(v.col[3:], t["ex"].col)


@pytest.mark.parametrize("screen", [True, False])
def test_score_topk_layouts(screen):
    from lgcnhs import ops
    t = _tables()
    want = _check_layouts(lambda eu, ei: ops.score_topk(eu, ei, 20, t["ex"], n_splits=3,
                                                        screen=screen), t["eu"], t["ei"])
    got = ops.score_topk(t["eu"], t["ei"], 20, t["ex_view"], n_splits=3, screen=screen)
    assert P.bit_equal(got, want)


def test_score_topk_wide_layouts():
    from lgcnhs import ops
    t = _tables()
    want = _check_layouts(lambda eu, ei: ops.score_topk(eu, ei, 256, t["ex"], n_splits=3),
                          t["eu"], t["ei"])
    assert P.bit_equal(ops.score_topk(t["eu"], t["ei"], 256, t["ex_view"], n_splits=3), want)


def test_score_topk_users_layouts():
    from lgcnhs import ops
    t = _tables()
    ids = torch.tensor([41, 3, 69, 0, 41], device=DEV)
    want = _check_layouts(lambda eu, ei: ops.score_topk_users(eu, ei, ids, 20, t["ex"]),
                          t["eu"], t["ei"])
    assert P.bit_equal(ops.score_topk_users(t["eu"], t["ei"], ids, 20, t["ex_view"]), want)
    # the ids themselves as a view 8 bytes off
    odd_ids = torch.cat([ids.new_zeros(1), ids])[1:]
    assert odd_ids.data_ptr() % 16 == 8
    assert P.bit_equal(ops.score_topk_users(t["eu"], t["ei"], odd_ids, 20, t["ex"]), want)


def _cand_rows():
    rng = np.random.default_rng(6)
    lens = [300, 0, 17, 300, 129, 5, 64, 300]
    rows = [np.sort(rng.permutation(I)[:n]) for n in lens]
    rp = np.zeros(9, np.int64)
    rp[1:] = np.cumsum(lens)
    return rp, np.concatenate(rows)


def test_score_topk_cand_layouts(monkeypatch):
    from lgcnhs import ops
    t = _tables()
    monkeypatch.setattr(ops, "CAND_MIN_SEG", 64)
    rp, col = _cand_rows()
    cand = _rowsets(rp, col, 8, I)
    big = _rowsets(np.concatenate([[0], rp + 3]), np.concatenate([[0, 1, 2], col]), 9, I)
    users = torch.tensor([5, 60, 7, 8, 33, 2, 69, 5], device=DEV)

    def call(eu, ei, c=cand):
        return ops.score_topk_cand(eu, ei, c, 20, t["ex"], users=users, max_len=300)

    want = _check_layouts(call, t["eu"], t["ei"])
    assert P.bit_equal(call(t["eu"], t["ei"], big.slice_rows(1, 9)), want)


def test_score_rank_layouts():
    from lgcnhs import ops
    t = _tables()
    rng = np.random.default_rng(7)
    rows = [np.sort(rng.permutation(I)[:u % 7]) for u in range(U)]
    rp = np.zeros(U + 1, np.int64)
    rp[1:] = np.cumsum([len(r) for r in rows])
    col = np.concatenate(rows)
    tg = _rowsets(rp, col, U, I)
    big = _rowsets(np.concatenate([[0], rp + 3]), np.concatenate([[0, 1, 2], col]), U + 1, I)

    def call(eu, ei, targets=tg, ex=None):
        return ops.score_rank(eu, ei, targets, t["ex"] if ex is None else ex, n_splits=3)

    want = _check_layouts(call, t["eu"], t["ei"])
    assert P.bit_equal(call(t["eu"], t["ei"], ex=t["ex_view"]), want)
    # a slice_rows view of the targets: its outputs are aligned with the whole col, the three
    # dummy entries in front belong to no row and get {-1, -inf}
    rk, sc = call(t["eu"], t["ei"], targets=big.slice_rows(1, U + 1))
    assert bool((rk[:3] == -1).all()) and bool((sc[:3] == float("-inf")).all())
    assert P.bit_equal((rk[3:], sc[3:]), want)


def test_bound_operands_layouts():
    from lgcnhs import ops
    t = _tables()
    _check_layouts(lambda eu, ei: ops.bound_operands(ei, with_err=True), t["eu"], t["ei"])


def test_score_dense_layouts():
    from lgcnhs import ops
    t = _tables()
    want = _check_layouts(lambda eu, ei: ops.score_dense(eu, ei[:333], None), t["eu"], t["ei"])
    ref = O.chain_scores(t["eu"].cpu().numpy(), t["ei"][:333].cpu().numpy())
    assert np.array_equal(want.cpu().numpy().view(np.uint32), ref.view(np.uint32))


def test_spread_resource_and_rows_topk_layouts():
    """fp64 W and F as views (W at an odd offset, as a column slice, transposed; F as the row
    block of a larger buffer, at an odd offset and transposed) and the fp32 tables of the G
    factor in every layout."""
    from lgcnhs import ops
    t = _tables()
    A = t["A"]
    W = ops.spread_hybrid(A, 0.4)
    F = ops.spread_resource(A, _fresh(W))
    for name in ("odd_offset", "column_slice", "transposed", "row_slices"):
        assert P.bit_equal(ops.spread_resource(A, LAYOUTS[name](W)), F), name
    # out=: a row block of a larger buffer and a wider buffer (row stride > I)
    buf = torch.full((U + 5, I), 7.0, dtype=torch.float64, device=DEV)
    assert ops.spread_resource(A, W, out=buf[2:U + 2]).data_ptr() == buf[2:].data_ptr()
    assert torch.equal(buf[2:U + 2], F) and bool((buf[:2] == 7.0).all()) \
        and bool((buf[U + 2:] == 7.0).all())
    wide = torch.full((U, I + 3), 7.0, dtype=torch.float64, device=DEV)
    ops.spread_resource(A, W, out=wide)
    assert torch.equal(wide[:, :I], F) and bool((wide[:, I:] == 7.0).all())
    with pytest.raises(TypeError):
        ops.spread_resource(A, W.float())
    with pytest.raises(ValueError):
        ops.spread_resource(A, W, out=buf[:, :I - 1])

    def call(eu, ei, Fv=F):
        return ops.rows_topk(Fv, 20, A.by_user, True, eu, ei)

    want = _check_layouts(call, t["eu"], t["ei"])
    Fn = F.cpu().numpy()
    G = O.chain_scores(t["eu"].cpu().numpy(), t["ei"].cpu().numpy()).astype(np.float64)
    ov, oi = O.rows_topk(G * Fn, 20, A.by_user.rowptr.cpu().numpy(), A.by_user.col.cpu().numpy())
    np.testing.assert_array_equal(want[1].cpu().numpy(), oi)
    assert np.array_equal(want[0].cpu().numpy().view(np.uint64), ov.view(np.uint64))
    for name in ("odd_offset", "column_slice", "transposed", "row_slices"):
        assert P.bit_equal(call(t["eu"], t["ei"], LAYOUTS[name](F)), want), name
    with pytest.raises(ValueError):
        ops.rows_topk(F, 20, A.by_user, True, t["eu"][:U - 1], t["ei"])


# -------------------------------------------------------------------------------- propagation
def test_propagate_forward_layouts():
    from lgcnhs import ops
    t = _tables()
    adj, e0 = t["adj"], t["e0"]
    want = ops.propagate(adj, _fresh(e0), 3)
    for name, view in LAYOUTS.items():
        assert P.bit_equal(ops.propagate(adj, view(e0), 3), want), name
        assert P.bit_equal(ops.propagate(adj, view(e0), 3, store=torch.float16),
                           ops.propagate(adj, _fresh(e0), 3, store=torch.float16)), name
    nodes = torch.tensor([5, 69, 70, 3069, 5], device=DEV)
    for name, view in LAYOUTS.items():
        assert P.bit_equal(ops.propagate_rows_mean(adj, view(e0), 3, nodes, force_masks=True),
                           want[nodes]), name
    # the layer entry itself refuses what it can not copy
    from lgcnhs import _native as N
    y = torch.empty_like(e0)
    with pytest.raises(ValueError):
        ops.spmm_layer(adj, _odd_offset(e0), y, None, None, None, N.LG_ACC_NONE, 1.0)
    with pytest.raises(ValueError):
        ops.spmm_layer(adj, _transposed(e0), y, None, None, None, N.LG_ACC_NONE, 1.0)
    with pytest.raises(ValueError):
        ops.spmm_layer(adj, e0, _odd_offset(y), None, None, None, N.LG_ACC_NONE, 1.0)
    with pytest.raises(TypeError):
        ops.spmm_layer(adj, e0.double(), None, None, None, None, N.LG_ACC_NONE, 1.0)


def test_propagate_backward_stride0_gradient_and_layouts():
    """out.sum().backward() hands the backward a stride-0 gradient; a leaf that is itself laid
    out oddly gets the same gradient values. Both equal the operator applied to ones
    (symmetric graph), on a fresh contiguous tensor."""
    from lgcnhs import ops
    t = _tables()
    adj, e0 = t["adj"], t["e0"]
    want = ops.propagate_mean(adj, torch.ones_like(e0), 3)
    a = _fresh(e0).requires_grad_(True)
    ops.propagate(adj, a, 3).sum().backward()
    assert P.bit_equal(a.grad, want)
    for name, view in LAYOUTS.items():
        b = view(e0).detach().requires_grad_(True)
        ops.propagate(adj, b, 3).sum().backward()
        assert torch.equal(b.grad, want), name
    # a weighted loss whose weights are a transposed tensor: a non-contiguous gradient
    w = _transposed(_emb(U + I, D, 9).to(DEV))
    c = _fresh(e0).requires_grad_(True)
    (ops.propagate(adj, c, 3) * w).sum().backward()
    assert P.bit_equal(c.grad, ops.propagate_mean(adj, _fresh(w), 3))


# ------------------------------------------------------------------------------- side streams
def _on_side_stream(call):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        out = call()
    torch.cuda.current_stream().wait_stream(s)
    return out


def test_side_stream_bits():
    from lgcnhs import ops
    t = _tables()
    rng = np.random.default_rng(7)
    rows = [np.sort(rng.permutation(I)[:u % 7]) for u in range(U)]
    rp = np.zeros(U + 1, np.int64)
    rp[1:] = np.cumsum([len(r) for r in rows])
    tg = _rowsets(rp, np.concatenate(rows), U, I)
    calls = {
        "propagate": lambda: ops.propagate(t["adj"], t["e0"], 3),
        "screened": lambda: ops.score_topk(t["eu"], t["ei"], 20, t["ex"], n_splits=3,
                                           screen=True),
        "wide": lambda: ops.score_topk(t["eu"], t["ei"], 256, t["ex"], n_splits=3),
        "rank": lambda: ops.score_rank(t["eu"], t["ei"], tg, t["ex"], n_splits=3),
    }
    torch.cuda.synchronize()
    for name, call in calls.items():
        want = call()
        assert P.bit_equal(_on_side_stream(call), want), name


def test_side_stream_tiled_spreading():
    """The tiled walk (fp64 LDS atomics): the same ids, values within the tiled-versus-dense
    tolerance."""
    from lgcnhs import ops
    from test_gpu_uninit import _tiled_same
    t = _tables()
    A = t["A"]

    def call():
        return ops.spread_topk_tiled(A, 0.4, 10, A.by_user, eu=t["eu"], ei=t["ei"], tile=64)

    want = call()
    torch.cuda.synchronize()
    assert _tiled_same(_on_side_stream(call), want)
