"""No result may depend on what an uninitialised buffer held.

Every entry below runs three times: plainly, with each torch.empty / empty_like of the library
starting from the final contents of the same buffer of a *decoy* problem (tests/_poison.py:
same shapes, graph, exclusions and candidates; embeddings scaled by 64 with the item rows
permuted, or another lambda / recs matrix where there are no embeddings -- so a stale float is
a score that dominates the real ones and a stale integer an id, count or cursor in range), and
with every such buffer filled with 0xFF bytes (NaN floats, -1 ids, set masks). The byte fill
runs only after the replay has passed. The three results are bit-identical (the tiled spreading
walk: identical ids, values within the tiled-versus-dense tolerance) and each equals the
reference the entry's own test file uses: the C chain oracle, the torch restatement of the
LightGCN forward, numpy's top-k over the dense fp64 F, or the numpy restatements of the metrics.

Shapes: the smallest at which every workspace region is live -- 70 users (a partial last
workgroup of every kernel), d = 64, several item splits / user blocks / chunks / segments
sharing one workspace.
"""
import numpy as np
import pytest
import torch

import _poison as P
from oracle import lgcn_oracle as O
from _compare import compare_lists_close

pytestmark = pytest.mark.gpu
DEV = "cuda"
U, D = 70, 64
NEG = float("-inf")


# ------------------------------------------------------------------------------ shared inputs
def _emb(n, d, seed, scale=0.1):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(n, d, generator=g) * scale).float()


def _rowsets(rp, col, n_rows, n_cols):
    from lgcnhs.graph import RowSets
    return RowSets(torch.as_tensor(np.asarray(rp, np.int64)).to(DEV),
                   torch.as_tensor(np.asarray(col, np.int32)).to(DEV), n_rows, n_cols)


def _decoy_tables(eu, ei):
    """Embeddings scaled by 64 (scores by 4096: every stale score beats every real one), the
    item rows permuted (every stale id names another item)."""
    perm = torch.randperm(ei.shape[0], generator=torch.Generator().manual_seed(99))
    return eu * 64.0, ei[perm] * 64.0


_TABLES = {}


def _tables(I, n_users=U, d=D):
    """n_users x I tables with 3 % exclusions: host copies, device copies of the real and the
    decoy embeddings, the exclusion CSR on both sides. Computed once, never written."""
    key = (I, n_users, d)
    if key not in _TABLES:
        eu, ei = _emb(n_users, d, 1000 + I), _emb(I, d, 2000 + I)
        rng = np.random.default_rng(I)
        n = int(n_users * I * 0.03)
        rp, col = O.exclusion_csr(n_users, I, (rng.integers(0, n_users, n),
                                               rng.integers(0, I, n)))
        du, di = _decoy_tables(eu, ei)
        _TABLES[key] = dict(eu=eu.numpy(), ei=ei.numpy(), rp=rp, col=col,
                            real=(eu.to(DEV), ei.to(DEV)), decoy=(du.to(DEV), di.to(DEV)),
                            ex=_rowsets(rp, col, n_users, I))
    return _TABLES[key]


_ORACLE = {}


def _chain(I, k, n_users=U):
    """O.chain_topk of the shared tables, once per (I, k)."""
    key = (I, k, n_users)
    if key not in _ORACLE:
        t = _tables(I, n_users)
        _ORACLE[key] = O.chain_topk(t["eu"], t["ei"], t["rp"], t["col"], k)
    return _ORACLE[key]


def _lists_equal(out, want, how, rows=None):
    """(values fp32, ids int64) on the device == the oracle's numpy lists, ids and value bits."""
    v, i = (x.cpu().numpy() for x in out)
    wv, wi = want if rows is None else (want[0][rows], want[1][rows])
    np.testing.assert_array_equal(i, wi, err_msg=how)
    assert np.array_equal(v.view(np.uint32), np.ascontiguousarray(wv).view(np.uint32)), how


def _score_topk_three_ways(I, k, n_users=U, **kw):
    from lgcnhs import ops
    t = _tables(I, n_users)

    def run(tabs):
        return ops.score_topk(tabs[0], tabs[1], k, t["ex"], **kw)

    want = _chain(I, k, n_users)
    return P.three_ways(lambda: run(t["real"]), lambda: run(t["decoy"]),
                        lambda out, how: _lists_equal(out, want, f"{how} I={I} k={k} {kw}"))


# --------------------------------------------------------------------------------- score_topk
@pytest.mark.parametrize("I,k,ns", [(600, 20, 1), (600, 20, 3), (600, 128, 1), (600, 128, 3),
                                    (300, 128, 3)])
def test_score_topk_plain(I, k, ns):
    """lg_score_topk_f32: the outputs (one split) and the [splits, users, k] partial lists the
    merge reads (several; 300 items in 3 splits: every partial list shorter than k, its tail
    padding the merge must see as such)."""
    _score_topk_three_ways(I, k, n_splits=ns, screen=False)


@pytest.mark.parametrize("ns", [1, 3])
@pytest.mark.parametrize("I,k", [(3000, 20), (40000, 20), (70000, 64), (3000, 100)])
def test_score_topk_screened(I, k, ns):
    """lg_score_topk_screened_f32: LDS lists without a seed (3000 x 20) and with the seed the
    seed pass parks in the K-th slot of out_val (40000 x 20; with 3 splits the per-split seeds
    in the partial rows and their combination), global list slabs with a seed (70000 x 64) and
    without (3000 x 100), the bf16 operands and norms of bound_operands."""
    _score_topk_three_ways(I, k, n_splits=ns, screen=True)


@pytest.mark.parametrize("ns", [1, 3])
def test_score_topk_wide(ns):
    """lg_score_topk_wide_f32 (k = 256): the slabs every insertion, compaction and the merge go
    through."""
    _score_topk_three_ways(3000, 256, n_splits=ns)


@pytest.mark.parametrize("ns", [1, 3])
def test_score_topk_wide_user_blocks_share_one_workspace(ns, monkeypatch):
    """150 users under a workspace cap of one workgroup's slabs: three consecutive user blocks
    (64, 64, 22) reuse one ws, so blocks two and three start from another block's lists in any
    run; the poisoned runs add stale lists to the first."""
    from lgcnhs import ops
    from lgcnhs import _native as N
    nu, I, k = 150, 3000, 256
    cap = N.lib().lg_score_topk_wide_ws_bytes(64, I, D, k, ns)
    monkeypatch.setattr(ops, "WIDE_WS_CAP_BYTES", cap)
    assert ops._wide_user_block(nu, I, D, k, ns, cap) == 64
    _score_topk_three_ways(I, k, n_users=nu, n_splits=ns)


# --------------------------------------------------------------------------- score_topk_users
def _restrict_np(rp, col, n_rows, cand):
    """tests/test_gpu_topk_items.py's numpy restatement of RowSets.restrict_cols."""
    rows = np.repeat(np.arange(n_rows), np.diff(rp))
    keep = np.isin(col, cand)
    return O.exclusion_csr(n_rows, len(cand), (rows[keep], np.searchsorted(cand, col[keep])))


_ITEM_ORACLE = {}


def _chain_items(I, k, cand):
    """The C chain oracle on the candidates' sub-table, ids mapped back (all users)."""
    key = (I, k, len(cand))
    if key not in _ITEM_ORACLE:
        t = _tables(I)
        srp, scol = _restrict_np(t["rp"], t["col"], U, cand)
        ov, oi = O.chain_topk(t["eu"], np.ascontiguousarray(t["ei"][cand]), srp, scol, k)
        _ITEM_ORACLE[key] = (ov, np.where(oi >= 0, cand[np.maximum(oi, 0)], -1))
    return _ITEM_ORACLE[key]


def _users_three_ways(ids, k, with_items):
    from lgcnhs import ops
    I = 3000
    t = _tables(I)
    cand = np.sort(np.random.default_rng(5).permutation(I)[:I // 10]).astype(np.int32)
    items = torch.as_tensor(cand).to(DEV) if with_items else None
    want = _chain_items(I, k, cand) if with_items else _chain(I, k)
    uid = torch.as_tensor(ids).to(DEV)

    def run(tabs):
        return ops.score_topk_users(tabs[0], tabs[1], uid, k, t["ex"], items=items)

    return P.three_ways(lambda: run(t["real"]), lambda: run(t["decoy"]),
                        lambda out, how: _lists_equal(out, want, f"{how} k={k}", rows=ids))


@pytest.mark.parametrize("with_items", [False, True])
@pytest.mark.parametrize("k", [20, 128])
def test_score_topk_users(k, with_items):
    """lg_score_topk_batch_f32 / lg_score_topk_batch_items_f32: one partial list per
    (workgroup, user) and their merge, 5 ids with a duplicate."""
    _users_three_ways(np.array([41, 3, 69, 0, 41]), k, with_items)


@pytest.mark.parametrize("with_items", [False, True])
@pytest.mark.parametrize("k", [20, 128])
def test_score_topk_users_chunks_share_one_workspace(k, with_items, monkeypatch):
    """130 ids under raised batch limits: _topk_lists loops chunks of 64 (full catalog: 64, 64,
    2) or 16 (candidates: nine) over one workspace sized for a full chunk; the short last chunk
    lays its lists out differently inside it."""
    from lgcnhs import ops
    monkeypatch.setattr(ops, "BATCH_MAX_USERS", 200)
    monkeypatch.setattr(ops, "ITEMS_BATCH_MAX_USERS", 200)
    ids = np.random.default_rng(8).integers(0, U, 130)
    _users_three_ways(ids, k, with_items)


# ----------------------------------------------------------------------- candidate-list top-k
def _cand_request(I):
    """8 rows of <= 700 ascending candidates over I items: row 2 empty, row 5 of 10 (shorter
    than either k), for 8 distinct users."""
    rng = np.random.default_rng(21)
    users = rng.permutation(U)[:8].astype(np.int64)
    lens = [700, 650, 0, 700, 333, 10, 700, 65]
    rows = [np.sort(rng.permutation(I)[:n]).astype(np.int32) for n in lens]
    rp = np.zeros(9, np.int64)
    rp[1:] = np.cumsum(lens)
    return users, rows, rp, np.concatenate(rows).astype(np.int32)


def _chain_row(t, u, cand, k):
    """tests/test_gpu_topk_cand.py's twin (b): the C chain oracle on one user's sub-problem."""
    if len(cand) == 0:
        return np.full(k, NEG, np.float32), np.full(k, -1, np.int64)
    ex = t["col"][t["rp"][u]:t["rp"][u + 1]]
    pos = np.nonzero(np.isin(cand, ex))[0].astype(np.int32)
    ov, oi = O.chain_topk(t["eu"][u:u + 1], np.ascontiguousarray(t["ei"][cand]),
                          np.array([0, len(pos)], np.int64), pos, k)
    return ov[0], np.where(oi[0] >= 0, cand[np.maximum(oi[0], 0)], -1)


@pytest.mark.parametrize("k", [20, 100])
def test_score_topk_cand(k, monkeypatch):
    """lg_score_topk_cand_f32 with CAND_MIN_SEG = 64: rows split into 11 segments whose partial
    lists are merged; an empty row and a row shorter than k come out as {-inf, -1} padding."""
    from lgcnhs import ops
    I = 5000
    t = _tables(I)
    users, rows, rp, col = _cand_request(I)
    monkeypatch.setattr(ops, "CAND_MIN_SEG", 64)
    assert ops.cand_segments(8, 700, k, DEV) == 11
    cand = _rowsets(rp, col, 8, I)
    uid = torch.as_tensor(users).to(DEV)
    want = [_chain_row(t, int(u), c, k) for u, c in zip(users, rows)]
    want = (np.stack([w[0] for w in want]), np.stack([w[1] for w in want]))

    def run(tabs):
        return ops.score_topk_cand(tabs[0], tabs[1], cand, k, t["ex"], users=uid, max_len=700)

    def check(out, how):
        _lists_equal(out, want, f"{how} k={k}")
        v, i = out
        assert bool((i[2] == -1).all()) and bool((v[2] == NEG).all()), how  # the empty row
        assert bool((i[5, 10:] == -1).all()) and bool((v[5, 10:] == NEG).all()), how
        assert bool((i[5, :10] >= 0).all()), how  # (excluded candidates rank, at the mask)

    P.three_ways(lambda: run(t["real"]), lambda: run(t["decoy"]), check)


def test_score_cand_allocates_nothing_uninitialised():
    """lg_score_cand_f32 writes into a -inf filled output and has no workspace: under the
    harness nothing is intercepted, and the scores equal the chain oracle's masked matrix."""
    from lgcnhs import ops
    I = 5000
    t = _tables(I)
    users, rows, rp, col = _cand_request(I)
    cand = _rowsets(rp, col, 8, I)
    G = O.chain_masked_matrix(t["eu"], t["ei"], t["rp"], t["col"])
    want = np.concatenate([G[u, c] for u, c in zip(users, rows)]).astype(np.float32)
    with P.fill_bytes(0xFF) as h:
        got = ops.score_cand(*t["real"], cand, t["ex"], users=torch.as_tensor(users).to(DEV),
                             max_len=700)
    assert h.count == 0
    assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32))


# --------------------------------------------------------------------------------- score_rank
def _rank_ref(G, rows):
    """tests/test_gpu_score_rank.py's definition on the masked matrix."""
    ids = np.arange(G.shape[1])
    rk, sc = [], []
    for u, row in enumerate(rows):
        for i in row:
            b = (G[u] > G[u, i]) | ((G[u] == G[u, i]) & (ids < i))
            b[i] = False
            rk.append(int(b.sum()))
            sc.append(G[u, i])
    return np.asarray(rk, np.int64), np.asarray(sc, np.float32)


@pytest.mark.parametrize("ns", [1, 3])
def test_score_rank(ns):
    """lg_score_rank_f32: the thresholds and target ids step 1 leaves for steps 2 and 3 and the
    per-split counts. User u has u % 10 targets, so rows above RANK_ROW_MAX become several
    kernel rows and the plan's padding rows exist; a quarter of the targets are excluded."""
    from lgcnhs import ops
    I = 3000
    t = _tables(I)
    rng = np.random.default_rng(31)
    rows = [np.sort(rng.permutation(I)[:u % 10]) for u in range(U)]
    assert max(len(r) for r in rows) > ops.RANK_ROW_MAX
    tu = np.asarray([u for u, r in enumerate(rows) for _ in r][::4])
    ti = np.asarray([i for r in rows for i in r][::4])
    rp, col = O.exclusion_csr(U, I, (np.repeat(np.arange(U), np.diff(t["rp"])), t["col"]),
                              (tu, ti))
    ex = _rowsets(rp, col, U, I)
    want = _rank_ref(O.chain_masked_matrix(t["eu"], t["ei"], rp, col), rows)
    trp = np.zeros(U + 1, np.int64)
    trp[1:] = np.cumsum([len(r) for r in rows])
    tg = _rowsets(trp, np.concatenate(rows), U, I)

    def run(tabs):
        return ops.score_rank(tabs[0], tabs[1], tg, ex, n_splits=ns)

    def check(out, how):
        rk, sc = out
        np.testing.assert_array_equal(rk.cpu().numpy(), want[0], err_msg=how)
        assert np.array_equal(sc.cpu().numpy().view(np.uint32), want[1].view(np.uint32)), how

    P.three_ways(lambda: run(t["real"]), lambda: run(t["decoy"]), check)


# ---------------------------------------------------------------- dense scores and the bounds
def test_score_dense():
    from lgcnhs import ops
    nu, I = 37, 333
    t = _tables(I, nu)
    want = O.chain_masked_matrix(t["eu"], t["ei"], t["rp"], t["col"])

    def check(out, how):
        assert np.array_equal(out.cpu().numpy().view(np.uint32), want.view(np.uint32)), how

    P.three_ways(lambda: ops.score_dense(*t["real"], t["ex"]),
                 lambda: ops.score_dense(*t["decoy"], t["ex"]), check)


@pytest.mark.parametrize("d", [64, 48])
def test_bound_operands(d):
    """lg_bound_prep_f32 (d = 48: the generic kernel): the bf16 copy is torch's round to nearest
    even, the norms are rounded up, within 1e-6 of the fp64 norms
    (tests/test_gpu_topk.py::test_bound_prep_rounds_and_bounds)."""
    from lgcnhs import ops
    x = _emb(333, d, 7) * torch.exp(_emb(333, 1, 8, scale=2.0))
    x[3] = 0.0
    xd, dd = x.to(DEV), (x * 64.0).flip(0).contiguous().to(DEV)
    xb_want = x.to(torch.bfloat16).view(torch.int16)
    n64 = x.double().norm(dim=1)
    e64 = (x.double() - x.to(torch.bfloat16).double()).norm(dim=1)

    def check(out, how):
        xb, nrm, err = (o.cpu() for o in out)
        assert torch.equal(xb, xb_want), how
        for got, ref in ((nrm, n64), (err, e64)):
            g = got.double()
            assert bool((g >= ref).all()), how
            assert bool(((g - ref) <= 1e-6 * ref + 1e-38).all()), how

    P.three_ways(lambda: ops.bound_operands(xd, with_err=True),
                 lambda: ops.bound_operands(dd, with_err=True), check)


def test_chunk_bounds_with_column_bounds():
    """lg_score_chunk_bound into a caller's gb and qout buffers: both cover the chain scores
    (tests/test_gpu_spread_tiled.py's property), whatever the buffers held."""
    from lgcnhs import ops
    nu, I, j0, W = 37, 333, 40, 200
    t = _tables(I, nu)
    G = O.chain_scores(t["eu"], t["ei"][j0:j0 + W]).astype(np.float64)
    qs = -(-W // 256) * 256

    def run(tabs):
        ub, un = ops.bound_operands(tabs[0])
        ib, inorm = ops.bound_operands(tabs[1])
        q = torch.empty((nu, qs), dtype=torch.uint8, device=DEV)
        gb, q = ops.chunk_bounds(ub, un, ib, inorm, D, j0, W, qout=q)
        return gb.clone(), q[:, :W].clone()  # (columns past the width are not written)

    def check(out, how):
        gb, q = (o.cpu().numpy().astype(np.float64) for o in out)
        assert np.isfinite(gb).all(), how
        chunk = np.arange(W) // 64
        assert bool((gb[:, chunk] >= G).all()), how
        assert bool((gb[:, chunk] * q / 255.0 >= G).all()), how

    P.three_ways(lambda: run(t["real"]), lambda: run(t["decoy"]), check)


# -------------------------------------------------------------------------------- propagation
_GRAPHS = {}


def _graph(n_users, n_items, E):
    """(users, items, coo) of a synthetic graph, once."""
    key = (n_users, n_items, E)
    if key not in _GRAPHS:
        from lgcnhs.synth import synth_interactions
        users, items = synth_interactions(n_users, n_items, E, seed=7)
        _GRAPHS[key] = (users, items, torch.as_tensor(O.coo_adjacency(n_users, n_items, users,
                                                                      items)))
    return _GRAPHS[key]


def _adjacency(n_users, n_items, E):
    """A fresh Adjacency (its dis / edge weights / long-row plan are allocated by whoever uses
    it first: inside the harness they are poisoned too)."""
    from lgcnhs.graph import Adjacency
    users, items, _ = _graph(n_users, n_items, E)
    return Adjacency.from_interactions(torch.as_tensor(users), torch.as_tensor(items), n_users,
                                       n_items, DEV)


def _e0_pair(n, d):
    e0 = _emb(n, d, 11 + d)
    return e0, e0.to(DEV), (e0 * 64.0).flip(0).contiguous().to(DEV)


@pytest.mark.parametrize("shape,d", [((3000, 2000, 60000), 64), ((3000, 2000, 60000), 256),
                                     ((10000, 8, 60000), 64)])
def test_propagate_forward(shape, d):
    """Three layers: the ping-pong layer buffers, dis, the edge weights and, on the graph of 8
    items with ~7,500 users each (rows above LONG_ROW_THRESHOLD), plan.partial."""
    from lgcnhs import ops
    from lgcnhs import graph as G
    nu, ni, E = shape
    coo = _graph(*shape)[2]
    e0, real, decoy = _e0_pair(nu + ni, d)
    if ni == 8:
        adj = _adjacency(*shape)
        assert adj.long_plan().n_long == 8 and adj.long_plan().n_seg > 8
        assert int((adj.rowptr[1:] - adj.rowptr[:-1]).max()) > G.LONG_ROW_THRESHOLD
    uf, itf = O.lightgcn_forward(coo, e0[:nu], e0[nu:], 3)
    want = torch.cat([uf, itf]).numpy()

    def check(out, how):
        np.testing.assert_allclose(out.cpu().numpy(), want, rtol=0, atol=1e-4, err_msg=how)

    P.three_ways(lambda: ops.propagate(_adjacency(*shape), real, 3),
                 lambda: ops.propagate(_adjacency(*shape), decoy, 3), check)


@pytest.mark.parametrize("shape", [(3000, 2000, 60000), (10000, 8, 60000)])
def test_propagate_half_storage(shape):
    """store=torch.float16: the float16 ping-pong buffers; bitwise the loop over the fp32 kernel
    on the widened operands (tests/test_gpu_half_storage.py's definition)."""
    from lgcnhs import ops
    from test_gpu_half_storage import _loop_reference
    nu, ni, E = shape
    _, real, decoy = _e0_pair(nu + ni, D)
    want = _loop_reference(_adjacency(*shape), real, 3)

    def check(out, how):
        assert torch.equal(out.view(torch.int32), want.view(torch.int32)), how

    P.three_ways(lambda: ops.propagate(_adjacency(*shape), real, 3, store=torch.float16),
                 lambda: ops.propagate(_adjacency(*shape), decoy, 3, store=torch.float16), check)


def test_propagate_backward_live_rows():
    """The backward of a loss over 40 rows: the gradient's live rows go through
    lg_spmm_layer_live_f32 (sparse_input), later layers through the dense kernel. The symmetric
    graph's backward is the forward operator: equal to the oracle's forward of the gradient."""
    from lgcnhs import ops
    shape = (3000, 2000, 60000)
    nu, ni, _ = shape
    n = nu + ni
    coo = _graph(*shape)[2]
    _, real, decoy = _e0_pair(n, D)
    rows = torch.randperm(n, generator=torch.Generator().manual_seed(3))[:40]
    w = _emb(40, D, 4, scale=1.0)
    g = torch.zeros(n, D)
    g[rows] = w
    uf, itf = O.lightgcn_forward(coo, g[:nu], g[nu:], 3)
    want = torch.cat([uf, itf]).numpy()
    rows_d, w_d = rows.to(DEV), w.to(DEV)

    def run(e0, scale):
        a = e0.clone().requires_grad_(True)
        (ops.propagate(_adjacency(*shape), a, 3)[rows_d] * (w_d * scale)).sum().backward()
        return a.grad

    def check(out, how):
        np.testing.assert_allclose(out.cpu().numpy(), want, rtol=0, atol=1e-4, err_msg=how)

    P.three_ways(lambda: run(real, 1.0), lambda: run(decoy, 64.0), check)


def test_propagate_rows_forced_masks():
    """propagate_rows_mean with every layer masked: rows outside the masks are never written
    (they keep whatever the buffers held) and never read."""
    from lgcnhs import ops
    shape = (3000, 2000, 60000)
    nu, ni, _ = shape
    coo = _graph(*shape)[2]
    e0, real, decoy = _e0_pair(nu + ni, D)
    nodes = torch.randint(0, nu + ni, (90,), generator=torch.Generator().manual_seed(5))
    nodes[5] = nodes[17]
    uf, itf = O.lightgcn_forward(coo, e0[:nu], e0[nu:], 3)
    want = torch.cat([uf, itf])[nodes].numpy()
    nd = nodes.to(DEV)

    def check(out, how):
        np.testing.assert_allclose(out.cpu().numpy(), want, rtol=0, atol=1e-4, err_msg=how)

    P.three_ways(
        lambda: ops.propagate_rows_mean(_adjacency(*shape), real, 3, nd, force_masks=True),
        lambda: ops.propagate_rows_mean(_adjacency(*shape), decoy, 3, nd, force_masks=True),
        check)


# ---------------------------------------------------------------------------- dense spreading
SU, SI, SE = 300, 900, 9000
_SPREAD = {}


def _spread():
    """The 300 x 900 graph (9000 interactions, Zipf items), its W and F for lambda = 0.4 from
    the plain dense path, and embeddings for the G factor. Once."""
    if not _SPREAD:
        from lgcnhs import ops
        from lgcnhs.synth import synth_interactions
        u, i = synth_interactions(SU, SI, SE, seed=31, dist="zipf")
        A = ops.Interactions.from_pairs(torch.as_tensor(u), torch.as_tensor(i), SU, SI, DEV)
        W = ops.spread_hybrid(A, 0.4)
        F = ops.spread_resource(A, W)
        eu, ei = _emb(SU, D, 41), _emb(SI, D, 42)
        du, di = _decoy_tables(eu, ei)
        _SPREAD.update(A=A, W=W, F=F, Fn=F.cpu().numpy(), pairs=(u, i),
                       An=O.interaction_matrix(SU, SI, u, i),
                       G=O.chain_scores(eu.numpy(), ei.numpy()).astype(np.float64),
                       real=(eu.to(DEV), ei.to(DEV)), decoy=(du.to(DEV), di.to(DEV)),
                       W2=ops.spread_hybrid(A, 0.9),
                       rp=A.by_user.rowptr.cpu().numpy(), col=A.by_user.col.cpu().numpy())
    return _SPREAD


def _f64_lists_equal(out, want, how):
    v, i = (x.cpu().numpy() for x in out)
    np.testing.assert_array_equal(i, want[1], err_msg=how)
    assert np.array_equal(np.ascontiguousarray(v).view(np.uint64),
                          np.ascontiguousarray(want[0]).view(np.uint64)), how


def test_spread_hybrid():
    """lg_spread_hybrid_f64: W and its workspace (the factors and the users' range starts);
    within 1e-12 of HybridS over getSpreadingGeneralMat in numpy."""
    from lgcnhs import ops
    s = _spread()
    want = O.hybrid_s(s["An"], O.spreading_general_mat(s["An"]), 0.4)

    def check(out, how):
        np.testing.assert_allclose(out.cpu().numpy(), want, rtol=1e-12, atol=0, err_msg=how)

    P.three_ways(lambda: ops.spread_hybrid(s["A"], 0.4), lambda: ops.spread_hybrid(s["A"], 0.9),
                 check)


@pytest.mark.parametrize("use_g", [False, True])
def test_spread_topk_blocks_share_one_buffer(use_g):
    """spread_topk with block_users = 64: five user blocks through one F buffer (the last block
    of 44 leaves 20 rows of the previous block's F in it)."""
    from lgcnhs import ops
    s = _spread()
    k = 20
    want = O.rows_topk(s["G"] * s["Fn"] if use_g else s["Fn"], k, s["rp"], s["col"])

    def run(W, tabs):
        eu, ei = tabs if use_g else (None, None)
        return ops.spread_topk(s["A"], W, k, s["A"].by_user, True, eu, ei, block_users=64)

    P.three_ways(lambda: run(s["W"], s["real"]), lambda: run(s["W2"], s["decoy"]),
                 lambda out, how: _f64_lists_equal(out, want, f"{how} G={use_g}"))


@pytest.mark.parametrize("use_g", [False, True])
@pytest.mark.parametrize("k", [20, 256])
def test_rows_topk(k, use_g):
    """lg_rows_topk_f64 (k = 20) and lg_rows_topk_wide_f64 (k = 256) on the dense F."""
    from lgcnhs import ops
    s = _spread()
    want = O.rows_topk(s["G"] * s["Fn"] if use_g else s["Fn"], k, s["rp"], s["col"])
    F2 = ops.spread_resource(s["A"], s["W2"])

    def run(F, tabs):
        eu, ei = tabs if use_g else (None, None)
        return ops.rows_topk(F, k, s["A"].by_user, True, eu, ei)

    def check(out, how):
        _f64_lists_equal(out, want, f"{how} k={k} G={use_g}")
    P.three_ways(lambda: run(s["F"], s["real"]), lambda: run(F2, s["decoy"]), check)


@pytest.mark.parametrize("k", [20, 256])
def test_spread_rows_topk_items(k):
    """lg_spread_rows_topk_items_f64 over a 10 % candidate set: numpy's top-k over those columns
    of the dense F, ids mapped back."""
    from lgcnhs import ops
    s = _spread()
    cand = np.sort(np.random.default_rng(6).permutation(SI)[:SI // 10]).astype(np.int32)
    srp, scol = _restrict_np(s["rp"], s["col"], SU, cand)
    ov, oi = O.rows_topk(np.ascontiguousarray(s["Fn"][:, cand]), k, srp, scol)
    want = (ov, np.where(oi >= 0, cand[np.maximum(oi, 0)], -1))
    cd = torch.as_tensor(cand).to(DEV)

    def run(W):
        return ops.spread_rows_topk_items(s["A"].by_user, W, cd, k, s["A"].by_user)

    def check(out, how):
        _f64_lists_equal(out, want, f"{how} k={k}")
        v, i = out
        if k == 256:  # (90 candidates: every row's tail is padding)
            assert bool((i[:, 90:] == -1).all()) and bool((v[:, 90:] == NEG).all()), how

    P.three_ways(lambda: run(s["W"]), lambda: run(s["W2"]), check)


@pytest.mark.parametrize("k", [64, 200])
def test_merge_topk_lists(k):
    """lg_topk_lists_merge_f64 / _wide_f64, three lists per row with ties, empty and full rows
    (tests/test_gpu_spread_wide.py's generator and numpy merge)."""
    from lgcnhs import ops
    from test_gpu_spread_wide import _np_merge, _sorted_lists
    vals, idxs = _sorted_lists(3, 21, k, seed=k)
    dvals, didxs = _sorted_lists(3, 21, k, seed=k + 1)
    want = _np_merge(vals, idxs, k)
    real = (torch.as_tensor(vals).to(DEV), torch.as_tensor(idxs).to(DEV))
    decoy = (torch.as_tensor(dvals * 64.0).to(DEV), torch.as_tensor(didxs).to(DEV))

    def check(out, how):
        _f64_lists_equal(out, want, f"{how} k={k}")
        assert bool((out[0][out[1] < 0] == NEG).all()), how

    P.three_ways(lambda: ops.merge_topk_lists(*real), lambda: ops.merge_topk_lists(*decoy),
                 check)


# ---------------------------------------------------------------------------- tiled spreading
def _tiled_same(a, b):
    """The walk sums F in LDS with fp64 atomics: ids identical, values within the tolerance of
    the tiled-versus-dense tests (1e-12 relative)."""
    (va, ia), (vb, ib) = a, b
    if not torch.equal(ia, ib):
        return False
    fin = ia >= 0
    if not torch.equal(va[~fin], vb[~fin]):
        return False
    x, y = va[fin], vb[fin]
    return bool(((x - y).abs() <= 1e-12 * y.abs().clamp(min=torch.finfo(torch.float64).tiny))
                .all())


@pytest.mark.parametrize("mode", ["G_drop", "none"])
@pytest.mark.parametrize("k", [10, 200])
def test_spread_topk_tiled(k, mode):
    """spread_topk_tiled with tile = 64 (15 tiles in one group; k = 200: two peeled passes): the
    TileWeights it builds inside the harness -- cursors, counts, records, bounds, units, lines,
    row lengths, the hub workspace -- the walk's running lists and, with G, the bound buffers.
    Against numpy's top-k over the dense F, as the tiled-versus-dense tests compare."""
    from lgcnhs import ops
    s = _spread()
    use_g, drop = mode == "G_drop", mode != "none"
    want = O.rows_topk(s["G"] * s["Fn"] if use_g else s["Fn"], k, s["rp"], s["col"], drop)

    def run(lam, tabs):
        eu, ei = tabs if use_g else (None, None)
        return ops.spread_topk_tiled(s["A"], lam, k, s["A"].by_user, drop=drop, eu=eu, ei=ei,
                                     tile=64)

    def check(out, how):
        v, i = (x.cpu().numpy() for x in out)
        compare_lists_close(v, i, want[0], want[1], label=f"{how} k={k} {mode}")
        assert bool((v[i < 0] == NEG).all()), how

    P.three_ways(lambda: run(0.4, s["real"]), lambda: run(0.9, s["decoy"]), check,
                 same=_tiled_same)


# ------------------------------------------------------------------------------------ metrics
_METRICS = {}


def _metric_inputs():
    """64 lists of 12 over 60 items (repeats, -1 pads), a 5000-user interaction matrix whose
    item 0 is a hub column longer than the 2048 users the kernel stages in LDS, and a decoy recs
    matrix."""
    if not _METRICS:
        from lgcnhs.graph import RowSets
        rng = np.random.default_rng(5)
        n_users, I, k = 5000, 60, 12
        A = (rng.random((n_users, I)) < 0.05).astype(np.float64)
        A[:, 0] = rng.random(n_users) < 0.8
        deg = A.sum(0).astype(np.int64)
        assert deg[0] > 2048
        deg[7] = 0
        recs = np.stack([rng.choice(I, size=k, replace=False) for _ in range(64)])
        recs[::2, 0] = 0
        recs[::7, 5] = recs[::7, 4]
        recs[::11, -3:] = -1
        decoy = np.stack([rng.choice(I, size=k, replace=False) for _ in range(64)])
        users, items = np.nonzero(A)
        by_item = RowSets.from_pairs(torch.as_tensor(items), torch.as_tensor(users), I, n_users,
                                     DEV)
        _METRICS.update(A=A, deg=deg, recs=recs, I=I, k=k, by_item=by_item,
                        real=torch.as_tensor(recs).to(DEV), decoy=torch.as_tensor(decoy).to(DEV))
    return _METRICS


def test_metric_hit_flags():
    from lgcnhs import metrics as M
    m = _metric_inputs()
    rng = np.random.default_rng(9)
    eval_rows = np.sort(rng.permutation(64)[:40])
    pos = [np.sort(rng.permutation(m["I"])[:1 + q % 9]) for q in range(40)]
    prp = np.zeros(41, np.int64)
    prp[1:] = np.cumsum([len(p) for p in pos])
    ps = _rowsets(prp, np.concatenate(pos), 40, m["I"])
    want = np.array([[int(it >= 0 and it in set(pos[q].tolist())) for it in m["recs"][u]]
                     for q, u in enumerate(eval_rows)], np.uint8)
    er = torch.as_tensor(eval_rows).to(DEV)

    def check(out, how):
        np.testing.assert_array_equal(out.cpu().numpy(), want, err_msg=how)

    P.three_ways(lambda: M.hit_flags(m["real"], er, ps), lambda: M.hit_flags(m["decoy"], er, ps),
                 check)


def test_metric_pair_overlap():
    """lg_rec_pair_overlap clears the per-item counts it accumulates into: another recs matrix's
    counts (or -1) in that buffer must not reach the total."""
    from lgcnhs import metrics as M
    m = _metric_inputs()
    B = np.zeros((64, m["I"]), np.int64)
    for u in range(64):
        B[u, np.unique(m["recs"][u][m["recs"][u] >= 0])] = 1
    Gm = B @ B.T
    want = int(Gm.sum() - np.trace(Gm))

    def check(out, how):
        assert int(out) == want, how

    P.three_ways(lambda: torch.tensor(M.pair_overlap(m["real"], m["I"])),
                 lambda: torch.tensor(M.pair_overlap(m["decoy"], m["I"])), check)


def test_metric_intra_similarity_parts():
    from lgcnhs import metrics as M
    m = _metric_inputs()
    A, deg, recs, k = m["A"], m["deg"], m["recs"], m["k"]
    want = np.zeros((64, k))
    for r in range(64):
        for p in range(k):
            a, s = recs[r, p], 0.0
            for q in range(p + 1, k):
                b = recs[r, q]
                if a == b or a < 0 or b < 0 or deg[a] == 0 or deg[b] == 0:
                    continue
                s += np.dot(A[:, a], A[:, b]) / np.sqrt(int(deg[a]) * int(deg[b]))
            want[r, p] = s
    dg = torch.as_tensor(deg)

    def check(out, how):
        assert np.array_equal(out.cpu().numpy().reshape(64, k), want), how

    P.three_ways(lambda: M.intra_similarity_parts(m["real"], m["by_item"], dg),
                 lambda: M.intra_similarity_parts(m["decoy"], m["by_item"], dg), check)
