"""GPU parity of K2b (lg_score_topk_batch_f32, csrc/topk_batch.hip): top-K for a short list
of user ids into the full tables. Every row is compared bit for bit (values, ids, order,
padding) with the same user's row of ops.score_topk(..., screen=False) -- lg_score_topk_f32 on
the whole table -- and a subset with the C chain oracle; then the Python layers on top of it
(RowSets.take, ops.score_topk_users, recommendForUsers, spread_recommend(users=))."""
import numpy as np
import pytest
import torch

from oracle import lgcn_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
U_TAB = 200  # users of the tables the ids point into


def _emb(n, d, seed, scale=0.1):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(n, d, generator=g) * scale).float()


def _excl(U, I, density, seed, extra=None):
    rng = np.random.default_rng(seed)
    n = int(U * I * density)
    u, i = rng.integers(0, U, n), rng.integers(0, I, n)
    if extra is not None:
        u, i = np.concatenate([u, extra[0]]), np.concatenate([i, extra[1]])
    return O.exclusion_csr(U, I, (u, i))


def _rowsets(rp, col, U, I):
    from lgcnhs.graph import RowSets
    return RowSets(torch.as_tensor(rp).to(DEV), torch.as_tensor(col).to(DEV), U, I)


def _ids(n, seed, hi=U_TAB):
    """n unsorted ids below hi, one of them twice (n >= 2)."""
    rng = np.random.default_rng(seed)
    ids = rng.permutation(hi)[:n]
    if n >= 2:
        ids[-1] = ids[0]
    return torch.as_tensor(ids.astype(np.int64))


def _batch(eu, ei, ids, k, ex=None, n_batch=None, mask=O.MASK):
    """lg_score_topk_batch_f32 through the C ABI (no host routing). ids: int64 tensor or None
    (then n_batch rows 0 .. n_batch-1)."""
    from lgcnhs import _native as N
    nu, d = eu.shape
    ni = ei.shape[0]
    if ids is not None:
        ids = ids.to(DEV)
        n_batch = ids.numel()
    ws_bytes = N.lib().lg_score_topk_batch_ws_bytes(n_batch, ni, d, k)
    ws = torch.empty(max(ws_bytes, 8), dtype=torch.uint8, device=DEV)
    val = torch.empty((n_batch, k), dtype=torch.float32, device=DEV)
    idx = torch.empty((n_batch, k), dtype=torch.int64, device=DEV)
    N.check(N.lib().lg_score_topk_batch_f32(
        N.ptr(eu), N.ptr(ei), N.ptr(ids), n_batch, nu, ni, d,
        N.ptr(ex.rowptr if ex else None), N.ptr(ex.col if ex else None), float(mask), int(k),
        N.ptr(val), N.ptr(idx), N.ptr(ws), ws_bytes, N.stream_handle(eu.device)),
        "lg_score_topk_batch_f32")
    return val, idx


def _same_rows(v, i, ref, ids, what=None):
    """(v, i) == rows ids of the all-users reference (rv, ri): ids equal, values bit for bit."""
    rv, ri = ref
    sel = ids.to(rv.device)
    assert torch.equal(i, ri[sel]), what
    assert torch.equal(v.view(torch.int32), rv[sel].view(torch.int32)), what


_TABLES = {}


def _tables(d, I=4097):
    """Shared inputs per width: 200 users, I items (odd, several workgroups), exact ties
    (duplicate item rows), 3 % exclusions; on the device, with the host CSR for the oracle."""
    key = (d, I)
    if key not in _TABLES:
        eu, ei = _emb(U_TAB, d, 100 + d), _emb(I, d, 200 + d)
        if I > 140:
            ei[100:140] = ei[60:100]
        rp, col = _excl(U_TAB, I, 0.03, 300 + d)
        _TABLES[key] = (eu.to(DEV), ei.to(DEV), _rowsets(rp, col, U_TAB, I), rp, col,
                        eu.numpy(), ei.numpy())
    return _TABLES[key]


_REFS = {}


def _ref(d, k, I=4097):
    """lg_score_topk_f32 on the whole table (computed once per shape, never modified)."""
    from lgcnhs import ops
    key = (d, k, I)
    if key not in _REFS:
        eu, ei, ex = _tables(d, I)[:3]
        _REFS[key] = ops.score_topk(eu, ei, k, ex, screen=False)
    return _REFS[key]


@pytest.mark.parametrize("d", [32, 64, 128])
@pytest.mark.parametrize("k", [1, 20, 33, 100, 128])
def test_batch_rows_bit_exact(d, k):
    """Every batch size around the 16-user groups (1, 15, 16, 17, 33, 64: 1, 2 and 4 groups,
    the last one partly filled), every list size (k <= 32 / 64 / 128) and width: rows equal
    lg_score_topk_f32's for unsorted ids with a duplicate; at k = 20 also the C chain oracle."""
    eu, ei, ex, rp, col, eun, ein = _tables(d)
    ref = _ref(d, k)
    if k == 20:
        ov, oi = O.chain_topk(eun, ein, rp, col, k)
        np.testing.assert_array_equal(ref[1].cpu().numpy(), oi)
        assert np.array_equal(ref[0].cpu().numpy().view(np.uint32), ov.view(np.uint32))
    for nb in (1, 15, 16, 17, 33, 64):
        ids = _ids(nb, 10 * nb + k)
        v, i = _batch(eu, ei, ids, k, ex)
        _same_rows(v, i, ref, ids, (d, k, nb))
        if k == 20:
            np.testing.assert_array_equal(i.cpu().numpy(), oi[ids.numpy()])


@pytest.mark.parametrize("I", [1, 15, 17])
def test_tiny_catalogs_and_short_rows(I):
    """Fewer items than a tile / than k: one workgroup, rows shorter than k padded with
    {-inf, -1} exactly as lg_score_topk_f32 pads them."""
    from lgcnhs import ops
    eu = _tables(64)[0]
    ei = _emb(I, 64, 7).to(DEV)
    rp, col = _excl(U_TAB, I, 0.2, 8)
    ex = _rowsets(rp, col, U_TAB, I)
    for k in (1, 20):
        ref = ops.score_topk(eu, ei, k, ex, screen=False)
        ids = _ids(17, I + k)
        v, i = _batch(eu, ei, ids, k, ex)
        _same_rows(v, i, ref, ids, (I, k))
        if k > I:
            assert (i[:, I:] == -1).all() and torch.isinf(v[:, I:]).all()


@pytest.mark.parametrize("nb,k", [(8, 20), (64, 128)])
def test_catalog_just_past_one_round_of_waves(nb, k):
    """A catalog of one 16-item tile per wave of the full grid plus 5 items (the grid from
    ops.batch_topk_grid, the launcher's arithmetic): not a multiple of 16, not divisible by the
    wave count. The tiles no longer go round once, so every wave takes two, the last busy wave
    a partial tile alone, and the workgroups behind it are not launched."""
    from lgcnhs import ops
    d = 32
    blocks, waves, _ = ops.batch_topk_grid(nb, 1 << 24, k, DEV)
    n_waves = blocks * waves
    I = n_waves * 16 + 5
    assert I % 16 and I % n_waves
    b2, w2, ipw = ops.batch_topk_grid(nb, I, k, DEV)
    assert w2 == waves and ipw == 32 and b2 * waves * ipw >= I > (b2 - 1) * waves * ipw
    eu = _tables(d)[0]
    ei = _emb(I, d, 11).to(DEV)
    rp, col = _excl(U_TAB, I, 0.002, 12)
    ex = _rowsets(rp, col, U_TAB, I)
    ref = ops.score_topk(eu, ei, k, ex, screen=False)
    ids = _ids(nb, 13)
    v, i = _batch(eu, ei, ids, k, ex)
    _same_rows(v, i, ref, ids)


def _half_excl(U, I, density, seed):
    """_excl with rows for the even users only: about half the users have exclusion rows."""
    rng = np.random.default_rng(seed)
    n = int(U * I * density)
    return O.exclusion_csr(U, I, (2 * rng.integers(0, U // 2, n), rng.integers(0, I, n)))


# (R partial lists, tight): tight = the last workgroup has one wave with one item and its other
# waves empty (R >= 2)
_LIST_CASES = [(R, False) for R in (1, 2, 16, 17, 33)] + [(R, True) for R in (2, 16, 17, 33)]


@pytest.mark.parametrize("R,tight", _LIST_CASES)
def test_partial_list_counts(R, tight):
    """R workgroups = R partial lists per user, one 16-item tile per wave (the grid from
    ops.batch_topk_grid, asserted): R = 1 writes the rows with no merge, 2 and 16 are the merge
    kernel's tree alone, at 17 a merge wave takes two lists, at 33 three. tight: 16 waves - 1
    items fewer, so the last workgroup's tree meets empty lists. B x k = {1, 16} x {20, 100}
    (4 waves per workgroup; merge <2> and <4>), (32, 128) (2 waves: one tree step) and
    (64, 128) (1 wave: no tree). Rows equal lg_score_topk_f32's bit for bit; every second user
    has exclusion rows."""
    from lgcnhs import ops
    d = 32
    eu = _tables(d)[0]
    refs = {}
    for nb, k in ((1, 20), (16, 20), (1, 100), (16, 100), (32, 128), (64, 128)):
        waves = ops.batch_topk_grid(nb, 1 << 20, k, DEV)[1]
        assert waves == {32: 2, 64: 1}.get(nb, 4)
        I = 16 * waves * R - ((16 * waves - 1) if tight else 0)
        assert ops.batch_topk_grid(nb, I, k, DEV) == (R, waves, 16)
        if (I, k) not in refs:
            ei = _emb(64 * 33, d, 61)[:I].contiguous().to(DEV)
            ex = _rowsets(*_half_excl(U_TAB, I, 0.2, 62 + I), U_TAB, I)
            refs[I, k] = ei, ex, ops.score_topk(eu, ei, k, ex, screen=False)
        ei, ex, ref = refs[I, k]
        ids = _ids(nb, 63 + nb)
        v, i = _batch(eu, ei, ids, k, ex)
        _same_rows(v, i, ref, ids, (R, tight, nb, k))


@pytest.mark.parametrize("nb,k,I", [(16, 20, 300001), (64, 128, 300001)])
def test_long_ranges_compact_mid_stream(nb, k, I):
    """Enough items per wave (~146 at 2,048 waves, ~1,172 at 256) that lists overflow and are
    compacted inside the stream, with the lazy exclusion check at each compaction."""
    from lgcnhs import ops
    d = 32
    eu = _tables(d)[0]
    ei = _emb(I, d, 21).to(DEV)
    rp, col = _excl(U_TAB, I, 0.001, 22)
    ex = _rowsets(rp, col, U_TAB, I)
    ref = ops.score_topk(eu, ei, k, ex, screen=False)
    ids = _ids(nb, 23)
    v, i = _batch(eu, ei, ids, k, ex)
    _same_rows(v, i, ref, ids)
    assert (i >= 0).all()


def test_ties_come_out_in_item_order():
    """Every item row equal: all scores of a user tie, so the list is items 0 .. k-1."""
    from lgcnhs import ops
    d, I, k = 64, 300, 40
    eu = _tables(d)[0]
    ei = _emb(1, d, 31).repeat(I, 1).to(DEV)
    ids = _ids(17, 32)
    v, i = _batch(eu, ei, ids, k)
    assert torch.equal(i, torch.arange(k, device=DEV).expand(17, k))
    _same_rows(v, i, ops.score_topk(eu, ei, k, None, screen=False), ids)


def test_exclusion_shapes():
    """No exclusions; a user with every item excluded (all its scores are the mask value: the
    first k items in order); a user whose best 150 items -- consecutive, inside one wave's
    range, more than one 64-entry run of the lazy check -- are excluded; ordinary rows."""
    from lgcnhs import ops
    d, I, k, nb = 32, 40000, 100, 64
    _, _, ipw = ops.batch_topk_grid(nb, I, k, DEV)
    assert ipw >= 160
    eu = _tables(d)[0].clone()
    ei = _emb(I, d, 41)
    ei[:150] = eu[5].cpu() * 3.0  # user 5's best items: 0 .. 149 (tied)
    ei = ei.to(DEV)
    extra = (np.concatenate([np.full(I, 3), np.full(150, 5)]),
             np.concatenate([np.arange(I), np.arange(150)]))
    rp, col = _excl(U_TAB, I, 0.001, 42, extra)
    ex = _rowsets(rp, col, U_TAB, I)
    ids = torch.cat([torch.tensor([5, 3]), _ids(nb - 2, 43)])
    for e in (None, ex):
        ref = ops.score_topk(eu, ei, k, e, screen=False)
        v, i = _batch(eu, ei, ids, k, e)
        _same_rows(v, i, ref, ids, e is None)
    assert torch.equal(i[1], torch.arange(k, device=DEV)) and (v[1] == O.MASK).all()
    assert (i[0] >= 150).all()  # excluded items rank at -1024: below every ordinary score
    v0, i0 = _batch(eu, ei, ids, k, None)
    assert (i0[0] < 150).all()


def test_non_finite_rows():
    """A NaN item row, an item with a +inf element, a NaN user row, a user with a -inf
    element (test_wide_non_finite_rows' inputs): NaN and -inf scores never rank, rows equal
    lg_score_topk_f32's."""
    from lgcnhs import ops
    U, I, d = 70, 3000, 64
    eu, ei = _emb(U, d, 41), _emb(I, d, 42)
    ei[1234] = float("nan")
    ei[2000, 5] = float("inf")
    eu[7] = float("nan")
    eu[11, 3] = -float("inf")
    eu[0] = float("nan")  # the row an out-of-range id would be clamped to
    rp, col = _excl(U, I, 0.01, 43)
    ex = _rowsets(rp, col, U, I)
    eu, ei = eu.to(DEV), ei.to(DEV)
    ids = torch.tensor([7, 11, 0, 1, 2, 7, 30, 69, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21])
    for k in (20, 100):
        ref = ops.score_topk(eu, ei, k, ex, n_splits=1, screen=False)
        v, i = _batch(eu, ei, ids, k, ex)
        _same_rows(v, i, ref, ids, k)
        assert (i[0] == -1).all() and (i[2] == -1).all() and not (i == 1234).any()
        assert (i[3:5] >= 0).all()


def test_null_ids_mean_the_first_rows():
    d, k = 64, 33
    eu, ei, ex = _tables(d)[:3]
    v0, i0 = _batch(eu, ei, None, k, ex, n_batch=33)
    v1, i1 = _batch(eu, ei, torch.arange(33), k, ex)
    assert torch.equal(i0, i1) and torch.equal(v0.view(torch.int32), v1.view(torch.int32))
    _same_rows(v0, i0, _ref(d, k), torch.arange(33))


def test_score_topk_users_chunks_and_falls_back(monkeypatch):
    """150 users: with BATCH_MAX_USERS = 150 three calls of the batch entry (64 + 64 + 22), with
    0 ops.score_topk on the gathered rows; both equal the all-users rows. 128 < k goes to the
    gathered call either way; a bad id in a list raises before any launch."""
    from lgcnhs import ops
    d, k = 64, 20
    eu, ei, ex = _tables(d)[:3]
    ref = _ref(d, k)
    rng = np.random.default_rng(5)
    ids = rng.integers(0, U_TAB, 150).tolist()
    t = torch.as_tensor(ids)
    monkeypatch.setattr(ops, "BATCH_MAX_USERS", 150)
    calls = []
    real = ops.score_topk
    monkeypatch.setattr(ops, "score_topk", lambda *a, **kw: calls.append(1) or real(*a, **kw))
    vb, ib = ops.score_topk_users(eu, ei, ids, k, ex)
    assert not calls
    vw, iw = ops.score_topk_users(eu, ei, t.to(DEV), 200, ex)
    assert len(calls) == 1
    monkeypatch.setattr(ops, "BATCH_MAX_USERS", 0)
    vf, if_ = ops.score_topk_users(eu, ei, t, k, ex)
    assert len(calls) == 2
    assert torch.equal(ib, if_) and torch.equal(vb.view(torch.int32), vf.view(torch.int32))
    _same_rows(vb, ib, ref, t)
    assert torch.equal(iw[:, :k], ib)
    with pytest.raises(ValueError):
        ops.score_topk_users(eu, ei, [0, U_TAB], k, ex)
    with pytest.raises(ValueError):
        ops.score_topk_users(eu, ei, torch.tensor([-1]), k, ex)


def test_rowsets_take():
    """RowSets.take(rows) == the rows rebuilt one by one (order kept, duplicates, empty rows),
    and return_index points at the same entries of col."""
    I = 4097
    ex, rp, col = _tables(64)[2:5]
    rows = [5, 199, 0, 5, 17, 17, 100]
    t, src = ex.take(rows, return_index=True)
    trp, tcol = t.rowptr.cpu().numpy(), t.col.cpu().numpy()
    assert t.n_rows == len(rows) and t.n_cols == I and trp[0] == 0
    for j, r in enumerate(rows):
        np.testing.assert_array_equal(tcol[trp[j]:trp[j + 1]], col[rp[r]:rp[r + 1]])
    np.testing.assert_array_equal(col[src.cpu().numpy()], tcol)
    e = ex.take(torch.zeros(0, dtype=torch.int64))
    assert e.n_rows == 0 and e.col.numel() == 0 and e.rowptr.tolist() == [0]
    from lgcnhs.graph import RowSets
    empty = RowSets.from_pairs([1], [2], 4, 8, DEV).take([0, 3, 0])
    assert empty.rowptr.tolist() == [0, 0, 0, 0] and empty.col.numel() == 0


@pytest.mark.parametrize("batch_max", [0, 64])
def test_recommend_for_users(golden, monkeypatch, batch_max):
    """recommendForUsers == the matching entries of recommendForAllUser (lightgcn_toy), through
    the batch kernel and through the gathered fallback; it writes no file."""
    from lgcnhs import ops
    from model.LightGCN.model import LightGCN
    from model.LightGCN.recommend import recommendForAllUser, recommendForUsers
    from model.LightGCNOpti.recommend import recommendForUsers as opti_for_users
    from utils.graph import convertEdgeIndexToAdjMatrix
    monkeypatch.setattr(ops, "BATCH_MAX_USERS", batch_max)
    g = golden("lightgcn_toy")
    U, I, k = int(g["n_users"]), int(g["n_items"]), int(g["k"])
    torch.manual_seed(42)
    m = LightGCN(U, I, 64, 3).to(DEV)
    tr = convertEdgeIndexToAdjMatrix(U, I, torch.as_tensor(g["train"].astype(np.int64)))
    va = convertEdgeIndexToAdjMatrix(U, I, torch.as_tensor(g["val"].astype(np.int64)))
    full = recommendForAllUser(m, U, I, tr, va, None, k)
    ids = [U - 1, 0, 3, 3, U // 2]
    monkeypatch.setattr("model.LightGCN.recommend.save_recs",
                        lambda *a, **kw: pytest.fail("recommendForUsers wrote a file"))
    for fn in (recommendForUsers, opti_for_users):
        got = fn(m, ids, U, I, tr, va, None, k)
        assert sorted(got) == sorted(set(ids))
        for u in ids:
            assert got[u] == full[u], u
    with pytest.raises(ValueError):
        recommendForUsers(m, [0, U], U, I, tr, va, None, k)


@pytest.mark.parametrize("tiled", [False, True])
@pytest.mark.parametrize("with_g", [False, True])
def test_spread_recommend_for_users(tiled, with_g):
    """spread_recommend(users=ids) is bitwise the all-users call's rows ids: dense
    (lg_spread_resource_f64 on the taken rows + rows_topk) and tiled (the walk on a taken
    user-side CSR, 5 tiles of 64 items), with and without the G factor; unsorted ids with a
    duplicate and a list instead of a tensor."""
    from lgcnhs import ops
    from lgcnhs.synth import synth_interactions
    U, I, k, lam = 60, 300, 10, 0.5
    u, i = synth_interactions(U, I, 1500, seed=3)
    A = ops.Interactions.from_pairs(torch.as_tensor(u), torch.as_tensor(i), U, I, DEV)
    eu = ei = None
    if with_g:
        eu, ei = _emb(U, 64, 51).to(DEV), _emb(I, 64, 52).to(DEV)
    kw = dict(drop=True, eu=eu, ei=ei, tiled=tiled, tile=64)
    fv, fi = ops.spread_recommend(A, lam, k, A.by_user, **kw)
    ids = [59, 0, 31, 7, 31, 2, 58]
    for users in (ids, torch.as_tensor(ids).to(DEV)):
        v, ix = ops.spread_recommend(A, lam, k, A.by_user, users=users, **kw)
        assert torch.equal(ix, fi[ids])
        assert torch.equal(v.view(torch.int64), fv[ids].view(torch.int64))
    with pytest.raises(ValueError):
        ops.spread_recommend(A, lam, k, A.by_user, users=[0, U], **kw)


def test_spread_method_topk_for_users():
    """The model-level entry passes users= through (SpreadMethod; SpreadLightGCN and its Opti
    twin share ops.spread_recommend's path tested above)."""
    import pandas as pd
    from lgcnhs.synth import synth_interactions
    from model.SpreadMethod.recommend import spread_method_topk
    U, I, k = 40, 120, 8
    u, i = synth_interactions(U, I, 600, seed=4)
    df = pd.DataFrame({"user_id": u, "item_id": i})
    tr, va = df.iloc[::2], df.iloc[1::2]
    fv, fi = spread_method_topk(U, I, tr, va, "HybridS", 0.5, "toy", k, tiled=False)
    ids = [39, 1, 1, 20]
    v, ix = spread_method_topk(U, I, tr, va, "HybridS", 0.5, "toy", k, tiled=False, users=ids)
    assert torch.equal(ix, fi[ids]) and torch.equal(v.view(torch.int64), fv[ids].view(torch.int64))
