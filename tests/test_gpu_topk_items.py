"""GPU parity of K2i (lg_score_topk_batch_items_f32, csrc/topk_items.hip): top-K for a short
list of user ids over a candidate item set. Every row is compared bit for bit (values, ids,
order, padding) with lg_score_topk_f32 on the gathered sub-table ei[cand] -- exclusion columns
renumbered in numpy, ids mapped back through cand -- and a subset with the C chain oracle on
the same sub-table; then the Python layers on top of it (ops.item_candidates,
RowSets.restrict_cols, ops.score_topk(items=), ops.score_topk_users(items=),
recommendForUsers(items=))."""
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


def _random_cand(I, n, seed):
    return np.sort(np.random.default_rng(seed).permutation(I)[:n]).astype(np.int32)


def _restrict_np(rp, col, U, cand):
    """The exclusion CSR (host) with only the columns in cand, renumbered to positions in cand:
    the numpy restatement (O.exclusion_csr on the renumbered pairs)."""
    rp, col = np.asarray(rp), np.asarray(col)
    rows = np.repeat(np.arange(U), np.diff(rp))
    keep = np.isin(col, cand)
    return O.exclusion_csr(U, len(cand), (rows[keep], np.searchsorted(cand, col[keep])))


def _items(eu, ei, ids, cand, k, ex=None, n_batch=None, mask=O.MASK, n_items=None):
    """lg_score_topk_batch_items_f32 through the C ABI (no host routing). ids: int64 tensor or
    None (rows 0 .. n_batch-1); cand: int32 array / tensor, passed as it is."""
    from lgcnhs import _native as N
    nu, d = eu.shape
    ni = ei.shape[0] if n_items is None else n_items
    if ids is not None:
        ids = ids.to(DEV)
        n_batch = ids.numel()
    c = torch.as_tensor(cand).to(DEV, torch.int32).contiguous()
    nc = c.numel()
    ws_bytes = N.lib().lg_score_topk_batch_items_ws_bytes(n_batch, nc, d, k)
    ws = torch.empty(max(ws_bytes, 8), dtype=torch.uint8, device=DEV)
    val = torch.empty((n_batch, k), dtype=torch.float32, device=DEV)
    idx = torch.empty((n_batch, k), dtype=torch.int64, device=DEV)
    N.check(N.lib().lg_score_topk_batch_items_f32(
        N.ptr(eu), N.ptr(ei), N.ptr(ids), n_batch, nu, ni, N.ptr(c), nc, d,
        N.ptr(ex.rowptr if ex else None), N.ptr(ex.col if ex else None), float(mask), int(k),
        N.ptr(val), N.ptr(idx), N.ptr(ws), ws_bytes, N.stream_handle(eu.device)),
        "lg_score_topk_batch_items_f32")
    return val, idx


def _batch(eu, ei, ids, k, ex):
    """lg_score_topk_batch_f32 (K2b, the full catalog) through the C ABI."""
    from lgcnhs import _native as N
    nu, d = eu.shape
    ni = ei.shape[0]
    ids = ids.to(DEV)
    nb = ids.numel()
    ws_bytes = N.lib().lg_score_topk_batch_ws_bytes(nb, ni, d, k)
    ws = torch.empty(max(ws_bytes, 8), dtype=torch.uint8, device=DEV)
    val = torch.empty((nb, k), dtype=torch.float32, device=DEV)
    idx = torch.empty((nb, k), dtype=torch.int64, device=DEV)
    N.check(N.lib().lg_score_topk_batch_f32(
        N.ptr(eu), N.ptr(ei), N.ptr(ids), nb, nu, ni, d, N.ptr(ex.rowptr), N.ptr(ex.col),
        float(O.MASK), int(k), N.ptr(val), N.ptr(idx), N.ptr(ws), ws_bytes,
        N.stream_handle(eu.device)), "lg_score_topk_batch_f32")
    return val, idx


def _twin(eu, ei, rp, col, cand, k, **kw):
    """The kernel twin, all users: lg_score_topk_f32 (screen=False) on the gathered sub-table
    with the numpy-renumbered exclusions, ids mapped back through cand (-1 kept)."""
    from lgcnhs import ops
    U = eu.shape[0]
    c = torch.as_tensor(np.asarray(cand)).to(DEV, torch.int64)
    ex = None
    if rp is not None:
        srp, scol = _restrict_np(rp, col, U, np.asarray(cand))
        ex = _rowsets(srp, scol, U, len(cand))
    v, i = ops.score_topk(eu, ei[c].contiguous(), k, ex, screen=False, **kw)
    return v, torch.where(i >= 0, c[i.clamp(min=0)], i)


def _chain(eun, ein, rp, col, cand, k):
    """The C chain oracle on the sub-table, ids mapped back."""
    cand = np.asarray(cand)
    srp, scol = _restrict_np(rp, col, eun.shape[0], cand)
    ov, oi = O.chain_topk(eun, np.ascontiguousarray(ein[cand]), srp, scol, k)
    return ov, np.where(oi >= 0, cand[np.maximum(oi, 0)], -1)


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
        ei[100:140] = ei[60:100]
        rp, col = _excl(U_TAB, I, 0.03, 300 + d)
        _TABLES[key] = (eu.to(DEV), ei.to(DEV), _rowsets(rp, col, U_TAB, I), rp, col,
                        eu.numpy(), ei.numpy())
    return _TABLES[key]


def _cand_sets(I=4097):
    return {
        "all": np.arange(I, dtype=np.int32),
        "half": _random_cand(I, I // 2, 1),
        "123": _random_cand(I, 123, 2),          # pads k = 128
        "37..2077": np.arange(37, 2077, dtype=np.int32),  # off the 16-item tile at both ends
        "50..150": np.arange(50, 150, dtype=np.int32),    # both copies of the ties
        "77": np.array([77], dtype=np.int32),
        "15": _random_cand(I, 15, 3),
        "16": _random_cand(I, 16, 4),
        "17": _random_cand(I, 17, 5),
    }


@pytest.mark.parametrize("d", [32, 64, 128])
@pytest.mark.parametrize("k", [1, 20, 33, 100, 128])
def test_items_rows_bit_exact(d, k):
    """Every width and list size, 1 / 15 / 16 users (unsorted ids with a duplicate), nine
    candidate sets: rows equal lg_score_topk_f32's on the gathered sub-table; with every item a
    candidate also lg_score_topk_batch_f32's rows; at k = 20 also the C chain oracle."""
    eu, ei, ex, rp, col, eun, ein = _tables(d)
    for name, cand in _cand_sets().items():
        ref = _twin(eu, ei, rp, col, cand, k)
        if k == 20:
            ov, oi = _chain(eun, ein, rp, col, cand, k)
            np.testing.assert_array_equal(ref[1].cpu().numpy(), oi, name)
            assert np.array_equal(ref[0].cpu().numpy().view(np.uint32), ov.view(np.uint32)), name
        if len(cand) < k:
            assert (ref[1][:, len(cand):] == -1).all(), name
        for nb in (1, 15, 16):
            ids = _ids(nb, 10 * nb + k)
            v, i = _items(eu, ei, ids, cand, k, ex)
            _same_rows(v, i, ref, ids, (d, k, nb, name))
            if len(cand) < k:
                assert (i[:, len(cand):] == -1).all() and torch.isinf(v[:, len(cand):]).all()
            if name == "all":
                bv, bi = _batch(eu, ei, ids, k, ex)
                assert torch.equal(i, bi) and torch.equal(v.view(torch.int32),
                                                          bv.view(torch.int32))


@pytest.mark.parametrize("nb,k", [(8, 20), (16, 128)])
def test_candidates_just_past_one_round_of_waves(nb, k):
    """One 16-candidate tile per wave of the full grid plus 5 candidates (the grid from
    ops.items_topk_grid, the launcher's arithmetic), drawn from a catalog twice that size:
    every wave takes two tiles, the last busy wave a partial tile alone, and the workgroups
    behind it are not launched."""
    from lgcnhs import ops
    d = 32
    blocks, waves, _ = ops.items_topk_grid(nb, 1 << 24, k, DEV)
    n_waves = blocks * waves
    nc = n_waves * 16 + 5
    I = 2 * nc
    b2, w2, ppw = ops.items_topk_grid(nb, nc, k, DEV)
    assert w2 == waves and ppw == 32 and b2 * waves * ppw >= nc > (b2 - 1) * waves * ppw
    eu = _tables(d)[0]
    ei = _emb(I, d, 11).to(DEV)
    rp, col = _excl(U_TAB, I, 0.002, 12)
    ex = _rowsets(rp, col, U_TAB, I)
    cand = _random_cand(I, nc, 13)
    ref = _twin(eu, ei, rp, col, cand, k)
    ids = _ids(nb, 14)
    v, i = _items(eu, ei, ids, cand, k, ex)
    _same_rows(v, i, ref, ids)


# (R partial lists, tight): tight = the last workgroup has one wave with one candidate and three
# empty waves (R >= 2)
_LIST_CASES = [(R, False) for R in (1, 2, 16, 17, 33)] + [(R, True) for R in (2, 16, 17, 33)]


@pytest.mark.parametrize("R,tight", _LIST_CASES)
def test_partial_list_counts(R, tight):
    """R workgroups = R partial lists per user, one 16-candidate tile per wave (the grid from
    ops.items_topk_grid, asserted): R = 1 writes the rows with no merge, 2 and 16 are the merge
    kernel's tree alone, at 17 a merge wave takes two lists, at 33 three. tight: 63 candidates
    fewer, so the last workgroup's tree meets empty lists. Candidates = every third item;
    B x k = {1, 16} x {20, 100} (merge <2> and <4>). Rows equal lg_score_topk_f32's on the
    gathered sub-table bit for bit; every second user has exclusion rows."""
    from lgcnhs import ops
    d = 32
    nc = 64 * R - (63 if tight else 0)
    I = 3 * nc
    cand = np.arange(0, I, 3, dtype=np.int32)
    eu = _tables(d)[0]
    ei = _emb(3 * 64 * 33, d, 61)[:I].contiguous().to(DEV)
    rng = np.random.default_rng(62 + nc)
    n = int(U_TAB * I * 0.2)
    rp, col = O.exclusion_csr(U_TAB, I, (2 * rng.integers(0, U_TAB // 2, n),
                                         rng.integers(0, I, n)))
    ex = _rowsets(rp, col, U_TAB, I)
    for k in (20, 100):
        ref = _twin(eu, ei, rp, col, cand, k)
        for nb in (1, 16):
            assert ops.items_topk_grid(nb, nc, k, DEV) == (R, 4, 16)
            ids = _ids(nb, 63 + nb)
            v, i = _items(eu, ei, ids, cand, k, ex)
            _same_rows(v, i, ref, ids, (R, tight, nb, k))


@pytest.mark.parametrize("nb,k", [(16, 20), (16, 128)])
def test_long_ranges_compact_mid_stream(nb, k):
    """Every second item of 300,001 (~150,000 candidates): enough positions per wave that lists
    overflow and are compacted inside the stream, the exclusion cursor advancing in id space
    over the gaps between candidates."""
    d, I = 32, 300001
    eu = _tables(d)[0]
    ei = _emb(I, d, 21).to(DEV)
    rp, col = _excl(U_TAB, I, 0.001, 22)
    ex = _rowsets(rp, col, U_TAB, I)
    cand = np.arange(0, I, 2, dtype=np.int32)
    ref = _twin(eu, ei, rp, col, cand, k)
    ids = _ids(nb, 23)
    v, i = _items(eu, ei, ids, cand, k, ex)
    _same_rows(v, i, ref, ids)
    assert (i >= 0).all() and (i % 2 == 0).all()


def test_exclusion_shapes():
    """No exclusions; a user with every candidate excluded (all its scores are the mask value:
    the first k candidates in order); a user whose best 150 candidates -- consecutive positions
    inside one wave's range, more than one 64-entry run of the lazy check, gaps between their
    ids -- are excluded; excluded items that are not candidates (no effect); ordinary rows."""
    from lgcnhs import ops
    d, I, k, nb = 32, 400000, 100, 16
    cand = np.arange(0, I, 2, dtype=np.int32)
    _, _, ppw = ops.items_topk_grid(nb, len(cand), k, DEV)
    assert ppw >= 160
    eu = _tables(d)[0].clone()
    ei = _emb(I, d, 41)
    ei[torch.as_tensor(cand[:150].astype(np.int64))] = eu[5].cpu() * 3.0  # user 5's best (tied)
    ei = ei.to(DEV)
    odd = np.arange(1, 2001, 2)  # not candidates
    base = (np.concatenate([np.full(len(cand), 3), np.full(150, 5)]),
            np.concatenate([cand, cand[:150]]))
    extra = (np.concatenate([base[0], np.full(len(odd), 7)]), np.concatenate([base[1], odd]))
    rp, col = _excl(U_TAB, I, 0.001, 42, extra)
    ex = _rowsets(rp, col, U_TAB, I)
    ids = torch.cat([torch.tensor([5, 3, 7]), _ids(nb - 3, 43)])
    for r, c, e in ((None, None, None), (rp, col, ex)):
        ref = _twin(eu, ei, r, c, cand, k)
        v, i = _items(eu, ei, ids, cand, k, e)
        _same_rows(v, i, ref, ids, e is None)
    assert torch.equal(i[1], torch.as_tensor(cand[:k].astype(np.int64)).to(DEV))
    assert (v[1] == O.MASK).all()
    assert (i[0] >= 300).all()  # excluded items rank at -1024: below every ordinary score
    v0, i0 = _items(eu, ei, ids, cand, k, None)
    assert (i0[0] < 300).all()
    # user 7 without its excluded non-candidates: the same row
    rp2, col2 = _excl(U_TAB, I, 0.001, 42, base)
    v2, i2 = _items(eu, ei, ids, cand, k, _rowsets(rp2, col2, U_TAB, I))
    assert torch.equal(i2[2], i[2]) and torch.equal(v2[2].view(torch.int32),
                                                    v[2].view(torch.int32))


def test_non_finite_rows():
    """A NaN item row and an item with a +inf element among the candidates, a NaN user row, a
    user with a -inf element (test_gpu_topk_batch's test_non_finite_rows inputs): NaN and -inf
    scores never rank, rows equal lg_score_topk_f32's on the sub-table; one run leaves the NaN
    item out of the candidates."""
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
    ids = torch.tensor([7, 11, 0, 1, 2, 7, 30, 69, 12, 13, 14, 15, 16, 17, 18, 19])
    half = _random_cand(I, I // 2, 44)
    with_nan = np.union1d(half, [1234, 2000]).astype(np.int32)
    without = np.setdiff1d(with_nan, [1234]).astype(np.int32)
    for cand in (with_nan, without):
        for k in (20, 100):
            ref = _twin(eu, ei, rp, col, cand, k, n_splits=1)
            v, i = _items(eu, ei, ids, cand, k, ex)
            _same_rows(v, i, ref, ids, k)
            assert (i[0] == -1).all() and (i[2] == -1).all() and not (i == 1234).any()
            assert (i[3:5] >= 0).all()


def test_ids_outside_the_catalog_never_rank():
    """Defined behaviour of the entry on a list with ids outside [0, n_items) -- here -5 in
    front of and n_items + 3 behind an ascending list: the call returns LG_OK, their row reads
    are clamped, they are never admitted, and every row equals the oracle on the valid
    candidates."""
    d, k = 64, 20
    eu, ei, ex, rp, col, eun, ein = _tables(d)
    I = ei.shape[0]
    valid = _random_cand(I, 500, 6)
    hostile = np.concatenate([[-5], valid, [I + 3]]).astype(np.int32)
    ref = _twin(eu, ei, rp, col, valid, k)
    ov, oi = _chain(eun, ein, rp, col, valid, k)
    np.testing.assert_array_equal(ref[1].cpu().numpy(), oi)
    for nb in (1, 16):
        ids = _ids(nb, 60 + nb)
        v, i = _items(eu, ei, ids, hostile, k, ex)
        assert not (i == -5).any() and not (i == I + 3).any()
        _same_rows(v, i, ref, ids, nb)


def test_null_ids_mean_the_first_rows():
    d, k = 64, 33
    eu, ei, ex, rp, col = _tables(d)[:5]
    cand = _cand_sets()["half"]
    v0, i0 = _items(eu, ei, None, cand, k, ex, n_batch=16)
    v1, i1 = _items(eu, ei, torch.arange(16), cand, k, ex)
    assert torch.equal(i0, i1) and torch.equal(v0.view(torch.int32), v1.view(torch.int32))
    _same_rows(v0, i0, _twin(eu, ei, rp, col, cand, k), torch.arange(16))


# ------------------------------------------------------------------------- Python layers
def test_rowsets_restrict_cols():
    """RowSets.restrict_cols(cand) == the numpy restatement (rows kept in order, columns
    renumbered to positions in cand), also on a row slice and for an empty candidate set."""
    I = 4097
    ex, rp, col = _tables(64)[2:5]
    for cand in (_cand_sets()["half"], _cand_sets()["77"], np.arange(I, dtype=np.int32)):
        r = ex.restrict_cols(torch.as_tensor(cand).to(DEV))
        srp, scol = _restrict_np(rp, col, U_TAB, cand)
        assert r.n_rows == U_TAB and r.n_cols == len(cand)
        np.testing.assert_array_equal(r.rowptr.cpu().numpy(), srp)
        np.testing.assert_array_equal(r.col.cpu().numpy(), scol)
        assert r.col.dtype == torch.int32 and r.rowptr.dtype == torch.int64
    cand = _cand_sets()["half"]
    s = ex.slice_rows(10, 50).restrict_cols(torch.as_tensor(cand).to(DEV))
    srp, scol = _restrict_np(rp, col, U_TAB, cand)
    a, b = s.rowptr.cpu().numpy(), s.col.cpu().numpy()
    for j in range(40):
        np.testing.assert_array_equal(b[a[j]:a[j + 1]], scol[srp[10 + j]:srp[11 + j]])
    e = ex.restrict_cols(torch.zeros(0, dtype=torch.int32, device=DEV))
    assert e.n_cols == 0 and e.col.numel() == 0 and not e.rowptr.any()


@pytest.mark.parametrize("screen", [False, True])
def test_score_topk_items_equals_the_oracle(screen):
    """ops.score_topk(items=) -- the gather route on the existing kernels, plain and screened --
    equals the C chain oracle on the sub-table, real item ids."""
    from lgcnhs import ops
    d, k = 64, 20
    eu, ei, ex, rp, col, eun, ein = _tables(d)
    for name in ("half", "123", "50..150", "77"):
        cand = _cand_sets()[name]
        ov, oi = _chain(eun, ein, rp, col, cand, k)
        v, i = ops.score_topk(eu, ei, k, ex, screen=screen, items=cand)
        np.testing.assert_array_equal(i.cpu().numpy(), oi, name)
        assert np.array_equal(v.cpu().numpy().view(np.uint32), ov.view(np.uint32)), name


@pytest.mark.parametrize("batch_max", [0, 64])
def test_score_topk_users_items_routes(monkeypatch, batch_max):
    """40 users: with ITEMS_BATCH_MAX_USERS = 64 three calls of the new entry (16 + 16 + 8),
    with 0 the gathered sub-table; row j == ops.score_topk(items=)'s row users[j] either way,
    and at k = 200 (the wide kernels on the sub-table)."""
    from lgcnhs import _native as N
    from lgcnhs import ops
    d = 64
    eu, ei, ex = _tables(d)[:3]
    cand = _cand_sets()["half"]
    ids = torch.as_tensor(np.random.default_rng(5).integers(0, U_TAB, 40))
    monkeypatch.setattr(ops, "ITEMS_BATCH_MAX_USERS", batch_max)
    calls = []
    real = N.lib().lg_score_topk_batch_items_f32

    class Spy:
        def __getattr__(self, name):
            if name == "lg_score_topk_batch_items_f32":
                return lambda *a: calls.append(a[3]) or real(*a)
            return getattr(N.load_library(), name)
    monkeypatch.setattr(N, "lib", lambda: Spy())  # (counts the entry's calls, passes all on)
    for k in (20, 200):
        full = ops.score_topk(eu, ei, k, ex, items=cand)
        v, i = ops.score_topk_users(eu, ei, ids, k, ex, items=cand)
        _same_rows(v, i, full, ids, k)
        assert (i >= 0).all()
    assert calls == ([16, 16, 8] if batch_max else [])
    with pytest.raises(ValueError):
        ops.score_topk_users(eu, ei, [0, 1], 20, ex, items=[0, ei.shape[0]])


def test_items_argument_forms_and_empty_sets():
    """items= as a bool mask, an unsorted list with duplicates and a device tensor give the
    same lists (kernel route and gather route); empty candidates give all padding."""
    from lgcnhs import ops
    d, k = 64, 20
    eu, ei, ex = _tables(d)[:3]
    I = ei.shape[0]
    cand = _cand_sets()["half"]
    mask = np.zeros(I, dtype=bool)
    mask[cand] = True
    rng = np.random.default_rng(9)
    shuffled = np.concatenate([rng.permutation(cand), cand[:10]]).tolist()
    ids = _ids(7, 70)
    assert len(ids) <= ops.ITEMS_CALL_USERS
    forms = (mask, torch.as_tensor(mask).to(DEV), shuffled, torch.as_tensor(cand).to(DEV))
    ref_u = ref_a = None
    for f in forms:
        vu, iu = ops.score_topk_users(eu, ei, ids, k, ex, items=f)
        va, ia = ops.score_topk(eu, ei, k, ex, items=f)
        if ref_u is None:
            ref_u, ref_a = (vu, iu), (va, ia)
            _same_rows(vu, iu, ref_a, ids)
        assert torch.equal(iu, ref_u[1]) and torch.equal(vu, ref_u[0])
        assert torch.equal(ia, ref_a[1]) and torch.equal(va, ref_a[0])
    for empty in ([], np.zeros(I, dtype=bool), torch.zeros(0, dtype=torch.int32, device=DEV)):
        for v, i in (ops.score_topk_users(eu, ei, ids, k, ex, items=empty),
                     ops.score_topk(eu, ei, k, ex, items=empty)):
            assert (i == -1).all() and (v == float("-inf")).all() and v.shape[1] == k
            assert i.dtype == torch.int64 and v.dtype == torch.float32
        assert ops.score_topk_users(eu, ei, ids, k, ex, items=empty)[0].shape[0] == 7
        assert ops.score_topk(eu, ei, k, ex, items=empty)[0].shape[0] == U_TAB


@pytest.mark.parametrize("batch_max", [0, 1 << 20])
def test_recommend_for_users_items_vs_reference(golden, monkeypatch, batch_max):
    """recommendForUsers(items=) on lightgcn_mid, every user, a seeded random half of the
    catalog: a user's candidates inside the reference's full top-k list (the fixture) are
    exactly the candidates scoring at least its k-th value, so they are the first m entries of
    the candidate ranking -- as sets, except users whose K-boundary gap (the fixture's own) is
    within the 1e-6 tie rule of the golden tests; at most 1 % of the users may be left out.
    (Checked on the CPU with the chain oracle before this was committed: no user of this
    fixture is within the rule.) Through the kernel and through the gather route; the Opti
    re-export follows."""
    from lgcnhs import ops
    from model.LightGCN.model import LightGCN
    from model.LightGCN.recommend import recommendForUsers
    from model.LightGCNOpti.recommend import recommendForUsers as opti_for_users
    from utils.graph import convertEdgeIndexToAdjMatrix
    monkeypatch.setattr(ops, "ITEMS_BATCH_MAX_USERS", batch_max)
    g = golden("lightgcn_mid")
    U, I, k = int(g["n_users"]), int(g["n_items"]), int(g["k"])
    torch.manual_seed(42)
    m = LightGCN(U, I, 64, 3).to(DEV)
    tr = convertEdgeIndexToAdjMatrix(U, I, torch.as_tensor(g["train"].astype(np.int64)))
    va = convertEdgeIndexToAdjMatrix(U, I, torch.as_tensor(g["val"].astype(np.int64)))
    cand = _random_cand(I, I // 2, 2024)
    cset = set(cand.tolist())
    users = np.random.default_rng(7).permutation(U).tolist()
    got = recommendForUsers(m, users, U, I, tr, va, None, k, items=cand.tolist())
    assert sorted(got) == list(range(U))
    gaps = g["rec_gaps"]
    ties = 0
    for u in range(U):
        want = [int(x) for x in g["recs"][u] if x >= 0 and int(x) in cset]
        assert set(got[u]) <= cset and len(got[u]) == k
        if set(got[u][:len(want)]) == set(want):
            continue
        assert not np.isnan(gaps[u, 1]) and abs(gaps[u, 0] - gaps[u, 1]) <= 1e-6, u
        ties += 1
    assert ties <= max(1, U // 100)
    # the lists are the chain oracle's on the sub-table, exactly
    rp, col = O.exclusion_csr(U, I, g["train"], g["val"])
    _, oi = _chain(m.users_emb.weight.detach().cpu().numpy(),
                   m.items_emb.weight.detach().cpu().numpy(), rp, col, cand, k)
    assert all(got[u] == oi[u].tolist() for u in range(U))
    some = opti_for_users(m, users[:5], U, I, tr, va, None, k,
                          items=torch.as_tensor(cand).to(DEV))
    assert all(some[u] == got[u] for u in users[:5])
