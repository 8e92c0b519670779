"""GPU parity of K2w (lg_score_topk_wide_f32, csrc/topk_wide.hip): full-catalog top-K for
128 < k <= 1024 with the candidate lists in global slabs. Every check is bit-exact (values
as uint32, ids equal) against the C chain oracle (oracle/score_chain.c, any k), the plain
k <= 128 kernel, or the dense masked score matrix sorted on the host."""
import numpy as np
import pytest
import torch

from oracle import lgcn_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _excl(U, I, density, seed):
    rng = np.random.default_rng(seed)
    n = int(U * I * density)
    u = rng.integers(0, U, n)
    i = rng.integers(0, I, n)
    return O.exclusion_csr(U, I, (u, i))


def _rowsets(rp, col, U, I):
    from lgcnhs.graph import RowSets
    return RowSets(torch.as_tensor(rp).to(DEV), torch.as_tensor(col).to(DEV), U, I)


def _emb(n, d, seed, scale=0.1):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(n, d, generator=g) * scale).float()


def _same(v, i, ov, oi, what=None):
    """(v, i) device tensors == (ov, oi) numpy arrays: ids equal, values bit for bit."""
    np.testing.assert_array_equal(i.cpu().numpy(), oi, err_msg=str(what))
    assert np.array_equal(v.cpu().numpy().view(np.uint32), ov.view(np.uint32)), what


def _wide_direct(eu, ei, k, ex, n_splits=1, mask=O.MASK):
    """lg_score_topk_wide_f32 through the C ABI (any k in [1, 1024]; no host routing)."""
    from lgcnhs import _native as N
    nu, d = eu.shape
    ni = ei.shape[0]
    ws_bytes = N.lib().lg_score_topk_wide_ws_bytes(nu, ni, d, k, n_splits)
    ws = torch.empty(max(ws_bytes, 8), dtype=torch.uint8, device=eu.device)
    val = torch.empty((nu, k), dtype=torch.float32, device=eu.device)
    idx = torch.empty((nu, k), dtype=torch.int64, device=eu.device)
    N.check(N.lib().lg_score_topk_wide_f32(
        N.ptr(eu), N.ptr(ei), nu, ni, d, N.ptr(ex.rowptr if ex else None),
        N.ptr(ex.col if ex else None), float(mask), int(k), int(n_splits), N.ptr(val),
        N.ptr(idx), N.ptr(ws), ws_bytes, N.stream_handle(eu.device)), "lg_score_topk_wide_f32")
    return val, idx


# ------------------------------------------------------------------------------ 1. grid
@pytest.mark.parametrize("d", [32, 64, 128])
@pytest.mark.parametrize("k", [129, 192, 256, 257, 512, 513, 1000, 1024])
def test_wide_topk_grid(d, k):
    """Every slab size (512 / 1024 / 2048 entries) on both sides of its k limits, every width,
    37 users (the last 16-user group is padded), 9000 items (several compactions per user at
    every slab size), one split, the host's choice and three (9000 / 3 is no multiple of 16)."""
    from lgcnhs import ops
    U, I = 37, 9000
    eu, ei = _emb(U, d, 10 + k), _emb(I, d, 20 + d)
    rp, col = _excl(U, I, 0.03, k)
    ov, oi = O.chain_topk(eu.numpy(), ei.numpy(), rp, col, k)
    for ns in (1, None, 3):
        v, i = ops.score_topk(eu.to(DEV), ei.to(DEV), k, _rowsets(rp, col, U, I), n_splits=ns)
        _same(v, i, ov, oi, ns)


# ------------------------------------------------- 2. the plain kernel's lists at k <= 128
def _non_finite_inputs(U, I, d):
    eu, ei = _emb(U, d, 41), _emb(I, d, 42)
    ei[1234] = float("nan")
    ei[2000, 5] = float("inf")
    eu[7] = float("nan")
    eu[11, 3] = -float("inf")
    eu[U - 1] = float("nan")  # the row padding users clamp to
    return eu, ei


@pytest.mark.parametrize("k", [20, 128])
def test_wide_equals_plain_kernel(k):
    """lg_score_topk_wide_f32 called directly at k <= 128 (slabs of 512) equals
    lg_score_topk_f32, on ordinary inputs and on test_screened_topk_non_finite_rows' (a NaN
    item row, a +inf element, a NaN user row, a -inf element, a NaN last user)."""
    from lgcnhs import ops
    U, I, d = 70, 3000, 64
    rp, col = _excl(U, I, 0.01, 43)
    ex = _rowsets(rp, col, U, I)
    for name, (eu, ei) in (("finite", (_emb(U, d, 44), _emb(I, d, 45))),
                           ("non-finite", _non_finite_inputs(U, I, d))):
        eu, ei = eu.to(DEV), ei.to(DEV)
        v0, i0 = ops.score_topk(eu, ei, k, ex, n_splits=1, screen=False)
        for ns in (1, 3):
            v, i = _wide_direct(eu, ei, k, ex, n_splits=ns)
            assert torch.equal(i, i0), (name, ns)
            assert torch.equal(v.view(torch.int32), v0.view(torch.int32)), (name, ns)
    assert not (i0 == 1234).any() and (i0[7] == -1).all() and (i0[U - 1] == -1).all()


# ------------------------------------------------------------------------------ 3. prefix
def test_wide_prefix_of_plain_and_screened():
    """200 users x 131072 items: the first 128 columns of the k = 256 and k = 1024 lists are
    the k = 128 lists of both k <= 128 kernels, and the full lists equal the oracle's (whose
    k = 256 list is the prefix of its k = 1024 list: one total order)."""
    from lgcnhs import ops
    U, I, d = 200, 131072, 64
    eu, ei = _emb(U, d, 71), _emb(I, d, 72)
    rp, col = _excl(U, I, 2e-4, 73)
    ex = _rowsets(rp, col, U, I)
    ov, oi = O.chain_topk(eu.numpy(), ei.numpy(), rp, col, 1024)
    eu, ei = eu.to(DEV), ei.to(DEV)
    small = [ops.score_topk(eu, ei, 128, ex, screen=s) for s in (False, True)]
    for k in (256, 1024):
        v, i = ops.score_topk(eu, ei, k, ex)
        _same(v, i, ov[:, :k], oi[:, :k], k)
        for v0, i0 in small:
            assert torch.equal(i[:, :128], i0)
            assert torch.equal(v[:, :128].view(torch.int32), v0.view(torch.int32))


# ------------------------------------------------------------- 4. short catalogs and masks
def test_wide_short_catalog_and_masks():
    """200 items, k = 300: every list is padded with -inf / -1; a user's excluded items follow
    its others at -1024 in item order; user 0 has every item excluded; excl=None."""
    from lgcnhs import ops
    U, I, k, d = 21, 200, 300, 64
    eu, ei = _emb(U, d, 81), _emb(I, d, 82)
    rng = np.random.default_rng(83)
    us = [0] * I + rng.integers(1, U - 1, 400).tolist()  # (the last user: no exclusions)
    its = list(range(I)) + rng.integers(0, I, 400).tolist()
    rp, col = O.exclusion_csr(U, I, (np.array(us), np.array(its)))
    ov, oi = O.chain_topk(eu.numpy(), ei.numpy(), rp, col, k)
    for ns in (1, 2):
        v, i = ops.score_topk(eu.to(DEV), ei.to(DEV), k, _rowsets(rp, col, U, I), n_splits=ns)
        _same(v, i, ov, oi, ns)
    assert (oi[:, I:] == -1).all() and np.isneginf(ov[:, I:]).all() and (oi[:, :I] >= 0).all()
    assert (ov[0, :I] == -1024.0).all() and (oi[0, :I] == np.arange(I)).all()
    n3 = int(rp[4] - rp[3])
    assert n3 > 0 and (ov[3, I - n3:I] == -1024.0).all()
    assert (np.diff(oi[3, I - n3:I]) > 0).all()
    assert rp[U] == rp[U - 1]
    ov, oi = O.chain_topk(eu.numpy(), ei.numpy(), None, None, k)
    v, i = ops.score_topk(eu.to(DEV), ei.to(DEV), k, None)
    _same(v, i, ov, oi, "no exclusions")


# ------------------------------------------------------------------- 5. exclusion runs
def test_wide_exclusion_runs():
    """User 0: 300 excluded items, all among its true top 400, which sit in one stretch of 400
    items that enters the k = 600 list (slab of 2048) between two compactions -- an excluded
    run longer than 64, so the cursor reads it in several batches. User 1: exclusions only
    among the last 10 items (past the last mid-stream compaction; they would rank first).
    User 2: a run of 700 consecutive excluded items at the start of the catalog."""
    from lgcnhs import ops
    U, I, k, d = 19, 9000, 600, 64
    eu, ei = _emb(U, d, 91), _emb(I, d, 92)
    c = torch.linspace(1.0, 3.0, 400).unsqueeze(1)
    ei[3000:3400] = eu[0] * c[torch.randperm(400, generator=torch.Generator().manual_seed(93))]
    ei[I - 10:] = eu[1] * torch.linspace(2.0, 3.0, 10).unsqueeze(1)
    G0 = O.chain_scores(eu[:1].numpy(), ei.numpy())[0]
    top400 = np.argsort(-G0, kind="stable")[:400]
    assert top400.min() >= 3000 and top400.max() < 3400
    ex0 = np.sort(top400[::4].tolist() + top400[1::4].tolist() + top400[2::4].tolist())
    assert len(ex0) == 300
    us = [0] * 300 + [1] * 6 + [2] * 700
    its = ex0.tolist() + [I - 9, I - 7, I - 4, I - 3, I - 2, I - 1] + list(range(700))
    rp, col = O.exclusion_csr(U, I, (np.array(us), np.array(its)))
    ov, oi = O.chain_topk(eu.numpy(), ei.numpy(), rp, col, k)
    assert not np.isin(oi[0], ex0).any() and not np.isin(oi[1], its[300:306]).any()
    for ns in (1, 3):
        v, i = ops.score_topk(eu.to(DEV), ei.to(DEV), k, _rowsets(rp, col, U, I), n_splits=ns)
        _same(v, i, ov, oi, ns)


# ------------------------------------------------------------------- 6. ties and order
@pytest.mark.parametrize("k", [256, 513])
def test_wide_ties_and_order(k):
    """40 item rows duplicated 8 times at scattered positions. User 0 reads dimension 0 and
    user 1 dimension 1 of the items: exactly k - 4 items score above one group of 8 equal
    rows, so the tie straddles positions k - 1 / k and the 4 lowest ids of the group make
    the list. User 2 is all zeros: every score is 0 and the list is the k lowest non-excluded
    ids."""
    from lgcnhs import ops
    U, I, d = 20, 6000, 64
    eu, ei = _emb(U, d, 101), _emb(I, d, 102)
    perm = torch.randperm(I, generator=torch.Generator().manual_seed(103)).numpy()
    dup = perm[:320].reshape(8, 40)       # dup[r, j]: copy r of base row j
    high = perm[320:320 + k - 4]          # the items above the tied group
    ei[:, :2] = ei[:, :2].clamp(-0.3, 0.3)
    ei[high, 0] = 1.0 + torch.rand(len(high), generator=torch.Generator().manual_seed(104))
    ei[high, 1] = 1.0 + torch.rand(len(high), generator=torch.Generator().manual_seed(105))
    for r in range(1, 8):
        ei[dup[r]] = ei[dup[0]]
    ei[dup[:, 0], 0] = 0.5                # group 0 ties for user 0
    ei[dup[:, 1], 1] = 0.5                # group 1 ties for user 1
    eu[0] = 0.0
    eu[0, 0] = 1.0
    eu[1] = 0.0
    eu[1, 1] = 1.0
    eu[2] = 0.0
    rp, col = _excl(U, I, 0.002, 106)
    # (users 0-2 unexcluded: their lists are fully determined above)
    keep = np.repeat(np.arange(U), np.diff(rp)) >= 3
    rp, col = O.exclusion_csr(U, I, (np.repeat(np.arange(U), np.diff(rp))[keep], col[keep]))
    ov, oi = O.chain_topk(eu.numpy(), ei.numpy(), rp, col, k)
    for u in (0, 1):
        assert sorted(oi[u, :k - 4]) == sorted(high)
        assert (oi[u, k - 4:] == np.sort(dup[:, u])[:4]).all() and (ov[u, k - 4:] == 0.5).all()
    assert (oi[2] == np.arange(k)).all() and (ov[2] == 0).all()
    for ns in (1, 3):
        v, i = ops.score_topk(eu.to(DEV), ei.to(DEV), k, _rowsets(rp, col, U, I), n_splits=ns)
        _same(v, i, ov, oi, ns)


# ------------------------------------------------------------------ 7. worst-case stream
@pytest.mark.parametrize("k", [129, 1024])
def test_wide_worst_case_stream(k):
    """Items c_i v with c_i increasing and users a v: every item beats every threshold, so
    each tile adds 16 entries per user and the kernel compacts as often as it can."""
    from lgcnhs import ops
    U, I, d = 18, 20000, 64
    v = _emb(1, d, 111, scale=1.0)
    ei = v * (1.0 + torch.arange(I, dtype=torch.float32).unsqueeze(1) / 1024.0)
    eu = v * torch.linspace(0.5, 2.0, U).unsqueeze(1)
    rp, col = _excl(U, I, 0.01, 112)
    ov, oi = O.chain_topk(eu.numpy(), ei.numpy(), rp, col, k)
    assert (np.diff(oi[0]) < 0).all() and oi[0, 0] >= I - 1 - k
    for ns in (1, 2):
        vv, i = ops.score_topk(eu.to(DEV), ei.to(DEV), k, _rowsets(rp, col, U, I), n_splits=ns)
        _same(vv, i, ov, oi, ns)


# --------------------------------------------------------------- 8. non-finite at wide k
def test_wide_non_finite_rows():
    """Test 2's non-finite inputs at k = 300, against ops.score_dense (the bit-exact chain and
    mask) sorted on the host by (value desc, id asc) and padded with -inf / -1. An item whose
    chain score is NaN or -inf never enters a list (the admission rule is sc > thr on the
    chain score, as in lg_score_topk_f32), so it is dropped by its unmasked score: an excluded
    item of a NaN user does not rank at the mask value either."""
    from lgcnhs import ops
    U, I, d, k = 70, 3000, 64, 300
    eu, ei = _non_finite_inputs(U, I, d)
    rp, col = _excl(U, I, 0.01, 43)
    ex = _rowsets(rp, col, U, I)
    eu, ei = eu.to(DEV), ei.to(DEV)
    raw = ops.score_dense(eu, ei).cpu().numpy()
    G = ops.score_dense(eu, ei, ex).cpu().numpy()
    ov = np.full((U, k), -np.inf, np.float32)
    oi = np.full((U, k), -1, np.int64)
    for u in range(U):
        ids = np.nonzero(~np.isnan(raw[u]) & ~np.isneginf(raw[u]))[0]
        order = ids[np.lexsort((ids, -G[u, ids]))][:k]
        ov[u, :len(order)] = G[u, order]
        oi[u, :len(order)] = order
    assert (oi[7] == -1).all() and (oi[U - 1] == -1).all() and not (oi == 1234).any()
    assert (oi[:, 0] == 2000).sum() > 0  # the +inf item ranks first where its chain is +inf
    assert (oi[[u for u in range(U) if u not in (7, 11, U - 1)]] >= 0).all()
    for ns in (1, None, 3):
        v, i = ops.score_topk(eu, ei, k, ex, n_splits=ns)
        _same(v, i, ov, oi, ns)


# ------------------------------------------------------------------------- 9. chunking
def test_wide_user_chunking(monkeypatch):
    """WIDE_WS_CAP_BYTES small enough for 3 user blocks (128 + 128 + 45 users): the result
    equals the unchunked one and the oracle's."""
    from lgcnhs import _native as N
    from lgcnhs import ops
    U, I, k, d = 301, 5000, 400, 64
    eu, ei = _emb(U, d, 121), _emb(I, d, 122)
    rp, col = _excl(U, I, 0.01, 123)
    ex = _rowsets(rp, col, U, I)
    ov, oi = O.chain_topk(eu.numpy(), ei.numpy(), rp, col, k)
    eu, ei = eu.to(DEV), ei.to(DEV)
    v0, i0 = ops.score_topk(eu, ei, k, ex, n_splits=2)
    _same(v0, i0, ov, oi, "unchunked")
    cap = N.lib().lg_score_topk_wide_ws_bytes(128, I, d, k, 2) + 4096
    assert ops._wide_user_block(U, I, d, k, 2, ops.WIDE_WS_CAP_BYTES) == U
    assert ops._wide_user_block(U, I, d, k, 2, cap) == 128
    monkeypatch.setattr(ops, "WIDE_WS_CAP_BYTES", cap)
    for ns in (2, None):
        v, i = ops.score_topk(eu, ei, k, ex, n_splits=ns)
        assert torch.equal(i, i0) and torch.equal(v.view(torch.int32), v0.view(torch.int32))
    # a cap below one workgroup's slabs still runs, 64 users at a time
    monkeypatch.setattr(ops, "WIDE_WS_CAP_BYTES", 1)
    v, i = ops.score_topk(eu, ei, k, ex, n_splits=1)
    _same(v, i, ov, oi, "64-user blocks")


# ------------------------------------------------------------------------------ 10. API
def test_wide_reference_api():
    """topk_for_all_users at k = 200 on a 150 x 900 synthetic graph == the oracle on the
    model's layer-0 weights with the train + val exclusions; k = 1025 and a screened wide
    call are refused."""
    from lgcnhs import ops
    from model.LightGCN.model import LightGCN
    from model.LightGCN.recommend import topk_for_all_users
    from utils.graph import convertEdgeIndexToAdjMatrix
    U, I, k = 150, 900, 200
    rng = np.random.default_rng(131)
    train = np.stack([rng.integers(0, U, 4000), rng.integers(0, I, 4000)])
    val = np.stack([rng.integers(0, U, 800), rng.integers(0, I, 800)])
    torch.manual_seed(42)
    m = LightGCN(U, I, 64, 3).to(DEV)
    tr = convertEdgeIndexToAdjMatrix(U, I, torch.as_tensor(train))
    va = convertEdgeIndexToAdjMatrix(U, I, torch.as_tensor(val))
    v, i = topk_for_all_users(m, U, I, tr, va, k)
    rp, col = O.exclusion_csr(U, I, train, val)
    ov, oi = O.chain_topk(m.users_emb.weight.detach().cpu().numpy(),
                          m.items_emb.weight.detach().cpu().numpy(), rp, col, k)
    _same(v, i, ov, oi)
    eu, ei = _emb(8, 64, 1).to(DEV), _emb(2000, 64, 2).to(DEV)
    with pytest.raises(ValueError):
        ops.score_topk(eu, ei, 1025)
    with pytest.raises(ValueError):
        ops.score_topk(eu, ei, 200, screen=True)
    assert ops.screen_pays(1, 10**9, 129) is False
