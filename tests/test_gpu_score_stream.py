"""GPU pins for what csrc/score_stream.h couples: k_score_topk (K2), k_score_topk_wide (K2w) and
k_score_topk_batch (K2b) take their tile loads, their filter, their threshold rule and their
lazy exclusion from one text. Two properties on one small shape -- 33 users (the last wave has
padding users), 2005 items (no multiple of the 16-item tile, nor are the splits' ends), about
30 excluded items per user with some on the last item of a split and the first of the next:
every kernel equals the dense masked scores' top-k bit for bit, and the three kernels agree
bit for bit at their shared boundary k = 128 / 129. Regression pins: the kernels of the
commit before the header pass them too."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
U, I = 33, 2005
# split_len(2005, 3) = 672: the items around the split ends, the table's ends, a tile's ends
EDGE_ITEMS = (0, 15, 16, 671, 672, 1343, 1344, 2003, 2004)

_CASES = {}


def _case(d):
    """(eu, ei, excl, ref_val, ref_idx) per width, computed once and never modified: the
    reference is the full sort of ops.score_dense's masked scores by (score desc, item asc)."""
    from lgcnhs import ops
    from lgcnhs.graph import RowSets
    if d not in _CASES:
        g = torch.Generator().manual_seed(1000 + d)
        eu = (torch.randn(U, d, generator=g) * 0.1).float().to(DEV)
        ei = (torch.randn(I, d, generator=g) * 0.1).float().to(DEV)
        rng = np.random.default_rng(2000 + d)
        rows = np.concatenate([np.repeat(np.arange(U), 21),
                               np.repeat(np.arange(U), len(EDGE_ITEMS))])
        cols = np.concatenate([rng.integers(0, I, U * 21), np.tile(EDGE_ITEMS, U)])
        excl = RowSets.from_pairs(torch.as_tensor(rows), torch.as_tensor(cols), U, I, DEV)
        G = ops.score_dense(eu, ei, excl)
        rv, ri = torch.sort(G, dim=1, descending=True, stable=True)  # ties: item ascending
        tv = torch.topk(G, 200, dim=1).values
        assert torch.equal(tv.view(torch.int32), rv[:, :200].view(torch.int32))
        _CASES[d] = (eu, ei, excl, rv, ri)
    return _CASES[d]


def _same(v, i, rv, ri, what):
    assert torch.equal(i, ri), what
    assert torch.equal(v.view(torch.int32), rv.view(torch.int32)), what


def _batch_abi(eu, ei, ids, k, ex):
    """lg_score_topk_batch_f32 through the C ABI: no host routing by the number of ids."""
    from lgcnhs import _native as N
    from lgcnhs import ops
    nu, d = eu.shape
    ni, nb = ei.shape[0], ids.numel()
    ws_bytes = N.lib().lg_score_topk_batch_ws_bytes(nb, ni, d, k)
    ws = torch.empty(max(ws_bytes, 8), dtype=torch.uint8, device=DEV)
    val = torch.empty((nb, k), dtype=torch.float32, device=DEV)
    idx = torch.empty((nb, k), dtype=torch.int64, device=DEV)
    N.check(N.lib().lg_score_topk_batch_f32(
        N.ptr(eu), N.ptr(ei), N.ptr(ids), nb, nu, ni, d, N.ptr(ex.rowptr), N.ptr(ex.col),
        float(ops.MASK_VALUE), int(k), N.ptr(val), N.ptr(idx), N.ptr(ws), ws_bytes,
        N.stream_handle(eu.device)), "lg_score_topk_batch_f32")
    return val, idx


@pytest.mark.parametrize("d", [32, 128])
@pytest.mark.parametrize("n_splits", [1, 3])
def test_range_ends_off_the_tile(d, n_splits):
    """Plain at k = 20 and wide at k = 200 over 1 and 3 splits, the batch entry on the ids
    [32, 0, 7] at k = 20 (its item ranges are the launch's own: 16 items per wave here): each
    equals the dense masked scores' top-k, values bitwise and ids exactly."""
    from lgcnhs import ops
    eu, ei, excl, rv, ri = _case(d)
    v, i = ops.score_topk(eu, ei, 20, excl, n_splits=n_splits, screen=False)
    _same(v, i, rv[:, :20], ri[:, :20], ("plain", d, n_splits))
    v, i = ops.score_topk(eu, ei, 200, excl, n_splits=n_splits)
    _same(v, i, rv[:, :200], ri[:, :200], ("wide", d, n_splits))
    ids = torch.tensor([32, 0, 7], dtype=torch.int64, device=DEV)
    assert ids.numel() <= ops.BATCH_MAX_USERS  # (the batch entry, not the gathered route)
    v, i = ops.score_topk_users(eu, ei, ids, 20, excl)
    _same(v, i, rv[ids, :20], ri[ids, :20], ("batch", d))


@pytest.mark.parametrize("d", [32, 128])
def test_three_kernels_agree_at_the_shared_boundary(d):
    """Plain at k = 128, the first 128 columns of wide at k = 129 and the batch entry at
    k = 128 on all 33 ids in one call: equal bit for bit."""
    from lgcnhs import ops
    eu, ei, excl, rv, ri = _case(d)
    pv, pi = ops.score_topk(eu, ei, 128, excl, screen=False)
    wv, wi = ops.score_topk(eu, ei, 129, excl)
    bv, bi = _batch_abi(eu, ei, torch.arange(U, dtype=torch.int64, device=DEV), 128, excl)
    _same(wv[:, :128].contiguous(), wi[:, :128].contiguous(), pv, pi, ("wide", d))
    _same(bv, bi, pv, pi, ("batch", d))
    _same(pv, pi, rv[:, :128], ri[:, :128], ("plain", d))
