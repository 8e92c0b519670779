"""The walk's counting finish on the GPU: lg_spread_tile_resource_rank_f64 (MODE_RANK of
csrc/spread_tiled.hip) through ops.spread_rank_tiled and the reference-API mirrors. The ranks
are compared exactly and the values by their bits with (1) the complete peeled lists of
ops.spread_topk_tiled -- I <= 1024, so k = 1024 holds every ranking column -- and (2)
ops.rows_rank over the F that the F-writing reference walk sums; against the dense
ops.spread_rank the values agree within 1e-12 and the ranks wherever the row has no near-tie."""
import numpy as np
import pytest
import torch

import _poison as P
import _ref_paths as RP

pytestmark = pytest.mark.gpu
DEV = "cuda"
U, I, D = 300, 1000, 64
LAM = 0.5
MODES = ("G_drop", "drop", "none")
_CACHE = {}


def _graph(name):
    """A: 3,000 distinct random pairs (items without any user, so zero columns; user 5 without
    interactions in A0); B: the Zipf graph of test_spread_topk_tiled_equals_dense (hub rows,
    overflow runs). -> (Interactions, pairs u, pairs i)"""
    if name in _CACHE:
        return _CACHE[name]
    from lgcnhs import ops
    from lgcnhs.synth import synth_interactions
    if name == "B":
        u, i = synth_interactions(U, I, 9000, seed=11, dist="zipf")
        u, i = np.asarray(u, np.int64), np.asarray(i, np.int64)
    else:
        flat = np.random.default_rng(7).choice(U * I, 3000, replace=False)
        u, i = flat // I, flat % I
        if name == "A0":
            keep = u != 5
            u, i = u[keep], i[keep]
    A = ops.Interactions.from_pairs(torch.as_tensor(u), torch.as_tensor(i), U, I, DEV)
    _CACHE[name] = (A, u, i)
    return _CACHE[name]


def _emb(d=D, seed=3):
    key = ("emb", d, seed)
    if key not in _CACHE:
        g = torch.Generator(device=DEV).manual_seed(seed)
        _CACHE[key] = (torch.randn(U, d, device=DEV, generator=g) * 0.1,
                       torch.randn(I, d, device=DEV, generator=g) * 0.1)
    return _CACHE[key]


def _rowsets(rows, n_cols=I):
    from lgcnhs.graph import RowSets
    rp = np.zeros(len(rows) + 1, np.int64)
    rp[1:] = np.cumsum([len(r) for r in rows])
    col = np.concatenate([np.asarray(r, np.int64) for r in rows]) if rp[-1] else np.zeros(0)
    return RowSets(torch.as_tensor(rp).to(DEV), torch.as_tensor(col.astype(np.int32)).to(DEV),
                   len(rows), n_cols)


def _targets(name):
    """3 random non-interacted items per user; for 20 users also one interacted (excluded)
    item and one duplicate of the row's first target."""
    key = ("tg", name)
    if key in _CACHE:
        return _CACHE[key]
    _, u, i = _graph(name)
    rng = np.random.default_rng(1)
    seen = [set() for _ in range(U)]
    for a, b in zip(u, i):
        seen[a].add(int(b))
    rows = []
    for r in range(U):
        free = np.setdiff1d(np.arange(I), np.fromiter(seen[r], np.int64, len(seen[r])))
        rows.append(list(rng.choice(free, 3, replace=False)))
    with_items = [r for r in range(U) if seen[r]]
    for r in rng.choice(with_items, 20, replace=False):
        rows[r] += [int(rng.choice(sorted(seen[r]))), rows[r][0]]
    _CACHE[key] = _rowsets(rows)
    return _CACHE[key]


def _kw(mode, d=D):
    eu, ei = _emb(d) if mode == "G_drop" else (None, None)
    return dict(drop=mode != "none", eu=eu, ei=ei)


def _lists(name, mode, tile, d=D, users=None):
    """The complete lists: every ranking column of every row, by the peeled walk."""
    key = ("lists", name, mode, tile, d, None if users is None else tuple(users))
    if key not in _CACHE:
        from lgcnhs import ops
        A = _graph(name)[0]
        v, i = ops.spread_topk_tiled(A, LAM, 1024, A.by_user, users=users, tile=tile,
                                     **_kw(mode, d))
        _CACHE[key] = (v.cpu().numpy(), i.cpu().numpy())
    return _CACHE[key]


def _ref_F(name, tile, vthr=None):
    """All of F [U, I] from the F-writing reference walk over TileWeights' tiles."""
    key = ("F", name, tile, vthr)
    if key not in _CACHE:
        from lgcnhs import ops
        A = _graph(name)[0]
        tw = ops.TileWeights(A, LAM, tile, vthr=vthr)
        F = torch.zeros((U, -(-I // tile) * tile), dtype=torch.float64, device=DEV)
        hubs = 0
        for j0 in range(0, I, tile):
            tw.build(j0)
            hubs += int(tw.is_hub.sum())
            RP.resource(tw, 0, U, F[:, j0:])
        _CACHE[key] = (F[:, :I], hubs)
    return _CACHE[key][0] if vthr is None else _CACHE[key]


def check_against_lists(tg, out, lists, what=""):
    """rank = the target's position in its row's complete list, -1 when it is not there; the
    value bit-equal to the list's. Returns (zero-valued targets, positive-valued targets
    exactly tied with another ranking column)."""
    lv, li = lists
    rp, col = tg.rowptr.cpu().numpy(), tg.col.cpu().numpy()
    rank, val = (x.cpu().numpy() for x in out)
    assert rank.dtype == np.int64 and val.dtype == np.float64 and len(rank) == len(col)
    zeros = tied = 0
    for r in range(tg.n_rows):
        pos = {int(c): p for p, c in enumerate(li[r]) if c >= 0}
        n_in = len(pos)
        for p in range(rp[r], rp[r + 1]):
            want = pos.get(int(col[p]), -1)
            assert rank[p] == want, (what, r, int(col[p]), int(rank[p]), want)
            if want < 0:
                continue
            assert val[p:p + 1].view(np.int64)[0] == lv[r, want:want + 1].view(np.int64)[0], \
                (what, r, int(col[p]))
            zeros += val[p] == 0
            tied += val[p] > 0 and ((want > 0 and lv[r, want - 1] == val[p]) or
                                    (want + 1 < n_in and lv[r, want + 1] == val[p]))
    return int(zeros), int(tied)


# ------------------------------------------------------------------- 1: complete-list oracle
@pytest.mark.parametrize("tile", [64, 333, 4096])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["A", "B"])
def test_ranks_are_the_positions_in_the_complete_lists(name, mode, tile):
    """16 tiles, a partial last tile, one tile; zero columns and exact ties (A), hub rows and
    overflow runs (B). The id tie rule decides many ranks: on A without G at least 100 targets
    have the value 0 and at least 100 positive ones are exactly tied with another column.

    With G the zero-valued targets (F = 0 times a finite score: an exact +-0) tie with every
    other zero column of the row: these cases hold only because the walk's top-K finish lets a
    column that ties the moving k-th value through to the (value, id) comparison."""
    from lgcnhs import ops
    A = _graph(name)[0]
    tg = _targets(name)
    out = ops.spread_rank_tiled(A, LAM, tg, A.by_user, tile=tile, **_kw(mode))
    zeros, tied = check_against_lists(tg, out, _lists(name, mode, tile), (name, mode, tile))
    rank = out[0].cpu().numpy()
    if mode != "none":  # the 20 interacted targets are dropped
        assert int((rank < 0).sum()) == 20
    else:
        assert int((rank < 0).sum()) == 0
    if name == "A":
        assert zeros >= 100, zeros
        if mode != "G_drop":
            assert tied >= 100, tied
    assert int(rank.max()) > 128  # (deeper than any single walk's list)


# --------------------------------------------------------------- 2: F-writing reference walk
@pytest.mark.parametrize("tile", [64, 333])
@pytest.mark.parametrize("mode", MODES)
def test_ranks_are_rows_rank_of_the_reference_walks_F(monkeypatch, mode, tile):
    """F assembled from the F-writing reference walk over the same tiles (vthr = 40: V rows,
    dense V rows and overflow runs on the Zipf graph), ranked by lg_rows_rank_f64."""
    from lgcnhs import ops
    A = _graph("B")[0]
    tg = _targets("B")
    real_tw = ops.TileWeights
    F, hubs = _ref_F("B", tile, vthr=40)
    assert hubs > 0
    kw = _kw(mode)
    want = ops.rows_rank(F, tg, A.by_user, kw["drop"], kw["eu"], kw["ei"])
    monkeypatch.setattr(ops, "TileWeights",
                        lambda A_, lam, t, **k: real_tw(A_, lam, t, vthr=40, **k))
    got = ops.spread_rank_tiled(A, LAM, tg, A.by_user, tile=tile, **kw)
    assert torch.equal(got[0], want[0])
    assert P.bit_equal(got[1], want[1])


# ---------------------------------------------------------------------- 3: targets per user
@pytest.mark.parametrize("mode", ["G_drop", "drop"])
def test_any_number_of_targets_per_user(mode):
    """Rows of 0, 1, the per-pass constant, the constant + 1, 70 (descending) and 300
    (shuffled) targets in one call, and a user without interactions."""
    from lgcnhs import ops
    M = ops.SPREAD_RANK_ROW_MAX
    assert M == 8
    A = _graph("A0")[0]
    assert int(A.by_user.degrees()[5]) == 0
    rng = np.random.default_rng(5)
    rows = [[] for _ in range(U)]
    rows[1] = [int(rng.integers(I))]
    rows[2] = list(rng.choice(I, M, replace=False))
    rows[3] = list(rng.choice(I, M + 1, replace=False))
    rows[4] = sorted(rng.choice(I, 70, replace=False))[::-1]
    rows[5] = list(rng.choice(I, 5, replace=False))
    rows[6] = list(rng.permutation(I)[:300])
    rows[299] = [0, I - 1, 0]
    tg = _rowsets(rows)
    kw = _kw(mode)
    out = ops.spread_rank_tiled(A, LAM, tg, A.by_user, tile=333, **kw)
    # the definition: lg_rows_rank_f64 over the F that the F-writing reference walk sums
    want = ops.rows_rank(_ref_F("A0", 333), tg, A.by_user, kw["drop"], kw["eu"], kw["ei"])
    assert torch.equal(out[0], want[0])
    assert P.bit_equal(out[1], want[1])
    check_against_lists(tg, out, _lists("A0", mode, 333), mode)
    rp = tg.rowptr.cpu().numpy()
    if mode == "drop":  # no interactions: F = 0 everywhere, the rank is the item id
        np.testing.assert_array_equal(out[0][rp[5]:rp[6]].cpu().numpy(), np.asarray(rows[5]))


def test_out_of_range_entries():
    """Ids outside the catalog and entries of col outside every row get {-1, -inf}."""
    from lgcnhs import ops
    from lgcnhs.graph import RowSets
    A = _graph("A")[0]
    rows = [[3, -1, I, 7]] + [[] for _ in range(U - 1)]
    tg = _rowsets(rows)
    rk, val = ops.spread_rank_tiled(A, LAM, tg, None, tile=64)
    assert rk[1] == -1 and rk[2] == -1 and rk[0] >= 0 and rk[3] >= 0
    assert val[1] == -np.inf and val[2] == -np.inf
    cut = RowSets(tg.rowptr.clamp(min=1, max=3), tg.col, U, I)  # row 0 = entries [1, 3)
    rk2, val2 = ops.spread_rank_tiled(A, LAM, cut, None, tile=64)
    assert rk2.tolist() == [-1, -1, -1, -1] and bool((val2 == -np.inf).all())


# ------------------------------------------------------------------------------- 4: users=
@pytest.mark.parametrize("mode", MODES)
def test_users_rows_are_the_all_users_rows(mode):
    from lgcnhs import ops
    A = _graph("B")[0]
    tg = _targets("B")
    ids = [7, 7, 299, 0]
    full = ops.spread_rank_tiled(A, LAM, tg, A.by_user, tile=333, **_kw(mode))
    part = ops.spread_rank_tiled(A, LAM, tg.take(torch.as_tensor(ids)), A.by_user, users=ids,
                                 tile=333, **_kw(mode))
    rp = tg.rowptr.cpu().numpy()
    sel = torch.as_tensor(np.concatenate([np.arange(rp[u], rp[u + 1]) for u in ids])).to(DEV)
    assert torch.equal(part[0], full[0][sel])
    assert P.bit_equal(part[1], full[1][sel])


# -------------------------------------------------------------------------------- 5: dims
@pytest.mark.parametrize("d", [32, 128])
def test_embedding_widths(d):
    from lgcnhs import ops
    A = _graph("B")[0]
    tg = _targets("B")
    out = ops.spread_rank_tiled(A, LAM, tg, A.by_user, tile=256, **_kw("G_drop", d))
    check_against_lists(tg, out, _lists("B", "G_drop", 256, d), d)


# ------------------------------------------------------------- 6: the dense ops.spread_rank
@pytest.mark.parametrize("mode", MODES)
def test_against_the_dense_path(mode):
    """Values within 1e-12 relative; ranks equal wherever the dense row has no other value
    within 1e-9 relative of the target's -- at least 90 % of the positive-valued targets."""
    from lgcnhs import ops
    A = _graph("B")[0]
    tg = _targets("B")
    kw = _kw(mode)
    W = ops.spread_hybrid(A, LAM)
    rd, vd = (x.cpu().numpy() for x in ops.spread_rank(A, LAM, tg, A.by_user, W=W, **kw))
    rt, vt = (x.cpu().numpy() for x in ops.spread_rank_tiled(A, LAM, tg, A.by_user, tile=333,
                                                             **kw))
    assert np.all(np.abs(vt - vd) <= 1e-12 * np.abs(vd))
    np.testing.assert_array_equal(rt < 0, rd < 0)
    F = ops.spread_resource(A, W).cpu().numpy()
    if kw["eu"] is not None:
        from oracle import lgcn_oracle as O
        F = O.chain_scores(kw["eu"].cpu().numpy(), kw["ei"].cpu().numpy()).astype(np.float64) * F
    rp, col = tg.rowptr.cpu().numpy(), tg.col.cpu().numpy()
    clear = np.zeros(len(col), bool)
    for r in range(U):
        for p in range(rp[r], rp[r + 1]):
            near = np.abs(F[r] - vd[p]) <= 1e-9 * abs(vd[p])
            near[col[p]] = False
            clear[p] = not near.any()
    pos = (vd > 0) & (rd >= 0)
    assert clear[pos].sum() >= 0.9 * pos.sum(), (int(clear[pos].sum()), int(pos.sum()))
    np.testing.assert_array_equal(rt[clear], rd[clear])


# ------------------------------------------------------------------------------ 7: mirrors
def _hold_out_last(train):
    """Split off the last train item of every user with >= 3 of them: (train', held) frames."""
    import pandas as pd
    u, i = train[0].astype(np.int64), train[1].astype(np.int64)
    cnt = np.bincount(u)
    last = {}
    for p, x in enumerate(u):
        last[x] = p
    held = np.array(sorted(p for x, p in last.items() if cnt[x] >= 3), np.int64)
    keep = np.ones(len(u), bool)
    keep[held] = False
    return (pd.DataFrame({"user_id": u[keep], "item_id": i[keep]}),
            pd.DataFrame({"user_id": u[held], "item_id": i[held]}))


def _ranks_agree_with_lists(targets, rank, idx, k):
    rp, col = targets.rowptr.cpu().numpy(), targets.col.cpu().numpy()
    rank, idx = rank.cpu().numpy(), idx.cpu().numpy()
    assert len(rank) == len(col) > 0
    inside = 0
    for u in range(targets.n_rows):
        for p in range(rp[u], rp[u + 1]):
            if 0 <= rank[p] < k:
                assert idx[u, rank[p]] == col[p], (u, col[p], rank[p])
                inside += 1
            else:
                assert col[p] not in idx[u], (u, col[p], rank[p])
    return inside


def test_spread_method_ranks_tiled_agree_with_the_topk_twin(golden, monkeypatch):
    import pandas as pd
    from lgcnhs import ops
    from model.SpreadMethod.recommend import spread_method_ranks, spread_method_topk
    g = golden("spread_ml100k")
    n_u, n_i = int(g["n_users"]), int(g["n_items"])
    tr, held = _hold_out_last(g["train"])
    va = pd.DataFrame({"user_id": g["val"][0].astype(np.int64),
                       "item_id": g["val"][1].astype(np.int64)})
    lam = float(g["hybrid_lambda"])
    args = (n_u, n_i, tr, va)
    targets, rank = spread_method_ranks(*args, held, "HybridS", lam, "movielens", tiled=True)
    _, idx = spread_method_topk(*args, "HybridS", lam, "movielens", 20, tiled=True)
    assert _ranks_agree_with_lists(targets, rank, idx, 20) > 0
    # a user slice: those rows of the same answer
    ids = [7, 7, 900, 0]
    t2, r2 = spread_method_ranks(*args, held, "HybridS", lam, "movielens", users=ids,
                                 tiled=True, tile=2048)
    rp = targets.rowptr.cpu().numpy()
    sel = np.concatenate([np.arange(rp[u], rp[u + 1]) for u in ids]).astype(np.int64)
    np.testing.assert_array_equal(r2.cpu().numpy(), rank.cpu().numpy()[sel])
    # tiled=None on a catalog whose dense matrices do not fit: the walk, not an error
    monkeypatch.setattr(ops, "dense_spread_fits", lambda n_items, device: False)
    t3, r3 = spread_method_ranks(*args, held, "HybridS", lam, "movielens", users=ids)
    np.testing.assert_array_equal(r3.cpu().numpy(), rank.cpu().numpy()[sel])


def test_spread_lightgcn_ranks_tiled_agree_with_the_topk_twin(golden):
    import pandas as pd
    from model.LightGCN.model import LightGCN
    from model.SpreadLightGCN.recommend import spread_lightgcn_ranks, spread_lightgcn_topk
    g = golden("lightgcn_mid")
    n_u, n_i = int(g["n_users"]), int(g["n_items"])
    torch.manual_seed(42)
    m = LightGCN(n_u, n_i, 64, 3).to(DEV)
    tr, held = _hold_out_last(g["train"])
    va = pd.DataFrame({"user_id": g["val"][0].astype(np.int64),
                       "item_id": g["val"][1].astype(np.int64)})
    lam = float(g["slgcn_lambda"])
    targets, rank = spread_lightgcn_ranks(m, n_u, n_i, tr, va, held, lam, tiled=True)
    _, idx = spread_lightgcn_topk(m, n_u, n_i, tr, va, lam, 20, tiled=True)
    assert _ranks_agree_with_lists(targets, rank, idx, 20) > 0


# ----------------------------------------------------------- 8: stale memory, call context
@pytest.mark.parametrize("mode", ["G_drop", "drop"])
def test_does_not_depend_on_what_memory_held(mode):
    """Plain, over a decoy's buffers (another lambda, other embeddings: the same allocation
    sequence), over 0xFF bytes: the outputs, val and cnt start from the library's own fills."""
    from lgcnhs import ops
    A = _graph("B")[0]
    tg = _targets("B")
    kw = _kw(mode)
    decoy_kw = dict(kw)
    if mode == "G_drop":
        decoy_kw["eu"], decoy_kw["ei"] = _emb(D, seed=9)
    lists = _lists("B", mode, 333)
    P.three_ways(lambda: ops.spread_rank_tiled(A, LAM, tg, A.by_user, tile=333, **kw),
                 lambda: ops.spread_rank_tiled(A, 0.9, tg, A.by_user, tile=333, **decoy_kw),
                 lambda out, how: check_against_lists(tg, out, lists, how))


def test_side_stream_and_stats():
    from lgcnhs import ops
    A = _graph("B")[0]
    tg = _targets("B")
    kw = _kw("G_drop")
    base = ops.spread_rank_tiled(A, LAM, tg, A.by_user, tile=333, **kw)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got = ops.spread_rank_tiled(A, LAM, tg, A.by_user, tile=333, **kw)
    side.synchronize()
    assert P.bit_equal(got, base)
    stats = {}
    again = ops.spread_rank_tiled(A, LAM, tg, A.by_user, tile=333, stats=stats, **kw)
    assert P.bit_equal(again, base)
    assert stats["count_launches"] == 4 and 1 <= stats["value_launches"] <= 4
    for name in ("t_build_ms", "t_bounds_ms", "t_value_ms", "t_count_ms"):
        assert stats[name] >= 0.0
