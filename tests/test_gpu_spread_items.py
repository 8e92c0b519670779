"""GPU tests of the spreading / LGCNHS top-K over a candidate item set (items=).

Dense (csrc/rows_topk_items.hip, lg_spread_rows_topk_items_f64): bit for bit
rows_topk(spread_resource(A, W)[:, C], k, excl.restrict_cols(C), drop, eu, ei[C]) with the ids
mapped back through C, and the fp64 oracle's rows on the same F columns. Tiled (the column view
of ops.TileWeights / TileWalk): bitwise the no-items walk for C = every item, within 1e-12
relative of the dense result otherwise (the walk's own summation order), the peel in id space.
"""
import ctypes

import numpy as np
import pytest
import torch

from _compare import compare_lists_close
from oracle import lgcn_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
KS = (1, 20, 64, 65, 128, 129, 256, 1024)


def bits(v):
    return v.contiguous().view(torch.int64)


def same(a, b):
    return bool(torch.equal(a[1], b[1]) and torch.equal(bits(a[0]), bits(b[0])))


def map_back(i, cand):
    c64 = cand.to(torch.int64)
    return torch.where(i >= 0, c64[i.clamp(min=0)], i)


def reference(F, cand, k, ex, drop=True, eu=None, ei=None):
    """The contract: rows_topk on the gathered columns, exclusions renumbered, ids mapped."""
    from lgcnhs import ops
    n = F.shape[0]
    if cand.numel() == 0:
        return (torch.full((n, k), float("-inf"), dtype=torch.float64, device=DEV),
                torch.full((n, k), -1, dtype=torch.int64, device=DEV))
    c64 = cand.to(torch.int64)
    exr = ex.restrict_cols(cand) if ex is not None else None
    if exr is not None and exr.col.numel() == 0:
        exr = None  # (no excluded candidate: an empty tensor has no pointer to pass)
    v, i = ops.rows_topk(F[:, c64].contiguous(), k, exr, drop, eu,
                         None if ei is None else ei[c64])
    return v, map_back(i, cand)


def oracle_rows(S, cand, k, ex, drop=True):
    """oracle.lgcn_oracle.rows_topk on the columns cand of the fp64 matrix S (host): entries
    that may not rank (NaN, -inf) leave the list."""
    c = cand.cpu().numpy().astype(np.int64)
    if c.size == 0:
        return np.full((S.shape[0], k), -np.inf), np.full((S.shape[0], k), -1, np.int64)
    exr = ex.restrict_cols(cand) if ex is not None else None
    Sc = np.where(np.isnan(S[:, c]), -np.inf, S[:, c])
    ov, oi = O.rows_topk(Sc, k, None if exr is None else exr.rowptr.cpu().numpy(),
                         None if exr is None else exr.col.cpu().numpy(), drop)
    oi = np.where(np.isneginf(ov), -1, oi)
    return ov, np.where(oi >= 0, c[np.clip(oi, 0, None)], -1)


# ---------------------------------------------------------------------------------- dense
class Small:
    """40 users x 300 items: user 0 without interactions (an all-zero F row: ties by id),
    users 1..5 of degree 1, 3, 4, 5, 9 (the unroll-by-4 tail), the rest 2..20. The exclusions
    are the users' own items plus the items X for every user."""

    def __init__(self):
        from lgcnhs import ops
        from lgcnhs.graph import RowSets
        U, I = 40, 300
        rng = np.random.default_rng(5)
        deg = [0, 1, 3, 4, 5, 9] + rng.integers(2, 21, U - 6).tolist()
        us = np.concatenate([np.full(d, u) for u, d in enumerate(deg)]).astype(np.int64)
        it = np.concatenate([rng.choice(I, d, replace=False) for d in deg]).astype(np.int64)
        self.U, self.I = U, I
        self.A = ops.Interactions.from_pairs(torch.as_tensor(us), torch.as_tensor(it), U, I, DEV)
        assert self.A.by_user.degrees()[:6].tolist() == [0, 1, 3, 4, 5, 9]
        self.W = ops.spread_hybrid(self.A, 0.5)
        self.F = ops.spread_resource(self.A, self.W)
        self.Fh = self.F.cpu().numpy()
        self.X = np.array([2, 50, 51, 120, 199, 200, 299])
        xs = np.tile(self.X, U)
        xu = np.repeat(np.arange(U), len(self.X))
        self.ex = RowSets.union(self.A.by_user,
                                RowSets.from_pairs(torch.as_tensor(xu), torch.as_tensor(xs), U, I,
                                                   DEV))
        self.sets = {
            "all": np.arange(I), "empty": np.zeros(0, np.int64), "one": np.array([137]),
            "first63": np.arange(63), "first64": np.arange(64), "first65": np.arange(65),
            "every_second": np.arange(0, I, 2),
            "random10": np.sort(rng.choice(I, I // 10, replace=False)),
            "only_excluded": self.X,
        }

    def cand(self, name):
        return torch.as_tensor(self.sets[name]).to(DEV, torch.int32)


@pytest.fixture(scope="module")
def small():
    return Small()


@pytest.mark.parametrize("name", ["all", "empty", "one", "first63", "first64", "first65",
                                  "every_second", "random10", "only_excluded"])
def test_dense_candidate_sets_bitwise(small, name):
    from lgcnhs import ops
    s, cand = small, small.cand(name)
    for k in KS:
        for drop in (True, False):
            got = ops.spread_rows_topk_items(s.A.by_user, s.W, cand, k, s.ex, drop)
            assert same(got, reference(s.F, cand, k, s.ex, drop)), (name, k, drop)
            ov, oi = oracle_rows(s.Fh, cand, k, s.ex, drop)
            assert np.array_equal(got[1].cpu().numpy(), oi), (name, k, drop)
            assert np.array_equal(got[0].cpu().numpy(), ov), (name, k, drop)
            ids = got[1][got[1] >= 0]
            assert bool(torch.isin(ids, cand.to(torch.int64)).all())
    # every user's exclusions hold X: all padding under DROP, ranked under NONE
    if name == "only_excluded":
        v, i = ops.spread_rows_topk_items(s.A.by_user, s.W, cand, 20, s.ex, True)
        assert bool((i == -1).all()) and bool(torch.isneginf(v).all())
        v, i = ops.spread_rows_topk_items(s.A.by_user, s.W, cand, 20, s.ex, False)
        assert bool((i[:, :7] >= 0).all()) and bool((i[:, 7:] == -1).all())
    if name == "empty":
        v, i = ops.spread_rows_topk_items(s.A.by_user, s.W, cand, 5, s.ex, True)
        assert bool((i == -1).all()) and bool(torch.isneginf(v).all())
    if name == "all":  # the user without interactions: F = 0 everywhere, ties go to the ids
        _, i = ops.spread_rows_topk_items(s.A.by_user, s.W, cand, 20, None, True)
        assert i[0].tolist() == list(range(20))


@pytest.mark.parametrize("d", [32, 64, 128])
def test_dense_with_g_factor_bitwise(small, d):
    """G * F with negative products; a NaN item row inside C never ranks, one outside C has no
    effect."""
    from lgcnhs import ops
    s = small
    g = torch.Generator().manual_seed(d)
    eu = (torch.randn(s.U, d, generator=g) * 0.1).to(DEV)
    ei = (torch.randn(s.I, d, generator=g) * 0.1).to(DEV)
    cand = s.cand("every_second")
    nan_in, nan_out = 40, 41
    ei_nan = ei.clone()
    ei_nan[nan_in] = float("nan")
    ei_both = ei_nan.clone()
    ei_both[nan_out] = float("nan")
    Gh = O.chain_scores(eu.cpu().numpy(), ei_nan.cpu().numpy()).astype(np.float64)
    Sh = Gh * s.Fh
    assert (Sh[:, cand.cpu().numpy()] < 0).any()
    for k in KS:
        got = ops.spread_rows_topk_items(s.A.by_user, s.W, cand, k, s.ex, True, eu, ei_both)
        assert same(got, reference(s.F, cand, k, s.ex, True, eu, ei_both)), k
        assert same(got, ops.spread_rows_topk_items(s.A.by_user, s.W, cand, k, s.ex, True, eu,
                                                    ei_nan)), k
        assert not bool((got[1] == nan_in).any())
        ov, oi = oracle_rows(Sh, cand, k, s.ex, True)
        assert np.array_equal(got[1].cpu().numpy(), oi), k
        assert np.array_equal(got[0].cpu().numpy(), ov), k
    full = s.cand("all")
    got = ops.spread_rows_topk_items(s.A.by_user, s.W, full, 300, s.ex, True, eu, ei_both)
    assert not bool(((got[1] == nan_in) | (got[1] == nan_out)).any())


@pytest.fixture(scope="module")
def wide():
    """60 users x 4,200 items, user 0 without interactions (ties across every seam)."""
    from lgcnhs import ops
    U, I = 60, 4200
    rng = np.random.default_rng(9)
    deg = [0] + rng.integers(1, 30, U - 1).tolist()
    us = np.concatenate([np.full(d, u) for u, d in enumerate(deg)]).astype(np.int64)
    it = np.concatenate([rng.choice(I, d, replace=False) for d in deg]).astype(np.int64)
    A = ops.Interactions.from_pairs(torch.as_tensor(us), torch.as_tensor(it), U, I, DEV)
    W = ops.spread_hybrid(A, 0.3)
    g = torch.Generator().manual_seed(1)
    eu = (torch.randn(U, 64, generator=g) * 0.1).to(DEV)
    ei = (torch.randn(I, 64, generator=g) * 0.1).to(DEV)
    return A, W, ops.spread_resource(A, W), eu, ei, rng


@pytest.mark.parametrize("off", [-1, 0, 1])
def test_dense_wave_seams(wide, off):
    """|C| around the several-waves-per-row threshold (ops.ROWS_ITEMS_SPLIT) and around 4096:
    the waves' position ranges, their seams and the pairwise merge."""
    from lgcnhs import ops
    A, W, F, eu, ei, rng = wide
    assert ops.ROWS_ITEMS_SPLIT == 512
    for base in (ops.ROWS_ITEMS_SPLIT, 4096):
        nc = base + off
        cand = torch.as_tensor(np.sort(rng.choice(A.n_items, nc, replace=False))) \
            .to(DEV, torch.int32)
        for k in (20, 129, 300, 1024):
            got = ops.spread_rows_topk_items(A.by_user, W, cand, k, A.by_user, True)
            assert same(got, reference(F, cand, k, A.by_user)), (nc, k)
            # the all-zero row: every candidate ties, the list is the k smallest ids, across
            # the waves' seams
            assert got[1][0].tolist() == cand[:k].tolist() + [-1] * max(0, k - nc), (nc, k)
            got = ops.spread_rows_topk_items(A.by_user, W, cand, k, A.by_user, True, eu, ei)
            assert same(got, reference(F, cand, k, A.by_user, True, eu, ei)), (nc, k)


def test_dense_users_rows_and_routes(small):
    """users= with duplicates and in reversed order: row j is row users[j] of the all-users
    call; both routes of the router give identical tensors; W= equals the rebuilt-W call."""
    from lgcnhs import ops
    s = small
    g = torch.Generator().manual_seed(7)
    eu = (torch.randn(s.U, 64, generator=g) * 0.1).to(DEV)
    ei = (torch.randn(s.I, 64, generator=g) * 0.1).to(DEV)
    users = [39, 5, 5, 0, 17, 4, 3, 2, 1, 0]
    ids = torch.as_tensor(users, device=DEV)
    for name in ("all", "every_second", "random10", "empty"):
        cand = s.cand(name)
        for kw in (dict(), dict(eu=eu, ei=ei)):
            for k in (20, 200):
                full = ops.spread_recommend(s.A, 0.5, k, s.ex, tiled=False, items=cand, W=s.W,
                                            **kw)
                part = ops.spread_recommend(s.A, 0.5, k, s.ex, tiled=False, items=cand, W=s.W,
                                            users=users, **kw)
                assert same(part, (full[0][ids], full[1][ids])), (name, k)
                rebuilt = ops.spread_recommend(s.A, 0.5, k, s.ex, tiled=False, items=cand, **kw)
                assert same(full, rebuilt), (name, k)
                e, i_ = kw.get("eu"), kw.get("ei")
                for sel in (None, ids):
                    a = ops._spread_topk_items(s.A, s.W, sel, cand, k, s.ex, True, e, i_,
                                               route="fused")
                    b = ops._spread_topk_items(s.A, s.W, sel, cand, k, s.ex, True, e, i_,
                                               route="gather")
                    assert same(a, b), (name, k)
                    assert same(a, full if sel is None else part), (name, k)
    # a mask and a list are the same candidates
    mask = torch.zeros(s.I, dtype=torch.bool)
    mask[s.sets["random10"]] = True
    a = ops.spread_recommend(s.A, 0.5, 20, s.ex, tiled=False, items=mask, W=s.W)
    b = ops.spread_recommend(s.A, 0.5, 20, s.ex, tiled=False, items=s.sets["random10"].tolist(),
                             W=s.W)
    assert same(a, b)
    # items=None with W= is today's call
    assert same(ops.spread_recommend(s.A, 0.5, 20, s.ex, tiled=False, W=s.W),
                ops.spread_recommend(s.A, 0.5, 20, s.ex, tiled=False))


def test_dense_ids_outside_the_catalog_never_rank(small):
    """Through the C ABI (ops.item_candidates refuses such lists): ids outside [0, n_items)
    never rank and the lists are those of the valid ids alone."""
    from lgcnhs import _native as N
    from lgcnhs import ops
    s, k = small, 20
    bad = torch.tensor([-5, 3, 10, 17, 300, 2**31 - 1], dtype=torch.int32, device=DEV)
    good = torch.tensor([3, 10, 17], dtype=torch.int32, device=DEV)
    val = torch.full((s.U + 1, k), 7.0, dtype=torch.float64, device=DEV)
    idx = torch.full((s.U + 1, k), 7, dtype=torch.int64, device=DEV)
    r = s.A.by_user
    N.check(N.lib().lg_spread_rows_topk_items_f64(
        N.ptr(r.rowptr), N.ptr(r.col), N.ptr(s.W), s.U, s.I, N.ptr(bad), bad.numel(),
        ctypes.c_void_p(0), ctypes.c_void_p(0), 0, ctypes.c_void_p(0), ctypes.c_void_p(0),
        N.LG_EXCL_DROP, k, N.ptr(val), N.ptr(idx), N.stream_handle(val.device)),
        "lg_spread_rows_topk_items_f64")
    want = ops.spread_rows_topk_items(r, s.W, good, k)
    assert same((val[:s.U], idx[:s.U]), want)
    assert bool((val[s.U] == 7.0).all()) and bool((idx[s.U] == 7).all())  # the row behind


# ---------------------------------------------------------------------------------- tiled
class Zipf:
    """200 users x 1,500 items, Zipf interactions (hub items: V rows), tile 256: six tiles
    for the whole catalog, two for the 30 % set (ragged last tile), one for the 2 % set. The
    seed is one for which the fp64 oracle's lists have no near-tie (1e-11 relative) at the
    cuts used below, with and without G."""
    U, I, E, lam, tile, d, seed = 200, 1500, 9000, 0.4, 256, 64, 8

    def __init__(self):
        from lgcnhs import ops
        from lgcnhs.synth import synth_interactions
        u, i = synth_interactions(self.U, self.I, self.E, seed=self.seed, dist="zipf")
        self.A = ops.Interactions.from_pairs(torch.as_tensor(u), torch.as_tensor(i), self.U,
                                             self.I, DEV)
        g = torch.Generator().manual_seed(100 + self.seed)
        self.eu = (torch.randn(self.U, self.d, generator=g) * 0.1).to(DEV)
        self.ei = (torch.randn(self.I, self.d, generator=g) * 0.1).to(DEV)
        rng = np.random.default_rng(self.seed)
        self.c30 = torch.as_tensor(np.sort(rng.choice(self.I, int(0.3 * self.I), replace=False))) \
            .to(DEV, torch.int32)
        self.c2 = torch.as_tensor(np.sort(rng.choice(self.I, int(0.02 * self.I), replace=False))) \
            .to(DEV, torch.int32)
        self.W = ops.spread_hybrid(self.A, self.lam)
        Ah = O.interaction_matrix(self.U, self.I, u, i)
        self.Fh = O.get_resource(Ah, O.hybrid_s(Ah, O.spreading_general_mat(Ah), self.lam))
        self.Gh = O.chain_scores(self.eu.cpu().numpy(), self.ei.cpu().numpy()).astype(np.float64)

    def kw(self, use_g):
        return dict(eu=self.eu, ei=self.ei) if use_g else {}


@pytest.fixture(scope="module")
def zipf():
    return Zipf()


@pytest.mark.parametrize("use_g", [False, True])
def test_tiled_every_item_and_slices_are_bitwise_todays(zipf, use_g):
    from lgcnhs import ops
    z, kw = zipf, zipf.kw(use_g)
    base = ops.spread_topk_tiled(z.A, z.lam, 20, z.A.by_user, tile=z.tile, **kw)
    every = ops.spread_topk_tiled(z.A, z.lam, 20, z.A.by_user, tile=z.tile,
                                  items=torch.arange(z.I, device=DEV, dtype=torch.int32), **kw)
    assert same(base, every)
    # an item range keeps its meaning and code (the multi-GPU shard): the lists of ranges cut
    # at tile boundaries -- the same tiles as the full walk's -- merge to the full lists
    a, b = z.tile, 4 * z.tile
    parts = [ops.spread_topk_tiled(z.A, z.lam, 20, z.A.by_user, tile=z.tile, items=sl, **kw)
             for sl in (slice(0, a), slice(a, b), slice(b, z.I))]
    mv, mi = ops.merge_topk_lists(torch.stack([p[0] for p in parts]),
                                  torch.stack([p[1] for p in parts]))
    assert same(base, (mv, mi))
    ids = parts[1][1][parts[1][1] >= 0]
    assert bool(((ids >= a) & (ids < b)).all())


@pytest.mark.parametrize("use_g", [False, True])
@pytest.mark.parametrize("share", ["c30", "c2"])
def test_tiled_candidates_close_to_dense(zipf, use_g, share):
    from lgcnhs import ops
    z, kw, k = zipf, zipf.kw(use_g), 20
    cand = getattr(z, share)
    cap = max(1, z.U // 100)
    dv, di = ops.spread_recommend(z.A, z.lam, k, z.A.by_user, tiled=False, items=cand, W=z.W,
                                  **kw)
    # the dense path alone against the fp64 oracle on this seed
    ov, oi = oracle_rows(z.Gh * z.Fh if use_g else z.Fh, cand, k, z.A.by_user)
    ties = compare_lists_close(dv.cpu().numpy(), di.cpu().numpy(), ov, oi, rtol=1e-12,
                               label=f"dense vs oracle {share} G={use_g}")
    assert ties <= cap
    tv, ti = ops.spread_recommend(z.A, z.lam, k, z.A.by_user, tiled=True, tile=z.tile,
                                  items=cand, **kw)
    ties = compare_lists_close(tv.cpu().numpy(), ti.cpu().numpy(), dv.cpu().numpy(),
                               di.cpu().numpy(), rtol=1e-12,
                               label=f"tiled vs dense {share} G={use_g}")
    assert ties <= cap
    ids = ti[ti >= 0]
    assert bool(torch.isin(ids, cand.to(torch.int64)).all())
    # users= on the column view: the rows of the all-users walk, bitwise
    users = [199, 3, 3, 0]
    pv, pi = ops.spread_recommend(z.A, z.lam, k, z.A.by_user, tiled=True, tile=z.tile,
                                  items=cand, users=users, **kw)
    sel = torch.as_tensor(users, device=DEV)
    assert same((pv, pi), (tv[sel], ti[sel]))


@pytest.mark.parametrize("use_g", [False, True])
def test_tiled_peel_in_id_space(zipf, use_g):
    """k = 200 on the 30 % set: the first 128 columns are bitwise the k = 128 call's, no id
    outside C, none twice; the whole list close to the dense one."""
    from lgcnhs import ops
    z, kw = zipf, zipf.kw(use_g)
    v128, i128 = ops.spread_topk_tiled(z.A, z.lam, 128, z.A.by_user, tile=z.tile, items=z.c30,
                                       **kw)
    v, i = ops.spread_topk_tiled(z.A, z.lam, 200, z.A.by_user, tile=z.tile, items=z.c30, **kw)
    assert same((v[:, :128], i[:, :128]), (v128, i128))
    assert bool(torch.isin(i[i >= 0], z.c30.to(torch.int64)).all())
    ih = i.cpu().numpy()
    for r in range(z.U):
        row = ih[r][ih[r] >= 0]
        assert len(set(row.tolist())) == len(row), r
    dv, di = ops.spread_recommend(z.A, z.lam, 200, z.A.by_user, tiled=False, items=z.c30,
                                  W=z.W, **kw)
    ties = compare_lists_close(v.cpu().numpy(), ih, dv.cpu().numpy(), di.cpu().numpy(),
                               rtol=1e-12, label=f"peel vs dense G={use_g}")
    assert ties <= max(1, z.U // 100)


def test_model_level_items_and_refusals(zipf):
    """spread_method_topk / spread_lightgcn_topk(items=mask) equal the ops call; W= with
    tiled=True raises; items with a shard raises."""
    import pandas as pd
    from lgcnhs import dist, ops
    from model.SpreadLightGCN.recommend import spread_lightgcn_topk
    from model.SpreadMethod.recommend import spread_method_topk
    import model.SpreadLightGCNOpti.recommend as opti
    z = zipf
    deg = z.A.by_user.degrees().cpu()
    df = pd.DataFrame({"user_id": torch.repeat_interleave(torch.arange(z.U), deg).numpy(),
                       "item_id": z.A.by_user.col.cpu().numpy().astype(np.int64)})
    tr, va = df.iloc[::2], df.iloc[1::2]
    mask = torch.zeros(z.I, dtype=torch.bool)
    mask[z.c30.cpu().to(torch.int64)] = True
    for tiled in (False, True):
        want = ops.spread_recommend(z.A, z.lam, 20, z.A.by_user, tiled=tiled, items=z.c30)
        got = spread_method_topk(z.U, z.I, tr, va, "HybridS", z.lam, "douban", 20, tiled=tiled,
                                 items=mask)
        assert same(got, want), tiled

        class M:  # the two embedding tables are all spread_lightgcn_topk reads
            users_emb = torch.nn.Embedding.from_pretrained(z.eu)
            items_emb = torch.nn.Embedding.from_pretrained(z.ei)
        want = ops.spread_recommend(z.A, z.lam, 20, z.A.by_user, eu=z.eu, ei=z.ei, tiled=tiled,
                                    items=z.c30)
        got = spread_lightgcn_topk(M, z.U, z.I, tr, va, z.lam, 20, tiled=tiled, items=mask)
        assert same(got, want), tiled
        assert opti.spread_lightgcn_topk is spread_lightgcn_topk
    with pytest.raises(ValueError, match="W="):
        ops.spread_recommend(z.A, z.lam, 20, z.A.by_user, tiled=True, W=z.W)
    with pytest.raises(ValueError, match="shard"):
        dist.sharded_spread_topk(z.A, z.lam, 20, z.A.by_user, items=z.c30)
    with pytest.raises(ValueError, match="candidate set"):
        ops.spread_recommend(z.A, z.lam, 20, z.A.by_user, tiled=False, items=slice(0, 5))
