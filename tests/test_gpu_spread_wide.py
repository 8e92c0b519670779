"""K4w: the spreading top-K for 128 < k <= 1024. lg_rows_topk_wide_f64 and
lg_topk_lists_merge_wide_f64 (lists in LDS) against the numpy oracle and their narrow twins,
bit for bit; ops.spread_topk_tiled's peeled passes against the oracle on the walk's own F;
the routing by k of ops.rows_topk / spread_topk / merge_topk_lists / spread_recommend /
spread_lambda_sweep."""
import numpy as np
import pytest
import torch

from _compare import compare_lists_close
import _ref_paths as RP
from oracle import lgcn_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _excl(n, m, count, seed):
    """`count` random (row, column) exclusions as (RowSets on the device, rowptr, col)."""
    from lgcnhs.graph import RowSets
    rng = np.random.default_rng(seed)
    r, c = rng.integers(0, n, count), rng.integers(0, m, count)
    rp, col = O.exclusion_csr(n, m, (r, c))
    return RowSets(torch.as_tensor(rp).to(DEV), torch.as_tensor(col).to(DEV), n, m), rp, col


def _same(got, want, label=""):
    """(values, indices) equal bit for bit; got on the device or host, want numpy."""
    gv, gi = (x.cpu().numpy() if isinstance(x, torch.Tensor) else x for x in got)
    wv, wi = (x.cpu().numpy() if isinstance(x, torch.Tensor) else x for x in want)
    assert gi.shape == wi.shape and gv.shape == wv.shape, label
    bad = np.nonzero((gi != wi).any(axis=1))[0]
    assert bad.size == 0, (label, "row", int(bad[0]), gi[bad[0]][:8], wi[bad[0]][:8])
    assert np.array_equal(np.ascontiguousarray(gv).view(np.uint64),
                          np.ascontiguousarray(wv).view(np.uint64)), label


def _direct(name, F, k, ex=None, drop=True, eu=None, ei=None):
    """One of the two rows entries called directly (no routing by k)."""
    from lgcnhs import _native as N
    n, m = F.shape
    val = torch.empty((n, k), dtype=torch.float64, device=F.device)
    idx = torch.empty((n, k), dtype=torch.int64, device=F.device)
    N.check(getattr(N.lib(), name)(
        N.ptr(F), F.stride(0), n, m, N.ptr(eu), N.ptr(ei), 0 if eu is None else eu.shape[1],
        N.ptr(ex.rowptr if ex else None), N.ptr(ex.col if ex else None),
        N.LG_EXCL_DROP if drop else N.LG_EXCL_NONE, k, N.ptr(val), N.ptr(idx),
        N.stream_handle(F.device)), name)
    return val, idx


def _merge_direct(name, vals, idxs):
    from lgcnhs import _native as N
    L, n, k = vals.shape
    ov = torch.empty((n, k), dtype=torch.float64, device=vals.device)
    oi = torch.empty((n, k), dtype=torch.int64, device=vals.device)
    N.check(getattr(N.lib(), name)(N.ptr(vals), N.ptr(idxs), L, n, k, N.ptr(ov), N.ptr(oi),
                                   N.stream_handle(vals.device)), name)
    return ov, oi


# ------------------------------------------------------------------ the shared matrices
@pytest.fixture(scope="module")
def small():
    """40 x 300 in eighths (many ties), 900 exclusions: one wave per row."""
    rng = np.random.default_rng(21)
    F = np.round(rng.random((40, 300)) * 8) / 8
    ex, rp, col = _excl(40, 300, 900, 22)
    return F, torch.as_tensor(F).to(DEV), ex, rp, col


@pytest.fixture(scope="module")
def wide():
    """12 x 5001 in quarters, row 3 constant, 3000 exclusions: several waves per row, ties
    across the waves' column ranges, a last step of one column."""
    rng = np.random.default_rng(23)
    F = np.round(rng.random((12, 5001)) * 4) / 4
    F[3] = 0.5
    ex, rp, col = _excl(12, 5001, 3000, 24)
    return F, torch.as_tensor(F).to(DEV), ex, rp, col


@pytest.fixture(scope="module")
def ramps():
    """3 x 20000: strictly ascending (every column a candidate: the most compactions),
    strictly descending, constant."""
    a = np.arange(20000, dtype=np.float64) / 16
    F = np.stack([a, a[::-1], np.full(20000, 2.5)])
    return F, torch.as_tensor(F).to(DEV)


# ------------------------------------------------------------------------ the rows kernel
def test_k129_and_range():
    """k = 129 (refused by lg_rows_topk_f64) returns the oracle's lists; k outside
    [1, 1024] is a ValueError before any native call."""
    from lgcnhs import ops
    rng = np.random.default_rng(1)
    F = rng.random((40, 300))
    Fd = torch.as_tensor(F).to(DEV)
    _same(ops.rows_topk(Fd, 129), O.rows_topk(F, 129))
    for k in (1025, 0):
        with pytest.raises(ValueError):
            ops.rows_topk(Fd, k)


@pytest.mark.parametrize("drop", [True, False])
@pytest.mark.parametrize("k", [129, 200, 256, 257, 300, 512, 513, 1024])
def test_small_rows_ties_and_padding(small, k, drop):
    from lgcnhs import ops
    F, Fd, ex, rp, col = small
    want = O.rows_topk(F, k, rp, col, drop)
    if k > 300 or (drop and k == 300):
        assert (want[1][:, -1] == -1).all()  # (k exceeds the survivors: padding)
    _same(ops.rows_topk(Fd, k, ex, drop), want, f"k={k} drop={drop}")


@pytest.mark.parametrize("k", [129, 256, 513, 1024])
def test_multi_wave_rows(wide, k):
    from lgcnhs import ops
    F, Fd, ex, rp, col = wide
    _same(ops.rows_topk(Fd, k, ex), O.rows_topk(F, k, rp, col), f"k={k}")


@pytest.mark.parametrize("k", [129, 1024])
def test_ramp_rows(ramps, k):
    from lgcnhs import ops
    F, Fd = ramps
    v, i = ops.rows_topk(Fd, k)
    _same((v, i), O.rows_topk(F, k), f"k={k}")
    assert torch.equal(i[2].cpu(), torch.arange(k))


@pytest.mark.parametrize("k", [129, 1024])
@pytest.mark.parametrize("d", [32, 64, 128])
def test_g_factor(wide, d, k):
    from lgcnhs import ops
    F, Fd, ex, rp, col = wide
    g = torch.Generator().manual_seed(d)
    eu = (torch.randn(12, d, generator=g) * 0.1).float()
    ei = (torch.randn(5001, d, generator=g) * 0.1).float()
    GF = O.chain_scores(eu.numpy(), ei.numpy()).astype(np.float64) * F
    got = ops.rows_topk(Fd, k, ex, True, eu.to(DEV), ei.to(DEV))
    _same(got, O.rows_topk(GF, k, rp, col), f"d={d} k={k}")


@pytest.mark.parametrize("k", [1, 64, 128])
def test_twin_agreement(small, wide, ramps, k):
    """At k <= 128 the wide entry returns lg_rows_topk_f64's lists bit for bit."""
    for name, fx in (("small", small), ("wide", wide), ("ramps", ramps)):
        Fd, ex = fx[1], (fx[2] if len(fx) > 2 else None)
        for drop in (True, False):
            _same(_direct("lg_rows_topk_wide_f64", Fd, k, ex, drop),
                  _direct("lg_rows_topk_f64", Fd, k, ex, drop), f"{name} k={k} drop={drop}")


# ---------------------------------------------------------------------------- dense blocks
def _inter(U, I, n, seed):
    from lgcnhs import ops
    from lgcnhs.synth import synth_interactions
    u, i = synth_interactions(U, I, n, seed=seed, dist="zipf")
    return ops.Interactions.from_pairs(torch.as_tensor(u), torch.as_tensor(i), U, I, DEV)


def _emb(U, I, d, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return (torch.randn(U, d, device=DEV, generator=g) * 0.1,
            torch.randn(I, d, device=DEV, generator=g) * 0.1)


@pytest.mark.parametrize("use_g", [False, True])
def test_spread_topk_dense_blocks(use_g):
    from lgcnhs import ops
    U, I, k = 60, 700, 300
    A = _inter(U, I, 2000, seed=31)
    W = ops.spread_hybrid(A, 0.4)
    F = ops.spread_resource(A, W).cpu().numpy()
    eu, ei = _emb(U, I, 64, 32) if use_g else (None, None)
    if use_g:
        F = O.chain_scores(eu.cpu().numpy(), ei.cpu().numpy()).astype(np.float64) * F
    rp, col = A.by_user.rowptr.cpu().numpy(), A.by_user.col.cpu().numpy()
    got = ops.spread_topk(A, W, k, A.by_user, True, eu, ei, block_users=7)
    _same(got, O.rows_topk(F, k, rp, col), f"G={use_g}")


# ------------------------------------------------------------------------- the peeled walk
PEEL_MODES = {"G_drop": (True, True), "drop": (False, True), "none": (False, False)}


@pytest.fixture(scope="module")
def walk():
    """U = 300, I = 700 Zipf graph, tile = 128, lambda = 0.6, and the walk's own F: the
    F-writing reference walk over the per-tile build, tile by tile (bitwise what the fused
    walk sums)."""
    from lgcnhs import ops
    U, I, tile, lam = 300, 700, 128, 0.6
    A = _inter(U, I, 9000, seed=41)
    tw = RP.PerTileWeights(A, lam, tile)
    F = torch.empty((U, I), dtype=torch.float64, device=DEV)
    Fb = torch.empty((U, tile), dtype=torch.float64, device=DEV)
    for j0 in range(0, I, tile):
        tw.build(j0)
        RP.resource(tw, 0, U, Fb)
        F[:, j0:j0 + tw.width] = Fb[:, :tw.width]
    eu, ei = _emb(U, I, 64, 42)
    G = O.chain_scores(eu.cpu().numpy(), ei.cpu().numpy()).astype(np.float64)
    F = F.cpu().numpy()
    rp, col = A.by_user.rowptr.cpu().numpy(), A.by_user.col.cpu().numpy()
    cache = {}

    def run(k, mode, **kw):
        """ops.spread_topk_tiled on these inputs (full runs cached by (k, mode))."""
        use_g, drop = PEEL_MODES[mode]
        key = (k, mode) if not kw else None
        if key not in cache:
            out = ops.spread_topk_tiled(A, lam, k, A.by_user, drop=drop, tile=tile,
                                        eu=eu if use_g else None, ei=ei if use_g else None,
                                        **kw)
            if key is None:
                return out
            cache[key] = out
        return cache[key]

    def oracle(k, mode):
        use_g, drop = PEEL_MODES[mode]
        return O.rows_topk(G * F if use_g else F, k, rp, col, drop)

    return dict(A=A, I=I, tile=tile, run=run, oracle=oracle)


@pytest.mark.parametrize("mode", list(PEEL_MODES))
@pytest.mark.parametrize("k", [129, 256, 300, 700])
def test_peeled_walk_exact(walk, k, mode):
    want = walk["oracle"](k, mode)
    if k == 700 and PEEL_MODES[mode][1]:
        assert (want[1][:, -1] == -1).all()  # (k exceeds the survivors: padding)
    _same(walk["run"](k, mode), want, f"k={k} {mode}")


@pytest.mark.parametrize("mode", list(PEEL_MODES))
def test_peel_prefix_is_the_k128_run(walk, mode):
    v, i = walk["run"](300, mode)
    v0, i0 = walk["run"](128, mode)
    _same((v[:, :128], i[:, :128]), (v0, i0), mode)


def test_peel_user_slice(walk):
    v, i = walk["run"](300, "G_drop")
    _same(walk["run"](300, "G_drop", users=slice(130, 131)), (v[130:131], i[130:131]))


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("mode", ["G_drop", "none"])
def test_peel_item_shards_merge_to_full(walk, mode, world):
    from lgcnhs import ops
    from lgcnhs.dist import item_range
    parts = [walk["run"](300, mode, items=slice(*item_range(walk["I"], walk["tile"], r, world)))
             for r in range(world)]
    got = ops.merge_topk_lists(torch.stack([p[0] for p in parts]),
                               torch.stack([p[1] for p in parts]))
    _same(got, walk["run"](300, mode), f"{mode} world={world}")


# ------------------------------------------------------------------------------- the merge
def _np_merge(vals, idxs, k):
    L, n, _ = vals.shape
    ov = np.full((n, k), -np.inf)
    oi = np.full((n, k), -1, np.int64)
    for r in range(n):
        v, i = vals[:, r].reshape(-1), idxs[:, r].reshape(-1)
        v, i = v[i >= 0], i[i >= 0]
        o = np.lexsort((i, -v))[:k]
        ov[r, :o.size], oi[r, :o.size] = v[o], i[o]
    return ov, oi


def _sorted_lists(L, n, k, seed):
    """Random sorted lists with ties, partially empty, fully empty and full rows."""
    rng = np.random.default_rng(seed)
    vals = np.full((L, n, k), -np.inf)
    idxs = np.full((L, n, k), -1, np.int64)
    for l in range(L):
        for r in range(n):
            m = int(rng.integers(0, k + 1)) if r % 5 else (0 if r % 2 else k)
            ids = rng.choice(np.arange(l * 2000, (l + 1) * 2000), size=m, replace=False)
            v = rng.integers(0, 6, size=m).astype(np.float64) * 0.25
            o = np.lexsort((ids, -v))
            vals[l, r, :m], idxs[l, r, :m] = v[o], ids[o]
    return vals, idxs


@pytest.mark.parametrize("k", [129, 1024])
@pytest.mark.parametrize("L", [2, 5])
def test_lists_merge_vs_numpy(k, L):
    from lgcnhs import ops
    vals, idxs = _sorted_lists(L, 21, k, seed=k + L)
    got = ops.merge_topk_lists(torch.as_tensor(vals).to(DEV), torch.as_tensor(idxs).to(DEV))
    _same(got, _np_merge(vals, idxs, k), f"k={k} L={L}")


@pytest.mark.parametrize("L", [2, 5])
def test_lists_merge_twin_agreement(L):
    vals, idxs = _sorted_lists(L, 21, 128, seed=L)
    v, i = torch.as_tensor(vals).to(DEV), torch.as_tensor(idxs).to(DEV)
    want = _merge_direct("lg_topk_lists_merge_f64", v, i)
    _same(_merge_direct("lg_topk_lists_merge_wide_f64", v, i), want)
    _same(want, _np_merge(vals, idxs, 128))


# ---------------------------------------------------------------------------- the dispatch
@pytest.fixture(scope="module")
def graph240():
    U, I = 240, 700
    return (_inter(U, I, 9000, seed=13),) + _emb(U, I, 64, 4)


def test_spread_recommend_tiled_vs_dense(graph240):
    from lgcnhs import ops
    A, eu, ei = graph240
    vt, it = ops.spread_recommend(A, 0.4, 150, A.by_user, True, eu, ei, tiled=True)
    vd, id_ = ops.spread_recommend(A, 0.4, 150, A.by_user, True, eu, ei, tiled=False)
    assert vt.shape == vd.shape == (240, 150)
    compare_lists_close(vt.cpu().numpy(), it.cpu().numpy(), vd.cpu().numpy(), id_.cpu().numpy(),
                        label="tiled vs dense k=150")


@pytest.mark.parametrize("tiled", [False, True])
def test_lambda_sweep_equals_recommend(graph240, tiled):
    from lgcnhs import ops
    A, eu, ei = graph240
    lams = [0.31, 0.85]
    got = list(ops.spread_lambda_sweep(A, lams, 150, A.by_user, True, eu, ei, tiled=tiled))
    assert [g[0] for g in got] == lams
    for lam, v, i in got:
        _same((v, i), ops.spread_recommend(A, lam, 150, A.by_user, True, eu, ei, tiled=tiled),
              f"lam={lam} tiled={tiled}")


def test_tiled_k_above_1024_is_refused(graph240):
    from lgcnhs import ops
    A = graph240[0]
    with pytest.raises(ValueError):
        ops.spread_topk_tiled(A, 0.5, 1025, A.by_user)
    with pytest.raises(ValueError):
        ops.merge_topk_lists(torch.zeros((2, 3, 1025), dtype=torch.float64, device=DEV),
                             torch.zeros((2, 3, 1025), dtype=torch.int64, device=DEV))
