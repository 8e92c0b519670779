"""K4k on the GPU: lg_rows_rank_f64 (csrc/rows_rank.hip) through ops.rows_rank, ops.spread_rank
and the reference-API mirrors. Every comparison is exact -- ranks as integers, values by their
int64 bit views -- against numpy on the definition: with V = F or chain score (fp32, promoted)
x F, a column ranks iff V > -inf and it is not dropped; rank = the ranking columns before the
target under (value desc, column asc), -1 for a target that does not rank."""
import numpy as np
import pytest
import torch

from oracle import lgcn_oracle as O
import _poison as P

pytestmark = pytest.mark.gpu
DEV = "cuda"
NEG = -np.inf


def _rowsets(rp, col, n_rows, n_cols):
    from lgcnhs.graph import RowSets
    return RowSets(torch.as_tensor(np.asarray(rp, np.int64)).to(DEV),
                   torch.as_tensor(np.asarray(col).astype(np.int32)).to(DEV), n_rows, n_cols)


def rank_ref(V, rows, rp=None, col=None, drop=True):
    """The definition, row by row: (rank int64 [nnz], value fp64 [nnz]) in the rows' own order.
    rows: one array of target ids per row of V (ids outside the columns: {-1, -inf})."""
    m = V.shape[1]
    ids = np.arange(m)
    rk, val = [], []
    with np.errstate(invalid="ignore"):
        for r, tg in enumerate(rows):
            v = V[r]
            ranks = v > NEG  # (False for NaN)
            if drop and rp is not None:
                ranks[col[rp[r]:rp[r + 1]]] = False
            tg = np.asarray(tg, np.int64)
            ok = (tg >= 0) & (tg < m)
            t = np.where(ok, tg, 0)
            tv = v[t]
            before = (v[None, :] > tv[:, None]) | ((v[None, :] == tv[:, None])
                                                   & (ids[None, :] < t[:, None]))
            before &= ranks[None, :]
            before[np.arange(len(t)), t] = False
            cnt = before.sum(1)
            rk.append(np.where(ok & ranks[t], cnt, -1))
            val.append(np.where(ok, tv, NEG))
    return (np.concatenate(rk).astype(np.int64) if rk else np.zeros(0, np.int64),
            np.concatenate(val).astype(np.float64) if val else np.zeros(0))


def assert_exact(out, want, what=""):
    rk, val = (x.cpu().numpy() for x in out)
    np.testing.assert_array_equal(rk, want[0], err_msg=str(what))
    assert rk.dtype == np.int64 and val.dtype == np.float64
    assert np.array_equal(val.view(np.int64), want[1].view(np.int64)), what


# ------------------------------------------------------------------------- 1, 2: the shapes
LENS = (0, 1, 2, 63, 64, 65, 257)
N_ROWS = 37
_CASES = {}


def _case(m, d):
    """37 rows x m columns (+ two rows of ROW_MAX and ROW_MAX + 1 targets when m = 4133): F
    about 60 % exact zeros, eighths elsewhere, a block of 80 columns at one positive value;
    with G negative products and -0.0. Targets per row cycle through LENS, descending ids,
    the last column and column 0 among them; 3 % exclusions plus every fourth target. Built and
    ranked once per (m, d); the device results are shared by the tests."""
    key = (m, d)
    if key in _CASES:
        return _CASES[key]
    from lgcnhs import ops
    M = ops.ROWS_RANK_ROW_MAX
    rng = np.random.default_rng(100 + m + d)
    lens = [LENS[r % len(LENS)] for r in range(N_ROWS)]
    if m > M + 1:
        lens += [M, M + 1]
    n = len(lens)
    F = np.round(rng.random((n, m)) * 8) / 8
    F[rng.random((n, m)) < 0.6] = 0.0
    F[:, 100:180] = 0.375
    rows = []
    for ln in lens:
        if ln >= 2:
            mid = rng.permutation(np.arange(1, m - 1))[:ln - 2]
            tg = np.sort(np.concatenate([mid, [0, m - 1]]))[::-1]
        else:
            tg = rng.permutation(m)[:ln]
        rows.append(np.ascontiguousarray(tg, dtype=np.int64))
    tu = np.concatenate([np.full(len(t[::4]), r) for r, t in enumerate(rows)]).astype(np.int64)
    ti = np.concatenate([t[::4] for t in rows]).astype(np.int64)
    n_ex = int(0.03 * n * m)
    rp, col = O.exclusion_csr(n, m, (rng.integers(0, n, n_ex), rng.integers(0, m, n_ex)),
                              (tu, ti))
    trp = np.zeros(n + 1, np.int64)
    trp[1:] = np.cumsum(lens)
    c = dict(n=n, m=m, d=d, F=F, rows=rows, rp=rp, col=col, Fd=torch.as_tensor(F).to(DEV),
             ex=_rowsets(rp, col, n, m), tg=_rowsets(trp, np.concatenate(rows), n, m), V=F,
             eu=None, ei=None)
    if d:
        eu = (rng.standard_normal((n, d)) * 0.1).astype(np.float32)
        ei = (rng.standard_normal((m, d)) * 0.1).astype(np.float32)
        c["V"] = O.chain_scores(eu, ei).astype(np.float64) * F
        c["eu"], c["ei"] = torch.as_tensor(eu).to(DEV), torch.as_tensor(ei).to(DEV)
        assert (c["V"] < 0).any() and np.signbit(c["V"][c["V"] == 0]).any()
    c["want"] = rank_ref(c["V"], rows, rp, col, drop=True)
    c["got"] = ops.rows_rank(c["Fd"], c["tg"], c["ex"], True, c["eu"], c["ei"])
    _CASES[key] = c
    return c


SHAPES = [(1005, 0), (1005, 32), (1005, 64), (1005, 128),
          (4133, 0), (4133, 32), (4133, 64), (4133, 128)]


@pytest.mark.parametrize("m,d", SHAPES)
def test_rows_rank_is_the_definition(m, d):
    """One wave per row with a 45-column tail step (1,005 columns) and eight waves per row with
    spans off the 64-column grid (4,133); no G and every embedding width; 0 .. 257 targets per
    row, and in the wide case ROW_MAX and ROW_MAX + 1 (two kernel rows)."""
    c = _case(m, d)
    assert_exact(c["got"], c["want"], (m, d))
    rk = c["got"][0].cpu().numpy()
    assert (rk == -1).sum() >= len(rk) // 4   # every fourth target is excluded
    assert (rk >= 0).sum() > len(rk) // 2


@pytest.mark.parametrize("m", [1005, 4133])
def test_rows_rank_keeps_exclusions_without_drop(m):
    from lgcnhs import ops
    c = _case(m, 0)
    want = rank_ref(c["V"], c["rows"], c["rp"], c["col"], drop=False)
    assert (want[0] >= 0).all()
    assert_exact(ops.rows_rank(c["Fd"], c["tg"], c["ex"], False), want, m)
    # ... which is the call without any exclusions
    assert_exact(ops.rows_rank(c["Fd"], c["tg"]), want, m)


@pytest.mark.parametrize("m,d", SHAPES)
def test_rows_rank_agrees_with_the_lists(m, d):
    """rows_topk(k = 1024) on the same inputs: a target with rank < 1024 sits at idx[r, rank]
    with a bit-equal value, every other target of the row is absent from it."""
    from lgcnhs import ops
    c = _case(m, d)
    v, i = ops.rows_topk(c["Fd"], 1024, c["ex"], True, c["eu"], c["ei"])
    v, i = v.cpu().numpy(), i.cpu().numpy()
    rk, val = (x.cpu().numpy() for x in c["got"])
    p, inside = 0, 0
    for r, tg in enumerate(c["rows"]):
        for t in tg:
            if 0 <= rk[p] < 1024:
                assert i[r, rk[p]] == t, (r, t, rk[p])
                assert v[r, rk[p]].view(np.int64) == val[p].view(np.int64), (r, t)
                inside += 1
            else:
                assert t not in i[r], (r, t, rk[p])
            p += 1
    assert p == len(rk) and inside > 0
    if m == 4133:
        assert (rk >= 1024).any()  # the lists say nothing about these


def test_rows_rank_request_sized_calls_skip_the_row_plan(monkeypatch):
    """At most ROW_MAX targets in all: the target rows are the kernel rows and ops.rank_rows is
    not run; one more and it is. One row each, of exactly ROW_MAX and ROW_MAX + 1 targets:
    the same ranks and values as in the call on all rows."""
    from lgcnhs import ops
    c = _case(4133, 0)
    M = ops.ROWS_RANK_ROW_MAX
    calls = []
    real = ops.rank_rows
    monkeypatch.setattr(ops, "rank_rows", lambda *a, **k: calls.append(1) or real(*a, **k))
    start = np.cumsum([0] + [len(t) for t in c["rows"]])
    for r, planned in ((N_ROWS, 0), (N_ROWS + 1, 1)):
        tg = c["rows"][r]
        assert len(tg) == M + planned
        del calls[:]
        got = ops.rows_rank(c["Fd"][r:r + 1], _rowsets([0, len(tg)], tg, 1, 4133),
                            c["ex"].slice_rows(r, r + 1), True)
        assert len(calls) == planned
        assert_exact(got, tuple(w[start[r]:start[r + 1]] for w in c["want"]), r)


# ------------------------------------------------------------------------------ 3: non-finite
def test_rows_rank_non_finite():
    """NaN and -inf targets get -1 and count for nobody; +inf targets rank by id among the +inf
    columns."""
    from lgcnhs import ops
    rng = np.random.default_rng(5)
    n, m = 3, 300
    F = np.round(rng.random((n, m)) * 4) / 4
    nan_c, ninf_c, pinf_c = [3, 90, 299], [0, 17, 150], [7, 50, 200]
    F[1, nan_c], F[1, ninf_c], F[1, pinf_c] = np.nan, NEG, np.inf
    F[2, :] = np.nan
    F[2, 10] = 1.0
    rows = [np.array([5, 1]), np.array(nan_c + ninf_c + pinf_c[::-1] + [100, 101, 8]),
            np.array([10, 11])]
    trp = np.cumsum([0] + [len(r) for r in rows])
    want = rank_ref(F, rows)
    got = ops.rows_rank(torch.as_tensor(F).to(DEV), _rowsets(trp, np.concatenate(rows), n, m))
    assert_exact(got, want)
    rk = got[0].cpu().numpy()
    r1 = rk[2:2 + len(rows[1])]
    assert (r1[:6] == -1).all()                   # NaN and -inf targets
    assert r1[6:9].tolist() == [2, 1, 0]          # +inf: 200, 50, 7 by id
    # the finite targets of row 1: above them only ranking columns (not the 3 NaN, 3 -inf)
    with np.errstate(invalid="ignore"):
        assert r1[9] == 3 + int(((F[1] > F[1, 100]) & np.isfinite(F[1])).sum()
                                + ((F[1] == F[1, 100]) & (np.arange(m) < 100)).sum())
    assert rk[-2:].tolist() == [0, -1]            # a row of NaN but one column


# ------------------------------------------------------------------- 4: duplicates and strays
def test_rows_rank_duplicates_and_strays():
    from lgcnhs import _native as N
    from lgcnhs import ops
    rng = np.random.default_rng(6)
    n, m = 4, 700
    F = np.round(rng.random((n, m)) * 16) / 16
    Fd = torch.as_tensor(F).to(DEV)
    # the same target twice (and a third time at the end of the row)
    rows = [np.array([9, 650, 9, 3, 9]), np.array([], np.int64), np.array([699, 699]),
            np.array([0])]
    trp = np.cumsum([0] + [len(r) for r in rows])
    got = ops.rows_rank(Fd, _rowsets(trp, np.concatenate(rows), n, m))
    assert_exact(got, rank_ref(F, rows))
    rk = got[0].cpu().numpy()
    assert rk[0] == rk[2] == rk[4] >= 0 and rk[5] == rk[6] >= 0
    # entries of col outside every row (before the first row, between none, behind the last)
    col = np.concatenate([[11, 12], np.concatenate(rows), [13, 14, 15]])
    rk2, v2 = ops.rows_rank(Fd, _rowsets(trp + 2, col, n, m))
    assert_exact((rk2[2:-3], v2[2:-3]), rank_ref(F, rows))
    for s in (slice(0, 2), slice(-3, None)):
        assert (rk2[s] == -1).all() and (v2[s] == NEG).all()
    # ids outside [0, n_cols) reach only the C entry (candidate_rows validates host inputs):
    # {-1, -inf} over whatever the outputs held
    tcol = torch.tensor([5, m, -1, m + 5, 6], dtype=torch.int32, device=DEV)
    krp = torch.tensor([0, 5], dtype=torch.int64, device=DEV)
    krow = torch.tensor([2], dtype=torch.int64, device=DEV)
    rk3 = torch.full((5,), -7, dtype=torch.int64, device=DEV)
    v3 = torch.full((5,), 123.0, dtype=torch.float64, device=DEV)
    N.check(N.lib().lg_rows_rank_f64(
        N.ptr(Fd), Fd.stride(0), n, m, None, None, 0, None, None, N.LG_EXCL_DROP, 1,
        N.ptr(krow), N.ptr(krp), N.ptr(tcol), N.ptr(rk3), N.ptr(v3), N.stream_handle(Fd.device)),
        "lg_rows_rank_f64")
    w = rank_ref(F[2:3], [np.array([5, 6])])
    assert rk3.tolist() == [w[0][0], -1, -1, -1, w[0][1]]
    assert v3.tolist() == [w[1][0], NEG, NEG, NEG, w[1][1]]
    # ... and a kernel row that names an F row outside the matrix: {-1, -inf} throughout
    krow[0] = n
    N.check(N.lib().lg_rows_rank_f64(
        N.ptr(Fd), Fd.stride(0), n, m, None, None, 0, None, None, N.LG_EXCL_DROP, 1,
        N.ptr(krow), N.ptr(krp), N.ptr(tcol), N.ptr(rk3), N.ptr(v3), N.stream_handle(Fd.device)),
        "lg_rows_rank_f64")
    assert rk3.tolist() == [-1] * 5 and v3.tolist() == [NEG] * 5


# ------------------------------------------------------------------ 5: spread_rank end to end
SU, SI, SD = 70, 300, 64
_SPREAD = {}


def _spread():
    """A 70-user x 300-item random graph, held-out targets disjoint from it (0 .. 6 per user,
    descending ids), W for lambda = 0.4 and 0.9, F read back, embeddings and a decoy pair."""
    if not _SPREAD:
        from lgcnhs import ops
        rng = np.random.default_rng(17)
        An = rng.random((SU, SI)) < 0.08
        u, i = np.nonzero(An)
        A = ops.Interactions.from_pairs(torch.as_tensor(u), torch.as_tensor(i), SU, SI, DEV)
        rows = []
        for r in range(SU):
            free = np.nonzero(~An[r])[0]
            rows.append(np.sort(rng.permutation(free)[:r % 7])[::-1].astype(np.int64))
        trp = np.cumsum([0] + [len(t) for t in rows])
        W = ops.spread_hybrid(A, 0.4)
        Fn = ops.spread_resource(A, W).cpu().numpy()
        eu = (rng.standard_normal((SU, SD)) * 0.1).astype(np.float32)
        ei = (rng.standard_normal((SI, SD)) * 0.1).astype(np.float32)
        du = (rng.standard_normal((SU, SD)) * 0.3).astype(np.float32)
        di = (rng.standard_normal((SI, SD)) * 0.3).astype(np.float32)
        rp, col = A.by_user.rowptr.cpu().numpy(), A.by_user.col.cpu().numpy()
        G = O.chain_scores(eu, ei).astype(np.float64)
        _SPREAD.update(
            A=A, W=W, W2=ops.spread_hybrid(A, 0.9), rows=rows, trp=trp, rp=rp, col=col,
            tg=_rowsets(trp, np.concatenate(rows), SU, SI), Fn=Fn, GFn=G * Fn,
            real=(torch.as_tensor(eu).to(DEV), torch.as_tensor(ei).to(DEV)),
            decoy=(torch.as_tensor(du).to(DEV), torch.as_tensor(di).to(DEV)),
            want={False: rank_ref(Fn, rows, rp, col), True: rank_ref(G * Fn, rows, rp, col)})
    return _SPREAD


def _spread_rank(s, use_g, **kw):
    from lgcnhs import ops
    eu, ei = s["real"] if use_g else (None, None)
    return ops.spread_rank(s["A"], 0.4, kw.pop("targets", s["tg"]), s["A"].by_user, True, eu,
                           ei, **kw)


@pytest.mark.parametrize("use_g", [False, True])
def test_spread_rank_end_to_end(use_g, monkeypatch):
    from lgcnhs import ops
    s = _spread()
    want = s["want"][use_g]
    base = _spread_rank(s, use_g)
    assert_exact(base, want, use_g)
    assert (want[0] >= 0).all()  # held-out items are not excluded: all of them rank
    # users=: the listed users' rows, duplicates and any order
    ids = [5, 5, 69, 0]
    sub = s["tg"].take(torch.tensor(ids))
    got = _spread_rank(s, use_g, targets=sub, users=ids)
    sel = np.concatenate([np.arange(s["trp"][u], s["trp"][u + 1]) for u in ids]).astype(np.int64)
    assert_exact(got, (want[0][sel], want[1][sel]), ("users", use_g))
    # W= prebuilt equals the rebuilt one (lam is then not read)
    eu, ei = s["real"] if use_g else (None, None)
    assert P.bit_equal(ops.spread_rank(s["A"], 123.0, s["tg"], s["A"].by_user, True, eu, ei,
                                       W=s["W"]), base)
    # three blocks of users through one F buffer (24, 24, 22)
    calls = []
    real_rows_rank = ops.rows_rank
    monkeypatch.setattr(ops, "rows_rank",
                        lambda F, *a, **k: calls.append(F.shape[0]) or real_rows_rank(F, *a, **k))
    assert P.bit_equal(_spread_rank(s, use_g, block_users=24), base)
    assert calls == [24, 24, 22]


def test_spread_rank_has_no_tiled_path():
    s = _spread()
    with pytest.raises(ValueError, match="bounded lists.*no rank"):
        _spread_rank(s, False, tiled=True)


# --------------------------------------------------------------------------------- 6: mirrors
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


@pytest.mark.parametrize("tag", ["hybrid", "probs_ml", "heats_db"])
def test_spread_method_ranks_agree_with_the_topk_twin(golden, tag):
    import pandas as pd
    from model.SpreadMethod.recommend import spread_method_ranks, spread_method_topk
    g = golden("spread_ml100k")
    U, I = int(g["n_users"]), int(g["n_items"])
    method, dataset = {"hybrid": ("HybridS", "movielens"), "probs_ml": ("ProbS", "movielens"),
                       "heats_db": ("HeatS", "douban")}[tag]
    unfiltered = tag == "probs_ml"  # (the reference's unfiltered branch: nothing dropped)
    tr, held = _hold_out_last(g["train"])
    va = pd.DataFrame({"user_id": g["val"][0].astype(np.int64),
                       "item_id": g["val"][1].astype(np.int64)})
    lam = float(g[f"{tag}_lambda"])
    targets, rank = spread_method_ranks(U, I, tr, va, held, method, lam, dataset,
                                        unfiltered=unfiltered)
    _, idx = spread_method_topk(U, I, tr, va, method, lam, dataset, 20, unfiltered=unfiltered,
                                tiled=False)
    assert targets.n_rows == U and int(targets.col.numel()) == len(held)
    inside = _ranks_agree_with_lists(targets, rank, idx, 20)
    if unfiltered:
        # nothing is dropped: the train items fill the first 20 places and no held-out item is
        # among them; the lists of 1,024 reach some
        _, idx = spread_method_topk(U, I, tr, va, method, lam, dataset, 1024, unfiltered=True,
                                    tiled=False)
        inside = _ranks_agree_with_lists(targets, rank, idx, 1024)
    assert inside > 0
    # users=: those rows of the same answer
    ids = [7, 7, 900, 0]
    t2, r2 = spread_method_ranks(U, I, tr, va, held, method, lam, dataset,
                                 unfiltered=unfiltered, users=ids)
    rp = targets.rowptr.cpu().numpy()
    sel = np.concatenate([np.arange(rp[u], rp[u + 1]) for u in ids]).astype(np.int64)
    np.testing.assert_array_equal(r2.cpu().numpy(), rank.cpu().numpy()[sel])
    np.testing.assert_array_equal(t2.col.cpu().numpy(), targets.col.cpu().numpy()[sel])


def test_spread_lightgcn_ranks_agree_with_the_topk_twin(golden):
    import pandas as pd
    from model.LightGCN.model import LightGCN
    from model.SpreadLightGCN.recommend import spread_lightgcn_ranks, spread_lightgcn_topk
    from model.SpreadLightGCNOpti import recommend as opti
    assert opti.spread_lightgcn_ranks is spread_lightgcn_ranks
    g = golden("lightgcn_mid")
    U, I = int(g["n_users"]), int(g["n_items"])
    torch.manual_seed(42)
    m = LightGCN(U, I, 64, 3).to(DEV)
    tr, held = _hold_out_last(g["train"])
    va = pd.DataFrame({"user_id": g["val"][0].astype(np.int64),
                       "item_id": g["val"][1].astype(np.int64)})
    lam = float(g["slgcn_lambda"])
    targets, rank = spread_lightgcn_ranks(m, U, I, tr, va, held, lam)
    _, idx = spread_lightgcn_topk(m, U, I, tr, va, lam, 20, tiled=False)
    assert _ranks_agree_with_lists(targets, rank, idx, 20) > 0


# ------------------------------------------------------- 7: uninitialised memory, call context
@pytest.mark.parametrize("use_g", [False, True])
def test_rows_rank_does_not_depend_on_what_memory_held(use_g):
    """lg_spread_resource_f64's F buffer and lg_rows_rank_f64 on it (rows_rank itself allocates
    nothing uninitialised: its outputs start from {-1, -inf}): plain, over a decoy's buffers,
    over 0xFF bytes."""
    from lgcnhs import ops
    s = _spread()

    def run(W, tabs):
        eu, ei = tabs if use_g else (None, None)
        return ops.rows_rank(ops.spread_resource(s["A"], W), s["tg"], s["A"].by_user, True,
                             eu, ei)

    P.three_ways(lambda: run(s["W"], s["real"]), lambda: run(s["W2"], s["decoy"]),
                 lambda out, how: assert_exact(out, s["want"][use_g], how))


@pytest.mark.parametrize("use_g", [False, True])
def test_spread_rank_does_not_depend_on_what_memory_held(use_g):
    """spread_rank with three user blocks through one F buffer, W rebuilt inside."""
    from lgcnhs import ops
    s = _spread()

    def run(lam, tabs):
        eu, ei = tabs if use_g else (None, None)
        return ops.spread_rank(s["A"], lam, s["tg"], s["A"].by_user, True, eu, ei,
                               block_users=24)

    P.three_ways(lambda: run(0.4, s["real"]), lambda: run(0.9, s["decoy"]),
                 lambda out, how: assert_exact(out, s["want"][use_g], how))


def test_rows_rank_views_and_streams():
    """An odd-element-offset view of F, a row-strided slice of a wider buffer, a slice_rows view
    of the targets and a side stream: all bit-equal to the call on fresh copies."""
    from lgcnhs import ops
    s = _spread()
    F = torch.as_tensor(s["Fn"]).to(DEV)
    eu, ei = s["real"]
    ex = s["A"].by_user
    for tabs in ((None, None), (eu, ei)):
        base = ops.rows_rank(F, s["tg"], ex, True, *tabs)
        assert_exact(base, s["want"][tabs[0] is not None])
        # F at an odd element offset of another tensor (8 mod 16 bytes)
        flat = torch.zeros(SU * SI + 1, dtype=torch.float64, device=DEV)
        flat[1:] = F.reshape(-1)
        odd = flat[1:].view(SU, SI)
        assert odd.data_ptr() % 16 == 8
        assert P.bit_equal(ops.rows_rank(odd, s["tg"], ex, True, *tabs), base)
        # the first SI columns of a wider buffer (row stride SI + 3: odd rows at 8 mod 16)
        wide = torch.full((SU, SI + 3), float("nan"), dtype=torch.float64, device=DEV)
        wide[:, :SI] = F
        assert P.bit_equal(ops.rows_rank(wide[:, :SI], s["tg"], ex, True, *tabs), base)
        # embeddings at an odd offset
        if tabs[0] is not None:
            fe = torch.zeros(SU * SD + 1, dtype=torch.float32, device=DEV)
            fe[1:] = eu.reshape(-1)
            assert P.bit_equal(ops.rows_rank(F, s["tg"], ex, True, fe[1:].view(SU, SD), ei),
                               base)
        # rows [20, 50) of everything: targets and exclusions keep their absolute offsets
        a, b = 20, 50
        part = ops.rows_rank(F[a:b], s["tg"].slice_rows(a, b), ex.slice_rows(a, b), True,
                             None if tabs[0] is None else eu[a:b], tabs[1])
        lo, hi = int(s["trp"][a]), int(s["trp"][b])
        assert P.bit_equal((part[0][lo:hi], part[1][lo:hi]), (base[0][lo:hi], base[1][lo:hi]))
        assert bool((part[0][:lo] == -1).all()) and bool((part[0][hi:] == -1).all())
        assert bool((part[1][:lo] == NEG).all()) and bool((part[1][hi:] == NEG).all())
        # a side stream
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            got = ops.rows_rank(F, s["tg"], ex, True, *tabs)
        side.synchronize()
        assert P.bit_equal(got, base)
