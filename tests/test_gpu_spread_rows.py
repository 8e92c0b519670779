"""K3r on the GPU: spreading for item baskets that are not rows of A (csrc/spread_rows.hip;
ops.spread_rows_resource / spread_rows_recommend / spread_rows_rank / spread_related_items).

Values against the numpy oracle B @ HybridS(A, general_W, lam) and against the dense path
rows @ spread_hybrid(A, lam), within 1e-12 relative with the same zeros (the project's
dense-versus-factored tolerance, _compare.compare_lists_close); lists against the dense path
through W=; and the bitwise properties the order rule gives: a row does not depend on the other
baskets of the call, their number or order, on what the buffers held, on the stream or on how
eu lies in memory.

G1 is 2 SEG + 70 users x 300 items with item lists of 0 / 1 / 63 / 64 / 65 / SEG-1 / SEG /
SEG+1 / 2 SEG+1 users (every step count of a wave and every segment count of pass 2). No user
of a 300-item graph has more than SEG items, so pass 1's long lists run on a second, wide graph
(40 users x 2 SEG + 5 items), and a Zipf(1.1) graph closes; both against the oracle's
spread_rows_spmv regrouping restated for foreign rows (the dense I x I oracle of the wide
graph would be 0.5 GB)."""
import numpy as np
import pytest
import torch

import _poison as P
from _compare import compare_lists_close
from oracle import lgcn_oracle as O

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
I1 = 300
LAMS = (0.0, 0.5, 1.0)
RTOL = 1e-12


def _consts():
    from lgcnhs import _native as N
    return N.LG_SPREAD_ROWS_SEG, N.LG_SPREAD_ROWS_BLOCK


# --------------------------------------------------------------------------------- graph G1
def _g1_pairs():
    SEG, _ = _consts()
    U = 2 * SEG + 70
    rng = np.random.default_rng(20240611)
    FIRST = 7                                  # users 0..6 have prescribed degrees
    col_len = {0: 0, 1: 1, 2: 63, 3: 64, 4: 65, 5: SEG - 1, 6: SEG, 7: SEG + 1, 8: 2 * SEG + 1}
    us, its = [1], [1]                         # user 1: degree 1, item 1's only user
    for j, n in col_len.items():
        if j < 2:
            continue
        v = rng.choice(np.arange(FIRST, U), size=n, replace=False)
        us.append(v), its.append(np.full(n, j))
    us = [np.atleast_1d(np.asarray(x, np.int64)) for x in us]
    its = [np.atleast_1d(np.asarray(x, np.int64)) for x in its]
    hub_deg = np.bincount(np.concatenate(us), minlength=U)
    # the special users: degrees 0 (user 0), 1 (above), 3, 4, 5, 9 and about 200; user 2's
    # items 290..292 are in no random basket
    for v, pick in ((2, np.arange(290, 293)), (3, rng.choice(np.arange(9, 290), 4, False)),
                    (4, rng.choice(np.arange(9, 290), 5, False)),
                    (5, rng.choice(np.arange(9, 290), 9, False)),
                    (6, rng.choice(np.arange(9, 300), 200, False))):
        us.append(np.full(pick.size, v)), its.append(pick)
    # the rest: 2..20 items, the hub columns included
    want = rng.integers(2, 21, size=U)
    for v in range(FIRST, U):
        more = int(want[v]) - int(hub_deg[v])
        if more > 0:
            pick = rng.choice(np.arange(9, 300), more, False)
            us.append(np.full(more, v)), its.append(pick)
    u, i = np.concatenate(us), np.concatenate(its)
    keys = np.unique(u * I1 + i)
    return U, keys // I1, keys % I1


@pytest.fixture(scope="module")
def g1():
    from lgcnhs import ops
    SEG, _ = _consts()
    U, u, i = _g1_pairs()
    Ad = O.interaction_matrix(U, I1, u, i)
    ku, ki = Ad.sum(1), Ad.sum(0)
    assert [int(ki[j]) for j in range(9)] == [0, 1, 63, 64, 65, SEG - 1, SEG, SEG + 1,
                                              2 * SEG + 1]
    assert [int(ku[v]) for v in range(7)] == [0, 1, 3, 4, 5, 9, 200]
    assert ku[7:].min() >= 2 and ku[7:].max() <= 20
    A = ops.Interactions.from_pairs(torch.as_tensor(u), torch.as_tensor(i), U, I1, DEV)
    gW = O.spreading_general_mat(Ad)
    Wo = {lam: O.hybrid_s(Ad, gW, lam) for lam in LAMS}
    W = {lam: ops.spread_hybrid(A, lam) for lam in LAMS}
    return dict(U=U, Ad=Ad, A=A, Wo=Wo, W=W)


def _baskets(g1):
    """2 BLOCK + 3 baskets: the named ones, then random ones of 1..60 items (of items < 290)."""
    _, BLOCK = _consts()
    rng = np.random.default_rng(7)
    row6 = np.nonzero(g1["Ad"][6])[0].tolist()
    bs = [[], [17], [0], [8], list(range(I1)), row6, list(row6)]
    while len(bs) < 2 * BLOCK + 3:
        bs.append(sorted(rng.choice(290, int(rng.integers(1, 61)), False).tolist()))
    return bs


@pytest.fixture(scope="module")
def baskets(g1):
    return _baskets(g1)


def _dense01(bs, n_items):
    B = np.zeros((len(bs), n_items))
    for r, b in enumerate(bs):
        B[r, b] = 1
    return B


def _close(F, ref, label):
    """Within RTOL relative, and exactly zero where the reference is."""
    F = F.cpu().numpy() if isinstance(F, torch.Tensor) else F
    ref = ref.cpu().numpy() if isinstance(ref, torch.Tensor) else ref
    assert F.shape == ref.shape, label
    assert np.array_equal(F == 0, ref == 0), f"{label}: zero patterns differ"
    nz = ref != 0
    err = float(np.max(np.abs(F[nz] - ref[nz]) / np.abs(ref[nz]))) if nz.any() else 0.0
    print(f"[{label}] max rel err {err:.2e}")
    assert err <= RTOL, f"{label}: rel err {err:.2e} > {RTOL}"


@pytest.fixture(scope="module")
def f_all(g1, baskets):
    """spread_rows_resource of all baskets per lambda: computed once, shared, never written."""
    from lgcnhs import ops
    return {lam: ops.spread_rows_resource(g1["A"], baskets, lam) for lam in LAMS}


# -------------------------------------------------------------------------------------- values
@pytest.mark.parametrize("lam", LAMS)
def test_resource_against_the_oracle_and_the_dense_path(g1, baskets, f_all, lam):
    from lgcnhs import ops
    F = f_all[lam]
    assert F.shape == (len(baskets), I1) and F.dtype == torch.float64
    Bd = _dense01(baskets, I1)
    _close(F, Bd @ g1["Wo"][lam], f"oracle lam={lam}")
    rows = ops.candidate_rows(baskets, len(baskets), I1, DEV)
    Fd = ops.spread_resource(ops.Interactions(rows), g1["W"][lam])   # rows @ W, the dense path
    _close(F, Fd, f"dense lam={lam}")
    assert not F[0].any() and not F[2].any()      # the empty basket, the degree-0 item alone
    assert bool((F[3] > 0).sum() > 200)           # the longest column reaches most items


# ------------------------------------------------------------------------- bitwise properties
@pytest.mark.parametrize("lam", LAMS)
def test_rows_do_not_depend_on_the_batch(g1, baskets, f_all, lam):
    from lgcnhs import ops
    _, BLOCK = _consts()
    A, F = g1["A"], f_all[lam]
    n = len(baskets)
    assert n == 2 * BLOCK + 3
    assert P.bit_equal(ops.spread_rows_resource(A, baskets, lam), F), "a repeated call"
    for m in (BLOCK - 1, BLOCK, BLOCK + 1):
        assert P.bit_equal(ops.spread_rows_resource(A, baskets[:m], lam), F[:m]), m
    for b in (0, 1, 2, 3, 4, 5, BLOCK - 1, BLOCK, 2 * BLOCK + 2):
        one = ops.spread_rows_resource(A, [baskets[b]], lam)
        assert P.bit_equal(one, F[b:b + 1]), f"basket {b} alone"
    perm = np.random.default_rng(3).permutation(n)
    Fp = ops.spread_rows_resource(A, [baskets[p] for p in perm], lam)
    assert P.bit_equal(Fp, F[torch.as_tensor(perm, device=DEV)]), "a permutation of the baskets"
    assert P.bit_equal(F[5], F[6]), "two identical baskets"
    # an existing user's row: the same bits named by take or spelled out
    taken = A.by_user.take(torch.tensor([6, 6, 5]))
    Ft = ops.spread_rows_resource(A, taken, lam)
    assert P.bit_equal(Ft[0], F[5]) and P.bit_equal(Ft[1], F[5])
    row5 = np.nonzero(g1["Ad"][5])[0].tolist()
    assert P.bit_equal(Ft[2:3], ops.spread_rows_resource(A, [row5], lam))


def test_items_named_twice_count_once(g1, f_all):
    from lgcnhs import ops
    from lgcnhs.graph import RowSets
    A = g1["A"]
    twice = ops.spread_rows_resource(A, [[17, 17, 17], [8, 17, 8]], 0.5)
    once = ops.spread_rows_resource(A, [[17], [8, 17]], 0.5)
    assert P.bit_equal(twice, once) and P.bit_equal(once[0], f_all[0.5][1])
    # a RowSets is taken as it is: the kernel still counts a repeated id once
    raw = RowSets(torch.tensor([0, 3], device=DEV), torch.tensor([17, 17, 17], dtype=torch.int32,
                                                                device=DEV), 1, I1)
    assert P.bit_equal(ops.spread_rows_resource(A, raw, 0.5), once[:1])


def test_out_may_be_a_row_strided_view(g1, baskets, f_all):
    from lgcnhs import ops
    n = 70
    big = torch.full((n + 3, I1 + 5), 7.25, dtype=torch.float64, device=DEV)
    out = big[1:]
    got = ops.spread_rows_resource(g1["A"], baskets[:n], 0.5, out=out)
    assert got.data_ptr() == out.data_ptr()
    assert P.bit_equal(out[:n, :I1], f_all[0.5][:n])
    keep = torch.ones_like(big, dtype=torch.bool)
    keep[1:n + 1, :I1] = False
    assert bool((big[keep] == 7.25).all()), "written outside rows [0, n) x columns [0, I)"


# --------------------------------------------------------------------------------------- lists
@pytest.mark.parametrize("k", [1, 20, 128, 129, 1024])
def test_recommend_against_the_dense_path(g1, baskets, k):
    from lgcnhs import ops
    A, lam = g1["A"], 0.5
    v, i = ops.spread_rows_recommend(A, baskets, lam, k)
    dv, di = ops.spread_rows_recommend(A, baskets, lam, k, W=g1["W"][lam])
    assert v.shape == (len(baskets), k) and i.dtype == torch.int64
    compare_lists_close(v.cpu(), i.cpu(), dv.cpu(), di.cpu(), RTOL, f"rows vs W= k={k}")
    i = i.cpu().numpy()
    for r, b in enumerate(baskets):   # excl=None drops exactly the basket
        got = i[r][i[r] >= 0]
        assert not set(got.tolist()) & set(b), r
        assert got.size == min(k, I1 - len(b)), r
    # an all-zero F row: the lowest undropped ids (basket 2 = the degree-0 item 0)
    assert i[2].tolist()[:min(k, I1 - 1)] == list(range(1, 1 + min(k, I1 - 1)))
    assert i[0].tolist()[:min(k, I1)] == list(range(min(k, I1)))
    assert (i[4] == -1).all() and bool(torch.isinf(v[4]).all())   # every item dropped


def test_recommend_keeps_the_basket_without_drop(g1, baskets):
    from lgcnhs import ops
    A, lam, k = g1["A"], 0.5, 1024
    v, i = ops.spread_rows_recommend(A, baskets, lam, k, drop=False)
    dv, di = ops.spread_rows_recommend(A, baskets, lam, k, drop=False, W=g1["W"][lam])
    compare_lists_close(v.cpu(), i.cpu(), dv.cpu(), di.cpu(), RTOL, "drop=False")
    assert bool(((i >= 0).sum(1) == I1).all())
    # an exclusion of the caller's: one row per basket, instead of the basket itself
    ex = ops.candidate_rows([[1, 2, 3]] * len(baskets), len(baskets), I1, DEV)
    _, ie = ops.spread_rows_recommend(A, baskets, lam, k, excl=ex)
    assert bool(((ie >= 0).sum(1) == I1 - 3).all())
    assert not bool(((ie >= 1) & (ie <= 3)).any())


@pytest.fixture(scope="module")
def emb(baskets):
    g = torch.Generator().manual_seed(11)
    eu = torch.randn(len(baskets), 64, generator=g).to(DEV)
    ei = torch.randn(I1, 64, generator=g).to(DEV)
    return eu, ei


@pytest.mark.parametrize("k", [20, 129])
def test_recommend_with_a_G_factor(g1, baskets, f_all, emb, k):
    from lgcnhs import ops
    A, lam = g1["A"], 0.5
    eu, ei = emb
    rows = ops.candidate_rows(baskets, len(baskets), I1, DEV)
    v, i = ops.spread_rows_recommend(A, baskets, lam, k, eu=eu, ei=ei)
    Fd = ops.spread_resource(ops.Interactions(rows), g1["W"][lam])
    dv, di = ops.rows_topk(Fd, k, rows, True, eu, ei)
    compare_lists_close(v.cpu(), i.cpu(), dv.cpu(), di.cpu(), RTOL, f"G k={k}")
    # ... and bitwise rows_topk of this path's own F
    assert P.bit_equal((v, i), ops.rows_topk(f_all[lam], k, rows, True, eu, ei))
    wv, wi = ops.spread_rows_recommend(A, baskets, lam, k, eu=eu, ei=ei, W=g1["W"][lam])
    assert P.bit_equal((wv, wi), (dv, di))


def _items_reference(F, cand, k, ex, drop=True, eu=None, ei=None):
    """The contract of tests/test_gpu_spread_items.py::reference: rows_topk on the gathered
    columns, exclusions renumbered, real item ids."""
    from lgcnhs import ops
    n = F.shape[0]
    if cand.numel() == 0:
        return (torch.full((n, k), float("-inf"), dtype=torch.float64, device=DEV),
                torch.full((n, k), -1, dtype=torch.int64, device=DEV))
    c64 = cand.to(torch.int64)
    exr = ex.restrict_cols(cand) if ex is not None else None
    if exr is not None and exr.col.numel() == 0:
        exr = None
    v, i = ops.rows_topk(F[:, c64].contiguous(), k, exr, drop, eu,
                         None if ei is None else ei[c64])
    return v, torch.where(i >= 0, c64[i.clamp(min=0)], i)


@pytest.mark.parametrize("which", ["all", "empty", "one", "tenth"])
def test_recommend_over_a_candidate_item_set(g1, baskets, f_all, emb, which):
    from lgcnhs import ops
    A, lam, k = g1["A"], 0.5, 20
    rng = np.random.default_rng(5)
    items = {"all": np.arange(I1), "empty": np.zeros(0, np.int64), "one": np.array([42]),
             "tenth": np.sort(rng.choice(I1, I1 // 10, False))}[which]
    cand = ops.item_candidates(items, I1, DEV)
    rows = ops.candidate_rows(baskets, len(baskets), I1, DEV)
    got = ops.spread_rows_recommend(A, baskets, lam, k, items=items)
    assert P.bit_equal(got, _items_reference(f_all[lam], cand, k, rows))
    ids = got[1][got[1] >= 0]
    assert bool(torch.isin(ids, cand.to(torch.int64)).all())
    eu, ei = emb
    got = ops.spread_rows_recommend(A, baskets, lam, k, eu=eu, ei=ei, items=items)
    assert P.bit_equal(got, _items_reference(f_all[lam], cand, k, rows, True, eu, ei))
    dv, di = ops.spread_rows_recommend(A, baskets, lam, k, items=items, W=g1["W"][lam])
    v, i = ops.spread_rows_recommend(A, baskets, lam, k, items=items)
    compare_lists_close(v.cpu(), i.cpu(), dv.cpu(), di.cpu(), RTOL, f"items={which} vs W=")


@pytest.mark.parametrize("which", ["empty", "tenth"])
def test_recommend_keeps_the_basket_over_a_candidate_item_set(g1, baskets, f_all, which):
    """drop=False with items= (no exclusion at all): the basket's own items rank among the
    candidates, on the two passes and through W=."""
    from lgcnhs import ops
    A, lam, k = g1["A"], 0.5, 20
    rng = np.random.default_rng(6)
    items = {"empty": np.zeros(0, np.int64),
             "tenth": np.sort(rng.choice(I1, I1 // 10, False))}[which]
    cand = ops.item_candidates(items, I1, DEV)
    got = ops.spread_rows_recommend(A, baskets, lam, k, drop=False, items=items)
    assert P.bit_equal(got, _items_reference(f_all[lam], cand, k, None, False))
    dv, di = ops.spread_rows_recommend(A, baskets, lam, k, drop=False, items=items,
                                       W=g1["W"][lam])
    compare_lists_close(got[0].cpu(), got[1].cpu(), dv.cpu(), di.cpu(), RTOL,
                        f"drop=False items={which} vs W=")
    if which == "tenth":   # basket 4 holds every item: all k places are its own items
        assert bool((got[1][4] >= 0).all())
        kept = ops.spread_rows_recommend(A, baskets, lam, k, items=items)[1][4]
        assert bool((kept == -1).all())


# --------------------------------------------------------------------------------------- ranks
@pytest.mark.parametrize("with_g", [False, True])
def test_rank_is_the_position_in_the_list(g1, baskets, emb, with_g):
    from lgcnhs import ops
    A, lam = g1["A"], 0.5
    eu, ei = emb if with_g else (None, None)
    rng = np.random.default_rng(9)
    targets = []
    for b in baskets:       # some of the basket's own items (dropped) among random ones
        t = set(rng.choice(I1, 12, False).tolist()) | set(b[:2])
        targets.append(sorted(t))
    T = ops.candidate_rows(targets, len(baskets), I1, DEV)
    rank, val = ops.spread_rows_rank(A, baskets, lam, T, eu=eu, ei=ei)
    rank, val = rank.cpu().numpy(), val.cpu()
    rp, col = T.rowptr.cpu().numpy(), T.col.cpu().numpy()
    for r, b in enumerate(baskets):
        for p in range(rp[r], rp[r + 1]):
            assert (rank[p] == -1) == (col[p] in set(b)), (r, col[p])   # a dropped target
    assert (rank >= 0).sum() > 1000
    for k in (20, 129):
        v, i = ops.spread_rows_recommend(A, baskets, lam, k, eu=eu, ei=ei)
        vb, i = v.cpu().numpy().view(np.int64), i.cpu().numpy()
        valb = val.numpy().view(np.int64)   # (bits, not values)
        for r in range(len(baskets)):
            for p in range(rp[r], rp[r + 1]):
                if 0 <= rank[p] < k:
                    assert i[r, rank[p]] == col[p], (r, p)
                    assert vb[r, rank[p]] == valb[p], (r, p)
                else:
                    assert col[p] not in i[r], (r, p)


def test_related_items(g1, f_all):
    from lgcnhs import ops
    A, lam, k = g1["A"], 0.5, 20
    ids = [17, 8, 0, 17, 299]
    got = ops.spread_related_items(A, ids, lam, k)
    assert P.bit_equal(got, ops.spread_rows_recommend(A, [[x] for x in ids], lam, k))
    for r, x in enumerate(ids):
        assert x not in got[1][r].tolist()
    assert P.bit_equal(got[0][0], got[0][3]) and P.bit_equal(got[1][0], got[1][3])
    cand = [3, 8, 17, 100, 299]
    gi = ops.spread_related_items(A, torch.tensor(ids), lam, 4, items=cand)
    assert P.bit_equal(gi, ops.spread_rows_recommend(A, [[x] for x in ids], lam, 4, items=cand))


# -------------------------------------------------------------------------------- call context
def test_what_the_buffers_held_does_not_matter(g1, baskets, f_all, emb):
    """Plain, started from a decoy's final buffers, started from 0xFF bytes: the same bits.
    (The decoy is another problem of the same tensor shapes -- another lambda, other baskets,
    embeddings scaled by 64 -- because _poison.replay demands the same allocation sequence.)"""
    from lgcnhs import ops
    A, k = g1["A"], 20
    eu, ei = emb
    n = len(baskets)
    other = [sorted(np.random.default_rng(100 + r).choice(I1, 1 + r % 50, False).tolist())
             for r in range(n)]
    rows = ops.candidate_rows(baskets, n, I1, DEV)
    want = ops.rows_topk(f_all[0.5], k, rows, True, eu, ei)

    def real():
        F = ops.spread_rows_resource(A, rows, 0.5)
        return (F,) + tuple(ops.spread_rows_recommend(A, rows, 0.5, k, eu=eu, ei=ei))

    def decoy():
        orows = ops.candidate_rows(other, n, I1, DEV)
        ops.spread_rows_resource(A, orows, 0.9)
        ops.spread_rows_recommend(A, orows, 0.9, k, eu=eu * 64, ei=ei)

    def check(out, how):
        assert P.bit_equal(out[0], f_all[0.5]), how
        assert P.bit_equal(out[1:], want), how

    P.three_ways(real, decoy, check)


def _on_side_stream(call):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        out = call()
    torch.cuda.current_stream().wait_stream(s)
    return out


def test_side_stream_and_strided_embeddings(g1, baskets, f_all, emb):
    from lgcnhs import ops
    A, k = g1["A"], 20
    eu, ei = emb
    want = ops.spread_rows_recommend(A, baskets, 0.5, k, eu=eu, ei=ei)
    assert P.bit_equal(_on_side_stream(lambda: ops.spread_rows_resource(A, baskets, 0.5)),
                       f_all[0.5])
    assert P.bit_equal(_on_side_stream(
        lambda: ops.spread_rows_recommend(A, baskets, 0.5, k, eu=eu, ei=ei)), want)
    wide = torch.zeros(eu.shape[0], 128, device=DEV)
    wide[:, ::2] = eu
    eu_nc = wide[:, ::2]
    assert not eu_nc.is_contiguous()
    assert P.bit_equal(ops.spread_rows_recommend(A, baskets, 0.5, k, eu=eu_nc, ei=ei), want)
    T = ops.candidate_rows([[5, 40]] * len(baskets), len(baskets), I1, DEV)
    assert P.bit_equal(ops.spread_rows_rank(A, baskets, 0.5, T, eu=eu_nc, ei=ei),
                       ops.spread_rows_rank(A, baskets, 0.5, T, eu=eu, ei=ei))


def test_f_blocks_do_not_change_the_result(g1, baskets, monkeypatch):
    """F_BLOCK_BYTES cuts the baskets into F blocks (here 50 rows: not a multiple of BLOCK)."""
    from lgcnhs import ops
    A = g1["A"]
    want = ops.spread_rows_recommend(A, baskets, 0.5, 20)
    T = ops.candidate_rows([[5, 40, 200]] * len(baskets), len(baskets), I1, DEV)
    want_r = ops.spread_rows_rank(A, baskets, 0.5, T)
    monkeypatch.setattr(ops, "F_BLOCK_BYTES", 50 * I1 * 8)
    assert P.bit_equal(ops.spread_rows_recommend(A, baskets, 0.5, 20), want)
    assert P.bit_equal(ops.spread_rows_rank(A, baskets, 0.5, T), want_r)


# ------------------------------------------------------------ the regrouping, restated (numpy)
def _two_pass_numpy(Ad, Bd, lam):
    """oracle.lgcn_oracle.spread_rows_spmv's regrouping for rows Bd that need not be rows of
    Ad: F = ((Bd / k_i^(1-lam)) A^T / k_v) A / k_j^lam, zero factors -> 1."""
    ku, ki = Ad.sum(1), Ad.sum(0)
    ku[ku == 0] = 1
    alpha, beta = np.power(ki, 1 - lam), np.power(ki, lam)
    alpha[alpha == 0] = 1
    beta[beta == 0] = 1
    C = (Bd / alpha[None, :]) @ Ad.T
    return ((C / ku[None, :]) @ Ad) / beta[None, :]


@pytest.mark.parametrize("lam", [0.3, 1.0])
def test_long_user_lists(lam):
    """Pass 1's segments: users of 2 SEG + 5 (three segments), SEG + 1 and SEG items."""
    from lgcnhs import ops
    SEG, BLOCK = _consts()
    U, I = 40, 2 * SEG + 5
    rng = np.random.default_rng(17)
    us = [np.zeros(I, np.int64), np.full(SEG + 1, 1), np.full(SEG, 2)]
    its = [np.arange(I), rng.choice(I, SEG + 1, False), rng.choice(I, SEG, False)]
    for v in range(3, U):
        n = int(rng.integers(1, 31))
        us.append(np.full(n, v)), its.append(rng.choice(I, n, False))
    keys = np.unique(np.concatenate(us) * I + np.concatenate(its))
    u, i = keys // I, keys % I
    Ad = O.interaction_matrix(U, I, u, i)
    A = ops.Interactions.from_pairs(torch.as_tensor(u), torch.as_tensor(i), U, I, DEV)
    assert int(A.by_user.degrees().max()) == I
    bs = [[], [3], list(range(I)), np.nonzero(Ad[1])[0].tolist(), list(range(SEG - 1, SEG + 2))]
    while len(bs) < BLOCK + 2:
        bs.append(sorted(rng.choice(I, int(rng.integers(1, 200)), False).tolist()))
    F = ops.spread_rows_resource(A, bs, lam)
    _close(F, _two_pass_numpy(Ad, _dense01(bs, I), lam), f"wide graph lam={lam}")
    for b in (2, 3, BLOCK + 1):
        assert P.bit_equal(ops.spread_rows_resource(A, [bs[b]], lam), F[b:b + 1]), b
    taken = ops.spread_rows_resource(A, A.by_user.take(torch.tensor([1])), lam)
    assert P.bit_equal(taken, F[3:4])


def test_zipf_graph():
    from lgcnhs import ops
    from lgcnhs.synth import synth_interactions
    U, I, lam = 4000, 2000, 0.5
    u, i = synth_interactions(U, I, 60000, seed=4, dist="zipf", zipf_s=1.1)
    Ad = O.interaction_matrix(U, I, u, i)
    A = ops.Interactions.from_pairs(torch.as_tensor(u), torch.as_tensor(i), U, I, DEV)
    rng = np.random.default_rng(23)
    hub = int(np.argmax(Ad.sum(0)))
    bs = [[hub], np.nonzero(Ad[0])[0].tolist()]
    while len(bs) < 16:
        bs.append(sorted(rng.choice(I, int(rng.integers(1, 101)), False).tolist()))
    F = ops.spread_rows_resource(A, bs, lam)
    ref = _two_pass_numpy(Ad, _dense01(bs, I), lam)
    _close(F, ref, "zipf")
    v, i_ = ops.spread_rows_recommend(A, bs, lam, 20)
    rows = ops.candidate_rows(bs, 16, I, DEV)
    ov, oi = O.rows_topk(ref, 20, rows.rowptr.cpu().numpy(), rows.col.cpu().numpy(), True)
    compare_lists_close(v.cpu(), i_.cpu(), ov, oi, RTOL, "zipf lists")


# --------------------------------------------------------------------- reference-API mirrors
def test_reference_api_mirrors():
    """recommendForBaskets / spread_lightgcn_baskets: {key: real item ids}, short rows shorter,
    the per-method lambda overrides of spread_method_topk, G from the caller's basket rows."""
    from types import SimpleNamespace

    import pandas as pd

    from lgcnhs import ops
    from lgcnhs.synth import synth_interactions
    from model.SpreadLightGCN.recommend import spread_lightgcn_baskets
    from model.SpreadMethod.recommend import recommendForBaskets
    U, I, k = 80, 120, 10
    u, i = synth_interactions(U, I, 1500, seed=1)
    df = pd.DataFrame({"user_id": u, "item_id": i})
    tr, va = df.iloc[::2], df.iloc[1::2]
    A = ops.Interactions.from_pairs(torch.as_tensor(u), torch.as_tensor(i), U, I, DEV)
    baskets = {"cart": [3, 50, 7, 3], "one": [9], "new": [], "most": list(range(I - 4))}
    rows = [sorted(set(b)) for b in baskets.values()]

    def lists(idx):
        return {key: [x for x in idx[r].tolist() if x >= 0] for r, key in enumerate(baskets)}

    got = recommendForBaskets(baskets, U, I, tr, va, "HybridS", 0.3, "douban", k)
    assert got == lists(ops.spread_rows_recommend(A, rows, 0.3, k)[1])
    assert list(got) == list(baskets) and len(got["most"]) == 4 and len(got["cart"]) == k
    got = recommendForBaskets(baskets, U, I, tr, va, "ProbS", 0.3, "movielens", k)
    assert got == lists(ops.spread_rows_recommend(A, rows, 0.01, k)[1])
    got = recommendForBaskets(baskets, U, I, tr, va, "HeatS", 0.3, "douban", k, items=[1, 5, 9])
    assert got == lists(ops.spread_rows_recommend(A, rows, 0.99, k, items=[1, 5, 9])[1])
    assert got["one"] == [x for x in got["one"] if x in (1, 5)]

    g = torch.Generator().manual_seed(2)
    ei = torch.randn(I, 64, generator=g)
    emb = torch.randn(len(baskets), 64, generator=g)
    model = SimpleNamespace(items_emb=SimpleNamespace(weight=ei.to(DEV)))
    got = spread_lightgcn_baskets(model, baskets, emb, U, I, tr, va, 0.5, k)
    want = ops.spread_rows_recommend(A, rows, 0.5, k, eu=emb.to(DEV), ei=ei.to(DEV))[1]
    assert got == lists(want)
