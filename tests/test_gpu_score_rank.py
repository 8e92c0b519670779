"""GPU parity of K2k (lg_score_rank_f32, csrc/rank.hip; ops.score_rank): the rank of given
(user, item) pairs over the full catalog. The reference in every case is numpy on
oracle.lgcn_oracle.chain_masked_matrix with the definition
    rank(u, i) = #{ j != i : v(u, j) > v(u, i) or (v(u, j) == v(u, i) and j < i) }
Ranks are compared exactly and scores bit for bit (int32 views): no tolerance anywhere."""
import numpy as np
import pytest
import torch

from oracle import lgcn_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
MASK = float(-(1 << 10))
NEG = float("-inf")
SPLITS = (1, 3, 7)


def _emb(n, d, seed, scale=0.1):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(n, d, generator=g) * scale).float()


def _rowsets(rp, col, n_rows, n_cols):
    from lgcnhs.graph import RowSets
    return RowSets(torch.as_tensor(np.asarray(rp, np.int64)).to(DEV),
                   torch.as_tensor(np.asarray(col, np.int32)).to(DEV), n_rows, n_cols)


def _csr(rows):
    """Host lists of ids -> (rowptr, col) numpy, the rows taken as they are (any order)."""
    rp = np.zeros(len(rows) + 1, np.int64)
    rp[1:] = np.cumsum([len(r) for r in rows])
    col = np.concatenate([np.asarray(r, np.int64) for r in rows] + [np.zeros(0, np.int64)])
    return rp, col.astype(np.int32)


def _ref(G, users, rows):
    """The definition on the masked matrix G [table users, items]: (rank, score) of every target
    of every row, in the rows' own order. NaN follows > / == literally."""
    ids = np.arange(G.shape[1])
    rk, sc = [], []
    with np.errstate(invalid="ignore"):
        for u, row in zip(users, rows):
            for i in row:
                t = G[u, i]
                b = (G[u] > t) | ((G[u] == t) & (ids < i))
                b[i] = False
                rk.append(int(b.sum()))
                sc.append(t)
    return np.asarray(rk, np.int64), np.asarray(sc, np.float32)


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.int32)


def _check(got, want, what=""):
    (rk, sc), (wrk, wsc) = got, want
    assert rk.dtype == torch.int64 and sc.dtype == torch.float32
    np.testing.assert_array_equal(rk.cpu().numpy(), wrk, err_msg=f"ranks {what}")
    np.testing.assert_array_equal(_bits(sc.cpu().numpy()), _bits(wsc), err_msg=f"scores {what}")


def _excl(n_users, n_items, density, seed, *extra):
    rng = np.random.default_rng(seed)
    n = int(n_users * n_items * density)
    return O.exclusion_csr(n_users, n_items, (rng.integers(0, n_users, n),
                                              rng.integers(0, n_items, n)), *extra)


def _target_rows(n_rows, n_items, lens, seed, last=True):
    """Rows of lens[r % len(lens)] distinct targets in NON-ascending order; the table's last item
    (in the 13-item tail tile) and item 0 among them."""
    rng = np.random.default_rng(seed)
    rows = []
    for r in range(n_rows):
        n = lens[r % len(lens)]
        c = rng.permutation(n_items - 2)[:n] + 1
        if n and last and r % 3 == 0:
            c[0] = n_items - 1
        if n > 1 and r % 5 == 0:
            c[-1] = 0
        rows.append(np.sort(c)[::-1].copy() if r % 2 else c)
    return rows


@pytest.mark.parametrize("d", [32, 64, 128])
def test_shapes_and_splits(d):
    """37 rows (one past two 16-row groups) x 1,005 items (a 13-item tail tile), n_splits in
    {1, 3, 7} (336- and 144-item splits: boundaries off the tile grid's end), rows of 0, 1, MAX,
    MAX + 1 and 2 MAX + 1 targets (split into kernel rows by ops) in non-ascending order, 3 %
    exclusions: equal to the definition and identical over n_splits."""
    from lgcnhs import ops
    M = ops.RANK_ROW_MAX
    U, I = 37, 1005
    eu, ei = _emb(U, d, 10 + d), _emb(I, d, 20 + d)
    rows = _target_rows(U, I, (0, 1, M, M + 1, 2 * M + 1), 30 + d)
    # some targets are themselves excluded
    tu = [u for u, r in enumerate(rows) for _ in r][::4]
    ti = [i for r in rows for i in r][::4]
    rp, col = _excl(U, I, 0.03, 40 + d, (np.asarray(tu), np.asarray(ti)))
    want = _ref(O.chain_masked_matrix(eu.numpy(), ei.numpy(), rp, col), range(U), rows)
    trp, tcol = _csr(rows)
    tg, ex = _rowsets(trp, tcol, U, I), _rowsets(rp, col, U, I)
    first = None
    for ns in SPLITS:
        got = ops.score_rank(eu.to(DEV), ei.to(DEV), tg, ex, n_splits=ns)
        _check(got, want, f"d={d} n_splits={ns}")
        if first is None:
            first = got
        assert torch.equal(first[0], got[0]) and torch.equal(first[1], got[1])
    _check(ops.score_rank(eu.to(DEV), ei.to(DEV), tg, ex), want, "planned splits")
    # the host forms of the targets (sorted per row by candidate_rows): aligned with that CSR
    as_lists = ops.candidate_rows([r.tolist() for r in rows], U, I, DEV)
    want_sorted = _ref(O.chain_masked_matrix(eu.numpy(), ei.numpy(), rp, col), range(U),
                       [np.sort(r) for r in rows])
    _check(ops.score_rank(eu.to(DEV), ei.to(DEV), [r.tolist() for r in rows], ex), want_sorted)
    _check(ops.score_rank(eu.to(DEV), ei.to(DEV), as_lists, ex, n_splits=3), want_sorted)
    # no targets: nothing launched
    e = ops.score_rank(eu.to(DEV), ei.to(DEV), {}, ex)
    assert e[0].numel() == 0 and e[1].numel() == 0 and e[0].dtype == torch.int64


@pytest.mark.parametrize("d", [32, 64, 128])
def test_threshold_widths(d):
    """k_rank_count keeps 1, 2 or 4 thresholds per row, chosen per wave of 32 kernel rows from
    the rows it holds: 70 users whose first 32 have one target each, the next 32 one or two,
    the last 6 three (every user has a target, so kernel row = user), exclusions and tied
    embedding rows included -- one launch runs all three loops, with and without splits."""
    from lgcnhs import ops
    U, I = 70, 1005
    eu, ei = _emb(U, d, 50 + d), _emb(I, d, 60 + d)
    ei[10:20] = ei[500:510]
    rng = np.random.default_rng(70 + d)
    lens = [1] * 32 + [1 + u % 2 for u in range(32)] + [3] * 6
    rows = [rng.permutation(I)[:n] for n in lens]
    rows[0][0], rows[40][0], rows[65][0] = 505, 15, I - 1
    rp, col = _excl(U, I, 0.03, 80 + d, (np.array([0, 40, 65]), np.array([15, 505, 12])))
    want = _ref(O.chain_masked_matrix(eu.numpy(), ei.numpy(), rp, col), range(U), rows)
    trp, tcol = _csr(rows)
    tg, ex = _rowsets(trp, tcol, U, I), _rowsets(rp, col, U, I)
    krp, kids = ops.rank_rows(tg)
    assert kids[:U].tolist() == list(range(U)) and krp[:U + 1].tolist() == trp.tolist()
    for ns in (1, 7):
        _check(ops.score_rank(eu.to(DEV), ei.to(DEV), tg, ex, n_splits=ns), want,
               f"d={d} n_splits={ns}")


@pytest.mark.parametrize("d", [32, 128])
def test_ties(d):
    """Embeddings from {-1, 0, 1}: integer scores with tens to hundreds of exact ties per target,
    so the id rule enters most ranks. User 5 is all zero: every score is 0 and a target's rank is
    its id minus the excluded ids below it (they rank at the mask value), by the formula. Item
    rows 300 and 700 are copies of row 500, a target of every user: one tie at a lower id, one at
    a higher."""
    from lgcnhs import ops
    U, I = 37, 1005
    g = torch.Generator().manual_seed(7 + d)
    eu = torch.randint(-1, 2, (U, d), generator=g).float()
    ei = torch.randint(-1, 2, (I, d), generator=g).float()
    eu[5] = 0
    ei[300] = ei[500]
    ei[700] = ei[500]
    rows = [np.array([500, 1004, 0, 299][:1 + u % 4]) for u in range(U)]
    rp, col = _excl(U, I, 0.05, 8 + d)
    G = O.chain_masked_matrix(eu.numpy(), ei.numpy(), rp, col)
    want = _ref(G, range(U), rows)
    # the ties are there: some 70-100 items per user score exactly what target 500 does
    assert sum(int((G[u] == G[u, 500]).sum()) for u in range(U)) > 2000
    trp, tcol = _csr(rows)
    tg, ex = _rowsets(trp, tcol, U, I), _rowsets(rp, col, U, I)
    for ns in SPLITS:
        got = ops.score_rank(eu.to(DEV), ei.to(DEV), tg, ex, n_splits=ns)
        _check(got, want, f"n_splits={ns}")
    ex5 = col[rp[5]:rp[5 + 1]]
    r5 = got[0][trp[5]:trp[6]].cpu().numpy()
    for i, r in zip(rows[5], r5):
        if i not in ex5:
            assert r == i - (ex5 < i).sum()


def test_exclusion_cases():
    """Hand-placed rows (d = 64, 1,005 items). User 0: excluded items scoring above and below
    the target, and excluded copies of the target's embedding row at a lower and a higher id
    (the correction's raw score must be the stream's, bit for bit, or the rank is off by one).
    User 1: the target is itself excluded (it ranks at the mask value, behind every other
    finite item but ahead of higher-id excluded ones). User 2: a target scoring below
    mask_value, so the masked items rank above it. Then excl=None."""
    from lgcnhs import ops
    U, I, d = 20, 1005, 64
    eu, ei = _emb(U, d, 1), _emb(I, d, 2)
    ei[100] = ei[600]
    ei[900] = ei[600]
    ei[777] = -40.0 * eu[2] / (eu[2] @ eu[2]) * 64.0  # score of (2, 777) about -2560
    raw = O.chain_scores(eu.numpy(), ei.numpy())
    assert raw[2, 777] < MASK
    order0 = np.argsort(-raw[0])
    t0 = 600
    above = [j for j in order0[:40] if raw[0, j] > raw[0, t0] and j not in (100, 600, 900)][:5]
    below = [j for j in order0[::-1][:40] if raw[0, j] < raw[0, t0]][:5]
    assert len(above) == 5 and len(below) == 5
    pu = [0] * 12 + [1] * 4 + [2] * 30
    pi = above + below + [100, 900] + [3, 400, 401, 1004] + list(range(200, 230))
    rp, col = _excl(U, I, 0.02, 3, (np.asarray(pu), np.asarray(pi)))
    rows = [np.array([t0, int(order0[0]), int(order0[-1])]), np.array([400, 3, 1004, 17]),
            np.array([777, 205, 5])] + [np.array([u, 1004 - u]) for u in range(3, U)]
    trp, tcol = _csr(rows)
    tg = _rowsets(trp, tcol, U, I)
    for excl, G in ((_rowsets(rp, col, U, I),
                     O.chain_masked_matrix(eu.numpy(), ei.numpy(), rp, col)), (None, raw)):
        want = _ref(G, range(U), rows)
        for ns in (1, 7):
            _check(ops.score_rank(eu.to(DEV), ei.to(DEV), tg, excl, n_splits=ns), want,
                   f"excl={excl is not None} n_splits={ns}")
    # what the rows were built to show (on the masked reference)
    G = O.chain_masked_matrix(eu.numpy(), ei.numpy(), rp, col)
    wr, ws = _ref(G, range(U), rows)
    assert ws[trp[1]] == MASK and ws[trp[2]] == raw[2, 777]
    assert wr[trp[2]] == I - 1  # everything, the masked items too, is above (2, 777)


def test_users_subset_and_bad_ids():
    """users=: a subset of the table in non-ascending order with a repeated id, the exclusion
    CSR indexed by user id. Through the C ABI: a user id outside the table gives {-1, -inf} for
    its whole row, a target id outside [0, n_items) {-1, -inf} for that target, positions at or
    past max_targets {-1, -inf}; every other entry is unaffected."""
    from lgcnhs import _native as N
    from lgcnhs import ops
    U, I, d = 50, 1005, 32
    eu, ei = _emb(U, d, 11), _emb(I, d, 12)
    rp, col = _excl(U, I, 0.04, 13)
    G = O.chain_masked_matrix(eu.numpy(), ei.numpy(), rp, col)
    ex = _rowsets(rp, col, U, I)
    users = np.array([41, 7, 7, 49, 0, 30, 12, 3, 41])
    rows = _target_rows(len(users), I, (1, 3, 6, 0, 2), 14)
    trp, tcol = _csr(rows)
    tg = _rowsets(trp, tcol, len(users), I)
    want = _ref(G, users, rows)
    for us in (users.tolist(), torch.as_tensor(users).to(DEV)):
        _check(ops.score_rank(eu.to(DEV), ei.to(DEV), tg, ex, users=us, n_splits=3), want)

    # C ABI: rows of at most 4 targets, max_targets = 3
    ids = np.array([41, U, 7, -1, 49, 0, 2**40, 30], np.int64)
    crow = [np.array([5, I, 1004]), np.array([1, 2]), np.array([-1, 9, 2**31 - 1]),
            np.array([4]), np.array([8, 1, 0, 900]), np.array([], np.int64), np.array([7]),
            np.array([I - 1, -7, 0])]
    crp, ccol = _csr(crow)
    n = len(ccol)
    eud, eid = eu.to(DEV), ei.to(DEV)
    idt = torch.as_tensor(ids).to(DEV)
    rpt, colt = torch.as_tensor(crp).to(DEV), torch.as_tensor(ccol).to(DEV)
    for ns in (1, 7):
        rk = torch.full((n,), -5, dtype=torch.int64, device=DEV)
        sc = torch.full((n,), 5.0, dtype=torch.float32, device=DEV)
        nbytes = N.lib().lg_score_rank_ws_bytes(len(ids), len(ids) * 3, d, ns)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
        N.check(N.lib().lg_score_rank_f32(
            N.ptr(eud), N.ptr(eid), N.ptr(idt), len(ids), U, I, N.ptr(rpt), N.ptr(colt), 3, d,
            N.ptr(ex.rowptr), N.ptr(ex.col), MASK, ns, N.ptr(rk), N.ptr(sc), N.ptr(ws), nbytes,
            N.stream_handle(torch.device(DEV))), "lg_score_rank_f32")
        rk, sc = rk.cpu().numpy(), sc.cpu().numpy()
        for r, (u, row) in enumerate(zip(ids, crow)):
            for p, i in enumerate(row):
                e = crp[r] + p
                if 0 <= u < U and 0 <= i < I and p < 3:
                    wr, wsc = _ref(G, [u], [[i]])
                    assert rk[e] == wr[0] and _bits(sc[e]) == _bits(wsc[0]), (r, p)
                else:
                    assert rk[e] == -1 and sc[e] == NEG, (r, p, rk[e], sc[e])


def test_non_finite():
    """Item 100 holds one +inf, item 200 one NaN (every score of it is NaN); one target sits on
    the NaN item, one on the +inf item; both are also excluded for some users. Ranks equal the
    formula on the oracle's matrix: a NaN is never better and nothing is better than a NaN."""
    from lgcnhs import ops
    U, I, d = 37, 1005, 64
    eu, ei = _emb(U, d, 21), _emb(I, d, 22)
    ei[100, 3] = float("inf")
    ei[200, 40] = float("nan")
    pu, pi = np.array([1, 2, 3, 4]), np.array([100, 200, 100, 200])
    rp, col = _excl(U, I, 0.03, 23, (pu, pi))
    G = O.chain_masked_matrix(eu.numpy(), ei.numpy(), rp, col)
    assert np.isnan(G[0, 200]) and np.isinf(G[0, 100])
    rows = [np.array([200, 100, 50 + u, 1004][:2 + u % 3]) for u in range(U)]
    want = _ref(G, range(U), rows)
    trp, tcol = _csr(rows)
    for ns in (1, 3):
        _check(ops.score_rank(eu.to(DEV), ei.to(DEV), _rowsets(trp, tcol, U, I),
                              _rowsets(rp, col, U, I), n_splits=ns), want, f"n_splits={ns}")
    assert want[0][0] == 0  # (0, 200): a NaN target, nothing is better


def test_against_the_lists():
    """300 users x 20,005 items, d = 64, random normal embeddings, 2 % exclusions, 1-8 held-out
    items per user (some users none): every target with rank < 1024 sits at position rank of
    score_topk's k = 1024 list with the same value bits, no target with rank >= 1024 is in its
    row, and recall / precision / NDCG at 20 from the ranks equal metrics.accuracy on the list's
    first 20 columns to 1e-12."""
    from lgcnhs import metrics, ops
    U, I, d, k = 300, 20005, 64, 1024
    eu, ei = _emb(U, d, 31).to(DEV), _emb(I, d, 32).to(DEV)
    rp, col = _excl(U, I, 0.02, 33)
    ex = _rowsets(rp, col, U, I)
    rng = np.random.default_rng(34)
    rows = []
    for u in range(U):
        n = int(rng.integers(1, 9)) if u % 11 else 0
        rows.append(np.sort(rng.permutation(I)[:n]))
    # ... and some held-out items the model likes: from the best of a cheap fp32 product
    top = torch.topk(eu @ ei.T, 40, dim=1).indices.cpu().numpy()
    for u in range(0, U, 2):
        if len(rows[u]):
            rows[u] = np.unique(np.concatenate([rows[u], top[u, rng.integers(0, 40, 2)]]))
    trp, tcol = _csr(rows)
    test = _rowsets(trp, tcol, U, I)
    rank, score = ops.score_rank(eu, ei, test, ex)
    val, idx = ops.score_topk(eu, ei, k, ex)
    row_of = torch.repeat_interleave(torch.arange(U, device=DEV), test.degrees())
    item = test.col.to(torch.int64)
    assert int(rank.min()) >= 0
    inside = rank < k
    assert int(inside.sum()) > 100 and int((~inside).sum()) > 100
    at = rank.clamp(max=k - 1)
    assert torch.equal(idx[row_of, at][inside], item[inside])
    assert torch.equal(val[row_of, at][inside].view(torch.int32), score[inside].view(torch.int32))
    listed = (idx[row_of] == item[:, None]).any(dim=1)
    assert not bool(listed[~inside].any())
    m = metrics.rank_metrics(rank, test, I, ks=(20,))
    a = metrics.accuracy(idx[:, :20].contiguous(), test, 20)
    assert m["n_eval"] == a["n_eval"] and m["n_skipped"] == 0
    for name in ("recall", "precision", "ndcg"):
        assert abs(m[f"{name}@20"] - a[name]) <= 1e-12, (name, m[f"{name}@20"], a[name])
    assert m["recall@20"] > 0  # (the planted items: the equality is not of zeros)


def test_get_held_out_ranks():
    """getHeldOutRanks on a small synthetic graph equals ops.score_rank called by hand: layer-0
    embeddings, the train positives excluded at -1024, the held-out positives as targets; and
    LightGCNOpti re-exports the function."""
    from lgcnhs import ops
    from lgcnhs.graph import RowSets
    from lgcnhs.synth import synth_interactions
    from model.LightGCN.evaluation import MASK_VALUE, getHeldOutRanks
    from model.LightGCN.model import LightGCN
    from model.LightGCNOpti import evaluation as opti_eval
    assert opti_eval.getHeldOutRanks is getHeldOutRanks
    U, I, E = 120, 700, 4000
    users, items = synth_interactions(U, I, E, seed=3)
    held = np.arange(len(users)) % 5 == 0
    tr = torch.as_tensor(O.coo_adjacency(U, I, users[~held], items[~held]))
    he = torch.as_tensor(O.coo_adjacency(U, I, users[held], items[held]))
    torch.manual_seed(0)
    model = LightGCN(U, I, 64, 3).to(DEV)
    targets, rank = getHeldOutRanks(model, U, I, tr, he)
    assert isinstance(targets, RowSets) and (targets.n_rows, targets.n_cols) == (U, I)
    assert rank.dtype == torch.int64 and rank.numel() == targets.col.numel() > 0
    eu = model.users_emb.weight.detach().float().contiguous()
    ei = model.items_emb.weight.detach().float().contiguous()
    ex = RowSets.from_pairs(users[~held], items[~held], U, I, DEV)
    tg = RowSets.from_pairs(users[held], items[held], U, I, DEV)
    assert torch.equal(targets.rowptr, tg.rowptr) and torch.equal(targets.col, tg.col)
    want, _ = ops.score_rank(eu, ei, tg, ex, mask_value=MASK_VALUE)
    assert torch.equal(rank, want)
    # ... and the definition, on the oracle's matrix
    rp, col = O.exclusion_csr(U, I, (users[~held], items[~held]))
    trp, tcol = tg.rowptr.cpu().numpy(), tg.col.cpu().numpy()
    rows = [tcol[trp[u]:trp[u + 1]] for u in range(U)]
    wr, _ = _ref(O.chain_masked_matrix(eu.cpu().numpy(), ei.cpu().numpy(), rp, col), range(U),
                 rows)
    np.testing.assert_array_equal(rank.cpu().numpy(), wr)
