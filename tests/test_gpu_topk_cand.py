"""GPU parity of K2c (lg_score_topk_cand_f32 / lg_score_cand_f32, csrc/topk_cand.hip): top-K
where every row has its own candidate list. Every row is compared bit for bit (values as int32
views, ids, order, padding) with its twin -- lg_score_topk_f32 (ops.score_topk, screen=False) on
the one-user sub-problem (eu[u], ei[cand_r]) with the exclusion columns renumbered in numpy and
the ids mapped back -- and a subset with the C chain oracle on the same sub-problem; then the
Python layers (ops.score_topk_cand, ops.score_cand, recommendFromCandidates). No tolerance
anywhere: every comparison is against the same chain."""
import numpy as np
import pytest
import torch

from oracle import lgcn_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
U_TAB, I_TAB = 200, 4097
LENGTHS = (0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 300, 1000, 2049, 4097)
N_ROWS = 40
SEGS = (2, 3, 7, 64)
KS = (1, 20, 32, 33, 64, 65, 128)
NEG = float("-inf")


def _emb(n, d, seed, scale=0.1):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(n, d, generator=g) * scale).float()


def _rowsets(rp, col, n_rows, n_cols):
    from lgcnhs.graph import RowSets
    return RowSets(torch.as_tensor(np.asarray(rp, np.int64)).to(DEV),
                   torch.as_tensor(np.asarray(col, np.int32)).to(DEV), n_rows, n_cols)


def _csr(rows):
    """Host lists of ids -> (rowptr, col) numpy, the rows taken as they are."""
    rp = np.zeros(len(rows) + 1, np.int64)
    rp[1:] = np.cumsum([len(r) for r in rows])
    col = np.concatenate([np.asarray(r, np.int64) for r in rows] + [np.zeros(0, np.int64)])
    return rp, col.astype(np.int32)


def _seg_len(max_len, n_seg):
    """split_len of csrc/score_stream.h."""
    return max(16, -(-(-(-max_len // n_seg)) // 16) * 16)


_ROWS = None


def _rows():
    """The shared request: 40 rows with lengths cycling over LENGTHS, random ascending subsets
    that always hold the table's last item; users = a shuffled id list with one duplicate; and
    the exclusion pairs planted on them: on the last candidate of a segment and the first of
    the next for every n_seg of SEGS, on tile ends, every candidate of row 14 (300 long), and
    all but 5 candidates of row 13 (129 long)."""
    global _ROWS
    if _ROWS is None:
        rng = np.random.default_rng(77)
        users = rng.permutation(U_TAB)[:N_ROWS].astype(np.int64)
        users[-1] = users[0]
        rows = []
        for j in range(N_ROWS):
            n = LENGTHS[j % len(LENGTHS)]
            c = np.sort(rng.permutation(I_TAB - 1)[:max(n - 1, 0)])
            rows.append(np.concatenate([c, [I_TAB - 1]]).astype(np.int32) if n else
                        np.zeros(0, np.int32))
        pu, pi = [], []
        for j, c in enumerate(rows):
            pos = {15, 16, 31, 32, len(c) - 1}
            for ns in SEGS:
                seg = _seg_len(I_TAB, ns)
                pos |= {s * seg - 1 for s in range(1, 4)} | {s * seg for s in range(1, 4)}
            if j == 14:
                pos = set(range(len(c)))
            if j == 13:
                pos = set(range(len(c))) - {3, 40, 64, 100, 128}
            pos = sorted(p for p in pos if 0 <= p < len(c))
            pu += [users[j]] * len(pos)
            pi += c[pos].tolist()
        _ROWS = (users, rows, (np.asarray(pu, np.int64), np.asarray(pi, np.int64)))
    return _ROWS


_TABLES = {}


def _tables(d):
    """Shared inputs per width: 200 users x 4,097 items, exact ties (duplicate item rows), 3 %
    exclusions plus the planted pairs of _rows(); on the device, with the host CSR."""
    if d not in _TABLES:
        eu, ei = _emb(U_TAB, d, 100 + d), _emb(I_TAB, d, 200 + d)
        ei[100:140] = ei[60:100]
        rng = np.random.default_rng(300 + d)
        n = int(U_TAB * I_TAB * 0.03)
        rp, col = O.exclusion_csr(U_TAB, I_TAB, (rng.integers(0, U_TAB, n),
                                                 rng.integers(0, I_TAB, n)), _rows()[2])
        _TABLES[d] = (eu.to(DEV), ei.to(DEV), _rowsets(rp, col, U_TAB, I_TAB), rp, col,
                      eu.numpy(), ei.numpy())
    return _TABLES[d]


def _sub_excl(rp, col, u, cand):
    """User u's exclusion row restricted to cand and renumbered to positions in cand, as a
    one-row CSR (numpy)."""
    if rp is None:
        return np.zeros(2, np.int64), np.zeros(0, np.int32)
    pos = np.nonzero(np.isin(cand, col[rp[u]:rp[u + 1]]))[0].astype(np.int32)
    return np.array([0, len(pos)], np.int64), pos


def _twin_row(eu, ei, rp, col, u, cand, k):
    """Twin (a) of one row: lg_score_topk_f32 on (eu[u], ei[cand]), ids mapped back."""
    from lgcnhs import ops
    if len(cand) == 0:
        return (torch.full((k,), NEG, device=DEV), torch.full((k,), -1, dtype=torch.int64,
                                                               device=DEV))
    c = torch.as_tensor(np.asarray(cand, np.int64)).to(DEV)
    srp, scol = _sub_excl(rp, col, u, np.asarray(cand))
    ex = _rowsets(srp, scol, 1, len(cand)) if len(scol) else None
    v, i = ops.score_topk(eu[u:u + 1].contiguous(), ei[c].contiguous(), k, ex, screen=False,
                          n_splits=1)
    return v[0], torch.where(i[0] >= 0, c[i[0].clamp(min=0)], i[0])


def _twin(eu, ei, rp, col, users, rows, k):
    vs, is_ = zip(*[_twin_row(eu, ei, rp, col, int(u), c, k) for u, c in zip(users, rows)])
    return torch.stack(vs), torch.stack(is_)


_TWINS = {}


def _grid_twin(d, k, max_len=None):
    """The twin of the shared request, computed once per (d, k, max_len) and left unchanged."""
    key = (d, k, max_len)
    if key not in _TWINS:
        eu, ei, _, rp, col = _tables(d)[:5]
        users, rows, _ = _rows()
        _TWINS[key] = _twin(eu, ei, rp, col, users, [c[:max_len] for c in rows], k)
    return _TWINS[key]


def _chain_row(eun, ein, rp, col, u, cand, k):
    """Twin (b): the C chain oracle on the same one-user sub-problem, ids mapped back."""
    cand = np.asarray(cand)
    srp, scol = _sub_excl(rp, col, u, cand)
    ov, oi = O.chain_topk(eun[u:u + 1], np.ascontiguousarray(ein[cand]), srp, scol, k)
    return ov[0], np.where(oi[0] >= 0, cand[np.maximum(oi[0], 0)], -1)


def _same(got, want, what=None):
    (v, i), (rv, ri) = got, want
    assert torch.equal(i, ri), what
    assert torch.equal(v.view(torch.int32), rv.view(torch.int32)), what


def _cand(rows, n_cols=I_TAB):
    rp, col = _csr(rows)
    return _rowsets(rp, col, len(rows), n_cols)


def _run(d, k, n_seg=1, max_len=None, rows=None, users=None, tables=None):
    from lgcnhs import ops
    eu, ei, ex = (tables or _tables(d))[:3]
    u0, r0, _ = _rows()
    users = u0 if users is None else users
    return ops.score_topk_cand(eu, ei, _cand(r0 if rows is None else rows), k, ex,
                               users=torch.as_tensor(users), max_len=max_len, n_seg=n_seg)


@pytest.mark.parametrize("d", [32, 64, 128])
@pytest.mark.parametrize("k", KS)
def test_grid_rows_bit_exact(d, k):
    """40 rows of every length class, one segment, every k class and width: each row equals its
    twin; rows shorter than k are padded with {-inf, -1}; at k = 20 eight rows also equal the C
    chain oracle."""
    users, rows, _ = _rows()
    want = _grid_twin(d, k)
    v, i = _run(d, k)
    _same((v, i), want, (d, k))
    for j, c in enumerate(rows):
        if len(c) < k:
            assert (i[j, len(c):] == -1).all() and (v[j, len(c):] == NEG).all(), j
            assert (i[j, :len(c)] >= 0).all(), j
    if k == 20:
        rp, col, eun, ein = _tables(d)[3:]
        for j in (1, 4, 9, 13, 14, 15, 16, 17):
            ov, oi = _chain_row(eun, ein, rp, col, int(users[j]), rows[j], k)
            np.testing.assert_array_equal(i[j].cpu().numpy(), oi, str(j))
            assert np.array_equal(v[j].cpu().numpy().view(np.uint32), ov.view(np.uint32)), j


@pytest.mark.parametrize("d,k", [(32, 20), (64, 1), (64, 33), (64, 128), (128, 65)])
def test_segments_give_the_same_bits(d, k):
    """The same rows at n_seg = 2, 3, 7 and 64 (short rows then have empty units; exclusions sit
    on the segments' and the tiles' edges) give the one-segment bits, which are the twin's."""
    want = _grid_twin(d, k)
    for ns in SEGS:
        _same(_run(d, k, n_seg=ns), want, (d, k, ns))


def test_masked_candidates_rank():
    """Row 14: every candidate excluded -- all its scores are the mask value, the first k
    candidates in id order. Row 13: only 5 candidates are not excluded -- they lead, masked ones
    follow in id order. At one segment and at 7."""
    users, rows, _ = _rows()
    k = 20
    for ns in (1, 7):
        v, i = _run(64, k, n_seg=ns)
        _same((v, i), _grid_twin(64, k), ns)
        assert (v[14] == O.MASK).all()
        assert i[14].tolist() == rows[14][:k].tolist()
        free = rows[13][[3, 40, 64, 100, 128]]
        assert sorted(i[13, :5].tolist()) == sorted(free.tolist())
        assert (v[13, :5] > O.MASK).all() and (v[13, 5:] == O.MASK).all()
        masked = [x for x in rows[13].tolist() if x not in set(free.tolist())]
        assert i[13, 5:].tolist() == masked[:k - 5]


@pytest.mark.parametrize("k", [1, 128])
def test_worst_case_stream(k):
    """The item table reordered so that one user's scores ascend with the item id (argsort of
    the chain scores): over a 2,049-candidate row every candidate enters the list, which is
    compacted every few tiles. One segment; equals the twin and the C chain oracle."""
    from lgcnhs import ops
    d = 64
    eu, _, ex, rp, col, eun, ein = _tables(d)
    u = 17
    order = np.argsort(O.chain_scores(eun[u:u + 1], ein)[0], kind="stable")
    ein2 = np.ascontiguousarray(ein[order])
    ei2 = torch.as_tensor(ein2).to(DEV)
    cand = np.sort(np.random.default_rng(5).permutation(I_TAB)[:2049]).astype(np.int32)
    s = O.chain_scores(eun[u:u + 1], ein2[cand])[0]
    assert (np.diff(s) >= 0).all()
    got = ops.score_topk_cand(eu, ei2, _cand([cand]), k, ex, users=[u], n_seg=1)
    tv, ti = _twin_row(eu, ei2, rp, col, u, cand, k)
    _same(got, (tv[None], ti[None]))
    ov, oi = _chain_row(eun, ein2, rp, col, u, cand, k)
    np.testing.assert_array_equal(got[1][0].cpu().numpy(), oi)
    assert np.array_equal(got[0][0].cpu().numpy().view(np.uint32), ov.view(np.uint32))


@pytest.mark.parametrize("k", [20, 128])
def test_max_len(k):
    """max_len = 100: rows longer than 100 are ranked over their first 100 candidates only (the
    twin on c[:100]); max_len = 10^6 changes nothing; both also in segments."""
    d = 64
    want = _grid_twin(d, k, 100)
    assert not torch.equal(want[1], _grid_twin(d, k)[1])
    _same(_run(d, k, max_len=100), want)
    _same(_run(d, k, max_len=100, n_seg=3), want)
    _same(_run(d, k, max_len=10**6), _grid_twin(d, k))
    _same(_run(d, k, max_len=10**6, n_seg=64), _grid_twin(d, k))


def test_non_finite_rows():
    """A NaN item row, an item with a +inf element and one with a -inf element among the
    candidates; a NaN user row: NaN and -inf scores never rank; every row equals its twin."""
    from lgcnhs import ops
    U, I, d = 70, 3000, 64
    eu, ei = _emb(U, d, 41), _emb(I, d, 42)
    ei[1234] = float("nan")
    ei[2000, 5] = float("inf")
    ei[2500, 3] = -float("inf")
    eu[7] = float("nan")
    eu[0] = float("nan")  # the row an out-of-range id would be clamped to
    rng = np.random.default_rng(43)
    n = int(U * I * 0.01)
    rp, col = O.exclusion_csr(U, I, (rng.integers(0, U, n), rng.integers(0, I, n)))
    ex = _rowsets(rp, col, U, I)
    eu, ei = eu.to(DEV), ei.to(DEV)
    users = np.array([7, 11, 1, 2, 30, 69, 12])
    rows = [np.union1d(np.random.default_rng(50 + j).permutation(I)[:n_c],
                       [1234, 2000, 2500]).astype(np.int32)
            for j, n_c in enumerate((500, 40, 700, 100, 1500, 18, 250))]
    for k in (20, 100):
        want = _twin(eu, ei, rp, col, users, rows, k)
        for ns in (1, 3):
            v, i = ops.score_topk_cand(eu, ei, _cand(rows, I), k, ex,
                                       users=torch.as_tensor(users), n_seg=ns)
            _same((v, i), want, (k, ns))
            assert (i[0] == -1).all() and not (i == 1234).any()
            assert (i[2:5, :18] >= 0).all()
        s = ops.score_cand(eu, ei, _cand(rows, I), ex, users=torch.as_tensor(users))
        # the NaN user's pairs: NaN, but the mask value where the pair is excluded
        masked = torch.as_tensor(np.isin(rows[0], col[rp[7]:rp[8]])).to(DEV)
        s0 = s[:len(rows[0])]
        assert torch.isnan(s0[~masked]).all() and (s0[masked] == O.MASK).all()


def test_bad_ids_on_device_tensors():
    """Device tensors are taken as given. A candidate id of -1 in front of and one of n_items
    behind an otherwise valid row: they read row 0, never rank, and the row equals the twin
    without them; a user id of n_table_users: all padding; the other rows are untouched."""
    from lgcnhs import ops
    d, k = 64, 20
    eu, ei, ex, rp, col = _tables(d)[:5]
    users, rows, _ = _rows()
    hostile = list(rows)
    for j in (12, 16):
        hostile[j] = np.concatenate([[-1], rows[j], [I_TAB]]).astype(np.int32)
    ids = torch.as_tensor(users).to(DEV).clone()
    ids[5] = U_TAB
    want_v, want_i = (t.clone() for t in _grid_twin(d, k))
    want_v[5], want_i[5] = NEG, -1
    for ns in (1, 3):
        v, i = ops.score_topk_cand(eu, ei, _cand(hostile), k, ex, users=ids, n_seg=ns)
        assert not (i == I_TAB).any() and (i >= -1).all()
        _same((v, i), (want_v, want_i), ns)
    s = ops.score_cand(eu, ei, _cand(hostile), ex, users=ids)
    rp_h = _csr(hostile)[0]
    for j in (12, 16):
        assert s[rp_h[j]] == NEG and s[rp_h[j + 1] - 1] == NEG
        assert torch.isfinite(s[rp_h[j] + 1:rp_h[j + 1] - 1]).all()
    assert (s[rp_h[5]:rp_h[6]] == NEG).all()


@pytest.mark.parametrize("d", [32, 64, 128])
def test_score_cand_every_position(d):
    """ops.score_cand: every position of cand.col, in its order, holds the C chain score of its
    (user, item) pair bit for bit, the mask value where the pair is excluded; with max_len = 100
    the positions >= 100 of their row hold -inf and the others are unchanged."""
    from lgcnhs import ops
    eu, ei, ex, rp, col, eun, ein = _tables(d)
    users, rows, _ = _rows()
    cand = _cand(rows)
    want = []
    for u, c in zip(users, rows):
        if len(c) == 0:
            continue
        s = O.chain_scores(eun[u:u + 1], np.ascontiguousarray(ein[c]))[0]
        s[np.isin(c, col[rp[u]:rp[u + 1]])] = O.MASK
        want.append(s)
    want = np.concatenate(want)
    assert (want == O.MASK).sum() > 300
    got = ops.score_cand(eu, ei, cand, ex, users=torch.as_tensor(users))
    assert got.dtype == torch.float32 and got.shape == (cand.col.numel(),)
    assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32))
    past = np.concatenate([np.arange(len(c)) >= 100 for c in rows])
    cut = ops.score_cand(eu, ei, cand, ex, users=torch.as_tensor(users), max_len=100)
    cut = cut.cpu().numpy()
    assert past.sum() > 0 and (cut[past] == NEG).all()
    assert np.array_equal(cut[~past].view(np.uint32), want[~past].view(np.uint32))
    # the top-K values are these scores
    v, i = _run(d, 20)
    j = 15
    r0 = _csr(rows)[0][j]
    best = np.sort(want[r0:r0 + len(rows[j])])[::-1][:20]
    assert np.array_equal(v[j].cpu().numpy(), best)


# ------------------------------------------------------------------------- Python layers
def test_users_none_is_one_row_per_user():
    """users=None: row r is user r, one row per table user; equals users=arange and, on eight
    rows, the twin."""
    from lgcnhs import ops
    d, k = 64, 20
    eu, ei, ex, rp, col = _tables(d)[:5]
    rng = np.random.default_rng(9)
    rows = [np.sort(rng.permutation(I_TAB)[:int(n)]).astype(np.int32)
            for n in rng.integers(0, 90, U_TAB)]
    cand = ops.candidate_rows([r.tolist() for r in rows], U_TAB, I_TAB, DEV)
    v0, i0 = ops.score_topk_cand(eu, ei, cand, k, ex)
    assert v0.shape == (U_TAB, k) and i0.dtype == torch.int64 and v0.dtype == torch.float32
    _same(ops.score_topk_cand(eu, ei, cand, k, ex, users=torch.arange(U_TAB)), (v0, i0))
    _same(ops.score_topk_cand(eu, ei, cand, k, ex, max_len=90, n_seg=2), (v0, i0))
    some = [0, 1, 50, 99, 100, 150, 198, 199]
    want = _twin(eu, ei, rp, col, some, [rows[u] for u in some], k)
    _same((v0[some], i0[some]), want)
    with pytest.raises(ValueError, match="user id"):
        ops.score_topk_cand(eu, ei, cand, k, ex, users=[U_TAB] * U_TAB)
    with pytest.raises(ValueError, match="users"):
        ops.score_topk_cand(eu, ei, cand, k, ex, users=[0, 1])


def test_k_limit_and_empty_candidates():
    """k = 129 raises, naming the limit; no rows or no candidates at all give padding."""
    from lgcnhs import ops
    eu, ei, ex = _tables(64)[:3]
    cand = _cand(_rows()[1])
    with pytest.raises(ValueError, match="128"):
        ops.score_topk_cand(eu, ei, cand, 129, ex, users=torch.as_tensor(_rows()[0]))
    with pytest.raises(ValueError):
        ops.score_topk_cand(eu, ei, cand, 0, ex, users=torch.as_tensor(_rows()[0]))
    for empty, R in ((ops.candidate_rows([[], [], []], 3, I_TAB, DEV), 3),
                     (ops.candidate_rows({}, 5, I_TAB, DEV), 5),
                     (ops.candidate_rows([], 0, I_TAB, DEV), 0)):
        v, i = ops.score_topk_cand(eu, ei, empty, 20, ex, users=list(range(R)))
        assert v.shape == (R, 20) and i.shape == (R, 20)
        assert (i == -1).all() and (v == NEG).all()
        assert i.dtype == torch.int64 and v.dtype == torch.float32
        assert ops.score_cand(eu, ei, empty, ex, users=list(range(R))).numel() == 0


def test_recommend_from_candidates_vs_recommend_for_users(golden):
    """recommendFromCandidates on lightgcn_mid, every user with its own random candidate list
    (some shorter than k, one empty): per user the list of recommendForUsers(items=cand_u);
    with user_ids= the same lists for a shuffled subset; a bad id raises."""
    from model.LightGCN.model import LightGCN
    from model.LightGCN.recommend import recommendForUsers, recommendFromCandidates
    from utils.graph import convertEdgeIndexToAdjMatrix
    g = golden("lightgcn_mid")
    U, I, k = int(g["n_users"]), int(g["n_items"]), int(g["k"])
    torch.manual_seed(42)
    m = LightGCN(U, I, 64, 3).to(DEV)
    tr = convertEdgeIndexToAdjMatrix(U, I, torch.as_tensor(g["train"].astype(np.int64)))
    va = convertEdgeIndexToAdjMatrix(U, I, torch.as_tensor(g["val"].astype(np.int64)))
    rng = np.random.default_rng(11)
    cands = {u: rng.permutation(I)[:int(n)].tolist()
             for u, n in enumerate(rng.integers(1, 120, U))}
    cands[3] = []
    cands[4] = cands[4][:5]
    got = recommendFromCandidates(m, cands, U, I, tr, va, None, k)
    assert sorted(got) == list(range(U)) and got[3] == [] and len(got[4]) == 5
    for u in range(U):
        want = recommendForUsers(m, [u], U, I, tr, va, None, k, items=cands[u])[u]
        assert got[u] == want, u
    sub = rng.permutation(U)[:17].tolist()
    some = recommendFromCandidates(m, [cands[u] for u in sub], U, I, tr, va, None, k,
                                   user_ids=sub)
    assert some == {u: got[u] for u in sub}
    with pytest.raises(ValueError):
        recommendFromCandidates(m, {0: [I]}, U, I, tr, va, None, k)
    with pytest.raises(ValueError):
        recommendFromCandidates(m, [[1]], U, I, tr, va, None, k, user_ids=[U])
