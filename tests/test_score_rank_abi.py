"""K2k (the full-catalog rank of given pairs, csrc/rank.hip), C ABI side: lg_score_rank_ws_bytes
and lg_score_rank_f32 are exported by both libraries, refuse every bad call before any launch
with the entry's name in lg_last_error(), and size the workspace by a threshold and an id per
target slot plus one count per (split, slot); ops.rank_splits plans the item ranges and
ops.rank_rows cuts target rows of any length into kernel rows on tensors of any device. CPU only
(no kernel runs)."""
import ctypes

import numpy as np
import pytest

NAMES = ("lg_score_rank_ws_bytes", "lg_score_rank_f32")
LG_OK, LG_ERR_ARG, LG_ERR_WORKSPACE = 0, 1, 3
ME = b"lg_score_rank_f32"

z = ctypes.c_void_p(0)
one = ctypes.c_void_p(16)  # never dereferenced: validation fails first


@pytest.fixture(scope="module")
def lib():
    from lgcnhs import _native as N
    return N.load_library()


def rank(lib, eu=one, ei=one, ids=one, n_rows=8, n_table=1000, n_items=1000, rp=one, col=one,
         max_targets=4, dim=64, ex_rp=z, ex_col=z, n_splits=1, out_rank=one, out_score=one,
         ws=one, ws_bytes=1 << 40):
    return lib.lg_score_rank_f32(eu, ei, ids, n_rows, n_table, n_items, rp, col, max_targets,
                                 dim, ex_rp, ex_col, -1024.0, n_splits, out_rank, out_score, ws,
                                 ws_bytes, z)


def refused(lib, **kw):
    """The call is refused with LG_ERR_ARG and the entry's own name in the message."""
    assert rank(lib, **kw) == LG_ERR_ARG, kw
    msg = lib.lg_last_error()
    assert ME in msg, (kw, msg)
    return msg


def test_exported_by_both_libraries():
    from lgcnhs import _native as N
    prod, ref = N.load_library(), N.ref_lib()
    for name in NAMES:
        assert name in N.SIGNATURES, name
        assert hasattr(prod, name), name
        assert hasattr(ref, name), name
    assert N.ABI_VERSION == 17 and prod.lg_abi_version() == 17  # entries added, none changed


def test_row_max_is_the_headers():
    """LG_RANK_ROW_MAX of include/lgcnhs.h, its Python mirrors and the entry's own limit agree."""
    import os
    import re
    from lgcnhs import _native as N
    from lgcnhs import ops
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(repo, "include", "lgcnhs.h")) as f:
        m = re.search(r"#define LG_RANK_ROW_MAX (\d+)", f.read())
    assert int(m.group(1)) == N.LG_RANK_ROW_MAX == ops.RANK_ROW_MAX
    assert N.LG_RANK_ROW_MAX in (4, 8)


def test_null_pointers_are_refused(lib):
    for name in ("eu", "ei", "rp", "col", "out_rank", "out_score"):
        assert b"null" in refused(lib, **{name: z})
    # user_ids may be NULL (row r is user r): the next check speaks, not the pointer check
    assert b"n_splits" in refused(lib, ids=z, n_splits=0)


def test_bad_counts_and_sizes_are_refused(lib):
    from lgcnhs import _native as N
    for n in (0, -1):
        assert b"n_rows" in refused(lib, n_rows=n)
    assert b"n_items" in refused(lib, n_items=0)
    assert b"n_items" in refused(lib, n_items=2**31 - 1)
    assert b"n_table_users" in refused(lib, n_table=0)
    for mt in (0, -1, N.LG_RANK_ROW_MAX + 1):
        assert b"max_targets" in refused(lib, max_targets=mt)
    for dim in (16, 48, 256):
        assert b"dim" in refused(lib, dim=dim)
    for ns in (0, -1, 4097):
        assert b"n_splits" in refused(lib, n_splits=ns)
    # (n_rows / 128 row tiles) x n_splits workgroups, and n_rows / 4 row workgroups, past the
    # grid limit of 2^31 - 1
    assert b"grid" in refused(lib, n_rows=2**27, n_splits=4096, n_items=2**20)
    assert b"grid" in refused(lib, n_rows=2**38, n_splits=1)
    assert b"grid" in refused(lib, n_rows=2**33 + 1, n_splits=1)
    # ... and inside it the call reaches the workspace check
    assert rank(lib, n_rows=2**25, n_splits=4096, n_items=2**20, ws=z) == LG_ERR_WORKSPACE


def test_half_set_exclusion_pair_is_refused(lib):
    assert b"ex_rowptr" in refused(lib, ex_rp=one, ex_col=z)
    assert b"ex_rowptr" in refused(lib, ex_rp=z, ex_col=one)


@pytest.mark.parametrize("n_rows,mt,n_splits", [(1, 1, 1), (8, 4, 3), (100, 3, 31)])
def test_short_workspace(lib, n_rows, mt, n_splits):
    need = lib.lg_score_rank_ws_bytes(n_rows, n_rows * mt, 64, n_splits)
    assert need == n_rows * mt * (8 + 4 * n_splits)
    for ws, nbytes in ((one, need - 1), (one, 0), (z, need), (z, 0)):
        assert rank(lib, n_rows=n_rows, max_targets=mt, n_splits=n_splits, n_items=10**5,
                    ws=ws, ws_bytes=nbytes) == LG_ERR_WORKSPACE
        msg = lib.lg_last_error()
        assert ME in msg and b"workspace" in msg


def test_ws_bytes_shape(lib):
    """A threshold and an id per slot and an int32 count per (split, slot); 0 for arguments
    the call refuses."""
    f = lib.lg_score_rank_ws_bytes
    assert f(100, 400, 64, 1) == 400 * 12
    assert f(100, 100, 128, 3) == 100 * 20
    assert f(1, 1, 32, 4096) == 8 + 4 * 4096
    for bad in ((0, 4, 64, 3), (-1, 4, 64, 3), (100, 0, 64, 3), (100, -4, 64, 3),
                (100, 400, 48, 3), (100, 400, 16, 3), (100, 400, 256, 3), (100, 400, 64, 0),
                (100, 400, 64, 4097), (2**27, 2**27, 64, 4096)):
        assert f(*bad) == 0, bad


@pytest.mark.parametrize("cus", [1, 8, 64, 256, 304])
def test_split_plan(lib, cus):
    """ops.rank_splits on `cus` compute units: an int in [1, 4096], every split of split_len
    (csrc/score_stream.h, restated) at least 16 items long and -- where the items are split --
    at least RANK_MIN_SPLIT / 2 of n_items / n_splits; one split when the rows alone give
    RANK_WAVES_PER_CU waves of 32 rows per compute unit or the catalog is shorter than two
    shortest splits; and the entry accepts the plan up to the workspace it was not given."""
    from lgcnhs import ops
    for n_rows in (1, 16, 33, 64, 4095, 32768, 10**6, 10**7):
        for n_items in (1, 15, 16, 17, 1005, 4096, 8191, 8192, 10**5, 10**6, 2**31 - 2):
            ns = ops.rank_splits(n_rows, n_items, None, cus=cus)
            what = (cus, n_rows, n_items, ns)
            assert isinstance(ns, int) and 1 <= ns <= 4096, what
            per = max(16, -(-(-(-n_items // ns)) // 16) * 16)
            used = -(-n_items // per)
            assert per >= 16 and 1 <= used <= ns, what
            if ns > 1:
                assert n_items - (used - 1) * per >= 1, what  # no empty split in use
                assert n_items / ns >= ops.RANK_MIN_SPLIT / 2, what
                assert -(-n_rows // 32) * (ns - 1) < ops.RANK_WAVES_PER_CU * cus, what
            if -(-n_rows // 32) >= ops.RANK_WAVES_PER_CU * cus or n_items < 2 * ops.RANK_MIN_SPLIT:
                assert ns == 1, what
            assert lib.lg_score_rank_ws_bytes(n_rows, n_rows * 4, 64, ns) \
                == n_rows * 4 * (8 + 4 * ns), what
            assert rank(lib, n_rows=n_rows, n_items=n_items, n_splits=ns, ws=z,
                        ws_bytes=0) == LG_ERR_WORKSPACE, what


def _rowsets(lists, n_cols=1000):
    import torch
    from lgcnhs.graph import RowSets
    rp = np.zeros(len(lists) + 1, np.int64)
    rp[1:] = np.cumsum([len(x) for x in lists])
    col = np.concatenate([np.asarray(x, np.int64) for x in lists] + [np.zeros(0, np.int64)])
    return RowSets(torch.as_tensor(rp), torch.as_tensor(col.astype(np.int32)), len(lists),
                   n_cols)


def _kernel_rows(krp, ids, row_max):
    """(user id, [positions in targets.col]) of every non-empty kernel row, checking that every
    row is a run of at most row_max positions and that the pointers never go back."""
    krp, ids = krp.tolist(), ids.tolist()
    assert len(krp) == len(ids) + 1
    out = []
    for j, u in enumerate(ids):
        assert 0 <= krp[j + 1] - krp[j] <= row_max, (j, krp)
        if krp[j + 1] > krp[j]:
            out.append((u, list(range(krp[j], krp[j + 1]))))
        else:
            assert u == 0  # padding rows name a user inside any table
    return out


def test_row_splitting_on_the_host():
    """ops.rank_rows on CPU tensors: a user with 2 MAX + 1 targets becomes three kernel rows
    over consecutive runs of its own positions of targets.col, MAX, MAX and 1 long; rows of 0, 1,
    MAX and MAX + 1 targets become 0, 1, 1 and 2; every position is covered exactly once, in
    order; the row count is the documented bound; `users` maps target rows to user ids."""
    import torch
    from lgcnhs import ops
    M = ops.RANK_ROW_MAX
    lens = [0, 2 * M + 1, 1, 0, M, M + 1, 0]
    lists, nxt = [], 0
    for n in lens:
        lists.append(list(range(nxt, nxt + n)))
        nxt += n
    t = _rowsets(lists)
    nnz = sum(lens)
    krp, ids = ops.rank_rows(t)
    assert krp.dtype == torch.int64 and ids.dtype == torch.int64
    assert ids.numel() == (nnz + (M - 1) * min(len(lens), nnz)) // M
    rows = _kernel_rows(krp, ids, M)
    start = np.cumsum([0] + lens)
    want = []
    for r, n in enumerate(lens):
        for c in range(0, n, M):
            want.append((r, list(range(start[r] + c, start[r] + min(c + M, n)))))
    assert rows == want
    assert [len(p) for u, p in rows if u == 1] == [M, M, 1]
    assert sorted(p for _, ps in rows for p in ps) == list(range(nnz))
    # users=: the ids of the target rows, repeated ones included
    users = torch.tensor([5, 9, 5, 7, 2, 9, 1])
    krp2, ids2 = ops.rank_rows(t, users)
    assert torch.equal(krp2, krp)
    assert [u for u, _ in _kernel_rows(krp2, ids2, M)] == [int(users[r]) for r, _ in want]
    # another row_max, rows that fit exactly, and a RowSets whose rows start inside col
    for row_max in (1, 2, 8):
        k3, i3 = ops.rank_rows(t, row_max=row_max)
        got = _kernel_rows(k3, i3, row_max)
        assert sorted(p for _, ps in got for p in ps) == list(range(nnz))
        assert sum(1 for u, _ in got if u == 1) == -(-(2 * M + 1) // row_max)
    sl = t.slice_rows(1, 3)  # rows 1 and 2, absolute offsets
    k4, i4 = ops.rank_rows(sl)
    got = _kernel_rows(k4, i4, M)
    assert [u for u, _ in got] == [0, 0, 0, 1]
    assert sorted(p for _, ps in got for p in ps) == list(range(0, 2 * M + 2))
    # no targets at all: no kernel rows
    k5, i5 = ops.rank_rows(_rowsets([[], []]))
    assert i5.numel() == 0 and k5.tolist() == [0]


def test_plan_rows():
    """ops.rank_plan_rows: between ceil(nnz / MAX) and rank_rows' bound, exact for rows of equal
    length <= MAX, at least 1."""
    from lgcnhs import ops
    M = ops.RANK_ROW_MAX
    assert ops.rank_plan_rows(32768, 32768) == 32768
    assert ops.rank_plan_rows(32768, 32768 * M) == 32768
    assert ops.rank_plan_rows(100000, 1000) == 1000
    assert ops.rank_plan_rows(5, 0) == 1
    for rows, nnz in ((4096, 40960), (1, 9), (1000, 1000 * M + 1), (7, 3)):
        p = ops.rank_plan_rows(rows, nnz)
        assert -(-nnz // M) <= p <= (nnz + (M - 1) * min(rows, nnz)) // M, (rows, nnz, p)
