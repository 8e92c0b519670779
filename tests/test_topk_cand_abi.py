"""K2c (top-K over every row's own candidate list, csrc/topk_cand.hip), C ABI side:
lg_score_topk_cand_ws_bytes, lg_score_topk_cand_f32 and lg_score_cand_f32 are exported by both
libraries, refuse every bad call before any launch with the entry's name in lg_last_error(),
and size the workspace by one partial list per (segment, row); ops.cand_segments plans the
segments and ops.candidate_rows normalises per-row candidates on the host. CPU only (no kernel
runs)."""
import ctypes

import numpy as np
import pytest

NAMES = ("lg_score_topk_cand_ws_bytes", "lg_score_topk_cand_f32", "lg_score_cand_f32")
LG_OK, LG_ERR_ARG, LG_ERR_WORKSPACE = 0, 1, 3
TOPK, PAIRS = b"lg_score_topk_cand_f32", b"lg_score_cand_f32"

z = ctypes.c_void_p(0)
one = ctypes.c_void_p(16)  # never dereferenced: validation fails first


@pytest.fixture(scope="module")
def lib():
    from lgcnhs import _native as N
    return N.load_library()


def topk(lib, eu=one, ei=one, ids=one, n_rows=8, n_table=1000, n_items=1000, rp=one, col=one,
         max_len=500, dim=64, ex_rp=z, ex_col=z, k=20, n_seg=1, val=one, idx=one, ws=one,
         ws_bytes=1 << 40):
    return lib.lg_score_topk_cand_f32(eu, ei, ids, n_rows, n_table, n_items, rp, col, max_len,
                                      dim, ex_rp, ex_col, -1024.0, k, n_seg, val, idx, ws,
                                      ws_bytes, z)


def pairs(lib, eu=one, ei=one, ids=one, n_rows=8, n_table=1000, n_items=1000, rp=one, col=one,
          max_len=500, dim=64, ex_rp=z, ex_col=z, out=one):
    return lib.lg_score_cand_f32(eu, ei, ids, n_rows, n_table, n_items, rp, col, max_len, dim,
                                 ex_rp, ex_col, -1024.0, out, z)


def refused(lib, fn=topk, **kw):
    """The call is refused with LG_ERR_ARG and the entry's own name in the message."""
    assert fn(lib, **kw) == LG_ERR_ARG, kw
    msg = lib.lg_last_error()
    assert (TOPK if fn is topk else PAIRS) in msg, (kw, msg)
    return msg


def test_exported_by_both_libraries():
    from lgcnhs import _native as N
    prod, ref = N.load_library(), N.ref_lib()
    for name in NAMES:
        assert name in N.SIGNATURES, name
        assert hasattr(prod, name), name
        assert hasattr(ref, name), name


def test_null_pointers_are_refused(lib):
    for name in ("eu", "ei", "rp", "col", "val", "idx"):
        assert b"null" in refused(lib, **{name: z})
    for name in ("eu", "ei", "rp", "col", "out"):
        assert b"null" in refused(lib, pairs, **{name: z})
    # user_ids may be NULL (row r is user r): the next check speaks, not the pointer check
    assert b"k=" in refused(lib, ids=z, k=0)


def test_bad_counts_and_sizes_are_refused(lib):
    for fn in (topk, pairs):
        for n in (0, -1):
            assert b"n_rows" in refused(lib, fn, n_rows=n)
        assert b"n_items" in refused(lib, fn, n_items=0)
        assert b"n_items" in refused(lib, fn, n_items=2**31 - 1)
        assert b"n_table_users" in refused(lib, fn, n_table=0)
        for ml in (0, -5, 2**31):
            assert b"max_len" in refused(lib, fn, max_len=ml)
        for dim in (16, 48, 256):
            assert b"dim" in refused(lib, fn, dim=dim)
    for k in (0, 129):
        assert b"k=" in refused(lib, k=k)
    for ns in (0, -1, 4097):
        assert b"n_seg" in refused(lib, n_seg=ns)
    # n_rows x n_seg / 4 workgroups past the grid limit of 2^31 - 1
    assert b"grid" in refused(lib, n_rows=2**31, n_seg=4096, max_len=2**20)
    assert b"grid" in refused(lib, n_rows=2**33, n_seg=1)
    assert b"grid" in refused(lib, pairs, n_rows=2**33, max_len=1)
    assert topk(lib, n_rows=2**31, n_seg=4096, max_len=2**20) == LG_ERR_ARG


def test_half_set_exclusion_pair_is_refused(lib):
    for fn in (topk, pairs):
        assert b"ex_rowptr" in refused(lib, fn, ex_rp=one, ex_col=z)
        assert b"ex_rowptr" in refused(lib, fn, ex_rp=z, ex_col=one)


@pytest.mark.parametrize("n_rows,k,n_seg", [(1, 1, 2), (8, 20, 3), (100, 128, 31)])
def test_short_workspace(lib, n_rows, k, n_seg):
    need = lib.lg_score_topk_cand_ws_bytes(n_rows, 64, k, n_seg)
    assert need == n_seg * n_rows * k * 8
    for ws, nbytes in ((one, need - 1), (one, 0), (z, need), (z, 0)):
        assert topk(lib, n_rows=n_rows, k=k, n_seg=n_seg, max_len=10**5, ws=ws,
                    ws_bytes=nbytes) == LG_ERR_WORKSPACE
        msg = lib.lg_last_error()
        assert TOPK in msg and b"workspace" in msg


def test_ws_bytes_shape(lib):
    """One partial list of k 8-byte entries per (segment, row); nothing for one segment; 0 for
    arguments the call refuses."""
    f = lib.lg_score_topk_cand_ws_bytes
    assert f(100, 64, 20, 1) == 0
    assert f(100, 64, 20, 3) == 3 * 100 * 20 * 8
    assert f(1, 32, 1, 4096) == 4096 * 8
    for bad in ((0, 64, 20, 3), (-1, 64, 20, 3), (100, 48, 20, 3), (100, 16, 20, 3),
                (100, 256, 20, 3), (100, 64, 0, 3), (100, 64, 129, 3), (100, 64, 20, 0),
                (100, 64, 20, 4097), (2**31, 64, 20, 4096)):
        assert f(*bad) == 0, bad


@pytest.mark.parametrize("cus", [1, 8, 64, 256, 304])
def test_segment_plan(lib, cus):
    """ops.cand_segments on `cus` compute units over row counts, row lengths around the tile
    and the shortest segment, and every k class: 1 <= n_seg <= 4096, no segment in use shorter
    than 16 candidates (split_len of csrc/score_stream.h, restated) nor -- where a row is split
    -- than CAND_MIN_SEG of max_len / n_seg, one segment whenever max_len <= CAND_MIN_SEG or
    the rows alone give 16 waves per compute unit, and a plan the workspace query accepts."""
    from lgcnhs import ops
    for n_rows in (1, 3, 64, 4095, 10**6):
        for max_len in (1, 15, 16, 17, 255, 256, 257, 10**5):
            for k in (1, 32, 33, 64, 65, 128):
                ns = ops.cand_segments(n_rows, max_len, k, None, cus=cus)
                what = (cus, n_rows, max_len, k, ns)
                assert isinstance(ns, int) and 1 <= ns <= 4096, what
                seg = max(16, -(-(-(-max_len // ns)) // 16) * 16)
                assert seg >= 16, what
                if max_len <= ops.CAND_MIN_SEG or n_rows >= 16 * cus:
                    assert ns == 1, what
                if ns > 1:
                    assert max_len / ns >= ops.CAND_MIN_SEG / 2, what
                    assert n_rows * (ns - 1) < 16 * cus, what
                want = 0 if ns == 1 else ns * n_rows * k * 8
                assert lib.lg_score_topk_cand_ws_bytes(n_rows, 64, k, ns) == want, what
                if ns > 1:  # the entry accepts the plan up to the workspace it was not given
                    assert -(-max_len // seg) > 1, what
                    assert topk(lib, n_rows=n_rows, max_len=max_len, k=k, n_seg=ns, ws=z,
                                ws_bytes=0) == LG_ERR_WORKSPACE, what


def test_candidate_rows_on_the_host():
    """ops.candidate_rows: a dict, a list of lists and a (rows, items) pair give the same CSR
    -- int64 row pointers, int32 ids ascending and unique per row; a RowSets passes through; a
    bad id, a float or a wrong row count raises before anything touches a device."""
    import torch
    from lgcnhs import ops
    from lgcnhs.graph import RowSets
    lists = [[7, 3, 9, 3, 0], [], [5], [9, 8, 8]]
    want_rp, want_col = [0, 4, 4, 5, 7], [0, 3, 7, 9, 5, 8, 9]
    as_dict = {3: [9, 8, 8], 0: np.array([7, 3, 9, 3, 0]), 2: torch.tensor([5])}
    rows = [3, 0, 0, 2, 0, 3, 0, 0, 3]
    items = [8, 7, 3, 5, 9, 9, 3, 0, 8]
    forms = (lists, as_dict, (rows, items), (np.array(rows), torch.tensor(items)))
    for f in forms:
        c = ops.candidate_rows(f, 4, 10, "cpu")
        assert isinstance(c, RowSets) and (c.n_rows, c.n_cols) == (4, 10)
        assert c.rowptr.dtype == torch.int64 and c.col.dtype == torch.int32
        assert c.rowptr.tolist() == want_rp and c.col.tolist() == want_col
    assert ops.candidate_rows(c, 4, 10, "cpu") is c
    e = ops.candidate_rows({}, 3, 10, "cpu")
    assert e.rowptr.tolist() == [0, 0, 0, 0] and e.col.numel() == 0
    assert ops.candidate_rows([[], []], 2, 10, "cpu").col.numel() == 0
    with pytest.raises(ValueError, match="item id"):
        ops.candidate_rows([[0, -1]], 1, 10, "cpu")
    with pytest.raises(ValueError, match="item id"):
        ops.candidate_rows({0: [0, 10]}, 1, 10, "cpu")
    with pytest.raises(ValueError, match="item id"):
        ops.candidate_rows(([0], [10]), 1, 10, "cpu")
    with pytest.raises(ValueError, match="row"):
        ops.candidate_rows({4: [1]}, 4, 10, "cpu")
    with pytest.raises(ValueError, match="row"):
        ops.candidate_rows(([-1], [1]), 4, 10, "cpu")
    with pytest.raises(ValueError, match="integers"):
        ops.candidate_rows([[0.5, 1.0]], 1, 10, "cpu")
    with pytest.raises(ValueError, match="integers"):
        ops.candidate_rows(([0], [1.0]), 1, 10, "cpu")
    with pytest.raises(ValueError, match="lists"):
        ops.candidate_rows([[1], [2]], 3, 10, "cpu")
    with pytest.raises(ValueError, match="rows"):
        ops.candidate_rows(([0, 1], [1]), 4, 10, "cpu")
    with pytest.raises(ValueError, match="rows"):
        ops.candidate_rows(c, 5, 10, "cpu")
