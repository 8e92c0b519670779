"""K4i (the spreading / LGCNHS top-K over a candidate item set, csrc/rows_topk_items.hip), C ABI
side: lg_spread_rows_topk_items_f64 is exported and bound without an ABI bump, refuses every bad
call before any launch with its own name in lg_last_error(); the host glue around it
(ops.item_candidates, RowSets.restrict_cols and the id map of the column view) on CPU tensors.
CPU only (no kernel runs)."""
import ctypes

import numpy as np
import pytest
import torch

NAME = "lg_spread_rows_topk_items_f64"
ME = NAME.encode()
LG_OK, LG_ERR_ARG = 0, 1
DROP, NONE = 0, 1

z = ctypes.c_void_p(0)
one = ctypes.c_void_p(16)  # never dereferenced: validation fails first


@pytest.fixture(scope="module")
def lib():
    from lgcnhs import _native as N
    return N.load_library()


def call(lib, rp=one, items=one, W=one, n_rows=4, n_items=100, cand=one, n_cand=50, eu=z, ei=z,
         dim=0, xrp=z, xcol=z, mode=DROP, k=20, val=one, idx=one):
    return lib.lg_spread_rows_topk_items_f64(rp, items, W, n_rows, n_items, cand, n_cand, eu, ei,
                                             dim, xrp, xcol, mode, k, val, idx, z)


def refused(lib, **kw):
    assert call(lib, **kw) == LG_ERR_ARG, kw
    msg = lib.lg_last_error()
    assert ME in msg, (kw, msg)
    return msg


def test_exported_and_bound_without_an_abi_bump():
    from lgcnhs import _native as N
    prod, ref = N.load_library(), N.ref_lib()
    assert N.ABI_VERSION == 17 == prod.lg_abi_version() == ref.lg_abi_version()
    assert NAME in N.SIGNATURES and NAME not in N.REF_SIGNATURES
    assert len(N.SIGNATURES[NAME][1]) == 17
    assert hasattr(prod, NAME) and hasattr(ref, NAME)


def test_null_pointers_are_refused(lib):
    for name in ("rp", "items", "W", "cand", "val", "idx"):
        assert b"null" in refused(lib, **{name: z})


def test_bad_k_dim_and_counts_are_refused(lib):
    for k in (0, 1025, -1):
        assert b"k=" in refused(lib, k=k)
    for dim in (48, 16, 256):
        assert b"dim" in refused(lib, eu=one, ei=one, dim=dim)
    assert b"n_cand" in refused(lib, n_cand=-1)
    assert b"n_cand" in refused(lib, n_cand=101)  # more candidates than items
    assert b"sizes" in refused(lib, n_rows=-1)
    assert b"sizes" in refused(lib, n_items=2**31 - 1)
    assert b"excl_mode" in refused(lib, mode=7)


def test_half_set_pairs_are_refused(lib):
    assert b"eu/ei" in refused(lib, eu=one, ei=z, dim=64)
    assert b"eu/ei" in refused(lib, eu=z, ei=one, dim=64)
    assert b"ex_rowptr" in refused(lib, xrp=one, xcol=z)
    assert b"ex_rowptr" in refused(lib, xrp=z, xcol=one)


def test_g_factor_with_kept_exclusions_is_refused(lib):
    assert b"LG_EXCL_DROP" in refused(lib, eu=one, ei=one, dim=64, xrp=one, xcol=one, mode=NONE)


def test_no_rows_is_ok_without_a_launch(lib):
    """n_rows = 0 returns before anything is launched (no GPU here): every k class and G."""
    for k in (1, 64, 65, 128, 129, 256, 512, 1024):
        assert call(lib, n_rows=0, k=k) == LG_OK
    assert call(lib, n_rows=0, n_cand=0, eu=one, ei=one, dim=128, xrp=one, xcol=one) == LG_OK


def test_item_candidates_on_the_host():
    from lgcnhs import ops
    mask = np.zeros(12, dtype=bool)
    mask[[1, 4, 11]] = True
    for m in (mask, torch.as_tensor(mask)):
        t = ops.item_candidates(m, 12, "cpu")
        assert t.dtype == torch.int32 and t.tolist() == [1, 4, 11]
    assert ops.item_candidates([9, 0, 9, 3], 12, "cpu").tolist() == [0, 3, 9]
    e = ops.item_candidates([], 12, "cpu")
    assert e.dtype == torch.int32 and e.numel() == 0
    with pytest.raises(ValueError, match="item id"):
        ops.item_candidates([12], 12, "cpu")


def _rowsets(seed, n_rows=7, n_cols=23):
    from lgcnhs.graph import RowSets
    rng = np.random.default_rng(seed)
    rows = [np.sort(rng.choice(n_cols, rng.integers(0, 9), replace=False)) for _ in range(n_rows)]
    rowptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    col = np.concatenate(rows).astype(np.int32) if rowptr[-1] else np.zeros(0, np.int32)
    return RowSets(torch.as_tensor(rowptr), torch.as_tensor(col), n_rows, n_cols), rows


def test_column_view_of_every_item_is_the_identity():
    """The tiled path's column view for C = arange(I): restrict_cols(C) leaves the CSR as it
    is and the id map sends every position to itself (-1 stays -1) -- why items=arange(I) is
    bitwise the no-items walk."""
    rs, _ = _rowsets(0)
    C = torch.arange(rs.n_cols, dtype=torch.int32)
    v = rs.restrict_cols(C)
    assert v.n_cols == rs.n_cols and v.n_rows == rs.n_rows
    assert torch.equal(v.rowptr, rs.rowptr) and torch.equal(v.col, rs.col)
    assert v.col.dtype == torch.int32 and v.rowptr.dtype == torch.int64
    idx = torch.tensor([[3, 0, 22, -1], [-1, -1, -1, -1]])
    c64 = C.to(torch.int64)
    assert torch.equal(torch.where(idx >= 0, c64[idx.clamp(min=0)], idx), idx)


def test_column_view_renumbers_and_maps_back():
    """restrict_cols(C) keeps exactly the columns in C, as ascending positions in C; mapping
    the positions through C gives the kept item ids back."""
    rs, rows = _rowsets(1)
    C = torch.tensor([0, 2, 3, 8, 13, 21, 22], dtype=torch.int32)
    v = rs.restrict_cols(C)
    assert v.n_cols == 7
    for r, items in enumerate(rows):
        pos = v.col[int(v.rowptr[r]):int(v.rowptr[r + 1])].to(torch.int64)
        assert bool((pos[1:] > pos[:-1]).all())
        assert C[pos].tolist() == [int(x) for x in items if int(x) in set(C.tolist())]
    empty = rs.restrict_cols(torch.zeros(0, dtype=torch.int32))
    assert empty.n_cols == 0 and int(empty.rowptr[-1]) == 0 and empty.col.numel() == 0


def test_routing_constants_name_their_measurement():
    """The dense router's bounds are named constants read off profiles/spread_items.json."""
    import inspect
    import json
    import os
    from conftest import REPO
    from lgcnhs import ops
    src = inspect.getsource(ops)
    at = src.index("SPREAD_ITEMS_FUSED_MAX_SHARE =")
    assert "profiles/spread_items.json" in src[at - 2500:at]
    prof = json.load(open(os.path.join(REPO, "profiles", "spread_items.json")))
    cases = prof["dense"]["cases"]
    assert len(cases) == 2 * 4 * 4 * 3
    assert all(all(c["lists_equal"].values()) for c in cases)
    # the router sends a case to the fused kernel only where the file says it wins
    I = prof["dense"]["shape"]["items"]
    for c in cases:
        if ops._spread_items_route(c["users"], c["candidates"], I) == "fused":
            assert c["fused_wins"], c
    assert ops.ROWS_ITEMS_SPLIT == 512
