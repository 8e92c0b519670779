"""K2i (top-K for a short list of users over a candidate item set, csrc/topk_items.hip), C ABI
side: lg_score_topk_batch_items_ws_bytes and lg_score_topk_batch_items_f32 are exported by both
libraries, refuse every bad call before any launch with the entry's name in lg_last_error(),
and size the workspace by one partial list per (workgroup, user); ops.item_candidates
normalises an items= argument on the host. CPU only (no kernel runs)."""
import ctypes

import numpy as np
import pytest

NAMES = ("lg_score_topk_batch_items_ws_bytes", "lg_score_topk_batch_items_f32")
LG_OK, LG_ERR_ARG, LG_ERR_WORKSPACE = 0, 1, 3
ME = b"lg_score_topk_batch_items_f32"

z = ctypes.c_void_p(0)
one = ctypes.c_void_p(16)  # never dereferenced: validation fails first


@pytest.fixture(scope="module")
def lib():
    from lgcnhs import _native as N
    return N.load_library()


def call(lib, eu=one, ei=one, ids=one, n_batch=8, n_table=1000, n_items=1000, items=one,
         n_cand=500, dim=64, rp=z, col=z, k=20, val=one, idx=one, ws=one, ws_bytes=1 << 40):
    return lib.lg_score_topk_batch_items_f32(eu, ei, ids, n_batch, n_table, n_items, items,
                                             n_cand, dim, rp, col, -1024.0, k, val, idx, ws,
                                             ws_bytes, z)


def refused(lib, **kw):
    assert call(lib, **kw) == LG_ERR_ARG, kw
    msg = lib.lg_last_error()
    assert ME in msg, (kw, msg)
    return msg


def test_exported_by_both_libraries():
    from lgcnhs import _native as N
    prod, ref = N.load_library(), N.ref_lib()
    assert N.ABI_VERSION == 17 == prod.lg_abi_version() == ref.lg_abi_version()
    for name in NAMES:
        assert name in N.SIGNATURES, name
        assert hasattr(prod, name), name
        assert hasattr(ref, name), name


def test_null_pointers_are_refused(lib):
    for name in ("eu", "ei", "items", "val", "idx"):
        assert b"null" in refused(lib, **{name: z})


def test_bad_batch_k_dim_and_counts_are_refused(lib):
    for nb in (0, 17, 65):
        assert b"n_batch" in refused(lib, n_batch=nb)
    for k in (0, 129):
        assert b"k=" in refused(lib, k=k)
    for dim in (16, 48, 256):
        assert b"dim" in refused(lib, dim=dim)
    for nc in (0, 1001):  # n_items + 1
        assert b"n_cand" in refused(lib, n_cand=nc)
    assert b"n_items" in refused(lib, n_items=0)
    assert b"n_items" in refused(lib, n_items=2**31 - 1)
    assert b"n_table_users" in refused(lib, n_table=0)


def test_half_set_exclusion_pair_is_refused(lib):
    assert b"ex_rowptr" in refused(lib, rp=one, col=z)
    assert b"ex_rowptr" in refused(lib, rp=z, col=one)


@pytest.mark.parametrize("nb,k", [(1, 1), (8, 20), (16, 128)])
def test_short_workspace(lib, nb, k):
    need = lib.lg_score_topk_batch_items_ws_bytes(nb, 500, 64, k)
    assert need > 0
    for ws, nbytes in ((one, need - 1), (one, 0), (z, need), (z, 0)):
        assert call(lib, n_batch=nb, k=k, ws=ws, ws_bytes=nbytes) == LG_ERR_WORKSPACE
        msg = lib.lg_last_error()
        assert ME in msg and b"workspace" in msg


def test_ws_bytes_shape(lib):
    """One partial list of k 8-byte entries per (workgroup, user): at most 512 workgroups and
    never more than 16-candidate tiles; 0 for arguments the call refuses."""
    f = lib.lg_score_topk_batch_items_ws_bytes
    assert f(8, 40, 64, 20) == 3 * 8 * 20 * 8  # 3 tiles
    assert f(16, 10**6, 64, 128) == 512 * 16 * 128 * 8
    assert f(1, 1, 32, 1) == 8
    for bad in ((0, 1000, 64, 20), (17, 1000, 64, 20), (65, 1000, 64, 20), (8, 0, 64, 20),
                (8, 2**31 - 1, 64, 20), (8, 1000, 48, 20), (8, 1000, 16, 20),
                (8, 1000, 256, 20), (8, 1000, 64, 0), (8, 1000, 64, 129)):
        assert f(*bad) == 0, bad


@pytest.mark.parametrize("cus", [1, 8, 64, 256, 304])
def test_grid_plan_fits_the_workspace(lib, cus):
    """The Python planner (ops.items_topk_grid on `cus` compute units) over catalog sizes around
    the tile and wave counts and every B and k class: positions per wave a multiple of 16, the
    grid covers n, no workgroup is empty, at most min(512, one per `waves` tiles) workgroups,
    and their partial lists fit lg_score_topk_batch_items_ws_bytes -- the bound the split of the
    workspace into values and ids rests on."""
    from lgcnhs import ops
    for n in (1, 15, 16, 17, 63, 64, 65, 1023, 8191, 8192, 8193, 10**6):
        for nb in (1, 8, 16):
            for k in (1, 32, 33, 64, 65, 128):
                blocks, waves, per_wave = ops.items_topk_grid(nb, n, k, None, cus=cus)
                what = (n, nb, k, blocks, waves, per_wave)
                assert per_wave % 16 == 0 and per_wave > 0, what
                assert blocks * waves * per_wave >= n, what
                assert (blocks - 1) * waves * per_wave < n, what
                assert 1 <= blocks <= min(512, -(-(-(-n // 16)) // waves)), what
                assert blocks * nb * k * 8 <= lib.lg_score_topk_batch_items_ws_bytes(nb, n, 64, k), what


def test_item_candidates_on_the_host():
    """ops.item_candidates: ids come back ascending and unique as int32; a bool mask gives its
    true positions; a bad id, a float or a mask of the wrong length raises before anything
    touches a device; an empty set is allowed."""
    import torch
    from lgcnhs import ops
    t = ops.item_candidates([7, 3, 9, 3, 0], 10, "cpu")
    assert t.dtype == torch.int32 and t.tolist() == [0, 3, 7, 9]
    assert ops.item_candidates(np.array([5, 1, 5]), 10, "cpu").tolist() == [1, 5]
    assert ops.item_candidates(torch.tensor([9, 2]), 10, "cpu").tolist() == [2, 9]
    mask = np.zeros(10, dtype=bool)
    mask[[2, 5, 9]] = True
    for m in (mask, torch.as_tensor(mask), mask.tolist()):
        t = ops.item_candidates(m, 10, "cpu")
        assert t.dtype == torch.int32 and t.tolist() == [2, 5, 9]
    with pytest.raises(ValueError, match="item id"):
        ops.item_candidates([0, -1], 10, "cpu")
    with pytest.raises(ValueError, match="item id"):
        ops.item_candidates([0, 10], 10, "cpu")
    with pytest.raises(ValueError, match="integers"):
        ops.item_candidates([0.5, 1.0], 10, "cpu")
    with pytest.raises(ValueError, match="mask"):
        ops.item_candidates(np.ones(9, dtype=bool), 10, "cpu")
    e = ops.item_candidates([], 10, "cpu")
    assert e.dtype == torch.int32 and e.numel() == 0
    assert ops.item_candidates(np.zeros(10, dtype=bool), 10, "cpu").numel() == 0
