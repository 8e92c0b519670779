"""K2w (full-catalog top-K for k <= 1024), C ABI side: lg_score_topk_wide_ws_bytes and
lg_score_topk_wide_f32 are exported by both libraries, refuse every bad call before any
launch with the entry's name in lg_last_error(), and size the workspace by the slab shape.
CPU only (no kernel runs)."""
import ctypes

import pytest

NAMES = ("lg_score_topk_wide_ws_bytes", "lg_score_topk_wide_f32")
LG_OK, LG_ERR_ARG, LG_ERR_WORKSPACE = 0, 1, 3
ME = b"lg_score_topk_wide_f32"

z = ctypes.c_void_p(0)
one = ctypes.c_void_p(16)  # never dereferenced: validation fails first
odd = ctypes.c_void_p(20)  # not 8-byte aligned


@pytest.fixture(scope="module")
def lib():
    from lgcnhs import _native as N
    return N.load_library()


def call(lib, eu=one, ei=one, n_users=10, n_items=1000, dim=64, rp=z, col=z, k=200, ns=1,
         val=one, idx=one, ws=one, ws_bytes=1 << 40):
    return lib.lg_score_topk_wide_f32(eu, ei, n_users, n_items, dim, rp, col, -1024.0, k, ns,
                                      val, idx, ws, ws_bytes, z)


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
    for name in ("eu", "ei", "val", "idx"):
        assert b"null" in refused(lib, **{name: z})


def test_bad_dim_k_and_splits_are_refused(lib):
    for dim in (0, 16, 48, 256):
        assert b"dim" in refused(lib, dim=dim)
    for k in (0, -1, 1025, 4096):
        assert b"k=" in refused(lib, k=k)
    for ns in (0, -3, 4097):
        assert b"n_splits" in refused(lib, ns=ns)
    assert b"n_items" in refused(lib, n_items=0)


def test_half_set_exclusion_pair_is_refused(lib):
    assert b"ex_rowptr" in refused(lib, rp=one, col=z)
    assert b"ex_rowptr" in refused(lib, rp=z, col=one)


def test_misaligned_workspace_is_refused(lib):
    assert b"aligned" in refused(lib, ws=odd)
    # ... even for an empty call: every bad argument is reported before anything else
    assert b"aligned" in refused(lib, ws=odd, n_users=0)


@pytest.mark.parametrize("k", [1, 128, 129, 1024])
def test_short_workspace(lib, k):
    need = lib.lg_score_topk_wide_ws_bytes(10, 1000, 64, k, 1)
    assert need > 0
    for ws, nbytes in ((one, need - 1), (one, 0), (z, need), (z, 0)):
        assert call(lib, k=k, ws=ws, ws_bytes=nbytes) == LG_ERR_WORKSPACE
        msg = lib.lg_last_error()
        assert ME in msg and b"workspace" in msg


def test_empty_call_is_ok(lib):
    assert call(lib, n_users=0) == LG_OK
    assert call(lib, n_users=0, ws=z, ws_bytes=0) == LG_OK
    assert call(lib, n_users=0, k=1024, ns=7) == LG_OK


def test_ws_bytes_shape(lib):
    """One slab of 512 / 1024 / 2048 8-byte entries per (split, user) for k <= 256 / 512 /
    1024: steps at 256 -> 257 and 512 -> 513, flat in between, linear in users, monotone in
    n_splits, and 0 for arguments the call refuses."""
    f = lib.lg_score_topk_wide_ws_bytes
    U, I = 100, 100_000
    for k, cap in ((1, 512), (128, 512), (129, 512), (256, 512), (257, 1024), (512, 1024),
                   (513, 2048), (1024, 2048)):
        assert f(U, I, 64, k, 1) == U * cap * 8, k
        assert f(U, I, 128, k, 3) == 3 * U * cap * 8, k
        assert f(3 * U, I, 32, k, 1) == 3 * U * cap * 8, k
    prev = 0
    for ns in (1, 2, 3, 4, 7, 16, 64, 4096):
        cur = f(U, I, 64, 300, ns)
        assert cur >= prev and cur % (U * 1024 * 8) == 0
        prev = cur
    assert f(U, I, 64, 300, 2) == 2 * f(U, I, 64, 300, 1)
    # (a tiny catalog has fewer 16-item splits than asked for: never more slabs than splits)
    assert f(U, 40, 64, 300, 64) == 3 * U * 1024 * 8
    for bad in ((0, I, 64, 300, 1), (U, 0, 64, 300, 1), (U, I, 64, 0, 1), (U, I, 64, 1025, 1),
                (U, I, 64, 300, 0), (U, I, 64, 300, 4097)):
        assert f(*bad) == 0, bad
    # 1M users x 2048 entries: the byte count passes 2^32 (64-bit sizes)
    assert f(1 << 20, 1_000_000, 64, 1024, 1) == (1 << 20) * 2048 * 8
