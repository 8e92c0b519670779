"""K4w (spreading top-K for k <= 1024), C ABI side: lg_rows_topk_wide_f64 and
lg_topk_lists_merge_wide_f64 are exported by both libraries and refuse every bad call before
any launch, with the entry's own name in lg_last_error(). CPU only (no kernel runs)."""
import ctypes

import pytest

ROWS, MERGE = b"lg_rows_topk_wide_f64", b"lg_topk_lists_merge_wide_f64"
LG_OK, LG_ERR_ARG = 0, 1
DROP, NONE = 0, 1

z = ctypes.c_void_p(0)
one = ctypes.c_void_p(16)  # never dereferenced: validation fails first


@pytest.fixture(scope="module")
def lib():
    from lgcnhs import _native as N
    return N.load_library()


def rows(lib, F=one, ldf=300, n_rows=4, n_cols=300, eu=z, ei=z, dim=0, rp=z, col=z, mode=DROP,
         k=200, val=one, idx=one):
    return lib.lg_rows_topk_wide_f64(F, ldf, n_rows, n_cols, eu, ei, dim, rp, col, mode, k, val,
                                     idx, z)


def merge(lib, iv=one, ii=one, n_lists=2, n_rows=4, k=200, ov=one, oi=one):
    return lib.lg_topk_lists_merge_wide_f64(iv, ii, n_lists, n_rows, k, ov, oi, z)


def refused(lib, fn, me, **kw):
    assert fn(lib, **kw) == LG_ERR_ARG, kw
    msg = lib.lg_last_error()
    assert msg.startswith(me), (kw, msg)
    return msg


def test_exported_by_both_libraries():
    from lgcnhs import _native as N
    prod, ref = N.load_library(), N.ref_lib()
    assert N.ABI_VERSION == 17 == prod.lg_abi_version() == ref.lg_abi_version()
    for name in (ROWS.decode(), MERGE.decode()):
        assert name in N.SIGNATURES, name
        assert hasattr(prod, name), name
        assert hasattr(ref, name), name
    assert N.SIGNATURES[ROWS.decode()] == N.SIGNATURES["lg_rows_topk_f64"]
    assert N.SIGNATURES[MERGE.decode()] == N.SIGNATURES["lg_topk_lists_merge_f64"]


def test_null_pointers_are_refused(lib):
    for name in ("F", "val", "idx"):
        refused(lib, rows, ROWS, **{name: z})
    for name in ("iv", "ii", "ov", "oi"):
        refused(lib, merge, MERGE, **{name: z})


@pytest.mark.parametrize("k", [0, -1, 1025])
def test_bad_k_is_refused(lib, k):
    assert b"k=%d" % k in refused(lib, rows, ROWS, k=k)
    assert b"k=%d" % k in refused(lib, merge, MERGE, k=k)
    # ... for an empty call too: every bad argument is reported before anything else
    assert b"k=%d" % k in refused(lib, rows, ROWS, k=k, n_rows=0)
    assert b"k=%d" % k in refused(lib, merge, MERGE, k=k, n_rows=0)


def test_rows_bad_shapes_are_refused(lib):
    refused(lib, rows, ROWS, ldf=299)
    refused(lib, rows, ROWS, n_rows=-1)
    refused(lib, rows, ROWS, n_cols=-1, ldf=0)
    refused(lib, rows, ROWS, n_cols=2**31 - 1, ldf=2**31)
    refused(lib, rows, ROWS, n_cols=2**31, ldf=2**31)


def test_rows_g_factor_arguments(lib):
    assert b"eu/ei" in refused(lib, rows, ROWS, eu=one, ei=z, dim=64)
    assert b"eu/ei" in refused(lib, rows, ROWS, eu=z, ei=one, dim=64)
    for dim in (0, 16, 48, 256):
        assert b"dim" in refused(lib, rows, ROWS, eu=one, ei=one, dim=dim)


def test_rows_exclusion_arguments(lib):
    for mode in (-1, 2, 7):
        assert b"excl_mode" in refused(lib, rows, ROWS, mode=mode)
    assert b"ex_rowptr" in refused(lib, rows, ROWS, rp=one, col=z)
    assert b"ex_rowptr" in refused(lib, rows, ROWS, rp=z, col=one)
    assert b"LG_EXCL_DROP" in refused(lib, rows, ROWS, eu=one, ei=one, dim=64, rp=one, col=one,
                                      mode=NONE)


def test_merge_bad_sizes_are_refused(lib):
    refused(lib, merge, MERGE, n_lists=0)
    refused(lib, merge, MERGE, n_rows=-1)


def test_empty_calls_are_ok(lib):
    for k in (1, 128, 129, 1024):
        assert rows(lib, n_rows=0, k=k) == LG_OK
        assert rows(lib, n_rows=0, k=k, eu=one, ei=one, dim=128, rp=one, col=one) == LG_OK
        assert merge(lib, n_rows=0, k=k) == LG_OK


def test_stale_library_names_the_missing_symbol(monkeypatch):
    """A library built before an entry existed keeps the ABI number (additions do not bump
    it): loading it says which symbol is missing and to rebuild."""
    from lgcnhs import _native as N
    monkeypatch.setattr(N, "_lib", None)
    monkeypatch.setitem(N.SIGNATURES, "lg_not_built_yet", (ctypes.c_int, []))
    with pytest.raises(RuntimeError, match="lg_not_built_yet.*rebuild"):
        N.load_library()
    assert N._lib is None
