"""K4k (the rank of given targets over dense fp64 rows, csrc/rows_rank.hip), C ABI side:
lg_rows_rank_f64 and LG_ROWS_RANK_ROW_MAX exist in the header, both libraries and the binding;
the entry refuses every bad call before any launch with its own name in lg_last_error(); no
kernel rows is LG_OK. CPU only (no kernel runs)."""
import ctypes
import os
import re

import pytest

LG_OK, LG_ERR_ARG = 0, 1
ME = b"lg_rows_rank_f64"
LG_EXCL_DROP, LG_EXCL_NONE = 0, 1

z = ctypes.c_void_p(0)
one = ctypes.c_void_p(16)  # never dereferenced: validation fails first


@pytest.fixture(scope="module")
def lib():
    from lgcnhs import _native as N
    return N.load_library()


def rows_rank(lib, F=one, ldf=1000, n_f_rows=8, n_cols=1000, eu=z, ei=z, dim=0, ex_rp=z,
              ex_col=z, excl_mode=LG_EXCL_DROP, n_krows=8, krow_f=one, t_rp=one, t_col=one,
              out_rank=one, out_val=one):
    return lib.lg_rows_rank_f64(F, ldf, n_f_rows, n_cols, eu, ei, dim, ex_rp, ex_col, excl_mode,
                                n_krows, krow_f, t_rp, t_col, out_rank, out_val, z)


def refused(lib, **kw):
    """The call is refused with LG_ERR_ARG and the entry's own name in the message. (A call
    that got past the checks would launch on the never-dereferenced pointers: n_krows > 0.)"""
    assert rows_rank(lib, **kw) == LG_ERR_ARG, kw
    msg = lib.lg_last_error()
    assert ME in msg, (kw, msg)
    return msg


def test_exported_by_both_libraries_and_bound():
    from lgcnhs import _native as N
    prod, ref = N.load_library(), N.ref_lib()
    assert "lg_rows_rank_f64" in N.SIGNATURES
    assert hasattr(prod, "lg_rows_rank_f64") and hasattr(ref, "lg_rows_rank_f64")
    assert N.ABI_VERSION == 17 and prod.lg_abi_version() == 17  # an entry added, none changed
    res, args = N.SIGNATURES["lg_rows_rank_f64"]
    assert res is ctypes.c_int and len(args) == 17


def test_row_max_is_the_headers():
    """LG_ROWS_RANK_ROW_MAX of include/lgcnhs.h and its Python mirrors agree."""
    from lgcnhs import _native as N
    from lgcnhs import ops
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(repo, "include", "lgcnhs.h")) as f:
        m = re.search(r"#define LG_ROWS_RANK_ROW_MAX (\d+)", f.read())
    assert int(m.group(1)) == N.LG_ROWS_RANK_ROW_MAX == ops.ROWS_RANK_ROW_MAX == 1024


def test_null_pointers_are_refused(lib):
    for name in ("F", "krow_f", "t_rp", "t_col", "out_rank", "out_val"):
        assert b"null" in refused(lib, **{name: z})


def test_bad_sizes_are_refused(lib):
    assert b"sizes" in refused(lib, n_f_rows=-1)
    assert b"sizes" in refused(lib, n_cols=-1)
    assert b"sizes" in refused(lib, ldf=999)            # a row stride below the row length
    assert b"sizes" in refused(lib, n_cols=2**31 - 1, ldf=2**31 - 1)  # int32 column ids
    assert b"n_krows" in refused(lib, n_krows=-1)
    assert b"n_krows" in refused(lib, n_krows=2**31 - 1)  # one block per kernel row


def test_bad_dim_is_refused(lib):
    for dim in (0, 16, 48, 256):
        assert b"dim" in refused(lib, eu=one, ei=one, dim=dim)


def test_half_set_embedding_pair_is_refused(lib):
    assert b"eu/ei" in refused(lib, eu=one, ei=z, dim=64)
    assert b"eu/ei" in refused(lib, eu=z, ei=one, dim=64)


def test_exclusion_arguments(lib):
    assert b"ex_rowptr" in refused(lib, ex_rp=one, ex_col=z)
    assert b"ex_rowptr" in refused(lib, ex_rp=z, ex_col=one)
    for mode in (-1, 2, 7):
        assert b"excl_mode" in refused(lib, excl_mode=mode)
    # G's -1024 mask would become observable: a G factor with exclusions must drop them
    assert b"LG_EXCL_DROP" in refused(lib, eu=one, ei=one, dim=64, ex_rp=one, ex_col=one,
                                      excl_mode=LG_EXCL_NONE)


def test_no_kernel_rows_is_ok(lib):
    """n_krows = 0 passes the checks and launches nothing -- with and without G, either mode."""
    assert rows_rank(lib, n_krows=0) == LG_OK
    assert rows_rank(lib, n_krows=0, eu=one, ei=one, dim=128, ex_rp=one, ex_col=one) == LG_OK
    assert rows_rank(lib, n_krows=0, ex_rp=one, ex_col=one, excl_mode=LG_EXCL_NONE) == LG_OK
    # ... but a bad argument is still refused first
    assert b"dim" in refused(lib, n_krows=0, eu=one, ei=one, dim=48)
