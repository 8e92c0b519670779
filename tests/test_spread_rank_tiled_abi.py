"""The walk's counting finish (MODE_RANK of csrc/spread_tiled.hip), C ABI side:
lg_spread_tile_resource_rank_f64 and its constants exist in the header, both libraries and the
binding with ABI 17; the entry refuses every bad call before any launch with its own name in
lg_last_error(); no users is LG_OK. CPU only (no kernel runs)."""
import ctypes
import os
import re

import pytest

LG_OK, LG_ERR_ARG = 0, 1
ME = b"lg_spread_tile_resource_rank_f64"
VALUES, COUNTS = 0, 1

z = ctypes.c_void_p(0)
one = ctypes.c_void_p(16)  # never dereferenced: validation fails first


@pytest.fixture(scope="module")
def lib():
    from lgcnhs import _native as N
    return N.load_library()


def rank(lib, u_rp=one, u_items=one, ra=one, n_users=8, lines=one, ovf=one, null_row=1000,
         rb=one, inv_cls=one, item_begin=0, tile=256, width=256, eu=z, ei=z, dim=0, gb=z,
         n_chunks=0, qb=z, qstride=0, ex_rp=z, ex_col=z, ex_cur=z, t_rp=one, t_col=one,
         phase=COUNTS, val=one, cnt=one, n_pos=100, n_ex=0):
    return lib.lg_spread_tile_resource_rank_f64(
        u_rp, u_items, ra, n_users, lines, ovf, null_row, rb, inv_cls, item_begin, tile, width,
        eu, ei, dim, gb, n_chunks, qb, qstride, ex_rp, ex_col, ex_cur, t_rp, t_col, phase, val,
        cnt, n_pos, n_ex, z)


def refused(lib, **kw):
    """The call is refused with LG_ERR_ARG and a message. (A call that got past the checks
    would launch on the never-dereferenced pointers: n_users > 0.)"""
    assert rank(lib, **kw) == LG_ERR_ARG, kw
    msg = lib.lg_last_error()
    assert msg, kw
    return msg


def test_exported_by_both_libraries_and_bound():
    from lgcnhs import _native as N
    prod, ref = N.load_library(), N.ref_lib()
    name = ME.decode()
    assert name in N.SIGNATURES
    assert hasattr(prod, name) and hasattr(ref, name)
    assert N.ABI_VERSION == 17 and prod.lg_abi_version() == 17  # an entry added, none changed
    res, args = N.SIGNATURES[name]
    assert res is ctypes.c_int and len(args) == 30


def test_in_the_header_with_its_constants():
    from lgcnhs import _native as N
    from lgcnhs import ops
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(repo, "include", "lgcnhs.h")) as f:
        text = f.read()
    assert re.search(r"\bint lg_spread_tile_resource_rank_f64\(", text)
    m = re.search(r"#define LG_SPREAD_RANK_ROW_MAX (\d+)", text)
    assert int(m.group(1)) == N.LG_SPREAD_RANK_ROW_MAX == ops.SPREAD_RANK_ROW_MAX
    assert int(re.search(r"#define LG_SPREAD_RANK_VALUES (\d+)", text).group(1)) == \
        N.LG_SPREAD_RANK_VALUES == VALUES
    assert int(re.search(r"#define LG_SPREAD_RANK_COUNTS (\d+)", text).group(1)) == \
        N.LG_SPREAD_RANK_COUNTS == COUNTS
    assert re.search(r"#define LG_ABI_VERSION 17\b", text)


def test_null_pointers_are_refused(lib):
    for name in ("u_rp", "u_items", "ra", "lines", "ovf", "rb", "inv_cls", "t_rp", "t_col",
                 "val"):
        assert ME in refused(lib, **{name: z})
    assert b"cnt" in refused(lib, cnt=z)            # the count phase adds to it
    assert rank(lib, n_users=0, phase=VALUES, cnt=z) == LG_OK  # ... the value phase does not


def test_bad_phase_and_sizes_are_refused(lib):
    for phase in (-1, 2, 7):
        assert b"phase" in refused(lib, phase=phase)
    assert ME in refused(lib, n_users=-1)
    assert ME in refused(lib, n_users=2**31 - 1)
    assert ME in refused(lib, item_begin=-1)
    assert b"32-bit" in refused(lib, n_pos=2**31 - 1)
    assert b"32-bit" in refused(lib, n_ex=2**31 - 1)
    assert b"32-bit" in refused(lib, n_pos=-1)
    for tile, width in ((0, 0), (8193, 100), (256, 0), (256, 257)):
        assert b"tile" in refused(lib, tile=tile, width=width)
    assert b"line offsets" in refused(lib, null_row=1 << 25)


def test_mismatched_g_arguments_are_refused(lib):
    g = dict(eu=one, ei=one, dim=64, gb=one, n_chunks=4)
    assert rank(lib, n_users=0, **g) == LG_OK
    assert b"eu and ei" in refused(lib, **{**g, "ei": z})
    assert b"eu and ei" in refused(lib, **{**g, "eu": z})
    assert b"gb" in refused(lib, **{**g, "gb": z})            # the count phase screens with it
    assert rank(lib, n_users=0, phase=VALUES, **{**g, "gb": z, "n_chunks": 0}) == LG_OK
    assert b"gb" in refused(lib, gb=one, n_chunks=4)          # bounds without embeddings
    for dim in (0, 16, 48, 256):
        assert b"dim" in refused(lib, **{**g, "dim": dim})
    assert b"n_chunks" in refused(lib, **{**g, "n_chunks": 3})
    assert b"qb" in refused(lib, **{**g, "qb": one, "qstride": 255})
    assert b"qb" in refused(lib, qb=one, qstride=256)
    assert b"4096" in refused(lib, tile=8192, width=4097, **{**g, "n_chunks": 65})


def test_exclusion_arguments_go_together(lib):
    for combo in (dict(ex_rp=one), dict(ex_col=one), dict(ex_cur=one),
                  dict(ex_rp=one, ex_col=one), dict(ex_rp=one, ex_cur=one)):
        assert b"ex_rowptr" in refused(lib, **combo)
    assert rank(lib, n_users=0, ex_rp=one, ex_col=one, ex_cur=one, n_ex=5) == LG_OK


def test_no_users_is_ok(lib):
    assert rank(lib, n_users=0) == LG_OK
    assert rank(lib, n_users=0, phase=VALUES) == LG_OK
    assert b"phase" in refused(lib, n_users=0, phase=3)  # a bad argument is still refused first
