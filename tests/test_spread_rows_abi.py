"""K3r (spreading for item baskets outside the graph, csrc/spread_rows.hip), C ABI side:
lg_spread_rows_weight_f64 / lg_spread_rows_resource_f64, their workspace sizes and
LG_SPREAD_ROWS_BLOCK / LG_SPREAD_ROWS_SEG exist in the header, both libraries and the binding;
each entry refuses every bad call before any launch with status 1 and its own name and the
argument in lg_last_error(). CPU only (no kernel runs)."""
import ctypes
import os
import re

import pytest

LG_OK, LG_ERR_ARG = 0, 1
NAMES = ("lg_spread_rows_weight_ws_bytes", "lg_spread_rows_weight_f64",
         "lg_spread_rows_resource_ws_bytes", "lg_spread_rows_resource_f64")

z = ctypes.c_void_p(0)
one = ctypes.c_void_p(16)  # never dereferenced: validation fails first
BIG = 1 << 40              # a workspace size that every check passes


@pytest.fixture(scope="module")
def lib():
    from lgcnhs import _native as N
    return N.load_library()


def weight(lib, u_rp=one, u_items=one, n_users=100, n_items=50, ra=one, inv=one, b_rp=one,
           b_items=one, nb=4, long_ids=z, long_ptr=z, n_long=0, n_units=0, T=one, marks=one,
           ws=one, ws_bytes=BIG):
    return lib.lg_spread_rows_weight_f64(u_rp, u_items, n_users, n_items, ra, inv, b_rp, b_items,
                                         nb, long_ids, long_ptr, n_long, n_units, T, marks, ws,
                                         ws_bytes, z)


def resource(lib, i_rp=one, i_users=one, n_items=50, n_users=100, T=one, marks=one, rb=one,
             nb=4, long_ids=z, long_ptr=z, n_long=0, n_units=0, F=one, ldf=50, ws=one,
             ws_bytes=BIG):
    return lib.lg_spread_rows_resource_f64(i_rp, i_users, n_items, n_users, T, marks, rb, nb,
                                           long_ids, long_ptr, n_long, n_units, F, ldf, ws,
                                           ws_bytes, z)


ENTRIES = {"lg_spread_rows_weight_f64": weight, "lg_spread_rows_resource_f64": resource}


def refused(lib, name, **kw):
    """Status 1 with the entry's own name in the message. (A call that got past the checks
    would launch on the never-dereferenced pointers.)"""
    assert ENTRIES[name](lib, **kw) == LG_ERR_ARG, (name, kw)
    msg = lib.lg_last_error()
    assert name.encode() in msg, (kw, msg)
    return msg


def test_exported_by_both_libraries_and_bound():
    from lgcnhs import _native as N
    prod, ref = N.load_library(), N.ref_lib()
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(repo, "include", "lgcnhs.h")) as f:
        header = f.read()
    for name in NAMES:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in N.SIGNATURES
        assert hasattr(prod, name) and hasattr(ref, name)
    assert N.ABI_VERSION == 17 and prod.lg_abi_version() == 17  # entries added, none changed
    assert ref.lg_abi_version() == 17
    assert len(N.SIGNATURES["lg_spread_rows_weight_f64"][1]) == 18
    assert len(N.SIGNATURES["lg_spread_rows_resource_f64"][1]) == 17
    assert N.SIGNATURES["lg_spread_rows_weight_ws_bytes"][0] is ctypes.c_size_t
    assert N.SIGNATURES["lg_spread_rows_resource_ws_bytes"][0] is ctypes.c_size_t


def test_constants_are_the_headers():
    from lgcnhs import _native as N
    from lgcnhs import ops
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(repo, "include", "lgcnhs.h")) as f:
        header = f.read()
    blk = int(re.search(r"#define LG_SPREAD_ROWS_BLOCK (\d+)", header).group(1))
    seg = int(re.search(r"#define LG_SPREAD_ROWS_SEG (\d+)", header).group(1))
    assert blk == N.LG_SPREAD_ROWS_BLOCK == ops.SPREAD_ROWS_BLOCK
    assert seg == N.LG_SPREAD_ROWS_SEG == ops.SPREAD_ROWS_SEG
    assert blk in (32, 64) and seg % 64 == 0


def test_workspace_sizes(lib):
    from lgcnhs import _native as N
    assert lib.lg_spread_rows_weight_ws_bytes(0, 0) == 0
    assert lib.lg_spread_rows_weight_ws_bytes(-5, -1) == 0
    assert lib.lg_spread_rows_weight_ws_bytes(1000, 0) == 8000  # one basket word per item
    per_unit = N.LG_SPREAD_ROWS_BLOCK * 8                       # a partial sum per basket
    assert lib.lg_spread_rows_weight_ws_bytes(1000, 3) == 8000 + 3 * per_unit
    assert lib.lg_spread_rows_resource_ws_bytes(0) == 0
    assert lib.lg_spread_rows_resource_ws_bytes(7) == 7 * per_unit


def test_null_pointers_are_refused(lib):
    for name in ("u_rp", "u_items", "ra", "inv", "b_rp", "b_items", "T", "marks"):
        assert b"null" in refused(lib, "lg_spread_rows_weight_f64", **{name: z})
    for name in ("i_rp", "i_users", "T", "marks", "rb", "F"):
        assert b"null" in refused(lib, "lg_spread_rows_resource_f64", **{name: z})


@pytest.mark.parametrize("name", list(ENTRIES))
def test_block_size_is_refused(lib, name):
    from lgcnhs import _native as N
    for nb in (0, -1, N.LG_SPREAD_ROWS_BLOCK + 1, 1 << 20):
        assert b"n_baskets" in refused(lib, name, nb=nb)
    assert b"n_baskets" not in (refused(lib, name, nb=N.LG_SPREAD_ROWS_BLOCK, n_users=-1))


@pytest.mark.parametrize("name", list(ENTRIES))
def test_bad_sizes_are_refused(lib, name):
    assert b"n_users" in refused(lib, name, n_users=-1)
    assert b"n_items" in refused(lib, name, n_items=-1)
    assert b"n_users" in refused(lib, name, n_users=2**31 - 1)   # int32 ids
    ldf = {"ldf": 2**31 - 1} if name == "lg_spread_rows_resource_f64" else {}
    assert b"n_items" in refused(lib, name, n_items=2**31 - 1, **ldf)


def test_short_row_stride_is_refused(lib):
    assert b"ldf" in refused(lib, "lg_spread_rows_resource_f64", ldf=49)
    assert b"ldf" in refused(lib, "lg_spread_rows_resource_f64", ldf=-1)


@pytest.mark.parametrize("name", list(ENTRIES))
def test_long_list_table_is_refused(lib, name):
    assert b"n_long" in refused(lib, name, n_long=-1)
    assert b"n_long" in refused(lib, name, n_units=-1)
    assert b"n_long" in refused(lib, name, n_long=2, n_units=0, long_ids=one, long_ptr=one)
    assert b"n_long" in refused(lib, name, n_long=0, n_units=3)
    assert b"n_long" in refused(lib, name, n_long=3, n_units=2, long_ids=one, long_ptr=one)
    assert b"long_ids" in refused(lib, name, n_long=1, n_units=2, long_ids=z, long_ptr=one)
    assert b"long_ptr" in refused(lib, name, n_long=1, n_units=2, long_ids=one, long_ptr=z)


def test_short_workspace_is_refused(lib):
    need = lib.lg_spread_rows_weight_ws_bytes(50, 2)
    kw = dict(n_long=1, n_units=2, long_ids=one, long_ptr=one)
    assert b"ws_bytes" in refused(lib, "lg_spread_rows_weight_f64", ws_bytes=need - 1, **kw)
    assert b"ws_bytes" in refused(lib, "lg_spread_rows_weight_f64", ws=z, **kw)
    assert b"ws_bytes" in refused(lib, "lg_spread_rows_weight_f64", ws_bytes=0)
    need = lib.lg_spread_rows_resource_ws_bytes(2)
    assert b"ws_bytes" in refused(lib, "lg_spread_rows_resource_f64", ws_bytes=need - 1, **kw)
    assert b"ws_bytes" in refused(lib, "lg_spread_rows_resource_f64", ws=z, **kw)


def test_nothing_to_do_is_ok(lib):
    """No users (pass 1) / no items (pass 2) pass the checks and launch nothing; without long
    lists pass 2 needs no workspace at all. A bad argument is still refused first."""
    assert weight(lib, n_users=0) == LG_OK
    assert resource(lib, n_items=0, ldf=0) == LG_OK
    assert resource(lib, n_items=0, ldf=0, ws=z, ws_bytes=0) == LG_OK
    assert b"n_baskets" in refused(lib, "lg_spread_rows_weight_f64", n_users=0, nb=65)
    assert b"ldf" in refused(lib, "lg_spread_rows_resource_f64", n_items=0, ldf=-1)
