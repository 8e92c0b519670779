"""fp16 layer storage, C ABI side: lg_rows_f32_to_f16, lg_spmm_layer_f16 and
lg_spmm_long_rows_f16 are exported by both libraries and refuse bad calls before any launch.
CPU only (no kernel runs)."""
import ctypes

import pytest

NAMES = ("lg_rows_f32_to_f16", "lg_spmm_layer_f16", "lg_spmm_long_rows_f16")
LG_OK, LG_ERR_ARG = 0, 1
LAST = 3

z = ctypes.c_void_p(0)
one = ctypes.c_void_p(16)  # never dereferenced: validation fails first
two = ctypes.c_void_p(32)


@pytest.fixture(scope="module")
def lib():
    from lgcnhs import _native as N
    return N.load_library()


def layer(lib, xh=one, yh=z, x0=z, acc=z, out=z, n_rows=10, dim=64, mode=0, denom=1.0):
    return lib.lg_spmm_layer_f16(one, one, one, z, xh, yh, x0, acc, out, n_rows, 0, dim, mode,
                                 denom, 0, z)


def long_rows(lib, xh=one, yh=z, x0=z, acc=z, out=z, n_long=1, dim=64, mode=0, denom=1.0):
    return lib.lg_spmm_long_rows_f16(one, one, one, 2, one, one, n_long, one, one, z, xh, yh,
                                     x0, acc, out, dim, mode, denom, one, z)


def test_exported_by_both_libraries():
    from lgcnhs import _native as N
    prod, ref = N.load_library(), N.ref_lib()
    for name in NAMES:
        assert name in N.SIGNATURES, name
        assert hasattr(prod, name), name
        assert hasattr(ref, name), name


def test_unsupported_dim_is_refused(lib):
    for call, name in ((layer, b"lg_spmm_layer_f16"), (long_rows, b"lg_spmm_long_rows_f16")):
        assert call(lib, dim=48) == LG_ERR_ARG
        msg = lib.lg_last_error()
        assert b"dim" in msg and name in msg
    assert lib.lg_rows_f32_to_f16(one, 10, 48, two, z) == LG_ERR_ARG
    msg = lib.lg_last_error()
    assert b"dim" in msg and b"lg_rows_f32_to_f16" in msg
    assert b"not in {32,64,128,256}" in msg


def test_null_operand_is_refused(lib):
    assert layer(lib, xh=z) == LG_ERR_ARG
    assert b"lg_spmm_layer_f16" in lib.lg_last_error()
    assert long_rows(lib, xh=z) == LG_ERR_ARG
    assert b"lg_spmm_long_rows_f16" in lib.lg_last_error()
    assert lib.lg_rows_f32_to_f16(z, 10, 64, two, z) == LG_ERR_ARG
    assert lib.lg_rows_f32_to_f16(one, 10, 64, z, z) == LG_ERR_ARG
    assert b"lg_rows_f32_to_f16" in lib.lg_last_error()


def test_aliased_output_is_refused(lib):
    assert layer(lib, xh=one, yh=one) == LG_ERR_ARG
    assert b"alias" in lib.lg_last_error()
    assert long_rows(lib, xh=one, yh=one) == LG_ERR_ARG
    assert b"alias" in lib.lg_last_error()
    assert lib.lg_rows_f32_to_f16(one, 10, 64, one, z) == LG_ERR_ARG
    assert b"alias" in lib.lg_last_error()


def test_last_mode_needs_acc_and_out(lib):
    for call in (layer, long_rows):
        assert call(lib, yh=two, mode=LAST, denom=4.0) == LG_ERR_ARG
        assert b"acc_mode" in lib.lg_last_error()
        assert call(lib, yh=two, acc=one, mode=LAST, denom=4.0) == LG_ERR_ARG  # no out
        assert call(lib, yh=two, acc=one, out=one, mode=LAST, denom=0.0) == LG_ERR_ARG
        assert call(lib, mode=7) == LG_ERR_ARG


def test_empty_calls_are_ok(lib):
    assert layer(lib, n_rows=0) == LG_OK
    assert long_rows(lib, n_long=0) == LG_OK
    assert lib.lg_rows_f32_to_f16(one, 0, 64, two, z) == LG_OK
