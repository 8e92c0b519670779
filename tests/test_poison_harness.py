"""The dirty-memory harness of tests/_poison.py, on CPU tensors (cuda_only=False): a toy that
reads what it never wrote is caught by decoy replay and by the byte fill, a toy that writes
first is not, differing allocation sequences raise, and the patch never outlives its block."""
import pytest
import torch

import _poison as P

_EMPTY, _EMPTY_LIKE, _NEW_EMPTY = torch.empty, torch.empty_like, torch.Tensor.new_empty


def _unpatched() -> bool:
    return (torch.empty is _EMPTY and torch.empty_like is _EMPTY_LIKE
            and torch.Tensor.new_empty is _NEW_EMPTY)


def _leaky(x: torch.Tensor) -> torch.Tensor:
    """Sums x into a buffer whose last slot it never writes (a stale list tail)."""
    buf = torch.empty(x.numel() + 1, dtype=x.dtype)
    buf[:-1] = x
    return buf.sum()


def _clean(x: torch.Tensor) -> torch.Tensor:
    buf = torch.empty_like(x)
    buf.copy_(x)
    ids = x.new_empty(3, dtype=torch.int64)
    ids[:] = torch.arange(3)
    return buf.sum() + ids.sum()


def _run(fn, x, decoy_x):
    with P.record(cuda_only=False) as rec:
        fn(decoy_x)
    with P.replay(rec, cuda_only=False) as h:
        r = fn(x)
    h.assert_consumed()
    with P.fill_bytes(0xFF, cuda_only=False) as b:
        f = fn(x)
    b.assert_used()
    return rec, r, f


def test_replay_and_bytes_catch_a_leak():
    x = torch.arange(1.0, 6.0)
    want = x.sum()
    rec, r, f = _run(_leaky, x, x * 64)
    assert rec.count == 1 and rec.keys[0] == ((6,), torch.float32, torch.device("cpu"))
    # the stale slot of the decoy's buffer was never written either: poison the recording the way
    # a recycled block would be, and the leak shows as a plausible wrong number
    rec.tensors[0][-1] = 4096.0
    with P.replay(rec, cuda_only=False):
        r = _leaky(x)
    assert r.item() == want.item() + 4096.0
    assert torch.isnan(f)  # (0xFF bytes read as NaN in every float format)
    assert _unpatched()


def test_byte_fill_values():
    with P.fill_bytes(0xFF, cuda_only=False) as h:
        got = [torch.empty(4, dtype=dt) for dt in (torch.float16, torch.bfloat16, torch.float32,
                                                   torch.float64)]
        ints = [torch.empty((2, 3), dtype=dt) for dt in (torch.int32, torch.int64)]
        mask = torch.empty(5, dtype=torch.uint8)
        like = torch.empty_like(torch.zeros(3, 2).t())  # (a dense, permuted layout)
    assert h.count == 8
    assert all(bool(torch.isnan(t).all()) for t in got + [like])
    assert all(bool((t == -1).all()) for t in ints) and bool((mask == 255).all())


def test_three_ways_flags_the_leak_and_passes_the_clean_toy():
    x = torch.arange(1.0, 6.0)

    def check(out, how):
        assert out.item() == 18.0, how

    plain, r, f = P.three_ways(lambda: _clean(x), lambda: _clean(x * 64), check,
                               cuda_only=False)
    assert P.bit_equal(plain, r) and P.bit_equal(plain, f)

    def decoy():  # the decoy leaves a dominating stale value where the real run never writes
        buf = torch.empty(6)
        buf.fill_(4096.0)

    with pytest.raises(AssertionError, match="depends on what the buffers held"):
        P.three_ways(lambda: _leaky(x), decoy, lambda out, how: None, cuda_only=False)
    assert _unpatched()


def test_sequence_mismatch_raises():
    x = torch.arange(1.0, 6.0)
    with P.record(cuda_only=False) as rec:
        _clean(x)
    assert rec.count == 2
    with pytest.raises(P.PoisonError, match="allocation 0 is"):
        with P.replay(rec, cuda_only=False):
            _clean(x[:4])  # another shape
    with pytest.raises(P.PoisonError, match="has only 2"):
        with P.replay(rec, cuda_only=False):
            _clean(x)
            torch.empty(1)  # one allocation too many
    with P.replay(rec, cuda_only=False) as h:
        torch.empty_like(x)  # one too few
    with pytest.raises(P.PoisonError, match="1 allocations replayed, 2 recorded"):
        h.assert_consumed()
    assert _unpatched()


def test_dtype_mismatch_raises():
    x = torch.arange(1.0, 6.0)
    with P.record(cuda_only=False) as rec:
        _clean(x)
    with pytest.raises(P.PoisonError, match="allocation 1 is"):
        with P.replay(rec, cuda_only=False):
            torch.empty_like(x)
            x.new_empty(3, dtype=torch.float32)
    assert _unpatched()


def test_patch_removed_after_an_exception_and_not_nested():
    with pytest.raises(ZeroDivisionError):
        with P.fill_bytes(cuda_only=False):
            assert not _unpatched()
            1 / 0
    assert _unpatched()
    with pytest.raises(P.PoisonError, match="entered twice"):
        with P.record(cuda_only=False):
            with P.record(cuda_only=False):
                pass
    assert _unpatched()
    with P.fill_bytes(cuda_only=False) as h:  # nothing allocated: the count says so
        pass
    with pytest.raises(P.PoisonError, match="no allocation"):
        h.assert_used()


def test_cpu_allocations_pass_by_default():
    with P.fill_bytes() as h:
        t = torch.empty(3)
    assert h.count == 0 and t.shape == (3,)
