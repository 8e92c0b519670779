"""Dirty-memory harness: what a result would be if every uninitialised allocation of the
library came back holding somebody else's data.

``torch.empty``, ``torch.empty_like`` and ``Tensor.new_empty`` (the only uninitialised
allocations lgcnhs makes) are patched for the duration of a ``with`` block:

    with record() as rec:            # the decoy problem: calls go through, tensors are kept
        decoy()
    with replay(rec) as h:           # the real problem starts from the decoy's final buffers
        out = real()
    h.assert_consumed()
    with fill_bytes(0xFF) as h:      # every allocation 0xFF: NaN floats, -1 ids, set masks
        out = real()
    h.assert_used()

Replay demands the same allocation sequence (shape, dtype, device) from both runs and raises
PoisonError otherwise. Only CUDA allocations are intercepted unless ``cuda_only=False``. Do not
enter any of these around a hipGraph capture: the fills are extra kernels on the stream.
"""
from __future__ import annotations

import contextlib

import torch


class PoisonError(AssertionError):
    """The harness itself was misused or the allocation sequences differ."""


class Harness:
    def __init__(self, mode: str, recording=None, byte: int = 0xFF, cuda_only: bool = True):
        self.mode, self.byte, self.cuda_only = mode, int(byte) & 0xFF, cuda_only
        self.source = recording
        self.tensors: list = []   # record: every intercepted tensor, in call order
        self.keys: list = []      # (shape, dtype, device) of each
        self.count = 0            # intercepted allocations
        self._busy = False

    # -- what one intercepted allocation becomes
    def _handle(self, t: torch.Tensor) -> torch.Tensor:
        if self.cuda_only and not t.is_cuda:
            return t
        key = (tuple(t.shape), t.dtype, t.device)
        i = self.count
        self.count += 1
        if self.mode == "record":
            self.tensors.append(t)
            self.keys.append(key)
        elif self.mode == "replay":
            src = self.source
            if i >= len(src.keys):
                raise PoisonError(f"allocation {i} {key}: the recording has only "
                                  f"{len(src.keys)} allocations")
            if src.keys[i] != key:
                raise PoisonError(f"allocation {i} is {key}, the recording has {src.keys[i]}")
            if t.numel():
                # (bytes, not values: NaN payloads and every integer survive)
                _bytes(t).copy_(_bytes(src.tensors[i]))
        else:
            if t.numel():
                _bytes(t).fill_(self.byte)
        return t

    def _wrap(self, fn):
        def patched(*args, **kwargs):
            t = fn(*args, **kwargs)
            if self._busy or not isinstance(t, torch.Tensor):
                return t
            self._busy = True  # (fills below may allocate through the patched names)
            try:
                return self._handle(t)
            finally:
                self._busy = False
        patched.__wrapped__ = fn
        return patched

    # -- what a test asserts afterwards
    def assert_used(self) -> None:
        if self.count <= 0:
            raise PoisonError("no allocation was intercepted")

    def assert_consumed(self) -> None:
        self.assert_used()
        if self.mode == "replay" and self.count != len(self.source.keys):
            raise PoisonError(f"{self.count} allocations replayed, {len(self.source.keys)} "
                              f"recorded")


def _bytes(t: torch.Tensor) -> torch.Tensor:
    """A flat uint8 view of the memory of a freshly allocated (dense) tensor."""
    flat = torch.tensor([], dtype=torch.uint8, device=t.device)
    return flat.set_(t.untyped_storage(), t.storage_offset() * t.element_size(),
                     (t.numel() * t.element_size(),), (1,))


_PATCHED = (("empty", torch), ("empty_like", torch), ("new_empty", torch.Tensor))


@contextlib.contextmanager
def _patched(h: Harness):
    saved = [(owner, name, getattr(owner, name)) for name, owner in _PATCHED]
    for owner, name, fn in saved:
        if hasattr(fn, "__wrapped__"):
            raise PoisonError("poison harness entered twice")
    try:
        for owner, name, fn in saved:
            setattr(owner, name, h._wrap(fn))
        yield h
    finally:
        for owner, name, fn in saved:
            setattr(owner, name, fn)


def record(cuda_only: bool = True):
    return _patched(Harness("record", cuda_only=cuda_only))


def replay(recording: Harness, cuda_only: bool = True):
    if not isinstance(recording, Harness) or recording.mode != "record":
        raise PoisonError("replay() takes the harness of a finished record() block")
    return _patched(Harness("replay", recording, cuda_only=cuda_only))


def fill_bytes(byte: int = 0xFF, cuda_only: bool = True):
    return _patched(Harness("bytes", byte=byte, cuda_only=cuda_only))


def bit_equal(a, b) -> bool:
    """Tensors (or nested tuples of them) equal in shape, dtype and every byte."""
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(bit_equal(x, y) for x, y in zip(a, b))
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    a, b = a.contiguous(), b.contiguous()
    return a.numel() == 0 or bool(torch.equal(_bytes(a), _bytes(b)))


def three_ways(real, decoy, check, same=bit_equal, cuda_only: bool = True):
    """real() plain, then started from decoy()'s final buffers, then from 0xFF bytes -- the byte
    fill runs only once the replay has passed. check(out, how) compares one result with the
    independent reference; same(a, b) relates the poisoned results to the plain one (bit
    equality unless the caller has a reason). Returns the three results."""
    plain = real()
    check(plain, "plain")
    with record(cuda_only) as rec:
        decoy()
    rec.assert_used()
    with replay(rec, cuda_only) as h:
        replayed = real()
    h.assert_consumed()
    assert same(plain, replayed), "the result depends on what the buffers held (decoy replay)"
    check(replayed, "replay")
    with fill_bytes(0xFF, cuda_only) as h:
        filled = real()
    h.assert_used()
    assert same(plain, filled), "the result depends on what the buffers held (0xFF fill)"
    check(filled, "0xFF")
    return plain, replayed, filled
