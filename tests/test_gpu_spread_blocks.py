"""The dense spreading routes with F in several blocks (ops._f_blocks): spread_recommend for all
users and for users=, the gather route of items= and spread_rank cut F by ops.F_BLOCK_BYTES,
which at test shapes holds every user at once. With the constant patched down to 24 rows of F
the 70 users take three blocks (24, 24, 22) through one buffer, and every result must be the
one-block call's, bit for bit. The blocks are counted on the native entry itself."""
import numpy as np
import pytest
import torch

import _poison as P

pytestmark = pytest.mark.gpu
DEV = "cuda"
SU, SI, SD = 70, 300, 64
BLOCK_BYTES = 24 * SI * 8            # 24 rows of fp64 F
USERS = [5, 5, 69, 0] + list(range(40))  # 44 rows: blocks of 24 and 20
_CASE = {}


def _case():
    """A 70-user x 300-item random graph of density 0.08, d = 64 embeddings scaled by 0.1,
    0 .. 6 held-out targets per user, every third item as candidates, W for lambda = 0.4."""
    if not _CASE:
        from lgcnhs import ops
        from lgcnhs.graph import RowSets
        rng = np.random.default_rng(29)
        An = rng.random((SU, SI)) < 0.08
        u, i = np.nonzero(An)
        A = ops.Interactions.from_pairs(torch.as_tensor(u), torch.as_tensor(i), SU, SI, DEV)
        rows = [np.sort(rng.permutation(np.nonzero(~An[r])[0])[:r % 7]) for r in range(SU)]
        trp = np.cumsum([0] + [len(t) for t in rows]).astype(np.int64)
        tg = RowSets(torch.as_tensor(trp).to(DEV),
                     torch.as_tensor(np.concatenate(rows).astype(np.int32)).to(DEV), SU, SI)
        eu = torch.as_tensor((rng.standard_normal((SU, SD)) * 0.1).astype(np.float32)).to(DEV)
        ei = torch.as_tensor((rng.standard_normal((SI, SD)) * 0.1).astype(np.float32)).to(DEV)
        _CASE.update(A=A, tg=tg, W=ops.spread_hybrid(A, 0.4), g={False: (None, None),
                                                                  True: (eu, ei)},
                     cand=ops.item_candidates(list(range(0, SI, 3)), SI, DEV))
    return _CASE


def _blocks(monkeypatch, patched, fn):
    """(fn()'s result, the row counts of its lg_spread_resource_f64 calls), with
    F_BLOCK_BYTES patched down to 24 rows or left alone."""
    from lgcnhs import _native as N
    from lgcnhs import ops
    calls = []
    real = N.load_library()

    class Spy:
        def __getattr__(self, name):
            entry = getattr(real, name)
            if name == "lg_spread_resource_f64":
                return lambda *a: calls.append(a[3]) or entry(*a)
            return entry
    with monkeypatch.context() as m:
        m.setattr(N, "lib", lambda: Spy())  # (counts the entry's calls, passes all on)
        if patched:
            m.setattr(ops, "F_BLOCK_BYTES", BLOCK_BYTES)
        return fn(), calls


@pytest.mark.parametrize("k", [20, 200])
@pytest.mark.parametrize("use_g", [False, True])
def test_recommend_all_users_in_three_blocks(monkeypatch, use_g, k):
    from lgcnhs import ops
    c = _case()
    A, (eu, ei) = c["A"], c["g"][use_g]

    def call():
        return ops.spread_recommend(A, 0.4, k, A.by_user, True, eu, ei, tiled=False)
    base, one = _blocks(monkeypatch, False, call)
    got, three = _blocks(monkeypatch, True, call)
    assert one == [SU] and three == [24, 24, 22]
    assert P.bit_equal(got, base)
    assert (base[1][:, :20] >= 0).all()


@pytest.mark.parametrize("k", [20, 200])
@pytest.mark.parametrize("use_g", [False, True])
def test_recommend_users_in_two_blocks(monkeypatch, use_g, k):
    from lgcnhs import ops
    c = _case()
    A, (eu, ei) = c["A"], c["g"][use_g]

    def call():
        return ops.spread_recommend(A, 0.4, k, A.by_user, True, eu, ei, tiled=False,
                                    users=USERS)
    base, one = _blocks(monkeypatch, False, call)
    got, two = _blocks(monkeypatch, True, call)
    assert one == [len(USERS)] and two == [24, 20]
    assert P.bit_equal(got, base)


@pytest.mark.parametrize("use_g", [False, True])
def test_items_gather_route_in_three_blocks(monkeypatch, use_g):
    from lgcnhs import ops
    c = _case()
    A, (eu, ei) = c["A"], c["g"][use_g]

    def call(route):
        return lambda: ops._spread_topk_items(A, c["W"], None, c["cand"], 20, A.by_user, True,
                                              eu, ei, route=route)
    base, one = _blocks(monkeypatch, False, call("gather"))
    fused, none = _blocks(monkeypatch, True, call("fused"))
    got, three = _blocks(monkeypatch, True, call("gather"))
    assert one == [SU] and none == [] and three == [24, 24, 22]
    assert P.bit_equal(got, base)
    assert P.bit_equal(got, fused)


@pytest.mark.parametrize("use_g", [False, True])
def test_spread_rank_in_three_blocks(monkeypatch, use_g):
    from lgcnhs import ops
    c = _case()
    A, (eu, ei) = c["A"], c["g"][use_g]

    def call():
        return ops.spread_rank(A, 0.4, c["tg"], A.by_user, True, eu, ei, W=c["W"])
    base, one = _blocks(monkeypatch, False, call)
    got, three = _blocks(monkeypatch, True, call)
    assert one == [SU] and three == [24, 24, 22]
    assert P.bit_equal(got, base)
    assert (base[0] >= 0).all()  # held-out items are not excluded: all of them rank
