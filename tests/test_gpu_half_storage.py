"""fp16 layer storage on the GPU (lg_rows_f32_to_f16, lg_spmm_layer_f16,
lg_spmm_long_rows_f16, ops.propagate(store=torch.float16), LightGCN.layer_storage).

The contract is exact: the fp32 sums of a float16-operand layer are lg_spmm_layer_f32's on the
widened operand bit for bit (ordinary and hub rows), the next operand is their round to
nearest even, and the layer mean runs in fp32 on the unrounded sums. So every kernel test
compares bitwise against the fp32 kernels; the end-to-end tests hold the result against the
reference fixtures (the project's 1e-4) and against an a-priori error bound."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
TOL = 1e-4
DEV = "cuda"
F16 = torch.float16
U, I, E = 3000, 2000, 60000


def _bits(t):
    return t.contiguous().view(torch.int16)


def _assert_f16_equal(got, want):
    """Bitwise, NaN compared by isnan."""
    assert got.dtype == F16 and want.dtype == F16 and got.shape == want.shape
    gn, wn = torch.isnan(got), torch.isnan(want)
    assert torch.equal(gn, wn)
    assert torch.equal(_bits(got)[~gn], _bits(want)[~wn])


@functools.lru_cache(maxsize=None)
def _graph(dist):
    from lgcnhs.graph import Adjacency
    from lgcnhs.synth import synth_interactions
    users, items = synth_interactions(U, I, E, seed=7, dist=dist)
    return Adjacency.from_interactions(torch.as_tensor(users), torch.as_tensor(items), U, I, DEV)


def _randn(n, d, seed, std=0.1):
    return (torch.randn(n, d, generator=torch.Generator().manual_seed(seed)) * std).to(DEV)


def _modes():
    from lgcnhs import _native as N
    return (N.LG_ACC_NONE, N.LG_ACC_FIRST, N.LG_ACC_MID, N.LG_ACC_LAST, N.LG_ACC_ONLY)


def _check_layer(adj, xh, plan=None, rows=None, modes=None):
    """One layer through the float16 entries against the fp32 entries on xh.float(): every acc
    mode with a y, and (but NONE) without one; x0 / acc / out prepared identically. ``rows`` =
    (first row, end row): a row-sliced call on the slice's own rowptr. Rows a call does not
    own keep their initial values in both runs, so whole arrays are compared."""
    from lgcnhs import ops, _native as N
    n, d = xh.shape
    lb, le = rows or (0, n)
    rowptr = adj.rowptr[lb:le + 1].contiguous()
    x32 = xh.float()
    x0 = _randn(n, d, 11)
    acc0 = _randn(n, d, 12)
    denom = 4.0
    last = None
    for mode in (modes or _modes()):
        for with_y in (True, False):
            if mode == N.LG_ACC_NONE and not with_y:
                continue
            res = []
            for x in (x32, xh):
                y = torch.zeros_like(x) if with_y else None
                acc = acc0.clone()
                out = torch.full_like(x0, -3.0)
                ops.run_layer(rowptr, adj.src, adj.dis(), adj.edge_weight(), x, y, x0, acc,
                              out, le - lb, lb, mode, denom, plan)
                res.append((y, acc, out))
            (y32, acc32, out32), (yh, acch, outh) = res
            assert torch.equal(acch, acc32), (mode, with_y)
            assert torch.equal(outh, out32), (mode, with_y)
            if with_y:
                _assert_f16_equal(yh, y32.to(F16))
                last = (y32, yh)
    return last


# ------------------------------------------------------------------------------ 1. conversion
def _crafted_block():
    x = torch.randn(64, 32, generator=torch.Generator().manual_seed(5)) * 0.1
    v = [0.0, -0.0, float("inf"), float("-inf"), float("nan"),
         65504.0, 65519.9, 65520.0, -65504.0, -65519.9, -65520.0, 1e6, -3e38,
         2.0 ** -24, 2.0 ** -25, 2.0 ** -25 * 1.0000001, 2.0 ** -26, 3 * 2.0 ** -25,
         5 * 2.0 ** -25, 1023 * 2.0 ** -24, 1023.5 * 2.0 ** -24, 2.0 ** -14,
         2.0 ** -14 - 2.0 ** -25, -(2.0 ** -24), -3 * 2.0 ** -25, 1e-45, 1e-39]
    # ties between adjacent halves, even and odd low bit, normal and subnormal, both signs
    for b in (0x3C00, 0x3C01, 0x3C02, 0x3FFF, 0x2E66, 0x2E67, 0x0001, 0x0002, 0x03FF, 0x0400,
              0x7BFE, 0x5555, 0x5556):
        h = torch.tensor([b, b + 1], dtype=torch.int16).view(F16).float()
        mid = float((h[0].double() + h[1].double()) / 2)
        v += [mid, -mid, float(np.nextafter(np.float32(mid), np.float32(0))),
              float(np.nextafter(np.float32(mid), np.float32(np.inf)))]
    flat = x.view(-1)
    flat[:len(v)] = torch.tensor(v, dtype=torch.float64).float()
    assert len(v) < flat.numel()
    return x


def test_conversion_crafted_values():
    from lgcnhs import ops
    x = _crafted_block()
    want = x.to(F16)
    assert torch.isinf(want).sum() >= 6 and torch.isnan(want).sum() == 1
    sub = (want.float().abs() < 2.0 ** -14) & (want.float() != 0)
    assert int(sub.sum()) >= 10  # subnormal halves are kept, not flushed
    _assert_f16_equal(ops.rows_to_f16(x.to(DEV)).cpu(), want)


@pytest.mark.parametrize("d", [32, 64, 128, 256])
def test_conversion_random_block(d):
    from lgcnhs import ops
    x = _randn(3000, d, 2)
    _assert_f16_equal(ops.rows_to_f16(x).cpu(), x.cpu().to(F16))


# --------------------------------------------------------------------- 2. one layer, bitwise
@pytest.mark.parametrize("dist", ["uniform", "zipf"])
@pytest.mark.parametrize("d", [32, 64, 128, 256])
def test_layer_bitwise_equals_fp32_kernel_on_widened_input(d, dist):
    adj = _graph(dist)
    xh = _randn(U + I, d, 3).to(F16)
    y32, _ = _check_layer(adj, xh)
    assert float(y32.abs().max()) > 0
    # a row slice that straddles the user / item boundary (row_offset != 0, n_rows < n)
    _check_layer(adj, xh, rows=(2501, 3703))


def test_dispatch_refuses_training_masks_and_fp32_y():
    from lgcnhs import ops, _native as N
    adj = _graph("uniform")
    xh = _randn(U + I, 64, 3).to(F16)
    mask = torch.ones(U + I, dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError):
        ops.spmm_layer(adj, xh, None, None, None, None, N.LG_ACC_NONE, 1.0, live=mask)
    with pytest.raises(ValueError):
        ops.spmm_layer(adj, xh, None, None, None, None, N.LG_ACC_NONE, 1.0, row_mask=mask)
    with pytest.raises(ValueError):
        ops.spmm_layer(adj, xh, torch.empty(U + I, 64, device=DEV), None, None, None,
                       N.LG_ACC_NONE, 1.0)


# ------------------------------------------------------------------------ 3. row-length edges
ROW_LENGTHS = (0, 1, 63, 64, 65, 127, 128, 129)


@functools.lru_cache(maxsize=None)
def _edge_graph():
    """~400 nodes: node t < 8 has ROW_LENGTHS[t] entries (the 64-edge chunk boundaries and the
    UNROLL x G boundaries of every d), node 8 has 2. Their sources are pool nodes 9.., each of
    in-degree 1 (a ring inside the pool), so every weight is deg(t)^-1/2. Node 8's two sources
    are reserved for it. Returns (adjacency, node 8's sources)."""
    from lgcnhs.graph import Adjacency
    n, first = 400, len(ROW_LENGTHS) + 1
    pool = np.arange(first + 2, n)
    hot = np.array([first, first + 1])
    rng = np.random.default_rng(4)
    src, tgt = [], []
    for t, k in enumerate(ROW_LENGTHS):
        src.append(rng.choice(pool, size=k, replace=False))
        tgt.append(np.full(k, t))
    src.append(hot)
    tgt.append(np.full(2, len(ROW_LENGTHS)))
    ring = np.arange(first, n)
    src.append(np.roll(ring, 1))
    tgt.append(ring)
    ei = torch.as_tensor(np.stack([np.concatenate(src), np.concatenate(tgt)]))
    adj = Adjacency.from_edge_index(ei, n, DEV)
    deg = (adj.rowptr[1:] - adj.rowptr[:-1]).cpu().tolist()
    assert tuple(deg[:first]) == ROW_LENGTHS + (2,) and set(deg[first:]) == {1}
    return adj, hot


@pytest.mark.parametrize("d", [32, 64, 128, 256])
def test_row_length_edges_and_overflow_row(d):
    adj, hot = _edge_graph()
    over = len(ROW_LENGTHS)
    xh = _randn(adj.n_nodes, d, 6).to(F16)
    xh[torch.as_tensor(hot, device=DEV)] = 60000.0  # 2 * 60000 / sqrt(2) = 84853 > 65504
    y32, yh = _check_layer(adj, xh)
    assert torch.all(yh[0] == 0)  # the empty row
    assert torch.all(torch.isposinf(yh[over])) and torch.all(torch.isfinite(y32[over]))
    # (out of that row is finite: checked bitwise against the fp32 kernel's in _check_layer)
    assert torch.isfinite(y32).all()
    assert int(torch.isinf(yh).sum()) == d


# ------------------------------------------------------------------------------- 4. hub rows
def test_hub_rows_segmented_bitwise_and_repeatable():
    from lgcnhs import ops, _native as N
    from lgcnhs.graph import Adjacency
    from lgcnhs.synth import synth_interactions
    hu, hi = 60_000, 5_000
    users, items = synth_interactions(hu, hi, 600_000, seed=9, dist="zipf")
    adj = Adjacency.from_interactions(torch.as_tensor(users), torch.as_tensor(items), hu, hi, DEV)
    plan = adj.long_plan()
    assert plan.n_long > 0
    xh = _randn(hu + hi, 64, 8).to(F16)
    _check_layer(adj, xh, plan=plan)
    x0 = _randn(hu + hi, 64, 11)
    runs = []
    for _ in range(2):
        y = torch.zeros_like(xh)
        out = torch.zeros_like(x0)
        ops.spmm_layer(adj, xh, y, x0, None, out, N.LG_ACC_ONLY, 2.0, long_rows=True)
        runs.append((y, out))
    assert torch.equal(_bits(runs[0][0]), _bits(runs[1][0]))
    assert torch.equal(runs[0][1], runs[1][1])
    long_nodes = plan.long_node.long()
    assert float(runs[0][0][long_nodes].float().abs().max()) > 0  # the hub rows were written


# -------------------------------------------------------------------- 5. end to end, bitwise
def _loop_reference(adj, e0, layers):
    """The definition, spelled with the fp32 kernel: each layer's operand is the previous
    fp32 layer sum rounded to float16 and widened again; the mean takes e0 and the unrounded
    sums through the same acc modes."""
    from lgcnhs import ops, _native as N
    out = torch.empty_like(e0)
    x = e0.to(F16)
    for l in range(layers):
        first, last = l == 0, l == layers - 1
        mode = (N.LG_ACC_ONLY if first and last else N.LG_ACC_FIRST if first
                else N.LG_ACC_LAST if last else N.LG_ACC_MID)
        y = torch.empty_like(e0)
        ops.spmm_layer(adj, x.float(), y, e0, out, out, mode, layers + 1)
        x = y.to(F16)
    return out


@pytest.mark.parametrize("layers", [1, 2, 3, 4])
def test_propagate_mean_store_equals_loop_over_fp32_kernel(layers):
    from lgcnhs import ops
    adj = _graph("uniform")
    e0 = _randn(U + I, 64, 1)
    got = ops.propagate_mean(adj, e0, layers, store=F16)
    assert got.dtype == torch.float32
    assert torch.equal(got, _loop_reference(adj, e0, layers))
    assert torch.equal(got, ops.propagate(adj, e0, layers, store=F16))
    assert not torch.equal(got, ops.propagate_mean(adj, e0, layers))  # the mode is really on


def test_propagate_mean_store_layers0_and_bad_arguments():
    from lgcnhs import ops
    adj = _graph("uniform")
    e0 = _randn(U + I, 64, 1)
    assert torch.equal(ops.propagate_mean(adj, e0, 0, store=F16), e0)
    with pytest.raises(ValueError):
        ops.propagate_mean(adj, e0, 2, store=torch.bfloat16)
    with pytest.raises(ValueError):
        ops.propagate(adj, e0, 2, store=torch.bfloat16)
    with pytest.raises(ValueError):
        ops.propagate_mean(adj, e0, 2, sparse_input=True, store=F16)
    eg = e0.clone().requires_grad_(True)
    with pytest.raises(ValueError):
        ops.propagate(adj, eg, 2, store=F16)
    with torch.no_grad():
        assert torch.equal(ops.propagate(adj, eg, 2, store=F16),
                           ops.propagate_mean(adj, e0, 2, store=F16))


# ------------------------------------------------------------------------ 6. reference fixtures
@pytest.mark.parametrize("name", ["lightgcn_toy", "lightgcn_edge", "lightgcn_mid"])
@pytest.mark.parametrize("L", [1, 2, 3])
def test_model_layer_storage_within_contract_of_reference(golden, name, L):
    from model.LightGCN.model import LightGCN
    g = golden(name)
    nu, ni = int(g["n_users"]), int(g["n_items"])
    coo = torch.as_tensor(g["train_coo"]).long()
    torch.manual_seed(42)
    m = LightGCN(nu, ni, 64, L).to(DEV)
    assert m.layer_storage is None
    torch.manual_seed(42)
    plain = LightGCN(nu, ni, 64, L).to(DEV)
    m.layer_storage = F16
    with torch.no_grad():
        uf, u0, itf, i0 = m.forward(coo)
        pu, _, pi, _ = plain.forward(coo)
    assert u0 is m.users_emb.weight and i0 is m.items_emb.weight
    assert np.array_equal(u0.detach().cpu().numpy(), g["e0_u"])
    eu = np.abs(uf.cpu().numpy() - g[f"out_u_L{L}"]).max()
    ei = np.abs(itf.cpu().numpy() - g[f"out_i_L{L}"]).max()
    print(f"{name} L={L}: max|err| users {eu:.3e} items {ei:.3e}")
    assert eu <= TOL and ei <= TOL, (eu, ei)
    assert not (torch.equal(uf, pu) and torch.equal(itf, pi))  # 16-bit storage was used
    # with grad enabled the same model runs the fp32 path exactly as a model without it
    a = m.forward(coo)
    b = plain.forward(coo)
    assert a[0].requires_grad
    assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2])
    assert torch.equal(a[0].detach(), pu) and torch.equal(a[2].detach(), pi)


# ----------------------------------------------------------------------- 7. a-priori bound
def test_error_within_a_priori_bound():
    """|out_h - out_f32| <= B + S elementwise (uniform graph: short rows, d = 128, L = 3).
    B: the operand of layer l is x^{l-1} + (error <= E^{l-1}) rounded to float16 (relative
    2^-11), so E^l = |A|(E^{l-1} + 2^-11 (|x^{l-1}| + E^{l-1})), E^0 = 0, B = sum_l E^l / (L+1).
    S: the fp32 summation error of both runs, 2 (deg + 4) 2^-24 (|A||x^{l-1}|) per layer,
    summed the same way. All in fp64."""
    from lgcnhs import ops
    L, d = 3, 128
    adj = _graph("uniform")
    n = adj.n_nodes
    e0 = _randn(n, d, 1)
    got = ops.propagate_mean(adj, e0, L, store=F16).cpu().double()
    ref = ops.propagate_mean(adj, e0, L).cpu().double()
    A = torch.sparse_csr_tensor(adj.rowptr.cpu(), adj.src.cpu().long(),
                                adj.edge_weight().cpu().double(), size=(n, n))
    deg = (adj.rowptr[1:] - adj.rowptr[:-1]).cpu().double().unsqueeze(1)
    x = e0.cpu().double()
    Eb = torch.zeros_like(x)
    B = torch.zeros_like(x)
    S = torch.zeros_like(x)
    for _ in range(L):
        ax = A @ x.abs()
        Eb = A @ (Eb + 2.0 ** -11 * (x.abs() + Eb))
        B += Eb
        S += 2 * (deg + 4) * 2.0 ** -24 * ax
        x = A @ x
    B /= L + 1
    S /= L + 1
    err = (got - ref).abs()
    print(f"max|out_h - out_f32| = {err.max():.3e}, max B = {B.max():.3e}, max S = {S.max():.3e}")
    assert err.max() > 0
    assert torch.all(err <= B + S), float((err - B - S).max())


def test_opti_model_layer_storage():
    """LightGCNOpti takes the same switch: float16 storage under no_grad, fp32 with grad."""
    from lgcnhs import ops
    from lgcnhs.graph import Adjacency
    from lgcnhs.synth import synth_interactions
    from model.LightGCNOpti.model import LightGCNOpti
    nu, ni = 300, 200
    users, items = synth_interactions(nu, ni, 4000, seed=2)
    adj = Adjacency.from_interactions(torch.as_tensor(users), torch.as_tensor(items), nu, ni, DEV)
    torch.manual_seed(42)
    m = LightGCNOpti(nu, ni, 64, 3, torch.randn(nu, 7), torch.randn(ni, 5)).to(DEV)
    assert m.layer_storage is None
    e0 = torch.cat([m.users_emb.weight, m.items_emb.weight]).detach()
    with torch.no_grad():
        plain = m.forward(adj)
        m.layer_storage = F16
        half = m.forward(adj)
    assert torch.equal(torch.cat([plain[0], plain[2]]), ops.propagate_mean(adj, e0, 3))
    assert torch.equal(torch.cat([half[0], half[2]]), ops.propagate_mean(adj, e0, 3, store=F16))
    assert half[1] is m.users_emb.weight and half[3] is m.items_emb.weight
    g = m.forward(adj)  # grad enabled: fp32, differentiable
    assert g[0].requires_grad and torch.equal(g[0].detach(), plain[0])
