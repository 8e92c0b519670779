"""Torch-facing wrappers of the HIP hot path (no CPU fallback: GPU tensors only).

propagate        LightGCN layers + layer mean      model/LightGCN/model.py:53-74
score_topk       e0 scores, -1024 mask, top-k      model/LightGCN/recommend.py:83-114
                 (k <= 128: K2 / K2r; 128 < k <= 1024: K2w, lists in global slabs)
score_dense      masked dense score matrix G       model/SpreadLightGCN/model.py:74-104
spread_general   general_W                         model/SpreadMethod/model.py:14-27
hybrid_weight    HybridS W                         model/SpreadMethod/model.py:63-85
spread_resource  F = A @ W                         model/SpreadMethod/model.py:88-99
rows_topk        argsort + filter + [:k], G * F    model/SpreadMethod/recommend.py:31-50,
                                                   model/SpreadLightGCN/model.py:151
                 (k <= 128: K4; 128 < k <= 1024: lists in LDS; csrc/rows_topk.hip)
rows_rank        the position of given items in    (same order, at any depth; K4k,
spread_rank      that order, F block by block       csrc/rows_rank.hip; dense path only)
spread_topk_tiled  the above over item tiles,     (same; for catalogs whose I x I W
                   never holding an I x I matrix    does not fit)
                   (k > 128: peeled passes of 128)
spread_recommend   dense or tiled, whichever fits  model/SpreadMethod/recommend.py:59-115
                   (items=: over a candidate item set -- csrc/rows_topk_items.hip on the
                   dense path, a column view of the tiles on the tiled one)
spread_rows_recommend  the same for item baskets   (no I x I matrix, no tile: two sweeps of
spread_rows_rank       that are not rows of A        A per 64 baskets, csrc/spread_rows.hip,
spread_related_items   (a cart, a session, an item)  finished by rows_topk / rows_rank)
"""
from __future__ import annotations

import numpy as np
import torch

from . import _native as N
from .graph import Adjacency, RowSets

MASK_VALUE = float(-(1 << 10))  # model/LightGCN/recommend.py:101,111


def _aligned(t: torch.Tensor) -> torch.Tensor:
    """t contiguous with a 16-byte aligned base address, as the kernels' vector loads assume
    (a copy when it is not: a column slice, a transposed table, a stride-0 gradient, a view at
    an odd element offset of another tensor)."""
    t = t.contiguous()
    if t.numel() and t.data_ptr() % 16:
        t = t.clone(memory_format=torch.contiguous_format)
    return t


def _typed(t, name: str, dtype, rank: int = 2) -> None:
    """TypeError unless t is a tensor of `dtype`, ValueError unless it has `rank` dimensions
    (no device check: a CPU tensor gets the same messages)."""
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a tensor, got {type(t).__name__}")
    if t.dtype != dtype:
        raise TypeError(f"{name} must be {str(dtype).replace('torch.', '')}, got {t.dtype}")
    if t.dim() != rank:
        raise ValueError(f"{name} must have {rank} dimensions, got shape {tuple(t.shape)}")


def _dense(t, name: str, dtype, rank: int = 2) -> torch.Tensor:
    """A dense kernel operand: _typed, on the GPU, then _aligned."""
    _typed(t, name, dtype, rank)
    N.require_gpu(t, name)
    return _aligned(t)


def _f32(t: torch.Tensor, name: str) -> torch.Tensor:
    return _dense(t, name, torch.float32)


def _f32_tables(eu: torch.Tensor, ei: torch.Tensor):
    """_f32 of the user and item tables, both types checked before either device."""
    _typed(eu, "eu", torch.float32)
    _typed(ei, "ei", torch.float32)
    return _f32(eu, "eu"), _f32(ei, "ei")


def _f64(t: torch.Tensor, name: str) -> torch.Tensor:
    return _dense(t, name, torch.float64)


def _same_device(t: torch.Tensor, name: str, ref: torch.Tensor, ref_name: str) -> None:
    if t.device != ref.device:
        raise ValueError(f"{name} is on {t.device}, {ref_name} on {ref.device}")


def _nonempty(rowsets):
    """rowsets, or None when it holds no entry at all (an empty tensor has no pointer to pass)."""
    return None if rowsets is None or rowsets.col.numel() == 0 else rowsets


def _g_guard(eu, ei, n: int, m: int, what: str = "") -> None:
    """The G factor's operands: TypeError unless eu and ei are both float32 matrices (a half-set
    pair fails here), ValueError unless they are [n, d] and [m, d]; ``what`` opens the message."""
    _typed(eu, "eu", torch.float32)
    _typed(ei, "ei", torch.float32)
    if eu.shape[0] != n or ei.shape[0] != m or eu.shape[1] != ei.shape[1]:
        raise ValueError(f"{what}eu must be [{n}, d] and ei [{m}, d], got "
                         f"{tuple(eu.shape)} and {tuple(ei.shape)}")


def _excl_guard(excl, n: int, what: str, g_keeps: bool = False) -> None:
    """ValueError unless excl (or None) has n rows, ``what`` naming them; g_keeps: the call has
    a G factor and drop=False, which no kernel serves together with exclusions."""
    if excl is None:
        return
    if excl.n_rows != n:
        raise ValueError(f"exclusion rows {excl.n_rows} != {what} {n}")
    if g_keeps:
        raise ValueError("a G factor with exclusions requires drop=True")


def _mark(evs, what) -> None:
    """stats= timing: one HIP event on the launch stream that ends the open stage and starts
    stage ``what`` (None: ends only). evs None (no stats= asked for): nothing, no event."""
    if evs is not None:
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        evs.append((what, e))


def _stage_ms(stats: dict, evs: list, dev, *stages) -> dict:
    """One synchronize, then stats["t_<stage>_ms"] grows by the marked spans of each stage;
    returns {stage: [ms per span]}."""
    torch.cuda.synchronize(dev)
    ms = {w: [] for w in stages}
    for (w, a), (_, b) in zip(evs, evs[1:]):
        if w is not None:
            ms[w].append(a.elapsed_time(b))
    for w, t in ms.items():
        stats[f"t_{w}_ms"] = stats.get(f"t_{w}_ms", 0.0) + sum(t)
    return ms


def _layer_operand(t, name: str, x: torch.Tensor, dtype) -> None:
    """y / x0 / acc / out of run_layer: None, or x's shape and device, contiguous, of `dtype`."""
    if t is None:
        return
    if t.dtype != dtype:
        raise TypeError(f"{name} must be {str(dtype).replace('torch.', '')}, got {t.dtype}")
    if t.shape != x.shape or not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous of x's shape {tuple(x.shape)}, got "
                         f"shape {tuple(t.shape)} strides {t.stride()}")
    _same_device(t, name, x, "x")
    if t.numel() and t.data_ptr() % 16:
        raise ValueError(f"{name} must start at a 16-byte aligned address")


# ------------------------------------------------------------------------------ propagation
def run_layer(rowptr, src, dis, w, x, y, x0, acc, out, n_rows: int, row_offset: int,
              mode: int, denom: float, plan=None, live=None, row_mask=None) -> None:
    """One propagation layer over a CSR slice: lg_spmm_layer_f32 for the ordinary rows (or
    lg_spmm_layer_live_f32 when a uint8 per-node ``live`` mask marks x's non-zero rows, or
    lg_spmm_layer_rows_f32 computing only the rows a uint8 per-node ``row_mask`` marks)
    and, when the slice has rows above the long-row threshold, lg_spmm_long_rows_f32 (its
    masked form with row_mask). A float16 ``x`` (fp16 layer storage, inference) goes to
    lg_spmm_layer_f16 / lg_spmm_long_rows_f16: ``y`` is then float16 or None, and live /
    row_mask (training paths) are refused. x is contiguous [nodes, dim] at a 16-byte aligned
    address and covers rows [row_offset, row_offset + n_rows); y has x's dtype, x0 / acc / out
    are float32, each None or of x's shape on x's device."""
    if not isinstance(x, torch.Tensor) or x.dtype not in (torch.float32, torch.float16):
        raise TypeError(f"x must be a float32 or float16 tensor, got "
                        f"{getattr(x, 'dtype', type(x).__name__)}")
    if x.dim() != 2 or not x.is_contiguous():
        raise ValueError(f"x must be contiguous [nodes, dim], got shape {tuple(x.shape)} "
                         f"strides {x.stride()}")
    if row_offset < 0 or n_rows < 0 or row_offset + n_rows > x.shape[0]:
        raise ValueError(f"rows [{row_offset}, {row_offset + n_rows}) outside x's "
                         f"{x.shape[0]} rows")
    if x.numel() and x.data_ptr() % 16:
        raise ValueError("x must start at a 16-byte aligned address")
    if x.dtype == torch.float16 and y is not None and y.dtype != torch.float16:
        raise ValueError(f"a float16 x needs a float16 y (or None), got {y.dtype}")
    _layer_operand(y, "y", x, x.dtype)
    for t, name in ((x0, "x0"), (acc, "acc"), (out, "out")):
        _layer_operand(t, name, x, torch.float32)
    half = x.dtype == torch.float16
    if half and (live is not None or row_mask is not None):
        raise ValueError("float16 layer storage is inference-only: no live / row_mask")
    if row_mask is not None and live is not None:
        raise ValueError("row_mask and live are exclusive")
    for m, name in ((live, "live"), (row_mask, "row_mask")):
        if m is not None and (m.dtype != torch.uint8 or m.numel() != x.shape[0]
                              or m.device != x.device or not m.is_contiguous()):
            raise ValueError(f"{name} must be a uint8 mask with one entry per row of x")
    N.require_gpu(x, "x")
    dim = x.shape[1]
    thr = plan.threshold if (plan is not None and plan.n_long) else 0
    strm = N.stream_handle(x.device)
    if half:
        N.check(N.lib().lg_spmm_layer_f16(
            N.ptr(rowptr), N.ptr(src), N.ptr(dis), N.ptr(w), N.ptr(x), N.ptr(y), N.ptr(x0),
            N.ptr(acc), N.ptr(out), n_rows, row_offset, dim, mode, float(denom), thr, strm),
            "lg_spmm_layer_f16")
    elif row_mask is not None:
        N.check(N.lib().lg_spmm_layer_rows_f32(
            N.ptr(rowptr), N.ptr(src), N.ptr(dis), N.ptr(w), N.ptr(x), N.ptr(y), N.ptr(x0),
            N.ptr(acc), N.ptr(out), n_rows, row_offset, dim, mode, float(denom), thr,
            N.ptr(row_mask), strm), "lg_spmm_layer_rows_f32")
    elif live is not None:
        N.check(N.lib().lg_spmm_layer_live_f32(
            N.ptr(rowptr), N.ptr(src), N.ptr(dis), N.ptr(w), N.ptr(x), N.ptr(y), N.ptr(x0),
            N.ptr(acc), N.ptr(out), n_rows, row_offset, dim, mode, float(denom), thr,
            N.ptr(live), strm), "lg_spmm_layer_live_f32")
    else:
        N.check(N.lib().lg_spmm_layer_f32(
            N.ptr(rowptr), N.ptr(src), N.ptr(dis), N.ptr(w), N.ptr(x), N.ptr(y), N.ptr(x0),
            N.ptr(acc), N.ptr(out), n_rows, row_offset, dim, mode, float(denom), thr, strm),
            "lg_spmm_layer_f32")
    if thr:
        part = plan.partial(dim, x.device)
        args = (N.ptr(plan.seg_beg), N.ptr(plan.seg_end), N.ptr(plan.seg_node), plan.n_seg,
                N.ptr(plan.long_node), N.ptr(plan.seg_ptr), plan.n_long, N.ptr(src),
                N.ptr(dis), N.ptr(w), N.ptr(x), N.ptr(y), N.ptr(x0), N.ptr(acc), N.ptr(out),
                dim, mode, float(denom), N.ptr(part))
        if half:
            N.check(N.lib().lg_spmm_long_rows_f16(*args, strm), "lg_spmm_long_rows_f16")
        elif row_mask is not None:
            N.check(N.lib().lg_spmm_long_rows_masked_f32(*args, N.ptr(row_mask), strm),
                    "lg_spmm_long_rows_masked_f32")
        else:
            N.check(N.lib().lg_spmm_long_rows_f32(*args, strm), "lg_spmm_long_rows_f32")


def spmm_layer(adj: Adjacency, x: torch.Tensor, y, x0, acc, out, mode: int, denom: float,
               stream_weights: bool = True, long_rows: bool = True, live=None,
               row_mask=None) -> None:
    """One layer over all rows of ``adj`` (or the rows ``row_mask`` marks); with
    stream_weights the precomputed gcn_norm edge weights are streamed (else recomputed from
    dis; identical values); with long_rows, hub rows go through the segmented path."""
    if isinstance(x, torch.Tensor) and x.dim() == 2 and x.shape[0] != adj.n_nodes:
        raise ValueError(f"x has {x.shape[0]} rows, graph has {adj.n_nodes} nodes")
    w = adj.edge_weight() if stream_weights else None
    run_layer(adj.rowptr, adj.src, adj.dis(), w, x, y, x0, acc, out, adj.n_nodes, 0, mode,
              denom, adj.long_plan() if long_rows else None, live, row_mask)


LIVE_FRACTION = 0.25  # below this share of non-zero input rows, skip the dead rows' gathers


def live_rows(x: torch.Tensor) -> torch.Tensor:
    """uint8 [rows]: 1 where row of x has a non-zero entry."""
    return (x != 0).any(dim=1).to(torch.uint8)


def rows_to_f16(x: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
    """f16(x) of an fp32 [n, d] array, round to nearest even (lg_rows_f32_to_f16)."""
    _typed(x, "x", torch.float32)
    if out is not None:
        _typed(out, "out", torch.float16)
        if out.shape != x.shape or not out.is_contiguous():
            raise ValueError(f"out must be contiguous of x's shape {tuple(x.shape)}, got "
                             f"shape {tuple(out.shape)} strides {out.stride()}")
        _same_device(out, "out", x, "x")
    x = _f32(x, "x")
    if out is None:
        out = torch.empty(x.shape, dtype=torch.float16, device=x.device)
    N.check(N.lib().lg_rows_f32_to_f16(N.ptr(x), x.shape[0], x.shape[1], N.ptr(out),
                                       N.stream_handle(x.device)), "lg_rows_f32_to_f16")
    return out


def _check_store(store, sparse_input: bool = False) -> None:
    if store is None:
        return
    if store != torch.float16:
        raise ValueError(f"layer storage {store} is not supported (torch.float16 or None)")
    if sparse_input:
        raise ValueError("store and sparse_input are exclusive (fp16 storage is inference-only)")


def _acc_mode(l: int, layers: int) -> int:
    first, last = l == 0, l == layers - 1
    if first and last:
        return N.LG_ACC_ONLY
    if first:
        return N.LG_ACC_FIRST
    return N.LG_ACC_LAST if last else N.LG_ACC_MID


def _propagate_mean_f16(adj: Adjacency, e0: torch.Tensor, layers: int) -> torch.Tensor:
    """propagate_mean with the layer embeddings held as float16 between layers: xh^0 =
    f16(e0), each layer gathers float16 rows, sums in fp32 exactly as lg_spmm_layer_f32 does
    on the widened rows, and writes the next float16 operand; the layer mean takes the fp32
    e0 and the unrounded fp32 layer sums. Two float16 ping-pong buffers."""
    out = torch.empty_like(e0)
    bufs = [torch.empty(e0.shape, dtype=torch.float16, device=e0.device),
            torch.empty(e0.shape, dtype=torch.float16, device=e0.device) if layers > 1 else None]
    x = rows_to_f16(e0, bufs[0])
    for l in range(layers):
        y = None if l == layers - 1 else bufs[(l + 1) % 2]
        spmm_layer(adj, x, y, e0, out, out, _acc_mode(l, layers), layers + 1)
        x = y
    return out


def propagate_mean(adj: Adjacency, e0: torch.Tensor, layers: int,
                   sparse_input: bool = False, store=None) -> torch.Tensor:
    """mean_{l=0..L} A_hat^l e0 with A_hat = D^-1/2 A D^-1/2 (no autograd). With
    sparse_input (the backward pass: e0 = dL/d(e_final), non-zero on a mini-batch's rows),
    each layer whose input has < LIVE_FRACTION non-zero rows gathers only those rows
    (lg_spmm_layer_live_f32; same sums). ``store=torch.float16`` (inference): the gathered
    layer embeddings are held in 16 bits (lg_spmm_layer_f16; e0 fp32 in, fp32 out)."""
    _check_store(store, sparse_input)
    e0 = _f32(e0, "e0")
    if e0.shape[0] != adj.n_nodes:
        raise ValueError(f"e0 has {e0.shape[0]} rows, graph has {adj.n_nodes} nodes")
    if layers <= 0:
        return e0.clone()
    if store is not None:
        return _propagate_mean_f16(adj, e0, layers)
    out = torch.empty_like(e0)
    bufs = [torch.empty_like(e0), torch.empty_like(e0) if layers > 2 else None]
    x = e0
    for l in range(layers):
        first, last = l == 0, l == layers - 1
        if first and last:
            mode = N.LG_ACC_ONLY
        elif first:
            mode = N.LG_ACC_FIRST
        elif last:
            mode = N.LG_ACC_LAST
        else:
            mode = N.LG_ACC_MID
        y = None if last else bufs[l % 2]
        live = None
        if sparse_input:
            live = live_rows(x)
            frac = int(live.sum()) / max(1, live.numel())
            if frac >= LIVE_FRACTION:
                live = None
            # the next input's non-zero rows are this one's neighbours: stop checking once
            # they are expected to pass the threshold (a mask pass + sync saved per layer)
            sparse_input = frac * adj.nnz / max(1, adj.n_nodes) < LIVE_FRACTION
        spmm_layer(adj, x, y, e0, out, out, mode, layers + 1, live=live)
        x = y
    return out


RESTRICT_FRACTION = 0.5  # a layer whose needed rows may exceed this share runs in full


def row_masks(adj: Adjacency, nodes: torch.Tensor, layers: int, force: bool = False) -> list:
    """Per layer l (0-based) the uint8 mask of the rows whose layer-l output the final
    embeddings at ``nodes`` depend on, or None for a full layer: layer L-1 at the nodes, each
    layer below also at the sources of the rows above it (lg_mark_neighbors_u8). A layer
    runs in full once its rows may exceed RESTRICT_FRACTION of the graph (estimated without a
    host sync: |nodes| times (1 + mean degree) per layer down), and so does every layer below
    it. ``force`` masks every layer (tests)."""
    n = adj.n_nodes
    masks = [None] * layers
    if layers == 0:
        return masks
    est = min(n, int(nodes.numel()))
    m = torch.zeros(n, dtype=torch.uint8, device=nodes.device)
    m[nodes] = 1
    strm = N.stream_handle(nodes.device)
    for l in range(layers - 1, -1, -1):
        if not force and est > RESTRICT_FRACTION * n:
            break
        masks[l] = m
        if l > 0:
            m2 = torch.zeros_like(m)
            N.check(N.lib().lg_mark_neighbors_u8(N.ptr(adj.rowptr), N.ptr(adj.src), n,
                                                 N.ptr(m), N.ptr(m2), strm),
                    "lg_mark_neighbors_u8")
            m = m2
            est = min(n, est * (1 + -(-adj.nnz // max(1, n))))
    return masks


def propagate_rows_mean(adj: Adjacency, e0: torch.Tensor, layers: int, nodes: torch.Tensor,
                        force_masks: bool = False) -> torch.Tensor:
    """propagate_mean's output at the rows ``nodes`` (int64, duplicates allowed), each row
    bitwise the full forward's: layer l computes only the rows row_masks marks (the training
    step's forward: the BPR loss reads the final embeddings at the mini-batch's <= 3 x batch
    rows only, reference model/LightGCN/train.py:30-45)."""
    e0 = _f32(e0, "e0")
    if e0.shape[0] != adj.n_nodes:
        raise ValueError(f"e0 has {e0.shape[0]} rows, graph has {adj.n_nodes} nodes")
    nodes = nodes.to(device=e0.device, dtype=torch.int64)
    if layers <= 0:
        return e0[nodes]
    masks = row_masks(adj, nodes, layers, force_masks)
    out = torch.empty_like(e0)
    bufs = [torch.empty_like(e0), torch.empty_like(e0) if layers > 2 else None]
    x = e0
    for l in range(layers):
        first, last = l == 0, l == layers - 1
        if first and last:
            mode = N.LG_ACC_ONLY
        elif first:
            mode = N.LG_ACC_FIRST
        elif last:
            mode = N.LG_ACC_LAST
        else:
            mode = N.LG_ACC_MID
        y = None if last else bufs[l % 2]
        spmm_layer(adj, x, y, e0, out, out, mode, layers + 1, row_mask=masks[l])
        x = y
    return out[nodes]


class _PropagateRows(torch.autograd.Function):
    """Forward: the final embeddings at ``nodes`` (output-restricted layers). Backward: the
    full operator's, grad_e0 = mean_l (A_hat^T)^l g with g scattered to the nodes' rows --
    what the full forward followed by the gather gives."""

    @staticmethod
    def forward(ctx, e0, adj, layers, nodes):
        ctx.adj, ctx.layers, ctx.n = adj, layers, e0.shape[0]
        ctx.save_for_backward(nodes)
        return propagate_rows_mean(adj, e0.detach(), layers, nodes)

    @staticmethod
    def backward(ctx, g):
        (nodes,) = ctx.saved_tensors
        gfull = torch.zeros((ctx.n, g.shape[1]), dtype=g.dtype, device=g.device)
        gfull.index_add_(0, nodes, g)
        gin = propagate_mean(ctx.adj.transpose(), gfull, ctx.layers, sparse_input=True)
        return gin, None, None, None


def propagate_rows(adj: Adjacency, e0: torch.Tensor, layers: int,
                   nodes: torch.Tensor) -> torch.Tensor:
    """propagate(adj, e0, layers)[nodes], computing only the rows it needs."""
    nodes = nodes.to(device=e0.device, dtype=torch.int64)
    if e0.requires_grad and torch.is_grad_enabled():
        return _PropagateRows.apply(e0, adj, layers, nodes)
    return propagate_rows_mean(adj, e0, layers, nodes)


class PropagationGraph:
    """The L-layer forward captured once into a hipGraph (torch.cuda.CUDAGraph on ROCm) and
    replayed: for small graphs (ML-100K/ML-1M shapes) the three layer kernels run for tens
    of microseconds and host launch overhead dominates. ``run(e0)`` copies e0 into the
    captured input buffer, replays, and returns the captured output buffer (overwritten by
    the next replay)."""

    def __init__(self, adj: Adjacency, dim: int, layers: int, device=None):
        dev = device or adj.device
        adj.dis()
        adj.edge_weight()
        adj.long_plan()  # host-side planning (syncs) must happen before capture
        self.e0 = torch.zeros(adj.n_nodes, dim, dtype=torch.float32, device=dev)
        s = torch.cuda.Stream(dev)
        s.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(s):  # warm the allocator outside the capture
            propagate_mean(adj, self.e0, layers)
        torch.cuda.current_stream(dev).wait_stream(s)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self.out = propagate_mean(adj, self.e0, layers)

    def run(self, e0: torch.Tensor) -> torch.Tensor:
        self.e0.copy_(e0)
        self.graph.replay()
        return self.out


class _Propagate(torch.autograd.Function):
    """Forward: mean of the L+1 layer embeddings. Backward: the same operator with A_hat^T
    (A_hat itself for the symmetric LightGCN graph): grad_e0 = mean_l (A_hat^T)^l g."""

    @staticmethod
    def forward(ctx, e0, adj, layers):
        ctx.adj, ctx.layers = adj, layers
        return propagate_mean(adj, e0.detach(), layers)

    @staticmethod
    def backward(ctx, g):
        gin = propagate_mean(ctx.adj.transpose(), g.contiguous(), ctx.layers,
                             sparse_input=True)
        return gin, None, None


def propagate(adj: Adjacency, e0: torch.Tensor, layers: int, store=None) -> torch.Tensor:
    """The L-layer forward with autograd. ``store=torch.float16`` holds the layer embeddings
    in 16 bits and is inference-only (the backward pass stays fp32): it raises when a
    gradient would be recorded."""
    if store is not None:
        _check_store(store)
        if e0.requires_grad and torch.is_grad_enabled():
            raise ValueError("store=torch.float16 is inference-only: run under "
                             "torch.no_grad() (training propagates in fp32)")
        return propagate_mean(adj, e0, layers, store=store)
    if e0.requires_grad and torch.is_grad_enabled():
        return _Propagate.apply(e0, adj, layers)
    return propagate_mean(adj, e0, layers)


# ------------------------------------------------------------------------------ scoring
def _resident_blocks(device, k: int = 64, screen: bool = False) -> int:
    """Workgroups resident at once: lg_score_topk_f32's take 64 KiB of LDS -> 2 per CU; the
    screened kernel's (k_topk_ring: 84-120 KiB of lists + the fragment ring) -> 1 per CU."""
    per_cu = 1 if screen else 2
    return per_cu * torch.cuda.get_device_properties(device).multi_processor_count


WIDE_K_MIN, WIDE_K_MAX = 129, 1024  # lg_score_topk_wide_f32's share of score_topk's k
# score_topk's wide path (128 < k <= 1024) keeps a slab of 512 / 1024 / 2048 8-byte entries
# per (split, user) in its workspace: 512 MiB per split for 32,768 users at k = 1024. Above
# this many bytes it runs consecutive user blocks instead.
WIDE_WS_CAP_BYTES = 1 << 30


def _wide_resident_blocks(device, k: int, d: int = 64) -> int:
    """Workgroups of k_score_topk_wide resident at once: 4 waves and 17 / 33 / 65 KiB of LDS
    each (k <= 256 / 512 / 1024), 106 VGPRs at d = 64 and 158 at d = 128."""
    per_cu = 2 if k > 512 else (3 if d > 64 else 4)
    return per_cu * torch.cuda.get_device_properties(device).multi_processor_count


def _users_per_block(k: int, screen: bool = False, d: int = 64) -> int:
    """Users per workgroup of the launches of csrc/topk_plain.hip (dispatch_topk) and
    csrc/topk.hip (dispatch_topk_screen) and, for k > 128, of csrc/topk_wide.hip's (4 waves x 16 users)."""
    if k > 128:
        return 64
    if screen:  # (8 waves x 2 groups; k > 64 at d <= 64: 1 group, LG_GL4_NG)
        return 128 if k > 64 and d <= 64 else 256
    return 128 if k <= 32 else (64 if k <= 64 else 32)


def _splits_for(n_users: int, n_items: int, k: int, resident: int = 512,
                screen: bool = False, d: int = 64) -> int:
    """Item-range splits for lg_score_topk_f32: the fewest splits that keep every CU busy.

    Each split restarts every user's candidate list from an empty threshold (the warm-up
    inserts ~k*ln(items/k) candidates), so more splits cost work; too few leave CUs idle
    in the last round of workgroups. Minimise rounds/splits (the makespan in units of one
    unsplit block) with a 2 % penalty per split."""
    per_block = _users_per_block(k, screen, d)
    tiles = (n_users + per_block - 1) // per_block
    best, best_cost = 1, None
    for s in range(1, min(64, max(1, n_items // 256)) + 1):
        rounds = -(-tiles * s // resident)
        cost = rounds / s * (1 + 0.02 * s)
        if best_cost is None or cost < best_cost - 1e-12:
            best, best_cost = s, cost
    return best


# |bf16 MFMA product - fp32 chain| <= 0.00785 ||u|| ||i|| (csrc/gbound.hip); 3 % slack for
# the fp32 roundings of the margin and of the screen's compare. The worst case of bf16
# rounding; the screened top-K uses the tighter screen_margins (below), this form remains the
# bound of lg_score_chunk_bound.
SCREEN_MARGIN = 0.0081
SCREEN_DEFAULT = True  # measured: 26.8 vs 31.9 ms (d=64), 45.8 vs 59.7 ms (d=128) at C5
# The screened kernel's fixed costs (bf16 operands, margins, seed pass) lose to the plain
# kernel below these user x item counts (profiles/r06_topk_guard.log, d = 64, 22 shapes from
# 1024 x 2000 to 2048 x 1M: at k = 20 the two meet near 6e8 -- 2048 x 300K 1.39 vs 1.41 ms --,
# the screen loses at 512 x 1M and wins at 4096 x 200K; at k = 100 near 1e9 -- it loses at
# 8192 x 100K and 16384 x 50K, wins at 32768 x 30K and 2048 x 1M)
SCREEN_MIN_WORK = {32: 6e8, 128: 1e9}  # k <= key -> least users x items for the screen


def screen_pays(n_users: int, n_items: int, k: int) -> bool:
    """Whether the default top-K dispatch takes the screened kernel for this shape."""
    for kmax, work in SCREEN_MIN_WORK.items():
        if k <= kmax:
            return float(n_users) * float(n_items) >= work
    return False  # (k > 128: the screened kernel does not take it)


def screen_margins(un: torch.Tensor, ue: torch.Tensor, inorm: torch.Tensor,
                   ierr: torch.Tensor, dim: int) -> torch.Tensor:
    """Per-user fp32 margins m_u >= |bf16 MFMA product - fp32 chain score| for every item
    (the contract of lg_score_topk_screened_f32's umarg, include/lgcnhs.h).

    With du = u - bf16(u) and di = i - bf16(i) (both exact in fp32):
      u.i - bf16(u).bf16(i) = du.i + bf16(u).di, so |.| <= ||du|| ||i|| + (||u|| + ||du||) ||di||
    (Cauchy-Schwarz, ||bf16(u)|| <= ||u|| + ||du||); the MFMA's and the chain's fp32
    accumulations add gamma_dim (||bf16(u)|| ||bf16(i)|| + ||u|| ||i||) <= 2.01 dim 2^-24 ||u|| ||i||,
    and 2^-22 ||u|| ||i|| covers the rounding of the screen's own fp32 sum fl(b + m_u) (|b + m_u|
    <= 1.02 ||u|| ||i||). With I = max ||i||, DI = max ||di|| (norms rounded up by
    lg_bound_prep_f32), times (1 + 2^-20), plus 1e-30 for flushed subnormal products, in fp64,
    rounded up to fp32. On N(0, 0.1^2) embeddings this is ~0.45x the worst-case 0.0081 ||u|| I
    of SCREEN_MARGIN (bf16 rounding errors are not all at their maximum), and the observed
    error stays below 0.37 of it. Non-finite norms give non-finite margins: the kernel then
    ranks every item of those users by the exact chain."""
    I = inorm.max().double()
    DI = ierr.max().double()
    u, e = un.double(), ue.double()
    m = (e * I + (u + e) * DI + (2.01 * dim * 2.0 ** -24 + 2.0 ** -22) * u * I) \
        * (1.0 + 2.0 ** -20) + 1e-30
    m32 = m.float()
    return torch.where(m32.double() < m, torch.nextafter(m32, torch.full_like(m32, float("inf"))),
                       m32)


def score_topk(eu: torch.Tensor, ei: torch.Tensor, k: int, excl: RowSets | None = None,
               mask_value: float = MASK_VALUE, n_splits: int | None = None,
               screen: bool | None = None, items=None):
    """Top-k items per user by the masked e0 score; returns (values fp32 [U,k],
    indices int64 [U,k]) sorted by (score desc, item asc). screen=True runs
    lg_score_topk_screened_f32: a bf16 MFMA bound decides which 16-item tiles get the exact
    fp32 chain; the results are lg_score_topk_f32's (screen=False) bit for bit. Default:
    SCREEN_DEFAULT where it pays for the shape (screen_pays).

    128 < k <= 1024 runs lg_score_topk_wide_f32 (same score, mask, order and padding; the
    lists live in workspace slabs). There is no screened wide kernel: screen=True raises.
    When the slabs would pass WIDE_WS_CAP_BYTES the users are processed in consecutive
    blocks; the result does not depend on the blocking.

    items: restrict every user's ranking to a candidate item set (item_candidates' forms). The
    all-users job runs the same kernels on the gathered sub-table ei[cand] with the exclusion
    columns renumbered (screened, plain and wide dispatch by the sub-table's shape) and maps
    the ids back: real item ids, rows shorter than k padded with {-inf, -1}. The gather is
    noise next to the scoring of every user; the request form that gathers nothing is
    score_topk_users(items=...)."""
    eu, ei = _f32_tables(eu, ei)
    nu, d = eu.shape
    ni = ei.shape[0]
    k = int(k)
    if items is not None:
        cand = item_candidates(items, ni, eu.device)
        if cand.numel() == 0:
            return _padding(nu, k, eu.device)
        return _score_topk_gathered(eu, ei, cand, k, excl, mask_value, n_splits=n_splits,
                                    screen=screen)
    if k > WIDE_K_MAX:
        raise ValueError(f"k={k} not in [1, {WIDE_K_MAX}]")
    if k >= WIDE_K_MIN:
        if screen:
            raise ValueError(f"screen=True takes k <= 128 (k={k}): no screened wide kernel")
        return _score_topk_wide(eu, ei, k, excl, mask_value, n_splits)
    if screen is None:
        screen = SCREEN_DEFAULT and screen_pays(nu, ni, k)
    if ei.shape[1] != d:
        raise ValueError("eu/ei dims differ")
    if excl is not None and excl.n_rows != nu:
        raise ValueError(f"exclusion rows {excl.n_rows} != users {nu}")
    ns = (_splits_for(nu, ni, k, _resident_blocks(eu.device, k, screen), screen, d)
          if n_splits is None else int(n_splits))
    ws_fn = (N.lib().lg_score_topk_screened_ws_bytes if screen and nu > 0
             else N.lib().lg_score_topk_ws_bytes)
    ws_bytes = ws_fn(nu, ni, d, k, ns)
    ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=eu.device)
    val = torch.empty((nu, k), dtype=torch.float32, device=eu.device)
    idx = torch.empty((nu, k), dtype=torch.int64, device=eu.device)
    ex_rp = N.ptr(excl.rowptr if excl else None)
    ex_c = N.ptr(excl.col if excl else None)
    if screen and nu > 0:
        ub, un, ue = bound_operands(eu, with_err=True)
        ib, inorm, ierr = bound_operands(ei, with_err=True)
        # (no host sync: a non-finite embedding gives non-finite margins, and the kernel then
        # ranks those users' items by the exact chain -- include/lgcnhs.h)
        umarg = screen_margins(un, ue, inorm, ierr, d)
        N.check(N.lib().lg_score_topk_screened_f32(
            N.ptr(eu), N.ptr(ei), N.ptr(ub), N.ptr(ib), N.ptr(umarg), nu, ni, d, ex_rp, ex_c,
            float(mask_value), int(k), ns, N.ptr(val), N.ptr(idx), N.ptr(ws), ws_bytes,
            N.stream_handle(eu.device)), "lg_score_topk_screened_f32")
        return val, idx
    N.check(N.lib().lg_score_topk_f32(
        N.ptr(eu), N.ptr(ei), nu, ni, d, ex_rp, ex_c, float(mask_value), int(k), ns,
        N.ptr(val), N.ptr(idx), N.ptr(ws), ws_bytes, N.stream_handle(eu.device)),
        "lg_score_topk_f32")
    return val, idx


def _wide_user_block(nu: int, ni: int, d: int, k: int, ns: int, cap_bytes: int) -> int:
    """Users per lg_score_topk_wide_f32 call so that its workspace stays within cap_bytes: all
    of them when that fits, else the largest multiple of the kernel's 64 users per workgroup
    that does (at least one workgroup)."""
    ws_fn = N.lib().lg_score_topk_wide_ws_bytes
    if nu <= 0 or ws_fn(nu, ni, d, k, ns) <= cap_bytes:
        return max(nu, 1)
    upb = _users_per_block(k, False, d)
    per_wg = ws_fn(upb, ni, d, k, ns)
    return upb * max(1, cap_bytes // max(per_wg, 1))


def _wide_plan(nu: int, ni: int, d: int, k: int, resident: int, cap_bytes: int):
    """(users per call, item splits) of the wide path: _splits_for's cost (rounds of resident
    workgroups per split, 2 % per split) summed over the calls that cap_bytes of slabs force.
    With every user in one call this is _splits_for's choice; under a tight cap more splits
    mean fewer users per call, so the fewest splits that fill the slabs win."""
    per_block = _users_per_block(k, False, d)
    best, best_cost = (max(nu, 1), 1), None
    for s in range(1, min(64, max(1, ni // 256)) + 1):
        blk = min(max(nu, 1), _wide_user_block(nu, ni, d, k, s, cap_bytes))
        tiles = -(-blk // per_block)
        calls = -(-max(nu, 1) // blk)
        cost = calls * -(-tiles * s // resident) / s * (1 + 0.02 * s)
        if best_cost is None or cost < best_cost - 1e-12:
            best, best_cost = (blk, s), cost
    return best


def _score_topk_wide(eu, ei, k: int, excl, mask_value: float, n_splits):
    """score_topk for 128 < k <= 1024 (also callable below: lg_score_topk_wide_f32 takes any
    k in [1, 1024]), in user blocks of at most WIDE_WS_CAP_BYTES of workspace."""
    nu, d = eu.shape
    ni = ei.shape[0]
    if ei.shape[1] != d:
        raise ValueError("eu/ei dims differ")
    if excl is not None and excl.n_rows != nu:
        raise ValueError(f"exclusion rows {excl.n_rows} != users {nu}")
    val = torch.empty((nu, k), dtype=torch.float32, device=eu.device)
    idx = torch.empty((nu, k), dtype=torch.int64, device=eu.device)
    if nu == 0:
        return val, idx
    resident = _wide_resident_blocks(eu.device, k, d)
    if n_splits is None:
        blk, ns = _wide_plan(nu, ni, d, k, resident, WIDE_WS_CAP_BYTES)
    else:
        ns = int(n_splits)
        blk = _wide_user_block(nu, ni, d, k, ns, WIDE_WS_CAP_BYTES)
    ws_bytes = N.lib().lg_score_topk_wide_ws_bytes(min(blk, nu), ni, d, k, ns)
    ws = torch.empty(max(ws_bytes, 8), dtype=torch.uint8, device=eu.device)
    for u0 in range(0, nu, blk):
        u1 = min(nu, u0 + blk)
        n = u1 - u0
        ex = excl.slice_rows(u0, u1) if excl is not None else None
        N.check(N.lib().lg_score_topk_wide_f32(
            N.ptr(eu[u0:u1]), N.ptr(ei), n, ni, d, N.ptr(ex.rowptr if ex else None),
            N.ptr(ex.col if ex else None), float(mask_value), k, ns, N.ptr(val[u0:u1]),
            N.ptr(idx[u0:u1]), N.ptr(ws), ws_bytes, N.stream_handle(eu.device)),
            "lg_score_topk_wide_f32")
    return val, idx


BATCH_CALL_USERS = 64  # users per lg_score_topk_batch_f32 call (csrc/topk_batch.hip)
BATCH_K_MAX = 128      # its largest k
# score_topk_users sends lists of up to this many users to lg_score_topk_batch_f32 (in chunks
# of BATCH_CALL_USERS) and longer ones to score_topk on gathered rows. Set from
# profiles/topk_batch.json (scripts/topk_batch_time.py): the largest B at which the batch
# kernel beats score_topk's best configuration (default dispatch or screen=False at 64 .. 4096
# splits, rows gathered outside the timing) by more than the spread at 100K and 1M items, every
# k and d timed: 0.38-0.88 of its time at B <= 16; at B = 32 it wins at k = 20 (0.60-0.74) and
# loses at k = 100 (1.12-1.42), at B >= 64 it loses everywhere (1.16-8.0).
BATCH_MAX_USERS = 16


def _list_grid(n: int, cus, waves: int, ng: int, k: int, device) -> tuple:
    """(workgroups, waves per workgroup, items or candidate positions per wave) of the scoring
    launch of lg_score_topk_batch_f32 / lg_score_topk_batch_items_f32 on a device of `cus`
    compute units, default `device`'s (plan_list_grid of csrc/batch_lists.h, restated): n
    entries in 16-entry tiles divided evenly over every wave of a grid that fills the device;
    a workgroup's lists are waves x ng user groups x M (k) units of 8 KiB."""
    if cus is None:
        cus = torch.cuda.get_device_properties(device).multi_processor_count
    m = 1 if k <= 32 else (2 if k <= 64 else 4)
    tiles = (n + 15) // 16
    blocks = min(512, cus * (2 if waves * ng * m <= 8 else 1), -(-tiles // waves))
    per_wave = -(-tiles // (blocks * waves)) * 16
    busy = -(-n // per_wave)  # waves with entries
    return -(-busy // waves), waves, per_wave


def batch_topk_grid(n_batch: int, n_items: int, k: int, device, cus: int | None = None) -> tuple:
    """(workgroups, waves per workgroup, items per wave) of lg_score_topk_batch_f32's scoring
    launch: every wave holds all n_batch users and scores items_per_wave consecutive items.
    cus: the compute units to plan for (default: `device`'s)."""
    ng = 1 if n_batch <= 16 else (2 if n_batch <= 32 else 4)
    m = 1 if k <= 32 else (2 if k <= 64 else 4)
    waves = 1 if ng * m >= 16 else (2 if ng * m >= 8 else 4)
    return _list_grid(n_items, cus, waves, ng, k, device)


def _user_ids(users, n_users: int, device) -> torch.Tensor:
    """An int64 device tensor of user ids; a list or a CPU tensor is validated on the host
    (a device tensor is taken as it is: no sync)."""
    t = torch.as_tensor(users)
    if t.numel() and (t.dtype == torch.bool or t.is_floating_point()):
        raise ValueError("user ids must be integers")
    t = t.reshape(-1).to(torch.int64)
    if not t.is_cuda:
        if t.numel() and (int(t.min()) < 0 or int(t.max()) >= n_users):
            raise ValueError(f"user id outside [0, {n_users})")
        t = t.to(device)
    return _aligned(t)


ITEMS_CALL_USERS = 16  # users per lg_score_topk_batch_items_f32 call (csrc/topk_items.hip)
# score_topk_users(items=...) sends lists of up to this many users (k <= 128) to
# lg_score_topk_batch_items_f32, in chunks of ITEMS_CALL_USERS, and longer ones to score_topk
# on the gathered sub-table. Set from profiles/topk_items.json (scripts/topk_items_time.py):
# the largest B at which the entry beats the gather route (ei[cand], the renumbered exclusion
# rows, score_topk_users on the sub-table, the id map) by more than the larger of the two
# spreads for every candidate share, k and d timed at 100K and 1M items: 0.12-0.73 of its time
# at B <= 16 (all 96 cases); at B = 32 it loses 8 of 32 cases (k = 100), at B = 64 every
# k = 100 case (1.6-2.9x).
ITEMS_BATCH_MAX_USERS = 16


def item_candidates(items, n_items: int, device) -> torch.Tensor:
    """The candidate set of an items= argument as the kernel takes it: an int32 tensor on
    `device` of strictly ascending ids in [0, n_items).

    A list, a numpy array or a CPU tensor of ids is sorted and de-duplicated on the host
    (ValueError on a non-integer id or one outside [0, n_items)). A bool mask of length n_items
    (host or device) gives its true positions. A device integer tensor is taken as it is -- the
    caller guarantees that it is strictly ascending, nothing is checked and nothing syncs (the
    kernel reads no memory outside the tables on any list: an id outside [0, n_items) never
    ranks, a list that is not ascending gives unspecified lists). Empty sets are allowed."""
    n_items = int(n_items)
    t = items if isinstance(items, torch.Tensor) else torch.as_tensor(np.asarray(items))
    if t.dtype == torch.bool:
        if t.dim() != 1 or t.numel() != n_items:
            raise ValueError(f"item mask of shape {tuple(t.shape)}, expected ({n_items},)")
        return torch.nonzero(t).reshape(-1).to(device, torch.int32)
    if t.numel() and (t.is_floating_point() or t.is_complex()):
        raise ValueError("item ids must be integers")
    t = t.reshape(-1)
    if t.is_cuda:
        return _aligned(t.to(device, torch.int32))
    t = torch.unique(t.to(torch.int64))  # (sorted)
    if t.numel() and (int(t[0]) < 0 or int(t[-1]) >= n_items):
        raise ValueError(f"item id outside [0, {n_items})")
    return t.to(torch.int32).to(device)


def items_topk_grid(n_batch: int, n_cand: int, k: int, device, cus: int | None = None) -> tuple:
    """(workgroups, waves per workgroup, candidate positions per wave) of
    lg_score_topk_batch_items_f32's scoring launch: batch_topk_grid's arithmetic for one user
    group and 4 waves over n_cand positions."""
    return _list_grid(n_cand, cus, 4, 1, k, device)


def _padding(n_rows: int, k: int, device):
    if not 1 <= k <= WIDE_K_MAX:
        raise ValueError(f"k={k} not in [1, {WIDE_K_MAX}]")
    return (torch.full((n_rows, k), float("-inf"), dtype=torch.float32, device=device),
            torch.full((n_rows, k), -1, dtype=torch.int64, device=device))


def _score_topk_gathered(eu, ei, cand, k, excl, mask_value, **kw):
    """score_topk on the sub-table ei[cand] (exclusion columns renumbered to positions in
    cand), ids mapped back through cand, -1 kept."""
    c64 = cand.to(torch.int64)
    ex = _nonempty(excl.restrict_cols(cand) if excl is not None else None)
    v, i = score_topk(eu, ei[c64], k, ex, mask_value, **kw)
    return v, torch.where(i >= 0, c64[i.clamp(min=0)], i)


def _topk_lists(entry: str, chunk: int, eu, ei, ids, k, excl, mask_value, cand=None):
    """score_topk_users through the C entry `entry`_f32 (lg_score_topk_batch or
    lg_score_topk_batch_items, the latter with its candidates `cand`): `chunk` users per call,
    one workspace of `entry`_ws_bytes for a full chunk."""
    lib, dev = N.lib(), eu.device
    (nu, d), ni, nb = eu.shape, ei.shape[0], int(ids.numel())
    n, mid = (ni, ()) if cand is None else (int(cand.numel()), (N.ptr(cand), int(cand.numel())))
    val = torch.empty((nb, k), dtype=torch.float32, device=dev)
    idx = torch.empty((nb, k), dtype=torch.int64, device=dev)
    ws_bytes = getattr(lib, entry + "_ws_bytes")(min(nb, chunk), n, d, k)
    ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=dev)
    for b0 in range(0, nb, chunk):
        b1 = min(nb, b0 + chunk)
        N.check(getattr(lib, entry + "_f32")(
            N.ptr(eu), N.ptr(ei), N.ptr(ids[b0:b1]), b1 - b0, nu, ni, *mid, d,
            N.ptr(excl.rowptr if excl else None), N.ptr(excl.col if excl else None),
            float(mask_value), k, N.ptr(val[b0:b1]), N.ptr(idx[b0:b1]), N.ptr(ws), ws_bytes,
            N.stream_handle(dev)), entry + "_f32")
    return val, idx


def score_topk_users(eu: torch.Tensor, ei: torch.Tensor, users, k: int,
                     excl: RowSets | None = None, mask_value: float = MASK_VALUE,
                     items=None):
    """Top-k items for the given users only: (values fp32 [B, k], indices int64 [B, k]), row j
    = score_topk's row users[j] of the full tables bit for bit. users: a list or tensor of ids
    into eu and excl (any order, duplicates allowed); a list or CPU tensor is checked on the
    host (ValueError on a bad id). Up to BATCH_MAX_USERS users (k <= 128) run
    lg_score_topk_batch_f32 in chunks of 64 -- no embedding or exclusion rows are gathered;
    longer lists and 128 < k <= 1024 run score_topk on the gathered rows.

    items: restrict the ranking to a candidate item set (item_candidates' forms: ids, a bool
    mask, or a strictly ascending device tensor). Row j is then the first k of the candidates
    under (score desc, item id asc), real item ids, rows shorter than k padded with
    {-inf, -1}: score_topk(..., items=items)'s row users[j] bit for bit. Up to
    ITEMS_BATCH_MAX_USERS users (k <= 128) run lg_score_topk_batch_items_f32 in chunks of 16
    -- no item row is gathered and only the candidates' rows are read; longer lists and k > 128
    run score_topk on the gathered sub-table. Empty candidates give all padding."""
    eu, ei = _f32_tables(eu, ei)
    nu, d = eu.shape
    ni = ei.shape[0]
    k = int(k)
    if ei.shape[1] != d:
        raise ValueError("eu/ei dims differ")
    if excl is not None and excl.n_rows != nu:
        raise ValueError(f"exclusion rows {excl.n_rows} != users {nu}")
    ids = _user_ids(users, nu, eu.device)
    nb = int(ids.numel())
    if items is not None:
        cand = item_candidates(items, ni, eu.device)
        nc = int(cand.numel())
        if nc == 0 or nb == 0:
            return _padding(nb, k, eu.device)
        if nb > ITEMS_BATCH_MAX_USERS or k > BATCH_K_MAX:
            return _score_topk_gathered(eu[ids], ei, cand, k,
                                        excl.take(ids) if excl is not None else None,
                                        mask_value)
        if k < 1:
            raise ValueError(f"k={k} not in [1, {WIDE_K_MAX}]")
        return _topk_lists("lg_score_topk_batch_items", ITEMS_CALL_USERS, eu, ei, ids, k,
                           _nonempty(excl), mask_value, cand)
    if nb == 0 or nb > BATCH_MAX_USERS or k > BATCH_K_MAX:
        return score_topk(eu[ids], ei, k, excl.take(ids) if excl is not None else None,
                          mask_value)
    if k < 1:
        raise ValueError(f"k={k} not in [1, {WIDE_K_MAX}]")
    return _topk_lists("lg_score_topk_batch", BATCH_CALL_USERS, eu, ei, ids, k, excl, mask_value)


CAND_K_MAX = 128       # lg_score_topk_cand_f32's largest k (csrc/topk_cand.hip)
CAND_SEG_MAX = 4096    # ... and its most segments per row
# cand_segments gives a row no segment shorter than this many candidates. Set from the
# `min_seg_sweep` of profiles/topk_cand.json (scripts/topk_cand_time.py: K2c at 64 x 10,000 and
# 16 x 100,000 candidates over 1M items, d in {64, 128}, k in {20, 100}, the plans for 128 ..
# 4096): 1024 is the fastest or within 5 % of it in all four 64-row cases and within 6-14 % of
# the fastest (2048) in the four 16-row cases; 256 costs 0.99-1.17x / 1.27-1.52x of 1024's time
# there, 2048 1.32-1.50x at 64 rows (too few waves), 128 and 4096 lose everywhere. Shorter
# segments pay a final sort, a partial list and a merge step each.
CAND_MIN_SEG = 1024


def candidate_rows(cands, n_rows: int, n_items: int, device) -> RowSets:
    """Per-row candidate lists as the kernel takes them: a RowSets of n_rows rows over n_items
    columns on `device` (rowptr int64, col int32 strictly ascending inside a row).

    cands: a RowSets (taken as it is); a dict {row: ids} (rows that are not keys are empty); a
    list of n_rows id lists; or a (rows, items) pair of equally long arrays. Host inputs are
    validated -- ValueError on a non-integer id, an item id outside [0, n_items) or a row
    outside [0, n_rows) -- then sorted and de-duplicated per row on the host. A pair of device
    tensors is taken as given: the caller guarantees (row, item) ascending order without
    duplicates, nothing is checked and nothing syncs (the kernel reads no memory outside the
    tables on any list; item_candidates' policy)."""
    n_rows, n_items = int(n_rows), int(n_items)
    if isinstance(cands, RowSets):
        if cands.n_rows != n_rows:
            raise ValueError(f"candidate rows {cands.n_rows} != rows {n_rows}")
        return cands

    def ints(x, what):
        t = x if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x))
        if t.numel() and (t.dtype == torch.bool or t.is_floating_point() or t.is_complex()):
            raise ValueError(f"{what} ids must be integers")
        return t.reshape(-1)

    if isinstance(cands, dict):
        keys = list(cands)
        lists = [ints(cands[r], "item").cpu().to(torch.int64) for r in keys]
        rows = torch.repeat_interleave(ints(keys, "row").to(torch.int64),
                                       torch.tensor([int(x.numel()) for x in lists],
                                                    dtype=torch.int64))
        items = torch.cat(lists) if lists else torch.zeros(0, dtype=torch.int64)
    elif isinstance(cands, tuple) and len(cands) == 2:
        rows, items = ints(cands[0], "row"), ints(cands[1], "item")
        if rows.numel() != items.numel():
            raise ValueError(f"{rows.numel()} rows for {items.numel()} items")
        if rows.is_cuda and items.is_cuda:
            keys = rows.to(device, torch.int64).contiguous()
            from .graph import _rowptr_from_sorted
            return RowSets(_rowptr_from_sorted(keys, n_rows),
                           items.to(device, torch.int32).contiguous(), n_rows, n_items)
        rows, items = rows.cpu().to(torch.int64), items.cpu().to(torch.int64)
    else:
        lists = [ints(x, "item").cpu().to(torch.int64) for x in cands]
        if len(lists) != n_rows:
            raise ValueError(f"{len(lists)} candidate lists for {n_rows} rows")
        rows = torch.repeat_interleave(torch.arange(n_rows, dtype=torch.int64),
                                       torch.tensor([int(x.numel()) for x in lists],
                                                    dtype=torch.int64))
        items = torch.cat(lists) if lists else torch.zeros(0, dtype=torch.int64)
    if rows.numel() and (int(rows.min()) < 0 or int(rows.max()) >= n_rows):
        raise ValueError(f"candidate row outside [0, {n_rows})")
    if items.numel() and (int(items.min()) < 0 or int(items.max()) >= n_items):
        raise ValueError(f"item id outside [0, {n_items})")
    keys = torch.unique(rows * n_items + items)  # (sorted)
    rowptr = torch.zeros(n_rows + 1, dtype=torch.int64)
    torch.cumsum(torch.bincount(keys // n_items, minlength=n_rows), 0, out=rowptr[1:])
    return RowSets(rowptr.to(device), (keys % n_items).to(torch.int32).to(device), n_rows,
                   n_items)


def cand_segments(n_rows: int, max_len: int, k: int, device, cus: int | None = None) -> int:
    """Segments per row (n_seg) for lg_score_topk_cand_f32, one wave each: 1 when the rows
    alone fill the device (16 waves per compute unit), else as many as reach that target, no
    segment shorter than CAND_MIN_SEG candidates, at most CAND_SEG_MAX. k is accepted for the
    planner's signature; the plan does not depend on it. cus: the compute units to plan for
    (default: `device`'s)."""
    if cus is None:
        cus = torch.cuda.get_device_properties(device).multi_processor_count
    n_rows, max_len, target = max(int(n_rows), 1), max(int(max_len), 1), 16 * int(cus)
    if n_rows >= target:
        return 1
    return max(1, min(-(-target // n_rows), -(-max_len // CAND_MIN_SEG), CAND_SEG_MAX))


def _cand_args(eu, ei, cand, excl, users, max_len):
    eu, ei = _f32_tables(eu, ei)
    nu, d = eu.shape
    if ei.shape[1] != d:
        raise ValueError("eu/ei dims differ")
    if not isinstance(cand, RowSets):
        raise ValueError("cand must be a RowSets (ops.candidate_rows)")
    if cand.n_cols != ei.shape[0]:
        raise ValueError(f"candidate columns {cand.n_cols} != items {ei.shape[0]}")
    if excl is not None and excl.n_rows != nu:
        raise ValueError(f"exclusion rows {excl.n_rows} != users {nu}")
    excl = _nonempty(excl)
    ids = None
    if users is not None:
        ids = _user_ids(users, nu, eu.device)
        if int(ids.numel()) != cand.n_rows:
            raise ValueError(f"{int(ids.numel())} users for {cand.n_rows} candidate rows")
    elif cand.n_rows > nu:
        raise ValueError(f"candidate rows {cand.n_rows} > users {nu}")
    if max_len is None and cand.n_rows and cand.col.numel():
        max_len = int(cand.degrees().max())  # (the one host read)
    return eu, ei, excl, ids, max(int(max_len or 1), 1)


def score_topk_cand(eu: torch.Tensor, ei: torch.Tensor, cand: RowSets, k: int,
                    excl: RowSets | None = None, mask_value: float = MASK_VALUE, users=None,
                    max_len: int | None = None, n_seg: int | None = None):
    """Top-k of every row's OWN candidate list (lg_score_topk_cand_f32): (values fp32 [R, k],
    ids int64 [R, k]), row r the first k of cand's row r scored for user users[r] (users=None:
    user r) under (score desc, item id asc), real item ids, rows with fewer than k ranking
    candidates padded with {-inf, -1}. The scores, the mask and the order are score_topk's:
    row r equals score_topk(eu[u:u+1], ei[cand_r], k, ...) with the exclusion columns
    renumbered and the ids mapped back, bit for bit; no row is gathered. cand: a RowSets over
    the items (ops.candidate_rows); excl: the full tables' exclusion sets, indexed by user id.

    max_len bounds the row length: candidates at positions >= max_len of their row are ignored.
    max_len=None reads cand.degrees().max() -- one device-to-host read; pass max_len to stay
    asynchronous. n_seg: segments per row (default: cand_segments); the result does not depend
    on it. k > CAND_K_MAX raises. No rows or no candidates at all: padding, no launch."""
    k = int(k)
    if not 1 <= k <= CAND_K_MAX:
        raise ValueError(f"k={k} not in [1, {CAND_K_MAX}]: lg_score_topk_cand_f32's limit is "
                         f"{CAND_K_MAX}")
    eu, ei, excl, ids, max_len = _cand_args(eu, ei, cand, excl, users, max_len)
    dev, R, d = eu.device, cand.n_rows, eu.shape[1]
    if R == 0 or cand.col.numel() == 0:
        return _padding(R, k, dev)
    ns = cand_segments(R, max_len, k, dev) if n_seg is None else int(n_seg)
    ws_bytes = N.lib().lg_score_topk_cand_ws_bytes(R, d, k, ns)
    ws = torch.empty(max(ws_bytes, 8), dtype=torch.uint8, device=dev)
    val = torch.empty((R, k), dtype=torch.float32, device=dev)
    idx = torch.empty((R, k), dtype=torch.int64, device=dev)
    N.check(N.lib().lg_score_topk_cand_f32(
        N.ptr(eu), N.ptr(ei), N.ptr(ids), R, eu.shape[0], ei.shape[0], N.ptr(cand.rowptr),
        N.ptr(cand.col), max_len, d, N.ptr(excl.rowptr if excl else None),
        N.ptr(excl.col if excl else None), float(mask_value), k, ns, N.ptr(val), N.ptr(idx),
        N.ptr(ws), ws_bytes, N.stream_handle(dev)), "lg_score_topk_cand_f32")
    return val, idx


def score_cand(eu: torch.Tensor, ei: torch.Tensor, cand: RowSets,
               excl: RowSets | None = None, mask_value: float = MASK_VALUE, users=None,
               max_len: int | None = None) -> torch.Tensor:
    """The scores of the (user, item) pairs of cand (lg_score_cand_f32): fp32 [nnz] in
    cand.col's order, entry p the chain score of (users[r], cand.col[p]), r the row of p, or
    mask_value where the item is in the user's exclusion row; -inf at positions >= max_len of
    their row. Bit for bit score_topk_cand's values. max_len as in score_topk_cand (None: one
    host read)."""
    eu, ei, excl, ids, max_len = _cand_args(eu, ei, cand, excl, users, max_len)
    dev = eu.device
    # (-inf: entries of cand.col outside every row, as a row slice has, are not written)
    out = torch.full((int(cand.col.numel()),), float("-inf"), dtype=torch.float32, device=dev)
    if cand.n_rows == 0 or out.numel() == 0:
        return out
    N.check(N.lib().lg_score_cand_f32(
        N.ptr(eu), N.ptr(ei), N.ptr(ids), cand.n_rows, eu.shape[0], ei.shape[0],
        N.ptr(cand.rowptr), N.ptr(cand.col), max_len, eu.shape[1],
        N.ptr(excl.rowptr if excl else None), N.ptr(excl.col if excl else None),
        float(mask_value), N.ptr(out), N.stream_handle(dev)), "lg_score_cand_f32")
    return out


RANK_ROW_MAX = N.LG_RANK_ROW_MAX  # targets per kernel row of lg_score_rank_f32 (csrc/rank.hip)
RANK_SPLITS_MAX = 4096           # ... and its most item ranges
RANK_ROWS_PER_WAVE = 32          # k_rank_count: 2 groups of 16 rows per wave, 4 waves per block
# rank_splits' constants, from the `split_sweep` of profiles/score_rank.json
# (scripts/score_rank_time.py, 1M items, d = 64). Many rows: the time falls with the waves on the
# device well past the resident set -- 32,768 users x 1 target 40.8 / 33.9 / 32.0 / 31.7 / 31.5 ms
# at 1 / 2 / 4 / 8 / 16 splits (4 .. 64 waves per compute unit), x 4 targets 67.2 / 48.3 / 43.8 /
# 42.2 / 41.3, 13,312 kernel rows 63.1 / 24.6 / 17.5 / 16.3 at 1 / 4 / 8 / 16 -- and gains under
# 2 % past 32 waves per compute unit at 32,768 users. Few rows: 16 and 64 users are fastest from 976
# splits of 1,024 items on (0.15 ms against 0.23 ms at 244 splits of 4,096); shorter splits gain
# nothing and lengthen k_rank_finish's sum.
RANK_WAVES_PER_CU = 32
RANK_MIN_SPLIT = 1024


def rank_splits(n_rows: int, n_items: int, device, cus: int | None = None) -> int:
    """Item ranges (n_splits) for lg_score_rank_f32: 1 when the rows alone give the device
    RANK_WAVES_PER_CU waves per compute unit (a wave counts for 32 rows), else as many as reach
    that target, no range shorter than RANK_MIN_SPLIT items (nor than 16), at most
    RANK_SPLITS_MAX. The ranks do not depend on it. cus: the compute units to plan for
    (default: `device`'s)."""
    if cus is None:
        cus = torch.cuda.get_device_properties(device).multi_processor_count
    waves = max(-(-max(int(n_rows), 1) // RANK_ROWS_PER_WAVE), 1)
    target = RANK_WAVES_PER_CU * int(cus)
    if waves >= target:
        return 1
    return max(1, min(-(-target // waves), int(n_items) // RANK_MIN_SPLIT, RANK_SPLITS_MAX))


def rank_plan_rows(n_rows: int, nnz: int, row_max: int = RANK_ROW_MAX) -> int:
    """The kernel rows rank_splits should plan for, from what the host knows (target rows and
    entries): at least ceil(nnz / row_max), about one per row when rows are short, never more
    than rank_rows' bound. Exact when every row has the same number of targets <= row_max; the
    real count is read nowhere."""
    n_rows, nnz, M = int(n_rows), int(nnz), int(row_max)
    bound = (nnz + (M - 1) * min(n_rows, nnz)) // M
    return max(1, min(bound, max(-(-nnz // M), min(n_rows, nnz))))


def rank_rows(targets: RowSets, users: torch.Tensor | None = None,
              row_max: int = RANK_ROW_MAX):
    """The kernel rows of lg_score_rank_f32 for target rows of any length: (rowptr int64
    [K + 1], user ids int64 [K]). Row r of `targets` with n > 0 targets becomes ceil(n / row_max)
    kernel rows over consecutive runs of its own entries of targets.col, so the kernel's outputs
    stay aligned with targets.col; a row without targets gets none. users: the user id of every
    target row (None: row r is user r). Tensor arithmetic on targets' device, no host read: K is
    the bound (nnz + (row_max - 1) min(n_rows, nnz)) // row_max on the sum of the ceilings, the
    kernel rows past the real ones are empty (user 0) and cost the kernel nothing."""
    rp = targets.rowptr
    dev = rp.device
    R, nnz, M = targets.n_rows, int(targets.col.numel()), int(row_max)
    if R == 0:
        return rp[:1].clone(), torch.zeros(0, dtype=torch.int64, device=dev)
    K = (nnz + (M - 1) * min(R, nnz)) // M
    deg = rp[1:] - rp[:-1]
    kend = torch.cumsum((deg + (M - 1)) // M, 0)  # kernel rows of target rows [0, r]
    j = torch.arange(K + 1, dtype=torch.int64, device=dev)
    src = torch.searchsorted(kend, j, right=True)  # the target row of kernel row j; R: padding
    real = src < R
    srcc = src.clamp(max=max(R - 1, 0))
    kstart = kend - (deg + (M - 1)) // M
    # padding rows and the closing pointer sit at the end of the last row: empty rows
    krp = torch.where(real, rp[srcc] + (j - kstart[srcc]) * M, rp[R:R + 1].expand(K + 1))
    ids = srcc if users is None else users.to(dev, torch.int64)[srcc]
    ids = torch.where(real, ids, torch.zeros_like(ids))[:K]
    return krp.contiguous(), ids.contiguous()


def score_rank(eu: torch.Tensor, ei: torch.Tensor, targets, excl: RowSets | None = None,
               users=None, mask_value: float = MASK_VALUE, n_splits: int | None = None):
    """Where the given (user, item) pairs stand among ALL items (lg_score_rank_f32): (rank int64
    [nnz], score fp32 [nnz]) aligned with the target CSR's col -- rank the number of items that
    come before the target in score_topk's order (score desc, item id asc; excluded items and an
    excluded target at mask_value), 0 = first, and score the target's own value. For finite
    scores rank < k iff score_topk's list of that user holds the item at position rank. The
    held-out-item question of an evaluation (lgcnhs.metrics.rank_metrics takes the ranks).

    targets: anything ops.candidate_rows takes (a dict, one list per row, a (rows, items) pair, a
    RowSets), one row per user -- or per entry of `users`, which has score_topk_cand's meaning.
    Rows of any length: rows longer than RANK_ROW_MAX become several kernel rows (rank_rows; no
    host read). excl: the full tables' exclusion sets, indexed by user id. n_splits: item ranges
    (default: rank_splits); the result does not depend on it. An entry of a RowSets' col outside
    every row, and a target id outside the items, gets {-1, -inf}. No targets: empty tensors (or
    all {-1, -inf}), no launch."""
    eu, ei = _f32_tables(eu, ei)
    nu, d = eu.shape
    dev = eu.device
    R = nu if users is None else int(torch.as_tensor(users).numel())
    if isinstance(targets, RowSets):
        R = targets.n_rows  # (checked against users by _cand_args)
    targets = candidate_rows(targets, R, ei.shape[0], dev)
    eu, ei, excl, ids, _ = _cand_args(eu, ei, targets, excl, users, 1)  # (max_len: no read)
    nnz = int(targets.col.numel())
    rank = torch.full((nnz,), -1, dtype=torch.int64, device=dev)
    score = torch.full((nnz,), float("-inf"), dtype=torch.float32, device=dev)
    if R == 0 or nnz == 0:
        return rank, score
    krp, kids = rank_rows(targets, ids)
    K = int(kids.numel())
    # (planned on the likely count of non-empty kernel rows: the padding rows stream nothing)
    ns = rank_splits(rank_plan_rows(R, nnz), ei.shape[0], dev) if n_splits is None \
        else int(n_splits)
    ws_bytes = N.lib().lg_score_rank_ws_bytes(K, K * RANK_ROW_MAX, d, ns)
    ws = torch.empty(max(ws_bytes, 8), dtype=torch.uint8, device=dev)
    N.check(N.lib().lg_score_rank_f32(
        N.ptr(eu), N.ptr(ei), N.ptr(kids), K, nu, ei.shape[0], N.ptr(krp), N.ptr(targets.col),
        RANK_ROW_MAX, d, N.ptr(excl.rowptr if excl else None),
        N.ptr(excl.col if excl else None), float(mask_value), ns, N.ptr(rank), N.ptr(score),
        N.ptr(ws), ws_bytes, N.stream_handle(dev)), "lg_score_rank_f32")
    return rank, score


def score_dense(eu: torch.Tensor, ei: torch.Tensor, excl: RowSets | None = None,
                mask_value: float = MASK_VALUE) -> torch.Tensor:
    eu, ei = _f32_tables(eu, ei)
    nu, d = eu.shape
    ni = ei.shape[0]
    G = torch.empty((nu, ni), dtype=torch.float32, device=eu.device)
    N.check(N.lib().lg_score_dense_f32(
        N.ptr(eu), N.ptr(ei), nu, ni, d, N.ptr(excl.rowptr if excl else None),
        N.ptr(excl.col if excl else None), float(mask_value), N.ptr(G), ni,
        N.stream_handle(eu.device)), "lg_score_dense_f32")
    return G


# ------------------------------------------------------------------------------ spreading
class Interactions:
    """The 0/1 interaction matrix A held sparse both ways, with degrees as fp64."""

    def __init__(self, by_user: RowSets):
        self.by_user = by_user
        self.by_item = by_user.transpose()
        self.n_users, self.n_items = by_user.n_rows, by_user.n_cols
        self.k_user = by_user.degrees().to(torch.float64)
        self.k_item = self.by_item.degrees().to(torch.float64)
        self._rows_long = None

    @property
    def rows_long(self):
        """(by user, by item) long-list tables of the basket spreading (_long_lists: the lists
        longer than SPREAD_ROWS_SEG), built on first use from by_user / by_item as they stand
        then -- an Interactions is not edited after construction."""
        if self._rows_long is None:
            self._rows_long = (_long_lists(self.by_user), _long_lists(self.by_item))
        return self._rows_long

    @classmethod
    def from_pairs(cls, users, items, n_users, n_items, device=None):
        return cls(RowSets.from_pairs(users, items, n_users, n_items, device))

    @classmethod
    def from_dense(cls, A: torch.Tensor):
        """From a dense [U, I] matrix (nonzero = interaction), e.g. the reference's A."""
        N.require_gpu(A, "A")
        nz = torch.nonzero(A != 0)
        return cls.from_pairs(nz[:, 0], nz[:, 1], A.shape[0], A.shape[1], A.device)


def spread_general(A: Interactions) -> torch.Tensor:
    gW = torch.empty((A.n_items, A.n_items), dtype=torch.float64, device=A.k_item.device)
    N.check(N.lib().lg_spread_general_f64(
        N.ptr(A.by_item.rowptr), N.ptr(A.by_item.col), N.ptr(A.by_user.rowptr),
        N.ptr(A.by_user.col), A.n_users, A.n_items, N.ptr(gW),
        N.stream_handle(gW.device)), "lg_spread_general_f64")
    return gW


def hybrid_weight(gW: torch.Tensor, k_item: torch.Tensor, lam: float,
                  transpose: bool = False) -> torch.Tensor:
    N.require_gpu(gW, "gW")
    gW = _aligned(gW.to(torch.float64))
    k_item = _aligned(k_item.to(torch.float64))
    W = torch.empty_like(gW)
    N.check(N.lib().lg_hybrid_weight_f64(N.ptr(gW), N.ptr(k_item), gW.shape[0], float(lam),
                                         int(bool(transpose)), N.ptr(W),
                                         N.stream_handle(gW.device)), "lg_hybrid_weight_f64")
    return W


def spread_hybrid(A: Interactions, lam: float) -> torch.Tensor:
    """hybrid_weight(spread_general(A), A.k_item, lam) (either transpose: general_W is
    exactly symmetric) bit for bit, without general_W in memory (lg_spread_hybrid_f64)."""
    dev = A.k_item.device
    I = A.n_items
    W = torch.empty((I, I), dtype=torch.float64, device=dev)
    ws = torch.empty(max(1, N.lib().lg_spread_hybrid_ws_bytes(I, A.n_users)),
                     dtype=torch.uint8, device=dev)
    N.check(N.lib().lg_spread_hybrid_f64(
        N.ptr(A.by_item.rowptr), N.ptr(A.by_item.col), N.ptr(A.by_user.rowptr),
        N.ptr(A.by_user.col), N.ptr(A.k_item), A.n_users, I, float(lam), N.ptr(W), N.ptr(ws),
        ws.numel(), N.stream_handle(dev)), "lg_spread_hybrid_f64")
    return W


def spread_resource(A: Interactions, W: torch.Tensor, users: slice | None = None,
                    out: torch.Tensor | None = None) -> torch.Tensor:
    """F rows for users [u0, u1) (all by default). W: float64 [I, I] on A's device. out: a
    float64 buffer of at least [u1 - u0, I] with unit column stride (rows [0, u1 - u0) and
    columns [0, I) are written; its row stride is kept)."""
    u0, u1 = (0, A.n_users) if users is None else (users.start, users.stop)
    I = A.n_items
    _check_W(W, I)
    _same_device(W, "W", A.by_user.col, "A")
    if not 0 <= u0 <= u1 <= A.n_users:
        raise ValueError(f"users [{u0}, {u1}) outside [0, {A.n_users}]")
    if out is not None:
        _typed(out, "out", torch.float64)
        if out.shape[0] < u1 - u0 or out.shape[1] < I or (out.numel() and out.stride(1) != 1):
            raise ValueError(f"out has shape {tuple(out.shape)} strides {out.stride()}, "
                             f"expected at least ({u1 - u0}, {I}) with unit column stride")
        _same_device(out, "out", W, "W")
    W = _f64(W, "W")
    F = out if out is not None else torch.empty((u1 - u0, I), dtype=torch.float64,
                                                device=W.device)
    _resource_rows(A.by_user.rowptr[u0:], A.by_user.col, W, u1 - u0, F)
    return F


F_BLOCK_BYTES = 1 << 30  # of F per block of _f_blocks (read at call time)


def _check_W(W, I: int, expected: str | None = None) -> None:
    """TypeError / ValueError unless W is a float64 [I, I] tensor (no device check): the one
    check of the W that _f_blocks and spread_resource read."""
    _typed(W, "W", torch.float64)
    if tuple(W.shape) != (I, I):
        raise ValueError(f"W has shape {tuple(W.shape)}, expected {expected or f'({I}, {I})'}")


def _resource_rows(rowptr, col, W, n: int, F) -> None:
    """F[:n] = the n rows that start at rowptr (offsets into col) times the checked W."""
    N.check(N.lib().lg_spread_resource_f64(
        N.ptr(rowptr), N.ptr(col), N.ptr(W), n, W.shape[0], N.ptr(F), F.stride(0),
        N.stream_handle(W.device)), "lg_spread_resource_f64")


def _f_blocks(rows: RowSets, W: torch.Tensor, block_users: int | None = None):
    """Yield (b0, b1, Fb) over row blocks of F = rows @ W (rows: A.by_user or taken rows of
    it): Fb = F[b0:b1] in one reused float64 buffer, overwritten by the next block.
    F_BLOCK_BYTES of F per block, or block_users rows. W: checked by the caller (_check_W)."""
    n, I = rows.n_rows, rows.n_cols
    _same_device(W, "W", rows.col, "A")
    N.require_gpu(W, "W")
    W = _aligned(W)
    block = max(1, min(n, F_BLOCK_BYTES // max(1, I * 8))) if block_users is None \
        else max(1, int(block_users))
    buf = torch.empty((min(block, n), I), dtype=torch.float64, device=W.device)
    for b0 in range(0, n, block):
        b1 = min(n, b0 + block)
        _resource_rows(rows.rowptr[b0:], rows.col, W, b1 - b0, buf)
        yield b0, b1, buf[: b1 - b0]


def rows_topk(F: torch.Tensor, k: int, excl: RowSets | None = None, drop: bool = True,
              eu: torch.Tensor | None = None, ei: torch.Tensor | None = None):
    """Per-row top-k of F (optionally times the fp32 score G = eu . ei), excluded columns
    dropped (drop=True) or kept (drop=False). Returns (values fp64, indices int64, -1 pad).
    k <= 128 runs lg_rows_topk_f64 (lists sorted in registers), 128 < k <= 1024
    lg_rows_topk_wide_f64 (same values, order and padding; lists in LDS)."""
    k = int(k)
    if k < 1 or k > 1024:
        raise ValueError(f"k={k} not in [1, 1024]")
    _typed(F, "F", torch.float64)
    n, m = F.shape
    if eu is not None:
        _g_guard(eu, ei, n, m, f"F is {n} x {m}: ")
    _excl_guard(excl, n, "rows of F")
    N.require_gpu(F, "F")
    if F.numel() and (F.stride(1) != 1 or F.data_ptr() % 16):
        F = _aligned(F)  # (a row-strided view of a larger buffer is taken as it is)
    d = 0
    if eu is not None:
        eu, ei = _f32_tables(eu, ei)
        d = eu.shape[1]
    val = torch.empty((n, k), dtype=torch.float64, device=F.device)
    idx = torch.empty((n, k), dtype=torch.int64, device=F.device)
    name = "lg_rows_topk_f64" if k <= 128 else "lg_rows_topk_wide_f64"
    N.check(getattr(N.lib(), name)(
        N.ptr(F), F.stride(0), n, m, N.ptr(eu), N.ptr(ei), d,
        N.ptr(excl.rowptr if excl else None), N.ptr(excl.col if excl else None),
        N.LG_EXCL_DROP if drop else N.LG_EXCL_NONE, k, N.ptr(val), N.ptr(idx),
        N.stream_handle(F.device)), name)
    return val, idx


def spread_topk(A: Interactions, W: torch.Tensor, k: int, excl: RowSets | None,
                drop: bool = True, eu: torch.Tensor | None = None,
                ei: torch.Tensor | None = None, block_users: int | None = None):
    """F = A @ W computed block by block and reduced to per-user top-k without ever
    holding all of F (the fused recommend path of SpreadMethod / SpreadLightGCN)."""
    return _blocks_topk(A.by_user, W, k, excl, drop, eu, ei, block_users)


def _blocks_topk(rows: RowSets, W: torch.Tensor, k: int, ex: RowSets | None, drop: bool,
                 eu_r, ei, block_users: int | None = None):
    """rows_topk of every F block of ``rows`` (ex, eu_r: their exclusion and eu rows)."""
    n = rows.n_rows
    _check_W(W, rows.n_cols)
    vals = torch.empty((n, k), dtype=torch.float64, device=W.device)
    idxs = torch.empty((n, k), dtype=torch.int64, device=W.device)
    for b0, b1, Fb in _f_blocks(rows, W, block_users):
        vals[b0:b1], idxs[b0:b1] = rows_topk(
            Fb, k, ex.slice_rows(b0, b1) if ex is not None else None, drop,
            None if eu_r is None else eu_r[b0:b1], ei)
    return vals, idxs


ROWS_RANK_ROW_MAX = N.LG_ROWS_RANK_ROW_MAX  # targets per kernel row (csrc/rows_rank.hip)


def rows_rank(F: torch.Tensor, targets, excl: RowSets | None = None, drop: bool = True,
              eu: torch.Tensor | None = None, ei: torch.Tensor | None = None, out=None):
    """Where the given (row, column) targets stand among ALL columns of F's rows
    (lg_rows_rank_f64): (rank int64 [nnz], value fp64 [nnz]) aligned with the target CSR's col.
    value is v(r, i) = F[r, i], or with eu / ei the fp32 chain score promoted to fp64 times
    F[r, i] -- rows_topk's values bit for bit. A column ranks iff its value is > -inf (NaN and
    -inf never rank) and, with drop=True, it is not in the row's exclusions; rank is the number
    of ranking columns before the target under (value desc, column asc), 0 = first, or -1 for
    a target that does not rank itself. For any k <= 1024: rank < k iff rows_topk(F, k, ...)
    holds the target at [r, rank].

    targets: anything candidate_rows takes, one row per row of F. A RowSets is taken as it is:
    its columns may come in any order, a column named twice gets the same rank twice, an
    entry of col outside every row and a column id outside F get {-1, -inf}. Rows of any length:
    longer than ROWS_RANK_ROW_MAX they become several kernel rows (rank_rows; no host read).
    No targets: no launch. out: a (rank, value) pair of contiguous [nnz] tensors to write
    into instead of fresh ones (only the entries of the targets' rows are written: callers
    that rank F block by block over row slices of one target CSR, as spread_rank does)."""
    _typed(F, "F", torch.float64)
    n, m = F.shape
    if eu is not None or ei is not None:
        _g_guard(eu, ei, n, m, f"F is {n} x {m}: ")
    _excl_guard(excl, n, "rows of F", eu is not None and not drop)
    if isinstance(targets, RowSets) and targets.n_rows != n:
        raise ValueError(f"target rows {targets.n_rows} != rows of F {n}")
    N.require_gpu(F, "F")
    dev = F.device
    targets = candidate_rows(targets, n, m, dev)
    if targets.col.device != dev:
        raise ValueError(f"targets are on {targets.col.device}, F on {dev}")
    if excl is not None and excl.col.device != dev:
        raise ValueError(f"excl is on {excl.col.device}, F on {dev}")
    if F.numel() and (F.stride(1) != 1 or F.data_ptr() % 16):
        F = _aligned(F)  # (a row-strided view of a larger buffer is taken as it is)
    d = 0
    if eu is not None:
        eu, ei = _f32_tables(eu, ei)
        d = eu.shape[1]
    excl = _nonempty(excl)
    nnz = int(targets.col.numel())
    if out is None:
        rank = torch.full((nnz,), -1, dtype=torch.int64, device=dev)
        val = torch.full((nnz,), float("-inf"), dtype=torch.float64, device=dev)
    else:
        rank, val = out
        _typed(rank, "out[0]", torch.int64, 1)
        _typed(val, "out[1]", torch.float64, 1)
        for t in (rank, val):
            if t.numel() != nnz or not t.is_contiguous() or t.device != dev:
                raise ValueError(f"out must be contiguous [{nnz}] tensors on {dev}")
    if n == 0 or m == 0 or nnz == 0:
        return rank, val
    if nnz <= ROWS_RANK_ROW_MAX:
        # no row can be longer than a kernel row: the target rows are the kernel rows (the
        # request-sized call -- a few users -- is host work, and rank_rows is most of it)
        krp, krow = targets.rowptr, torch.arange(n, dtype=torch.int64, device=dev)
    else:
        krp, krow = rank_rows(targets, None, row_max=ROWS_RANK_ROW_MAX)
    N.check(N.lib().lg_rows_rank_f64(
        N.ptr(F), F.stride(0), n, m, N.ptr(eu), N.ptr(ei), d,
        N.ptr(excl.rowptr if excl else None), N.ptr(excl.col if excl else None),
        N.LG_EXCL_DROP if drop else N.LG_EXCL_NONE, int(krow.numel()), N.ptr(krow), N.ptr(krp),
        N.ptr(targets.col), N.ptr(rank), N.ptr(val), N.stream_handle(dev)), "lg_rows_rank_f64")
    return rank, val


# ------------------------------------------------------------------- factored spreading
INV_TAB = 512      # degree classes cached in LDS by the walk (kInvTab, csrc/tile_lines.h)
MAX_CLASSES = 0x7FFF   # P slot words keep bit 31 clear (it marks V entries)
LINE_SLOTS, LINE_ENTS = 31, 7   # P slots / V entries in a row's 128-byte line
GROUP_MAX, GROUP_WIDE = 16, 8   # tiles per group build (tiles wider than 4096: 8)
OVF_UNITS_MAX = 1 << 29  # a group's overflow units (the rows' 29-bit overflow pointers)


def hybrid_recip(k_item: torch.Tensor, lam: float):
    """(ra, rb) = (1 / k_i^(1-lambda), 1 / k_i^lambda), a zero factor -> 1: the walk's
    HybridS factors (lg_hybrid_recip_f64)."""
    k_item = k_item.contiguous().to(torch.float64)
    n = k_item.shape[0]
    ra = torch.empty(n, dtype=torch.float64, device=k_item.device)
    rb = torch.empty_like(ra)
    N.check(N.lib().lg_hybrid_recip_f64(N.ptr(k_item), n, float(lam), N.ptr(ra), N.ptr(rb),
                                        N.stream_handle(k_item.device)), "lg_hybrid_recip_f64")
    return ra, rb


class HybridScale:
    """The lambda-dependent side of the factored spreading: rb = 1/beta per item and
    ra_edge = 1/alpha of the item of every interaction, aligned with A.by_user.col (so the
    walk reads a user's factors contiguously with its item ids). ``cols`` (a column view,
    see TileWeights): rb of those items only, by position; ra_edge is row-side and stays."""

    def __init__(self, A: "Interactions", lam: float, cols: torch.Tensor | None = None):
        self.lam = float(lam)
        ra, self.rb = hybrid_recip(A.k_item, lam)
        if cols is not None:
            self.rb = self.rb[cols.to(torch.int64)]
        # one entry past the interactions: the walk's padding rows read it (never used)
        self.ra_edge = torch.cat([ra[A.by_user.col.to(torch.int64)], ra.new_zeros(1)])


def degree_classes(deg: torch.Tensor):
    """(1-based class of each row's degree as uint16, fp64 table inv[c] = fl(1/k) of class
    c, inv[0] = 0): the slot code of the P rows of csrc/tile_lines.h. Classes are
    numbered by how many rows have the degree, so the common ones fall in the walk's LDS
    table (c < 512). Rows of degree 0 get class 0 (they are in no pair)."""
    dev = deg.device
    pos = deg[deg > 0]
    if pos.numel() == 0:
        return (torch.zeros(deg.numel(), dtype=torch.int16, device=dev).view(torch.uint16),
                torch.zeros(INV_TAB, dtype=torch.float64, device=dev))
    uniq, counts = torch.unique(pos, return_counts=True)
    if uniq.numel() >= MAX_CLASSES:
        raise ValueError(f"{uniq.numel()} distinct user degrees: the tile format encodes at "
                         f"most {MAX_CLASSES - 1} (use the dense spreading path)")
    order = torch.argsort(counts, descending=True, stable=True)
    rank = torch.empty_like(order)
    rank[order] = torch.arange(order.numel(), device=dev)
    cls = torch.zeros(deg.numel(), dtype=torch.int32, device=dev)
    m = deg > 0
    cls[m] = (rank[torch.searchsorted(uniq, deg[m])] + 1).to(torch.int32)
    inv = torch.zeros(max(INV_TAB, uniq.numel() + 1), dtype=torch.float64, device=dev)
    inv[1:uniq.numel() + 1] = 1.0 / uniq[order].to(torch.float64)
    return cls.to(torch.int16).view(torch.uint16), inv


def _run_units(length: torch.Tensor, hub: torch.Tensor) -> torch.Tensor:
    """Overflow units (run header + data) of rows with `length` pairs (P) / entries (V)."""
    p = torch.where(length > LINE_SLOTS, 1 + (length - LINE_SLOTS + 3) // 4,
                    torch.zeros_like(length))
    v = torch.where(length > LINE_ENTS, 1 + (length - LINE_ENTS), torch.zeros_like(length))
    return torch.where(hub, v, p)


class TileWeights:
    """general_W restricted to one item tile, in the line format of csrc/tile_lines.h
    (lg_spread_tile_rows_f64: one 128-byte line per item row at 128 * i, plus overflow runs;
    P rows = the (user, item) pairs behind the row as 4-byte slots, V rows = the merged fp64
    general_W values of hub items). The tile itself is lambda-independent; ``lam`` sets the
    HybridScale the walk applies. build() moves to the next tile; the buffers are
    reused and grown on demand. ``vthr``: rows with more pairs are V rows (default: the tile
    width).

    Tiles are built ``group`` at a time (1..16, default 16; at most 8 for tiles wider than
    4096): lg_spread_group_cursor / _bound / _units / _rows_f64 visit each (item row, user)
    pair once per group instead of once per tile and write the group's tiles side by side; build(j0) of a tile inside the built
    group only selects it. Every tile's words are those of the per-tile reference build
    (include/lgcnhs_ref.h) bit for bit (tests/test_gpu_spread_tiled.py).

    ``cols`` (a column view: strictly ascending int32 item ids on the device, the candidate
    set of spread_topk_tiled(items=...)): the tiles then hold the columns cols[0], cols[1], ..
    of general_W, numbered by position -- tile t is positions [t tile, (t + 1) tile) and there
    are ceil(len(cols) / tile) of them. The build kernels keep two id spaces apart: rows
    (A.by_item, the row count n_items, inv_deg and the degree classes: the full graph, full
    degrees) and columns (the user -> column CSR they cursor through, group_begin / tile /
    stop), and only the second becomes A.by_user.restrict_cols(cols). Without ``cols`` the
    column CSR is A.by_user itself and nothing is gathered."""

    def __init__(self, A: Interactions, lam: float, tile: int, vthr: int | None = None,
                 group: int | None = None, cols: torch.Tensor | None = None):
        if not 1 <= tile <= 8192:
            raise ValueError(f"tile {tile} not in [1, 8192]")
        self.A, self.tile, self.lam = A, int(tile), float(lam)
        dev = A.k_item.device
        self.dev = dev
        # the column side: user -> column sets and the column count
        self.cols = cols
        self.col_sets = A.by_user if cols is None else A.by_user.restrict_cols(cols)
        self.n_cols = A.n_items if cols is None else int(cols.numel())
        if vthr is None:
            vthr = self.tile
        self.vthr = max(LINE_SLOTS, int(vthr))
        gmax = GROUP_MAX if self.tile <= 4096 else GROUP_WIDE
        self._auto_group = group is None  # (a default group halves itself when too large)
        if group is None:
            group = gmax
        if not 1 <= group <= gmax:
            raise ValueError(f"group {group} not in [1, {gmax}] (tile {self.tile})")
        if self.vthr > 65535:
            raise ValueError(f"vthr {self.vthr} > 65535 (the group build counts 16-bit)")
        I = A.n_items
        self.group = int(min(group, max(1, -(-self.n_cols // self.tile))))
        S = self.group
        self.cur = self.col_sets.rowptr[:-1].contiguous().clone()
        self.end = torch.empty_like(self.cur)
        # 16 uint16 per user (two 16-byte halves: tiles 0-7, 8-15) + the rows pass's 16-byte
        # records
        if int(A.by_user.rowptr[-1]) >= 1 << 32:
            raise ValueError("more than 2^32 interactions: the group build's positions are "
                             "32-bit")
        self.counts = torch.empty((A.n_users, GROUP_MAX), dtype=torch.uint16, device=dev)
        self.rec = torch.empty((A.n_users, 4), dtype=torch.int32, device=dev)
        self.inv_deg = torch.empty(A.n_users, dtype=torch.float64, device=dev)
        N.check(N.lib().lg_inv_degree_f64(N.ptr(A.by_user.rowptr), A.n_users,
                                          N.ptr(self.inv_deg), N.stream_handle(dev)),
                "lg_inv_degree_f64")
        self.user_cls, self.inv_cls = degree_classes(A.by_user.degrees())
        self.g_bound = torch.empty((S, I), dtype=torch.int64, device=dev)
        # run units per (tile, row), their flat inclusive scan, the tiles' ends
        self.g_units = torch.empty(S * I, dtype=torch.int64, device=dev)
        self.g_incl = torch.empty(max(1, S * I), dtype=torch.int64, device=dev)
        self._tile_ends = torch.arange(1, S + 1, dtype=torch.int64, device=dev) * I - 1
        self._ends_host = torch.empty(S, dtype=torch.int64).pin_memory()
        self._ends_ev = torch.cuda.Event()
        # I + 1 lines per tile: line I (the walk's padding row) stays all zero
        self.g_lines = torch.empty((S, (I + 1) * 32), dtype=torch.int32, device=dev)
        self.g_lines[:, I * 32:].zero_()
        self.g_row_len = torch.empty((S, max(1, I)), dtype=torch.int32, device=dev)
        ws = N.lib().lg_spread_group_rows_ws_bytes(I, S)
        self.ws = torch.empty(max(1, ws), dtype=torch.uint8, device=dev)
        self.g_ovf = torch.zeros(64 * 4, dtype=torch.int32, device=dev)
        self._grp = None  # (first item, [widths], [ovf bases], [overflow units]) built
        self.j0 = None
        self.width = 0
        self._seek_at = None
        self._scale = None
        self.row_uses = None  # set by spread_topk_tiled(stats=...)

    @property
    def scale(self) -> HybridScale:
        if self._scale is None:
            self._scale = HybridScale(self.A, self.lam, self.cols)
        return self._scale

    @property
    def is_hub(self) -> torch.Tensor:
        """True for V (merged-value) rows of the current tile."""
        return self.bound > self.vthr

    def dense(self) -> torch.Tensor:
        """general_W of the current tile as a dense [I, width] fp64 matrix (host, test
        helper), decoded from the lines with the format invariants checked: P slots summed in
        slot order (users ascending: lg_spread_general_f64's order), V values as stored."""
        I = self.A.n_items
        lines = self.lines[:I * 32].cpu().numpy().view(np.uint32).reshape(I, 32)
        ovf = self.ovf.cpu().numpy().view(np.uint32)
        inv = self.inv_cls.cpu().numpy()
        rl = self.row_len.cpu().numpy()
        hub = self.is_hub.cpu().numpy()
        out = np.zeros((I, self.width))
        for i in range(I):
            h = int(lines[i, 0])
            isv, has, slow, ou = h >> 31, (h >> 30) & 1, (h >> 29) & 1, h & 0x1FFFFFFF
            assert bool(isv) == bool(hub[i]) and (slow or not isv)
            run = np.zeros((0, 4), np.uint32)
            if has and not (isv and int(ovf[4 * ou]) >> 31):
                n = int(ovf[4 * ou])
                assert np.all(ovf[4 * ou + 1:4 * ou + 4] == 0)
                run = ovf[4 * (ou + 1):4 * (ou + 1 + n)].reshape(n, 4)
            if isv and has and int(ovf[4 * ou]) >> 31:  # a dense V row
                nd = int(ovf[4 * ou]) & 0x7FFFFFFF
                assert nd == (self.width + 1) // 2 and np.all(lines[i, 1:] == 0)
                run = ovf[4 * (ou + 1):4 * (ou + 1 + nd)].reshape(nd, 4)
                vals = run.reshape(-1).view(np.uint64).view(np.float64)  # (lo, hi) pairs
                assert np.all(vals[self.width:] == 0) and int((vals != 0).sum()) == rl[i]
                assert rl[i] > self.width // 2 + 8
                out[i, :] = vals[:self.width]
                continue
            if isv:
                assert rl[i] <= self.width // 2 + 8
                assert np.all(lines[i, 1:4] == 0)
                units = np.concatenate([lines[i, 4:].reshape(7, 4), run])
                units = units[units[:, 0] != 0]
                assert units.shape[0] == rl[i] and np.all(units[:, 0] >> 31 == 1)
                col = (units[:, 0] & 0xFFFF).astype(np.int64)
                assert np.all(np.diff(col) > 0) and np.all(col < self.width)
                out[i, col] = (units[:, 1].astype(np.uint64) |
                               (units[:, 2].astype(np.uint64) << 32)).view(np.float64)
                continue
            words = np.concatenate([lines[i, 1:], run.reshape(-1)])
            n = int(rl[i])
            assert np.all(words[:n] != 0) and np.all(words[n:] == 0)
            col = (words[:n] & 0xFFFF).astype(np.int64)
            cls = (words[:n] >> 16).astype(np.int64)
            assert np.all(col < self.width) and np.all(cls > 0)
            assert bool(slow) == bool(np.any(cls >= INV_TAB))
            for c, q in zip(col, cls):
                out[i, c] += inv[q]
        return out

    def seek(self, j0: int) -> None:
        """Start the tile walk at item j0 instead of 0 (an item-range shard): the next
        build() must be build(j0)."""
        A, cs = self.A, self.col_sets
        if not 0 <= j0 <= self.n_cols:
            raise ValueError(f"seek({j0}) outside [0, {self.n_cols}]")
        N.check(N.lib().lg_spread_tile_seek(N.ptr(cs.rowptr), N.ptr(cs.col),
                                            A.n_users, j0, N.ptr(self.cur),
                                            N.stream_handle(self.dev)), "lg_spread_tile_seek")
        self._seek_at = j0

    def build(self, j0: int, stop: int | None = None) -> None:
        """Build the tile [j0, min(j0 + tile, stop)); tiles come in ascending order from 0
        (or from the item given to seek()). Builds the group starting at j0 unless j0 is the
        next tile of the group already built."""
        I = self.n_cols  # (the column count: the catalog's, or the column view's)
        stop = I if stop is None else min(int(stop), I)
        g = self._grp
        if (g is not None and self._seek_at is None and self.j0 is not None
                and j0 == self.j0 + self.width and j0 < g[0] + sum(g[1])):
            self._select((j0 - g[0]) // self.tile)
            return
        if self._seek_at is not None and j0 == self._seek_at:
            pass  # cursors placed by seek()
        elif j0 == 0:
            self.cur.copy_(self.col_sets.rowptr[:-1])
        elif self.j0 is None or j0 != self.j0 + self.width:
            raise ValueError("tiles must be built in ascending order")
        else:
            self.cur, self.end = self.end, self.cur
        self._seek_at = None
        if stop - j0 <= 0:
            raise ValueError(f"empty tile at {j0} (stop {stop})")
        widths = [min(self.tile, stop - t0) for t0 in
                  range(j0, min(stop, j0 + self.group * self.tile), self.tile)]
        self._build_group(j0, stop, widths)
        self._select(0)

    def _build_group(self, j0: int, stop: int, widths: list) -> None:
        A, I, L = self.A, self.A.n_items, N.lib()
        cs = self.col_sets  # (j0, stop and the tiles are column positions; I counts rows)
        strm = N.stream_handle(self.dev)
        nt = len(widths)
        # group: cursors, bounds, run units and their inclusive scan all on the device; one
        # event wait for the tiles' unit totals (to size ovf), then the rows
        N.check(L.lg_spread_group_cursor(N.ptr(cs.rowptr), N.ptr(cs.col),
                                         N.ptr(self.user_cls), A.n_users, j0, self.tile, nt,
                                         stop, N.ptr(self.cur), N.ptr(self.end),
                                         N.ptr(self.counts), N.ptr(self.rec), strm),
                "lg_spread_group_cursor")
        N.check(L.lg_spread_group_bound(N.ptr(A.by_item.rowptr), N.ptr(A.by_item.col), I,
                                        N.ptr(self.counts), nt, N.ptr(self.g_bound), strm),
                "lg_spread_group_bound")
        if I:
            units = self.g_units[:nt * I]
            N.check(L.lg_spread_group_units(N.ptr(self.g_bound), I, j0, self.tile, nt, stop,
                                            self.vthr, N.ptr(units), strm),
                    "lg_spread_group_units")
            incl = self.g_incl[:nt * I]
            torch.cumsum(units, 0, out=incl)
            ends = torch.index_select(incl, 0, self._tile_ends[:nt])
            self._ends_host[:nt].copy_(ends, non_blocking=True)
            self._ends_ev.record()
            self._ends_ev.synchronize()  # the tiles' last units (not the whole stream's work)
            ends = self._ends_host[:nt].tolist()
        else:
            ends = [0] * nt
        bases = [0] + ends[:-1]
        totals = [e - b for e, b in zip(ends, bases)]
        if ends[-1] + 64 >= OVF_UNITS_MAX:
            if self._auto_group and nt > 1:
                # the default group size: retry this group (and build the later ones) with
                # half as many tiles -- the cursor kernel reads cur and rewrites only end
                self.group = nt // 2
                self._build_group(j0, stop, widths[:self.group])
                return
            raise ValueError("tile group too large for the 29-bit overflow pointers (use a "
                             "smaller tile or group)")
        self._grow_ovf(ends[-1])
        N.check(L.lg_spread_group_rows_f64(
            N.ptr(A.by_item.rowptr), N.ptr(A.by_item.col), N.ptr(cs.col),
            N.ptr(self.inv_deg), I, N.ptr(self.cur), N.ptr(self.counts), N.ptr(self.rec),
            j0, self.tile, nt, stop, N.ptr(self.g_bound), self.vthr,
            N.ptr(self.g_incl), N.ptr(self.g_lines), N.ptr(self.g_ovf),
            N.ptr(self.g_row_len), N.ptr(self.ws), self.ws.numel(), strm),
            "lg_spread_group_rows_f64")
        self._grp = (j0, widths, bases, totals)

    def _grow_ovf(self, units: int) -> None:
        need = (units + 64) * 4
        if need > self.g_ovf.numel():
            self.g_ovf = torch.zeros(max(need, int(self.g_ovf.numel() * 1.25)),
                                     dtype=torch.int32, device=self.dev)

    def _select(self, t: int) -> None:
        """Make tile t of the built group the current tile (lines / ovf / bound / row_len
        views, j0, width, n_units)."""
        g0, widths, bases, totals = self._grp
        I = self.A.n_items
        self.j0, self.width = g0 + t * self.tile, widths[t]
        self.lines = self.g_lines[t]
        self.ovf = self.g_ovf[bases[t] * 4:]
        self.bound = self.g_bound[t]
        self.row_len = self.g_row_len[t]
        self.n_units = totals[t]
        if self.row_uses is not None:
            hub = self.is_hub
            ln = self.row_len[:I].to(torch.int64)
            self.paths_read += (self.row_uses * ln).sum()
            self.paths_hub += (self.row_uses * ln * hub[:I]).sum()  # (V rows' share)
            used = _run_units(ln, hub)
            # (dense V rows: ceil(width / 2) data units + the header, whatever their entries)
            used = torch.where(hub[:I] & (ln > self.width // 2 + 8),
                               torch.full_like(used, 1 + (self.width + 1) // 2), used)
            self.bytes_read += 128 * self.row_uses.sum() + 16 * (self.row_uses * used).sum()


def _walk_tile(tile: int, n_cols: int, g: bool) -> int:
    """The walk's tile width: no wider than its columns, than 4096 with a G factor (64 chunk
    bounds of 64 columns) and than 8192 without."""
    return min(int(tile), n_cols, 4096 if g else 8192)


def _user_side(A: Interactions, ids, excl: RowSets | None, eu, return_index: bool = False):
    """(rows, edge_src, ex, eu_r): the interaction, exclusion and eu rows of the users ``ids``
    (RowSets.take, eu[ids]; edge_src: with return_index the taken entries' positions in
    A.by_user.col, else None). ids None: A.by_user, None, excl and eu themselves -- no copy, no
    host read."""
    if ids is None:
        return A.by_user, None, excl, eu
    rows, src = A.by_user.take(ids, return_index=True) if return_index \
        else (A.by_user.take(ids), None)
    return (rows, src, None if excl is None else excl.take(ids),
            None if eu is None else eu[ids])


def spread_topk_tiled(A: Interactions, lam: float, k: int, excl: RowSets | None,
                      drop: bool = True, eu: torch.Tensor | None = None,
                      ei: torch.Tensor | None = None, users=None,
                      tile: int = 2048, items=None,
                      stats: dict | None = None, count_paths: bool = False,
                      col_bounds: bool = True, **_):
    """Per-user top-k of (G *) F, F = A @ HybridS(A, general_W, lam), over item tiles:
    never holds general_W, W (I x I) or F (U x I). The values of spread_topk(A,
    hybrid_weight(spread_general(A), A.k_item, lam), ...) within a few ulp (the walk's
    summation order), the lists equal except near-ties.

    Each tile of general_W (user-independent) is built once and walked by every user
    (lg_spread_tile_resource_topk_f64): the user's F columns are summed in LDS and merged
    into its running top-k list in the same pass. With a G factor (SpreadLightGCN) the
    per-(user, 64-column chunk) score bounds of lg_score_chunk_bound (bf16 MFMA) screen the
    columns, so only those whose bound times F can beat the list's k-th value get the exact
    fp32 score chain. ``users`` restricts the output to a row range (slice) or to any user ids
    (tensor / list, any order, duplicates allowed: the walk then runs on the taken user-side
    rows, bitwise the all-users rows); ``items`` as a slice restricts the
    candidates to an item range (the lists of disjoint item ranges merge, with
    merge_topk_lists, into the full lists: the multi-GPU item shard). Any other ``items``
    (ids, a bool mask, an ascending device tensor: item_candidates) is a candidate set C: the
    same kernels walk a column view of general_W (TileWeights / TileWalk ``cols``: the
    user -> column CSR restricted to C, rb[C], ei[C], the exclusions restricted to C),
    ceil(|C| / tile) tiles instead of ceil(I / tile), while the rows -- every path
    u -> i -> v -> j with the full degrees -- stay the whole graph's; the lists hold item
    ids. Which rows of a tile are merged (V) rows depends on the pairs behind them in that
    tile, so a candidate tile may sum a column in another order than the full walk: values
    within 1e-12 relative of the dense path, as without ``items``, and bitwise the
    no-``items`` call only for C = every item. (The two-kernel form
    -- F written per tile, then a top-K merge -- is a test reference, tests/_ref_paths.py.)
    ``stats`` (optional dict) receives the HIP-event times of the tile
    builds / score bounds / walk launches (t_*_ms, walk_launches) and the walk's (user, item)
    rows per launch; with ``count_paths`` also "w_paths": the paths the walk adds (sum over
    tiles and users u of sum_{i in items(u)} the pairs (P) / entries (V) of row i in the
    tile) and "w_bytes": the row bytes it gathers (one 128-byte line per (user, item) and
    tile, plus 16 bytes per overflow unit) -- extra GPU work per tile, so timed runs leave it
    off and take the counts from tile_traffic().

    The walk's lists hold k <= 128 entries. 128 < k <= 1024 is served by peeling: ceil(k / 128)
    complete walks, pass p asking for min(128, k - 128 p) entries with the items the earlier
    passes found added to its (dropped) exclusions, its lists written to columns
    [128 p, 128 p + its k). The walk is an exact top-k under (value desc, item asc) for any
    exclusion set and the F it sums depends on neither k nor the exclusions, so the
    concatenation is the exact top-k of the walk's own F and its first 128 columns are
    bitwise the k = 128 call's. Cost: ceil(k / 128) x the k = 128 job (plus the exclusion
    rebuilds, "t_excl_ms" in ``stats``); a pass after which every row is exhausted ends the
    peel."""
    k = int(k)
    if k > 1024:
        raise ValueError(f"k={k} not in [1, 1024]")
    if k > PEEL_K:
        return _spread_topk_tiled_peeled(A, lam, k, excl, drop, eu, ei, users, tile, items,
                                         stats, count_paths, col_bounds)
    dev = A.k_item.device
    # users: a row range (slice) or any user ids (tensor / list: rows in that order)
    ids = None if users is None or isinstance(users, slice) else _user_ids(users, A.n_users, dev)
    if ids is not None:
        u0, u1 = 0, int(ids.numel())
    else:
        u0, u1 = (0, A.n_users) if users is None else (users.start, users.stop)
    cand = None  # a candidate set: the walk's columns are then positions [0, |C|) in it
    if items is None or isinstance(items, slice):
        i0, i1 = (0, A.n_items) if items is None else (max(0, items.start),
                                                       min(A.n_items, items.stop))
    else:
        cand = item_candidates(items, A.n_items, dev)
        i0, i1 = 0, int(cand.numel())
    n = u1 - u0
    vals = torch.full((n, k), float("-inf"), dtype=torch.float64, device=dev)
    idxs = torch.full((n, k), -1, dtype=torch.int64, device=dev)
    if n == 0 or i1 <= i0:
        return vals, idxs
    tile = _walk_tile(tile, i1 - i0, eu is not None)
    tw = TileWeights(A, lam, tile, cols=cand)
    if i0:
        tw.seek(i0)
    rows = src = None
    if ids is not None:
        # the user side from the taken rows; the item side (the tiles) from the full A
        if stats is not None and count_paths:
            raise ValueError("count_paths takes a user range, not user ids")
        rows, src, ex, eu_r = _user_side(A, ids, excl, eu, return_index=True)
    else:
        ex = excl.slice_rows(u0, u1) if excl is not None else None
        eu_r = None if eu is None else eu[u0:u1]
    if stats is not None and count_paths:
        _count_rows(tw, A, u0, u1)
    walk = TileWalk(A, u0, u1, i0, k, ex if drop else None, eu_r, ei, tile, col_bounds,
                    rows=rows, edge_src=src, cols=cand)
    evs = [] if stats is not None else None  # (per tile: build / bounds / walk, back to back)
    for j0 in range(i0, i1, tile):
        _mark(evs, "build")
        tw.build(j0, stop=i1)
        _mark(evs, "bounds")
        bnd = walk.bounds(j0, tw.width, tw.scale)
        _mark(evs, "walk")
        walk.step(tw.lines, tw.ovf, tw.inv_cls, tw.scale, j0, tile, tw.width, j0 == i0, bnd)
    _mark(evs, None)
    vals.copy_(walk.vals)
    idxs.copy_(walk.item_ids())
    if evs is not None:
        ms = _stage_ms(stats, evs, dev, "build", "bounds", "walk")["walk"]
        stats["walk_launches"] = stats.get("walk_launches", 0) + len(ms)
        stats["walk_ms_list"] = stats.get("walk_ms_list", []) + ms
        stats["user_items"] = stats.get("user_items", 0) + len(ms) * int(
            rows.col.numel() if rows is not None
            else A.by_user.rowptr[u1] - A.by_user.rowptr[u0])
        stats["users"] = n
        stats["qstride"] = 0 if walk.d == 0 or walk.qbuf is None else walk.qbuf.shape[1]
        stats["nch"] = -(-tile // 64) if walk.d else 0
    if stats is not None and count_paths:
        stats["w_paths"] = stats.get("w_paths", 0) + int(tw.paths_read)
        stats["w_paths_hub"] = stats.get("w_paths_hub", 0) + int(tw.paths_hub)
        stats["w_bytes"] = stats.get("w_bytes", 0) + int(tw.bytes_read)
    return vals, idxs


PEEL_K = 128   # entries of the walk's register-sorted lists (csrc/spread_tiled.hip)


def _spread_topk_tiled_peeled(A: Interactions, lam: float, k: int, excl: RowSets | None,
                              drop: bool, eu, ei, users: slice | None, tile: int,
                              items: slice | None, stats: dict | None, count_paths: bool,
                              col_bounds: bool):
    """spread_topk_tiled for PEEL_K < k <= 1024 (see there): passes of <= PEEL_K entries, each
    excluding what the earlier ones found. A candidate set peels in item-id space: every pass
    gets the same candidates, the ids found are item ids and join the exclusions as such, and
    each pass restricts them to the candidates' positions itself."""
    dev = A.k_item.device
    if items is not None and not isinstance(items, slice):
        items = item_candidates(items, A.n_items, dev)  # (once: a device tensor passes as is)
    ids = None if users is None or isinstance(users, slice) else _user_ids(users, A.n_users, dev)
    if ids is not None:
        users, u0, u1 = ids, 0, int(ids.numel())
    else:
        u0, u1 = (0, A.n_users) if users is None else (users.start, users.stop)
    n = u1 - u0
    vals = torch.full((n, k), float("-inf"), dtype=torch.float64, device=dev)
    idxs = torch.full((n, k), -1, dtype=torch.int64, device=dev)
    ex = excl if drop else None
    n_rows = excl.n_rows if excl is not None else A.n_users
    evs = [] if stats is not None else None
    for c0 in range(0, k, PEEL_K):
        kp = min(PEEL_K, k - c0)
        v, i = spread_topk_tiled(A, lam, kp, ex, True, eu, ei, users=users, tile=tile,
                                 items=items, stats=stats, count_paths=count_paths,
                                 col_bounds=col_bounds)
        vals[:, c0:c0 + kp], idxs[:, c0:c0 + kp] = v, i
        if c0 + kp >= k or not bool((i[:, kp - 1] >= 0).any()):
            break  # (a row whose last entry is empty has no survivors left)
        _mark(evs, "excl")
        hit = (i >= 0).nonzero(as_tuple=True)
        found = RowSets.from_pairs(hit[0] + u0 if ids is None else ids[hit[0]], i[hit], n_rows,
                                   A.n_items, dev)
        ex = found if ex is None else RowSets.union(ex, found)
        _mark(evs, None)
    if evs is not None:
        _stage_ms(stats, evs, dev, "excl")
        stats["peel_passes"] = stats.get("peel_passes", 0) + c0 // PEEL_K + 1
    return vals, idxs


def _count_rows(tw: "TileWeights", A: Interactions, u0: int, u1: int) -> None:
    """Make tw accumulate the walk's paths / row bytes for users [u0, u1) as tiles are
    selected (the times each item's row is gathered per tile = its users in the range)."""
    cols = A.by_user.col[int(A.by_user.rowptr[u0]):int(A.by_user.rowptr[u1])]
    tw.row_uses = torch.bincount(cols, minlength=A.n_items).to(torch.int64)
    tw.paths_read = torch.zeros((), dtype=torch.int64, device=A.k_item.device)
    tw.paths_hub = torch.zeros((), dtype=torch.int64, device=A.k_item.device)
    tw.bytes_read = torch.zeros((), dtype=torch.int64, device=A.k_item.device)


def tile_traffic(A: Interactions, tile: int = 2048, users: slice | None = None,
                 items: slice | None = None, hub: bool = False) -> tuple:
    """(paths, row bytes) the tile walk of users / items gathers (the stats of
    spread_topk_tiled(count_paths=True)), from the tiles alone: builds every tile, no walk;
    with ``hub`` also the paths that come from V (hub) rows: (paths, row bytes, V paths)."""
    u0, u1 = (0, A.n_users) if users is None else (users.start, users.stop)
    i0, i1 = (0, A.n_items) if items is None else (max(0, items.start),
                                                   min(A.n_items, items.stop))
    if i1 <= i0 or u1 <= u0:
        return (0, 0, 0) if hub else (0, 0)
    tw = TileWeights(A, 0.5, min(int(tile), i1 - i0))
    if i0:
        tw.seek(i0)
    _count_rows(tw, A, u0, u1)
    for j0 in range(i0, i1, tw.tile):
        tw.build(j0, stop=i1)
    if hub:
        return int(tw.paths_read), int(tw.bytes_read), int(tw.paths_hub)
    return int(tw.paths_read), int(tw.bytes_read)


def bound_operands(x: torch.Tensor, with_err: bool = False):
    """(bf16 copy as int16 storage, fp32 row norms rounded up) of an fp32 [n, d] matrix:
    the operands of lg_score_chunk_bound; with_err also the rounded-up norms of
    x - bf16(x) (screen_margins' operand)."""
    x = _f32(x, "x")
    xb = torch.empty(x.shape, dtype=torch.int16, device=x.device)
    nrm = torch.empty(x.shape[0], dtype=torch.float32, device=x.device)
    err = torch.empty(x.shape[0], dtype=torch.float32, device=x.device) if with_err else None
    N.check(N.lib().lg_bound_prep_f32(N.ptr(x), x.shape[0], x.shape[1], N.ptr(xb), N.ptr(nrm),
                                      N.ptr(err), N.stream_handle(x.device)),
            "lg_bound_prep_f32")
    return (xb, nrm, err) if with_err else (xb, nrm)


def chunk_bounds(ub, un, ib, inorm, dim: int, j0: int, width: int,
                 out: torch.Tensor | None = None, qout: torch.Tensor | None = None):
    """[users, ceil(width/64)] fp32 upper bounds of the fp32 score chain over each 64-column
    chunk of items [j0, j0 + width) (lg_score_chunk_bound); with qout ([users, qstride]
    uint8, qstride >= width rounded up to 256) also the per-column 8-bit bounds. Returns gb,
    or (gb, q) with qout. width <= 4096 (LG_BOUND_MAX_WIDTH; the library refuses wider
    tiles). ub / ib: bound_operands' int16 [rows, dim] bf16 copies, un / inorm their float32
    norms; items [j0, j0 + width) lie inside ib."""
    dim, j0, width = int(dim), int(j0), int(width)
    _typed(ub, "ub", torch.int16)
    _typed(ib, "ib", torch.int16)
    _typed(un, "un", torch.float32, 1)
    _typed(inorm, "inorm", torch.float32, 1)
    if ub.shape[1] != dim or ib.shape[1] != dim:
        raise ValueError(f"ub {tuple(ub.shape)} / ib {tuple(ib.shape)} are not [rows, {dim}]")
    if un.numel() != ub.shape[0] or inorm.numel() != ib.shape[0]:
        raise ValueError(f"{un.numel()} / {inorm.numel()} norms for {ub.shape[0]} / "
                         f"{ib.shape[0]} rows")
    if j0 < 0 or width < 1 or j0 + width > ib.shape[0]:
        raise ValueError(f"items [{j0}, {j0 + width}) outside ib's {ib.shape[0]} rows")
    n = ub.shape[0]
    nch = -(-width // 64)
    if out is not None:  # (a flat scratch buffer, reused across tiles; replaced when too small)
        _typed(out, "out", torch.float32, 1)
        if not out.is_contiguous():
            raise ValueError("out must be contiguous")
    if qout is not None:
        _typed(qout, "qout", torch.uint8)
        if qout.shape[0] != n or qout.shape[1] < -(-width // 256) * 256 \
                or not qout.is_contiguous():
            raise ValueError(f"qout must be contiguous [{n}, >= {-(-width // 256) * 256}], got "
                             f"shape {tuple(qout.shape)} strides {qout.stride()}")
    for t, name in ((un, "un"), (ib, "ib"), (inorm, "inorm"), (out, "out"), (qout, "qout")):
        if t is not None:
            _same_device(t, name, ub, "ub")
    N.require_gpu(ub, "ub")
    ub, ib, un, inorm = _aligned(ub), _aligned(ib), _aligned(un), _aligned(inorm)
    if out is None or out.numel() < n * nch:
        out = torch.empty(n * nch, dtype=torch.float32, device=ub.device)
    gb = out[:n * nch].view(n, nch)
    qs = 0 if qout is None else qout.shape[1]
    N.check(N.lib().lg_score_chunk_bound(N.ptr(ub), N.ptr(un), n, N.ptr(ib), N.ptr(inorm),
                                         int(dim), int(j0), int(width), N.ptr(gb),
                                         N.ptr(qout), int(qs),
                                         N.stream_handle(ub.device)),
            "lg_score_chunk_bound")
    return gb if qout is None else (gb, qout)


class TileWalk:
    """The fused top-K walk of users [u0, u1) over general_W tiles
    (lg_spread_tile_resource_topk_f64 per tile, with lg_score_chunk_bound screening when
    there is a G factor). Holds the running lists (vals fp64 / idxs int64 [n, k]), the
    per-user exclusion cursors and the bf16 score operands, so several walks (a lambda sweep)
    can share them.

    ``cols`` (the column view of TileWeights(cols=...)): the walk's columns are positions in
    cols. Everything the walk indexes by column -- the exclusions and their cursors, ei and
    its bf16 bound operands -- is taken for those items here (ex.restrict_cols(cols),
    ei[cols]); the user side (A.by_user or ``rows``, ra_edge, the row count A.n_items) stays
    the full graph's. ``idxs`` then holds positions; item_ids() maps them back."""

    def __init__(self, A: Interactions, u0: int, u1: int, i0: int, k: int,
                 ex: RowSets | None, eu=None, ei=None, tile: int = 2048,
                 col_bounds: bool = True, rows: RowSets | None = None, edge_src=None,
                 cols: torch.Tensor | None = None):
        self.cols = cols
        if cols is not None:
            ex = _nonempty(ex.restrict_cols(cols) if ex is not None else None)
            ei = ei[cols.to(torch.int64)] if ei is not None else None
        self.A, self.u0, self.u1, self.i0, self.k, self.ex = A, u0, u1, i0, int(k), ex
        # the walk keeps its stream positions in 32 bits
        if A.by_user.col.numel() >= 2**31 or (ex is not None and ex.col.numel() >= 2**31):
            raise ValueError("the tile walk needs fewer than 2^31 interactions / exclusions")
        self.n = u1 - u0
        # the user side of the walk: rows [u0, u1) of A, or ``rows`` -- any rows of A.by_user
        # (RowSets.take(ids, return_index=True): edge_src = their positions in A.by_user.col,
        # which the per-interaction factors of HybridScale are gathered by); ex, eu are then
        # the taken rows too and u0 = 0, u1 = the number of rows
        self.rows, self.edge_src = rows, edge_src
        self._ra = (None, None)
        if rows is not None:
            if edge_src is None or (u0, u1) != (0, rows.n_rows):
                raise ValueError("TileWalk(rows=): edge_src and u0, u1 = 0, rows.n_rows")
            self.n = rows.n_rows
        self.dev = A.k_item.device
        self.vals = torch.full((self.n, self.k), float("-inf"), dtype=torch.float64,
                               device=self.dev)
        self.idxs = torch.full((self.n, self.k), -1, dtype=torch.int64, device=self.dev)
        self.d = 0
        self.eu = self.ei = None
        if eu is not None:
            self.eu, self.ei = _f32_tables(eu, ei)
            self.d = self.eu.shape[1]
            self.ub, self.un = bound_operands(self.eu)
            self.ib, self.inorm = bound_operands(self.ei)
            self.gbuf = torch.empty(self.n * -(-int(tile) // 64), dtype=torch.float32,
                                    device=self.dev)
            # per-column 8-bit bounds (col_bounds=False: chunk bounds only)
            self.qbuf = None
            if col_bounds:
                self.qbuf = torch.empty((self.n, -(-int(tile) // 256) * 256),
                                        dtype=torch.uint8, device=self.dev)
        self.ex_cur = None
        if ex is not None:
            self.ex_cur = torch.empty(self.n, dtype=torch.int64, device=self.dev)
        self.reset()

    def reset(self) -> None:
        """Empty lists; exclusion cursors back at the walk's first item."""
        self.vals.fill_(float("-inf"))
        self.idxs.fill_(-1)
        if self.ex is not None:
            N.check(N.lib().lg_spread_tile_seek(N.ptr(self.ex.rowptr), N.ptr(self.ex.col),
                                                self.n, self.i0, N.ptr(self.ex_cur),
                                                N.stream_handle(self.dev)),
                    "lg_spread_tile_seek")

    def item_ids(self) -> torch.Tensor:
        """The lists' items as item ids: idxs itself, or mapped through the column view (-1
        stays -1)."""
        if self.cols is None:
            return self.idxs
        c64 = self.cols.to(torch.int64)
        return torch.where(self.idxs >= 0, c64[self.idxs.clamp(min=0)], self.idxs)

    def bounds(self, j0: int, width: int, scale: "HybridScale | None" = None):
        """(gb, q) score bounds of tile [j0, j0 + width) (q None: chunk bounds only)."""
        if not self.d:
            return None
        if self.qbuf is None:
            return chunk_bounds(self.ub, self.un, self.ib, self.inorm, self.d, j0, width,
                                self.gbuf), None
        return chunk_bounds(self.ub, self.un, self.ib, self.inorm, self.d, j0, width,
                            self.gbuf, self.qbuf)

    def _user_side(self, scale: HybridScale):
        """(rowptr, items, ra per interaction) of the walk's rows: A's own, or the taken rows."""
        if self.rows is None:
            return self.A.by_user.rowptr[self.u0:], self.A.by_user.col, scale.ra_edge
        if self._ra[0] is not scale:  # (one gather per lambda, not per tile)
            self._ra = (scale, torch.cat([scale.ra_edge[self.edge_src],
                                          scale.ra_edge.new_zeros(1)]))
        return self.rows.rowptr, self.rows.col, self._ra[1]

    def count_step(self, lines, ovf, inv_cls, scale: HybridScale, j0: int, tile: int,
                   width: int, targets: RowSets, val: torch.Tensor, cnt: torch.Tensor,
                   bnd=None) -> None:
        """The count phase of lg_spread_tile_resource_rank_f64 for tile [j0, j0 + width): adds
        to cnt, for every target of the walk's rows, the tile's columns before it (val: the
        targets' values, from the value phase). Tiles in ascending order, as step()."""
        ex = self.ex
        if self.d and bnd is None:
            bnd = self.bounds(j0, width, scale)
        gb, q = bnd if bnd is not None else (None, None)
        u_rowptr, u_col, ra_edge = self._user_side(scale)
        N.check(N.lib().lg_spread_tile_resource_rank_f64(
            N.ptr(u_rowptr), N.ptr(u_col), N.ptr(ra_edge), self.n, N.ptr(lines), N.ptr(ovf),
            self.A.n_items, N.ptr(scale.rb), N.ptr(inv_cls), int(j0), int(tile), int(width),
            N.ptr(self.eu), N.ptr(self.ei), self.d, N.ptr(gb),
            gb.shape[1] if gb is not None else 0, N.ptr(q), 0 if q is None else q.shape[1],
            N.ptr(ex.rowptr if ex is not None else None),
            N.ptr(ex.col if ex is not None else None), N.ptr(self.ex_cur),
            N.ptr(targets.rowptr), N.ptr(targets.col), N.LG_SPREAD_RANK_COUNTS, N.ptr(val),
            N.ptr(cnt), u_col.numel(), ex.col.numel() if ex is not None else 0,
            N.stream_handle(self.dev)), "lg_spread_tile_resource_rank_f64")

    def step(self, lines, ovf, inv_cls, scale: HybridScale, j0: int, tile: int, width: int,
             first: bool, bnd=None) -> None:
        """Merge tile [j0, j0 + width) (its rows: lines / ovf) into the lists; bnd = the
        tile's bounds() (computed here when None)."""
        A, ex = self.A, self.ex
        if self.d and bnd is None:
            bnd = self.bounds(j0, width, scale)
        gb, q = bnd if bnd is not None else (None, None)
        nch = gb.shape[1] if gb is not None else 0
        u_rowptr, u_col, ra_edge = self._user_side(scale)
        N.check(N.lib().lg_spread_tile_resource_topk_f64(
            N.ptr(u_rowptr), N.ptr(u_col), N.ptr(ra_edge),
            self.n, N.ptr(lines), N.ptr(ovf), A.n_items, N.ptr(scale.rb), N.ptr(inv_cls), int(j0),
            int(tile), int(width), N.ptr(self.eu), N.ptr(self.ei), self.d, N.ptr(gb), nch,
            N.ptr(q), 0 if q is None else q.shape[1],
            N.ptr(ex.rowptr if ex is not None else None),
            N.ptr(ex.col if ex is not None else None), N.ptr(self.ex_cur), self.k,
            int(bool(first)), N.ptr(self.vals), N.ptr(self.idxs), u_col.numel(),
            ex.col.numel() if ex is not None else 0, N.stream_handle(self.dev)),
            "lg_spread_tile_resource_topk_f64")


def spread_lambda_sweep(A: Interactions, lams, k: int, excl: RowSets | None,
                        drop: bool = True, eu: torch.Tensor | None = None,
                        ei: torch.Tensor | None = None, tiled: bool | None = None,
                        tile: int = 2048, cache_bytes: int | None = None):
    """Yield (lam, values [U, k] fp64, items [U, k] int64) of spread_recommend for every
    lam of ``lams`` (the loop of findLambda.py:93-114: HybridS -> A @ W -> G * F -> top-k per
    lambda), reusing what does not depend on lambda:
      dense  general_W (lg_spread_general_f64) once; per lambda W (lg_hybrid_weight_f64) and
             the fused F / top-k.
      tiled  the general_W tiles (lambda-independent: ra / rb are applied by the walk) are
             built once and cached on the device while they fit ``cache_bytes`` (default:
             half the free memory); per lambda only the HybridScale (ra per interaction, rb
             per item) changes and the score bounds are recomputed (cheap; the per-column
             bounds of every tile would not fit). If the cache does not fit, each lambda
             rebuilds the tiles. At k > 128 the tiled route calls spread_topk_tiled per
             lambda (its peeled passes; no shared TileWalk, no tile cache).
    Every result is bitwise the one spread_recommend(A, lam, ...) returns. The sweep ranks the
    whole catalog: it takes no items= (spread_recommend's candidate set) yet."""
    lams = [float(x) for x in lams]
    k = int(k)
    dev = A.k_item.device
    if tiled is None:
        tiled = not dense_spread_fits(A.n_items, dev)
    if not tiled:
        gW = spread_general(A)
        for lam in lams:
            W = hybrid_weight(gW, A.k_item, lam)
            v, i = spread_topk(A, W, k, excl, drop, eu, ei)
            del W
            yield lam, v, i
        return
    if k > PEEL_K:
        for lam in lams:
            v, i = spread_topk_tiled(A, lam, k, excl, drop, eu, ei, tile=tile)
            yield lam, v, i
        return
    if cache_bytes is None:
        cache_bytes = torch.cuda.mem_get_info(dev)[0] // 2
    U, I = A.n_users, A.n_items
    tile = _walk_tile(tile, I, eu is not None) if I else 1
    ex = excl if drop else None
    walk = TileWalk(A, 0, U, 0, k, ex, eu, ei, tile)
    cache, used, cached = [], 0, True
    inv_cls = None
    for n, lam in enumerate(lams):
        scale = HybridScale(A, lam)
        walk.reset()
        if n > 0 and cached:
            for (j0, width, lines, ovf) in cache:
                walk.step(lines, ovf, inv_cls, scale, j0, tile, width, j0 == 0)
        else:
            tw = TileWeights(A, lam, tile)
            inv_cls = tw.inv_cls
            for j0 in range(0, I, tile):
                tw.build(j0)
                walk.step(tw.lines, tw.ovf, inv_cls, scale, j0, tile, tw.width, j0 == 0)
                if n == 0 and cached and len(lams) > 1:
                    nov = (tw.n_units + 64) * 4
                    need = tw.lines.numel() * 4 + nov * 4
                    if used + need <= cache_bytes:
                        cache.append((j0, tw.width, tw.lines.clone(), tw.ovf[:nov].clone()))
                        used += need
                    else:
                        cached = False
                        cache.clear()
            del tw
        yield lam, walk.vals.clone(), walk.idxs.clone()


def merge_topk_lists(vals: torch.Tensor, idxs: torch.Tensor):
    """[L, n, k] sorted lists (index -1 = empty) -> the [n, k] top-k of their union, same
    order (value desc, index asc). k <= 128: lg_topk_lists_merge_f64; 128 < k <= 1024:
    lg_topk_lists_merge_wide_f64 (the list in LDS)."""
    N.require_gpu(vals, "vals")
    if vals.dtype != torch.float64 or idxs.dtype != torch.int64 or vals.shape != idxs.shape \
            or vals.dim() != 3:
        raise ValueError("merge_topk_lists: vals fp64 / idxs int64 of one [L, n, k] shape")
    L, n, k = vals.shape
    if k < 1 or k > 1024:
        raise ValueError(f"merge_topk_lists: k={k} not in [1, 1024]")
    vals, idxs = vals.contiguous(), idxs.contiguous()
    ov = torch.empty((n, k), dtype=torch.float64, device=vals.device)
    oi = torch.empty((n, k), dtype=torch.int64, device=vals.device)
    name = "lg_topk_lists_merge_f64" if k <= 128 else "lg_topk_lists_merge_wide_f64"
    N.check(getattr(N.lib(), name)(N.ptr(vals), N.ptr(idxs), L, n, k, N.ptr(ov), N.ptr(oi),
                                   N.stream_handle(vals.device)), name)
    return ov, oi


def dense_spread_fits(n_items: int, device, fraction: float = 0.25) -> bool:
    """True when general_W and W (two fp64 I x I matrices) fit in ``fraction`` of the free
    device memory: the dense path; otherwise the factored tile path."""
    free, _ = torch.cuda.mem_get_info(device)
    return 2 * 8 * n_items * n_items <= fraction * free


def spread_recommend(A: Interactions, lam: float, k: int, excl: RowSets | None,
                     drop: bool = True, eu: torch.Tensor | None = None,
                     ei: torch.Tensor | None = None, transpose: bool = False,
                     tiled: bool | None = None, users=None, tile: int | None = None,
                     items=None, W: torch.Tensor | None = None):
    """Per-user top-k of (G *) A @ HybridS(A, general_W(^T), lam), dense (I x I matrices on
    the device) or factored over item tiles (tiled=None: dense when it fits). The two
    paths give the same values within a few ulp (the factored walk sums each column's paths
    in its own order) and the same lists except near-ties. general_W is exactly symmetric (entry (i, j) and (j, i) are
    the same sum, over the common users ascending, of the same fl(1/k_v)), so the
    reference's general_W.T overrides (model/SpreadMethod/recommend.py:89-91, :99-101)
    are served by either path unchanged.

    ``users`` (a tensor or list of user ids, any order, duplicates allowed) restricts the
    result to those users: row j is bitwise row users[j] of the all-users call on the same
    path. The user side (interaction rows, exclusion rows, eu rows) is taken for those ids;
    the item side (W, or the general_W tiles) comes from the full A. ``tile`` is the tiled
    path's tile width (default: spread_topk_tiled's).

    ``items`` (item_candidates' forms: ids, a bool mask, or a strictly ascending device
    tensor) restricts the ranking to a candidate item set C -- the in-stock items, one
    category, a retrieval stage's output. Only the ranked columns are restricted: the paths
    u -> i -> v -> j run over every item i and user v of the full graph with the full
    degrees, F_C[u, p] = sum_{i in items(u)} W[i, C[p]] with W built from the whole A. Row u
    is the first k of {(v(u, j), j) : j in C, j not dropped by u's exclusions} under (value
    desc, item id asc), real item ids, NaN and -inf never rank, short rows padded {-inf, -1};
    drop=False keeps excluded candidates. Dense: lg_spread_rows_topk_items_f64 (csrc/
    rows_topk_items.hip, any k <= 1024, all users or ``users``), or, where
    _spread_items_route measured it slower, the existing kernels and an F[:, C] gather --
    the same bits, and bit for bit rows_topk(spread_resource(A, W)[:, C], k,
    excl.restrict_cols(C), drop, eu, ei[C]) mapped back through C. Tiled: the column view of
    spread_topk_tiled (values within 1e-12 relative of the dense path).

    ``W``: a prebuilt spread_hybrid(A, lam) for the dense path (a per-request caller must not
    rebuild an I x I matrix per call; ``lam`` is then not read). With tiled=True it raises."""
    if tiled is None:
        tiled = W is None and not dense_spread_fits(A.n_items, A.k_item.device)
    if tiled:
        if W is not None:
            raise ValueError("spread_recommend: W= is the dense path's matrix; the tiled path "
                             "never holds one (tiled=True with W)")
        kw = {} if tile is None else {"tile": int(tile)}
        if items is not None:
            if isinstance(items, slice):
                raise ValueError("spread_recommend: items= is a candidate set (ids or a mask); "
                                 "item ranges are spread_topk_tiled's shards")
            kw["items"] = items
        return spread_topk_tiled(A, lam, k, excl, drop, eu, ei, users=users, **kw)
    ids = None if users is None else _user_ids(users, A.n_users, A.k_item.device)
    if W is None:
        W = spread_hybrid(A, lam)  # (= hybrid_weight(spread_general(A), ..., transpose))
    elif W.shape != (A.n_items, A.n_items) or W.dtype != torch.float64:
        raise ValueError(f"W of shape {tuple(W.shape)} / {W.dtype}, expected the fp64 "
                         f"({A.n_items}, {A.n_items}) matrix of spread_hybrid")
    if items is not None:
        if isinstance(items, slice):
            raise ValueError("spread_recommend: items= is a candidate set (ids or a mask)")
        cand = item_candidates(items, A.n_items, A.k_item.device)
        return _spread_topk_items(A, W, ids, cand, k, excl, drop, eu, ei)
    if ids is not None:
        return _spread_topk_users(A, W, ids, k, excl, drop, eu, ei)
    return spread_topk(A, W, k, excl, drop, eu, ei)


def _spread_topk_users(A: Interactions, W: torch.Tensor, ids: torch.Tensor, k: int,
                       excl: RowSets | None, drop: bool, eu, ei):
    """spread_topk for the users ``ids`` only: the F rows of the taken interaction rows, block
    by block, then rows_topk with the taken exclusion and eu rows."""
    rows, _, ex, eu_r = _user_side(A, ids, excl, eu)
    return _blocks_topk(rows, W, k, ex, drop, eu_r, ei)


def spread_rank(A: Interactions, lam: float, targets, excl: RowSets | None, drop: bool = True,
                eu: torch.Tensor | None = None, ei: torch.Tensor | None = None,
                transpose: bool = False, users=None, W: torch.Tensor | None = None,
                tiled: bool | None = None, block_users: int | None = None):
    """Where every user's held-out items stand among ALL items under the scores of
    spread_recommend's dense path, (G *) A @ HybridS(A, lam): (rank int64 [nnz], value fp64
    [nnz]) aligned with the target CSR's col, rows_rank's definitions -- for any k <= 1024,
    rank < k iff spread_recommend(A, lam, k, excl, drop, eu, ei, ...) holds the item at
    [row, rank], with a bit-equal value. F is computed block by block (lg_spread_resource_f64,
    about 1 GiB of F per block, or block_users rows; the result does not depend on it) and
    ranked by lg_rows_rank_f64; all of F is never held.

    targets: anything candidate_rows takes, one row per user -- or per entry of ``users`` (ids
    in any order, duplicates allowed), for which the interaction, exclusion and eu rows are
    taken as spread_recommend does. ``transpose`` and ``W`` have spread_recommend's meaning.
    tiled=True raises ValueError, as does tiled=None when dense_spread_fits says no: the
    factored walk prunes by bounds and keeps only bounded lists, so it has no rank -- its ranks
    come from a walk with a counting finish instead, spread_rank_tiled."""
    dev = A.k_item.device
    if tiled is None:
        tiled = W is None and not dense_spread_fits(A.n_items, dev)
    if tiled:
        raise ValueError("spread_rank: the factored (tiled) walk keeps only bounded lists of "
                         "every row, never a full row, and so has no rank; ranks need the "
                         "dense path (the I x I matrices on the device, tiled=False or W=)")
    I = A.n_items
    if W is not None:
        _check_W(W, I, f"the fp64 ({I}, {I}) matrix of spread_hybrid")
    if eu is not None or ei is not None:
        _g_guard(eu, ei, A.n_users, I)
    _excl_guard(excl, A.n_users, "users")
    ids = None if users is None else _user_ids(users, A.n_users, dev)
    n = A.n_users if ids is None else int(ids.numel())
    if isinstance(targets, RowSets) and targets.n_rows != n:
        raise ValueError(f"target rows {targets.n_rows} != {n} users")
    targets = candidate_rows(targets, n, I, dev)
    nnz = int(targets.col.numel())
    rank = torch.full((nnz,), -1, dtype=torch.int64, device=dev)
    val = torch.full((nnz,), float("-inf"), dtype=torch.float64, device=dev)
    if n == 0 or nnz == 0:
        return rank, val
    if W is None:
        W = spread_hybrid(A, lam)
    rows, _, ex, eu_r = _user_side(A, ids, excl, eu)
    for b0, b1, Fb in _f_blocks(rows, W, block_users):
        # the block's targets keep their absolute offsets into col: every block writes its own
        # entries of the [nnz] outputs
        rows_rank(Fb, targets.slice_rows(b0, b1),
                  ex.slice_rows(b0, b1) if ex is not None else None, drop,
                  None if eu_r is None else eu_r[b0:b1], ei, out=(rank, val))
    return rank, val


# targets per counting pass of the walk's rank finish (kRankPass, csrc/spread_tiled.hip); rows
# of any length work, longer ones take ceil(n / SPREAD_RANK_ROW_MAX) passes over the tile in LDS
SPREAD_RANK_ROW_MAX = N.LG_SPREAD_RANK_ROW_MAX


def _entry_rows(rowptr: torch.Tensor, nnz: int):
    """(row int64 [nnz], inside bool [nnz]) of the entries of a CSR's col: the row that holds
    position p, and whether any does (a sliced CSR's col has entries outside every row)."""
    pos = torch.arange(nnz, dtype=torch.int64, device=rowptr.device)
    row = torch.searchsorted(rowptr, pos, right=True) - 1
    inside = (pos >= rowptr[0]) & (pos < rowptr[-1])
    return row.clamp(0, max(rowptr.numel() - 2, 0)), inside


def _goto_tile(tw: "TileWeights", j0: int) -> None:
    """Make [j0, j0 + tile) tw's current tile, from any tile before it: selected when the
    group built last holds it, built as the next group when it follows the current tile, else
    built after a seek."""
    g = tw._grp
    if g is not None and tw._seek_at is None and g[0] <= j0 < g[0] + sum(g[1]):
        tw._select((j0 - g[0]) // tw.tile)
        return
    if j0 != 0 and (tw.j0 is None or j0 != tw.j0 + tw.width):
        tw.seek(j0)
    tw.build(j0)


def spread_rank_tiled(A: Interactions, lam: float, targets, excl: RowSets | None,
                      drop: bool = True, eu: torch.Tensor | None = None,
                      ei: torch.Tensor | None = None, users=None, tile: int = 2048,
                      stats: dict | None = None):
    """spread_rank on the factored tile walk: where every user's held-out items stand among
    ALL items under spread_topk_tiled's scores, (G *) A @ HybridS(A, lam), without general_W,
    W or a row of F ever in memory. (rank int64 [nnz], value fp64 [nnz]) aligned with the
    target CSR's col, rows_rank's definitions: rank = the ranking columns before the target
    under (value desc, item asc), 0 = first; -1 for a target that does not rank (its value is
    NaN or -inf, or drop=True and the user's exclusions name it; its value is still reported);
    a column named twice gets the same rank twice; an entry of col outside every row and an
    item id outside the catalog get {-1, -inf}. For every k <= 1024: rank < k iff
    spread_topk_tiled(A, lam, k, excl, drop, eu, ei, users=..., tile=...) holds the item at
    [row, rank] with a bit-equal value; the rank itself has no depth limit. Against the dense
    spread_rank the values agree within 1e-12 relative (the walk's summation order) and the
    ranks wherever no other value of the row is that close to the target's.

    Two sweeps of lg_spread_tile_resource_rank_f64 over the tiles of TileWeights. Values: the
    targets are grouped by tile; every tile that holds one is walked by the taken rows of the
    users with a target there only (bitwise the all-users rows), the kernel writing each
    target's value -- with one target per user about 1 / ceil(I / tile) of a sweep. Counts:
    one ascending walk of all rows over all tiles, each adding, per target, the tile's columns
    before it; with a G factor only columns whose score bound (TileWalk.bounds) reaches the
    user's worst ranking target value get the exact score. -1 / -inf are filled in on the
    device. One host read in all (the tiles' group sizes, before the sweeps) besides the tile
    build's own.

    targets / users as spread_rank: one target row per user, or per entry of ``users`` (ids,
    any order, duplicates allowed: the user side is taken, the tiles come from the full A).
    tile: the tile width (<= 4096 with a G factor, 8192 without). No target or no user: no
    launch. ``stats`` receives the HIP-event times t_build_ms / t_bounds_ms / t_value_ms /
    t_count_ms and the launches of the two sweeps (value_launches, count_launches)."""
    dev = A.k_item.device
    I = A.n_items
    if eu is not None or ei is not None:
        _g_guard(eu, ei, A.n_users, I)
        if eu.shape[1] not in (32, 64, 128):
            raise ValueError(f"embedding width {eu.shape[1]} not in (32, 64, 128)")
    _excl_guard(excl, A.n_users, "users", eu is not None and not drop)
    if int(tile) < 1:
        raise ValueError(f"tile {tile} < 1")
    ids = None if users is None else _user_ids(users, A.n_users, dev)
    n = A.n_users if ids is None else int(ids.numel())
    if isinstance(targets, RowSets) and targets.n_rows != n:
        raise ValueError(f"target rows {targets.n_rows} != {n} users")
    targets = candidate_rows(targets, n, I, dev)
    for t, name in ((targets.col, "targets"), (excl.col if excl is not None else None, "excl"),
                    (eu, "eu"), (ei, "ei")):
        if t is not None and t.device != dev:
            raise ValueError(f"{name} is on {t.device}, A on {dev}")
    nnz = int(targets.col.numel())
    rank = torch.full((nnz,), -1, dtype=torch.int64, device=dev)
    val = torch.full((nnz,), float("-inf"), dtype=torch.float64, device=dev)
    if n == 0 or nnz == 0 or I == 0:
        return rank, val
    N.require_gpu(A.k_item, "A")
    L = N.lib()
    strm = N.stream_handle(dev)
    tile = _walk_tile(tile, I, eu is not None)
    ntiles = -(-I // tile)
    tw = TileWeights(A, lam, tile)
    by = A.by_user
    rows, src, ex, eu_r = None, None, excl if drop else None, eu
    if ids is not None:
        rows, src, ex, eu_r = _user_side(A, ids, ex, eu, return_index=True)
    ex = _nonempty(ex)
    walk = TileWalk(A, 0, n, 0, 1, ex, eu_r, ei, tile, rows=rows, edge_src=src)
    scale = tw.scale
    d = walk.d

    # ---- the targets by (tile, row): sorted entries, one group per (tile, row) that has any
    col = targets.col.to(torch.int64)
    trow, inside = _entry_rows(targets.rowptr, nnz)
    valid = inside & (col >= 0) & (col < I)
    key = torch.where(valid, col // tile, torch.full_like(col, ntiles)) * n + trow
    skey, perm = torch.sort(key, stable=True)
    scol = targets.col[perm].contiguous()
    ukey, gcount = torch.unique_consecutive(skey, return_counts=True)
    gstart = torch.zeros(ukey.numel() + 1, dtype=torch.int64, device=dev)
    torch.cumsum(gcount, 0, out=gstart[1:])
    gtile, grow = ukey // n, ukey % n
    guser = grow if ids is None else ids[grow]
    gdeg = by.rowptr[guser + 1] - by.rowptr[guser]
    per_tile = torch.stack([
        torch.bincount(gtile, minlength=ntiles + 1),
        torch.bincount(gtile, weights=gdeg.to(torch.float64), minlength=ntiles + 1).to(torch.int64),
    ]).tolist()  # (the one host read: groups and walked interactions per tile)
    sval = torch.full((nnz,), float("-inf"), dtype=torch.float64, device=dev)
    evs = [] if stats is not None else None

    # ---- values: the tiles that hold a target, walked by the rows with a target there
    g0 = 0
    n_value = 0
    for t in range(ntiles):
        ng, total = per_tile[0][t], per_tile[1][t]
        if ng == 0:
            continue
        _mark(evs, "build")
        _goto_tile(tw, t * tile)
        _mark(evs, None)
        r = guser[g0:g0 + ng]
        deg = gdeg[g0:g0 + ng]
        rp_g = torch.zeros(ng + 1, dtype=torch.int64, device=dev)
        torch.cumsum(deg, 0, out=rp_g[1:])
        e_src = torch.repeat_interleave(by.rowptr[r] - rp_g[:-1], deg, output_size=total) \
            + torch.arange(total, dtype=torch.int64, device=dev)
        # (one spare entry each: rows without interactions still pass valid pointers)
        items_g = torch.cat([by.col[e_src], by.col.new_zeros(1)])
        ra_g = torch.cat([scale.ra_edge[e_src], scale.ra_edge.new_zeros(1)])
        eu_g = None if eu is None else walk.eu[grow[g0:g0 + ng]].contiguous()
        tp = gstart[g0:g0 + ng + 1]  # (absolute positions in scol / sval)
        _mark(evs, "value")
        N.check(L.lg_spread_tile_resource_rank_f64(
            N.ptr(rp_g), N.ptr(items_g), N.ptr(ra_g), ng, N.ptr(tw.lines), N.ptr(tw.ovf), I,
            N.ptr(scale.rb), N.ptr(tw.inv_cls), tw.j0, tile, tw.width, N.ptr(eu_g),
            N.ptr(walk.ei), d, None, 0, None, 0, None, None, None, N.ptr(tp), N.ptr(scol),
            N.LG_SPREAD_RANK_VALUES, N.ptr(sval), None, total, 0, strm),
            "lg_spread_tile_resource_rank_f64")
        _mark(evs, None)
        n_value += 1
        g0 += ng
    val[perm] = sval

    # ---- counts: every row over every tile, ascending
    cnt = torch.zeros(nnz, dtype=torch.int64, device=dev)
    for t in range(ntiles):
        _mark(evs, "build")
        _goto_tile(tw, t * tile)
        _mark(evs, "bounds")
        bnd = walk.bounds(tw.j0, tw.width, scale)
        _mark(evs, "count")
        walk.count_step(tw.lines, tw.ovf, tw.inv_cls, scale, tw.j0, tile, tw.width, targets, val,
                        cnt, bnd)
    _mark(evs, None)

    # ---- a target ranks iff its value is > -inf (not NaN) and no dropped exclusion names it
    ranks = val > float("-inf")
    if ex is not None:
        xrow, xin = _entry_rows(ex.rowptr, int(ex.col.numel()))
        xkey = torch.where(xin, xrow * I + ex.col.to(torch.int64), torch.full_like(xrow, -1))
        ranks &= ~torch.isin(trow * I + col, xkey)
    rank = torch.where(ranks, cnt, rank)
    if evs is not None:
        _stage_ms(stats, evs, dev, "build", "bounds", "value", "count")
        stats["value_launches"] = stats.get("value_launches", 0) + n_value
        stats["count_launches"] = stats.get("count_launches", 0) + ntiles
        stats["tiles"] = ntiles
    return rank, val


# ------------------------------------------------ dense spreading over a candidate item set
# rows of at least this many candidates get several waves each in lg_spread_rows_topk_items_f64
# (kSplitCand, csrc/rows_topk_items.hip), shorter ones one
ROWS_ITEMS_SPLIT = 512


def spread_rows_topk_items(rows: RowSets, W: torch.Tensor, cand: torch.Tensor, k: int,
                           excl: RowSets | None = None, drop: bool = True,
                           eu: torch.Tensor | None = None, ei: torch.Tensor | None = None):
    """lg_spread_rows_topk_items_f64: per row r of ``rows`` (interaction rows: A.by_user, or
    taken rows of it) the top-k of (G *) sum_{i in rows[r]} W[i, j] over the candidates j in
    ``cand`` (item_candidates' int32 tensor: strictly ascending ids), excluded items (``excl``:
    item-id columns, rows aligned with ``rows``) dropped or kept. W: the full fp64 [I, I]
    matrix; eu: the rows' embeddings, ei: the full item table. Returns (values fp64 [n, k],
    item ids int64 [n, k], {-inf, -1} padding). k in [1, 1024]; nothing is gathered."""
    k = int(k)
    if k < 1 or k > 1024:
        raise ValueError(f"k={k} not in [1, 1024]")
    N.require_gpu(W, "W")
    I = rows.n_cols
    if W.dtype != torch.float64 or W.dim() != 2 or W.shape != (I, I):
        raise ValueError(f"W must be the float64 ({I}, {I}) matrix, got {tuple(W.shape)} "
                         f"{W.dtype}")
    W = W.contiguous()
    dev = W.device
    if cand.dtype != torch.int32 or cand.device != dev:
        raise ValueError("cand must be item_candidates' int32 tensor on W's device")
    cand = cand.contiguous()
    n, nc = rows.n_rows, int(cand.numel())
    # (an empty tensor has no pointer to pass and the entry refuses NULL: a one-element stand-in
    # that is never read -- the entry pads every row on n_cand = 0, rows without items sum to 0)
    cand_p = cand if nc else torch.zeros(1, dtype=torch.int32, device=dev)
    col_p = rows.col if rows.col.numel() else torch.zeros(1, dtype=torch.int32, device=dev)
    _excl_guard(excl, n, "rows")
    excl = _nonempty(excl)
    d = 0
    if eu is not None:
        eu, ei = _f32_tables(eu, ei)
        d = eu.shape[1]
        if eu.shape[0] != n or ei.shape != (I, d):
            raise ValueError("eu: one row per row of `rows`; ei: the full item table")
    val = torch.empty((n, k), dtype=torch.float64, device=dev)
    idx = torch.empty((n, k), dtype=torch.int64, device=dev)
    N.check(N.lib().lg_spread_rows_topk_items_f64(
        N.ptr(rows.rowptr), N.ptr(col_p), N.ptr(W), n, I, N.ptr(cand_p), nc, N.ptr(eu),
        N.ptr(ei), d, N.ptr(excl.rowptr if excl else None), N.ptr(excl.col if excl else None),
        N.LG_EXCL_DROP if drop else N.LG_EXCL_NONE, k, N.ptr(val), N.ptr(idx),
        N.stream_handle(dev)), "lg_spread_rows_topk_items_f64")
    return val, idx


# spread_recommend(items=...) on the dense path sends a request to the fused kernel
# (lg_spread_rows_topk_items_f64) or to the existing pair -- the F blocks, an F[:, C]
# gather, rows_topk, the id map -- whichever profiles/spread_items.json
# (scripts/spread_items_time.py: 600 x 20,000, d = 64, with and without G, users 1 / 8 / 16 /
# 600, share 1.0 / 0.5 / 0.1 / 0.01, k 20 / 100 / 256) measured faster by more than the larger
# of the two spreads. There the fused kernel wins every k, with and without G, for all 600 users
# at a candidate share <= 0.1 (0.61-0.72 of gather's time at 0.1, 0.12-0.14 at 0.01); at share
# 0.5 it wins without G only (0.82-0.91; with G 0.91-0.94, inside the spread at k <= 100) and
# at 1.0 it loses with G (1.07-1.34). For 1 / 8 / 16 users both routes are 0.35-1.1 ms of
# mostly host work (the row takes, the launches): the fused median is 0.72-0.98 of gather's at
# share <= 0.1 and 1.02-1.47 above, never beyond the 0.2-0.7 spreads of such calls -- no win
# is established, so they stay on the existing kernels. Between 16 and 600 users nothing was
# timed: the bound is the smallest user count at which the win was measured.
SPREAD_ITEMS_FUSED_MIN_USERS = 600
SPREAD_ITEMS_FUSED_MAX_SHARE = 0.1


def _spread_items_route(n_rows: int, n_cand: int, n_items: int) -> str:
    """"fused" or "gather" (see SPREAD_ITEMS_FUSED_*); both give the same bits."""
    if n_rows >= SPREAD_ITEMS_FUSED_MIN_USERS and \
            n_cand <= SPREAD_ITEMS_FUSED_MAX_SHARE * n_items:
        return "fused"
    return "gather"


def _spread_topk_items(A: Interactions, W: torch.Tensor, ids, cand: torch.Tensor, k: int,
                       excl: RowSets | None, drop: bool, eu, ei, route: str | None = None):
    """spread_recommend's dense path over the candidates ``cand`` for all users (ids None)
    or the users ``ids`` (interaction, exclusion and eu rows taken as _spread_topk_users
    does). route: "fused" (lg_spread_rows_topk_items_f64), "gather" (F block by block,
    F[:, cand], rows_topk on the renumbered exclusions and ei[cand], ids mapped back) or
    None: _spread_items_route. Bitwise the same lists either way."""
    rows, _, ex, eu_r = _user_side(A, ids, excl, eu)
    n, nc = rows.n_rows, int(cand.numel())
    if route is None:
        route = _spread_items_route(n, nc, A.n_items)
    if route == "fused":
        return spread_rows_topk_items(rows, W, cand, k, ex, drop, eu_r, ei)
    if route != "gather":
        raise ValueError(f"route {route!r} not in ('fused', 'gather')")
    k = int(k)
    _check_W(W, A.n_items)
    dev = W.device
    vals = torch.full((n, k), float("-inf"), dtype=torch.float64, device=dev)
    idxs = torch.full((n, k), -1, dtype=torch.int64, device=dev)
    if n == 0 or nc == 0:
        if k < 1 or k > 1024:
            raise ValueError(f"k={k} not in [1, 1024]")
        return vals, idxs
    c64 = cand.to(torch.int64)
    exc = _nonempty(ex.restrict_cols(cand) if ex is not None else None)
    eic = None if ei is None else ei[c64]
    for b0, b1, Fb in _f_blocks(rows, W):
        v, i = rows_topk(Fb[:, c64], k, exc.slice_rows(b0, b1) if exc is not None else None,
                         drop, None if eu_r is None else eu_r[b0:b1], eic)
        vals[b0:b1], idxs[b0:b1] = v, torch.where(i >= 0, c64[i.clamp(min=0)], i)
    return vals, idxs


# ------------------------------------------- spreading for item baskets outside the graph
# baskets per call of lg_spread_rows_weight_f64 / lg_spread_rows_resource_f64 (lane b of a wave
# owns basket b) and the positions per segment of a long list (csrc/spread_rows.hip)
SPREAD_ROWS_BLOCK = N.LG_SPREAD_ROWS_BLOCK
SPREAD_ROWS_SEG = N.LG_SPREAD_ROWS_SEG


def _basket_rows(rows, n_items: int, device) -> RowSets:
    """The baskets of a spread_rows_* call as a RowSets over the items, one row per basket:
    a RowSets (taken as it is), a list of id lists, a dict {row: ids} (rows 0 .. max key) or a
    (rows, items) pair -- candidate_rows' forms and checks (host ids sorted and de-duplicated:
    an item named twice counts once, A is 0/1)."""
    if isinstance(rows, RowSets):
        if rows.n_cols != n_items:
            raise ValueError(f"baskets over {rows.n_cols} items, A has {n_items}")
        if rows.col.device != torch.device(device):
            raise ValueError(f"rows are on {rows.col.device}, A on {device}")
        return rows
    if isinstance(rows, dict):
        n = max((int(r) for r in rows), default=-1) + 1
    elif isinstance(rows, tuple) and len(rows) == 2:
        r = torch.as_tensor(rows[0])
        n = int(r.max()) + 1 if r.numel() else 0
    else:
        rows = list(rows)
        n = len(rows)
    return candidate_rows(rows, n, n_items, device)


def _long_lists(rs: RowSets):
    """(long_ids int32, long_ptr int64, n_long, n_units): the lists of ``rs`` longer than
    SPREAD_ROWS_SEG and the exclusive prefix sum of their segment counts, as the
    lg_spread_rows_* entries take them (both None when no list is long). One host read."""
    deg = rs.degrees()
    ids = torch.nonzero(deg > SPREAD_ROWS_SEG).reshape(-1)
    n_long = int(ids.numel())
    if n_long == 0:
        return None, None, 0, 0
    ptr = torch.zeros(n_long + 1, dtype=torch.int64, device=deg.device)
    torch.cumsum((deg[ids] + SPREAD_ROWS_SEG - 1) // SPREAD_ROWS_SEG, 0, out=ptr[1:])
    return ids.to(torch.int32), ptr, n_long, int(ptr[-1])


class _RowsPlan:
    """What the two passes read besides the baskets: ra / rb / inv_ku of (A, lam), computed
    once per call, the long-list tables (they depend on A alone: kept on it), the workspaces,
    T and the users' mark words for blocks of at most ``nb_max`` baskets."""

    def __init__(self, A: "Interactions", lam: float, nb_max: int):
        N.require_gpu(A.k_item, "A")
        dev = A.k_item.device
        self.A, self.dev = A, dev
        self.ra, self.rb = hybrid_recip(A.k_item, lam)
        self.inv_ku = torch.empty(max(1, A.n_users), dtype=torch.float64, device=dev)
        N.check(N.lib().lg_inv_degree_f64(N.ptr(A.by_user.rowptr), A.n_users,
                                          N.ptr(self.inv_ku), N.stream_handle(dev)),
                "lg_inv_degree_f64")
        self.long_u, self.long_i = A.rows_long
        self._one = None
        self.u_col = A.by_user.col if A.by_user.col.numel() else self._stand_in()
        self.i_col = A.by_item.col if A.by_item.col.numel() else self._stand_in()
        nb_max = max(1, min(int(nb_max), SPREAD_ROWS_BLOCK))
        self.T = torch.empty(max(1, A.n_users * nb_max), dtype=torch.float64, device=dev)
        self.marks = torch.empty(max(1, A.n_users), dtype=torch.int64, device=dev)
        self.ws1 = torch.empty(
            max(1, N.lib().lg_spread_rows_weight_ws_bytes(A.n_items, self.long_u[3])),
            dtype=torch.uint8, device=dev)
        self.ws2 = torch.empty(max(1, N.lib().lg_spread_rows_resource_ws_bytes(self.long_i[3])),
                               dtype=torch.uint8, device=dev)

    def _stand_in(self) -> torch.Tensor:
        """A one-element int32 array for an empty one (an empty tensor has no pointer to pass and
        the entries refuse NULL; never read: no row points into it), made on first need."""
        if self._one is None:
            self._one = torch.zeros(1, dtype=torch.int32, device=self.dev)
        return self._one

    def run(self, B: RowSets, b0: int, b1: int, F: torch.Tensor, evs=None) -> None:
        """F[:b1 - b0, :I] = the F rows of baskets [b0, b1) of B (at most SPREAD_ROWS_BLOCK)."""
        A, s = self.A, N.stream_handle(self.dev)
        nb = b1 - b0
        lu, li = self.long_u, self.long_i
        b_col = B.col if B.col.numel() else self._stand_in()
        _mark(evs, "pass1")
        N.check(N.lib().lg_spread_rows_weight_f64(
            N.ptr(A.by_user.rowptr), N.ptr(self.u_col), A.n_users, A.n_items,
            N.ptr(self.ra), N.ptr(self.inv_ku), N.ptr(B.rowptr[b0:]), N.ptr(b_col), nb,
            N.ptr(lu[0]), N.ptr(lu[1]), lu[2], lu[3], N.ptr(self.T), N.ptr(self.marks),
            N.ptr(self.ws1), self.ws1.numel(), s), "lg_spread_rows_weight_f64")
        _mark(evs, "pass2")
        N.check(N.lib().lg_spread_rows_resource_f64(
            N.ptr(A.by_item.rowptr), N.ptr(self.i_col), A.n_items, A.n_users,
            N.ptr(self.T), N.ptr(self.marks), N.ptr(self.rb), nb, N.ptr(li[0]), N.ptr(li[1]),
            li[2], li[3], N.ptr(F), F.stride(0), N.ptr(self.ws2), self.ws2.numel(), s),
            "lg_spread_rows_resource_f64")
        _mark(evs, None)


def _rows_fill(plan: _RowsPlan, B: RowSets, b0: int, b1: int, F: torch.Tensor, evs=None):
    """F[:b1 - b0] = the F rows of baskets [b0, b1), SPREAD_ROWS_BLOCK of them per call."""
    for c0 in range(b0, b1, SPREAD_ROWS_BLOCK):
        c1 = min(b1, c0 + SPREAD_ROWS_BLOCK)
        plan.run(B, c0, c1, F[c0 - b0:c1 - b0], evs)


def spread_rows_resource(A: Interactions, rows, lam: float,
                         out: torch.Tensor | None = None) -> torch.Tensor:
    """F [n, I] fp64 for n item baskets that need not be rows of A -- a new visitor's cart, a
    session, one item: F[b] = B_b @ HybridS(A, general_W, lam), the row spread_resource gives a
    user with exactly those items, computed as
        T[v] = fl(1/k_v) * sum_{i in items(v), i in B_b} ra_i,   F[b, j] = rb_j * sum_{v in users(j)} T[v]
    by two sweeps of A per block of SPREAD_ROWS_BLOCK baskets (lg_spread_rows_weight_f64,
    lg_spread_rows_resource_f64), with no I x I matrix and no tile. Within 1e-12 relative of the
    dense rows @ spread_hybrid(A, lam), exact zeros where that has them. Every sum runs in the
    order of its own list (csrc/spread_rows.hip): row b is bitwise the one-basket call's row,
    whatever the other baskets, their number and order.

    rows: a RowSets over the items, a list of id lists, a dict {row: ids} or a (rows, items)
    pair (candidate_rows' forms; items named twice count once). out: as in spread_resource."""
    I = A.n_items
    dev = A.k_item.device
    B = _basket_rows(rows, I, dev)
    n = B.n_rows
    if out is not None:
        _typed(out, "out", torch.float64)
        if out.shape[0] < n or out.shape[1] < I or (out.numel() and out.stride(1) != 1):
            raise ValueError(f"out has shape {tuple(out.shape)} strides {out.stride()}, "
                             f"expected at least ({n}, {I}) with unit column stride")
        _same_device(out, "out", A.k_item, "A")
    N.require_gpu(A.k_item, "A")
    F = out if out is not None else torch.empty((n, I), dtype=torch.float64, device=dev)
    if n and I:
        _rows_fill(_RowsPlan(A, lam, n), B, 0, n, F)
    return F


def _rows_f_blocks(A: Interactions, B: RowSets, lam: float, W, evs=None):
    """Yield (b0, b1, Fb) over blocks of the baskets' F rows in one reused buffer, F_BLOCK_BYTES
    of F per block: the two passes, or with W (checked by the caller) _f_blocks' dense rows."""
    if W is not None:
        yield from _f_blocks(B, W)
        return
    n, I = B.n_rows, B.n_cols
    block = max(1, min(n, F_BLOCK_BYTES // max(1, I * 8)))
    plan = _RowsPlan(A, lam, block)
    buf = torch.empty((block, I), dtype=torch.float64, device=plan.dev)
    for b0 in range(0, n, block):
        b1 = min(n, b0 + block)
        _rows_fill(plan, B, b0, b1, buf, evs)
        yield b0, b1, buf[: b1 - b0]


def _rows_guard(A, rows, excl, drop, eu, ei, W):
    """(B, ex) of a spread_rows_* call, every argument checked before the library is reached."""
    I = A.n_items
    dev = A.k_item.device
    B = _basket_rows(rows, I, dev)
    n = B.n_rows
    if eu is not None or ei is not None:
        _g_guard(eu, ei, n, I, f"{n} baskets over {I} items: ")
    if excl is not None and not isinstance(excl, RowSets):
        raise TypeError(f"excl must be a RowSets or None, got {type(excl).__name__}")
    # None: the reference drops what the user already has (drop=False: nothing to keep out)
    ex = (B if drop else None) if excl is None else excl
    _excl_guard(ex, n, "baskets", eu is not None and not drop)
    if ex is not None and ex.col.device != B.col.device:
        raise ValueError(f"excl is on {ex.col.device}, A on {B.col.device}")
    if W is not None:
        _check_W(W, I, f"the fp64 ({I}, {I}) matrix of spread_hybrid")
        _same_device(W, "W", A.k_item, "A")
    return B, ex


def spread_rows_recommend(A: Interactions, rows, lam: float, k: int,
                          excl: RowSets | None = None, drop: bool = True,
                          eu: torch.Tensor | None = None, ei: torch.Tensor | None = None,
                          items=None, W: torch.Tensor | None = None, stats: dict | None = None):
    """Top-k of (G *) spread_rows_resource(A, rows, lam) per basket: (values fp64 [n, k], item
    ids int64 [n, k], {-inf, -1} padding), rows_topk's order and modes, k <= 1024. F is computed
    F_BLOCK_BYTES at a time and never all held.

    excl: None drops each basket's own items (drop=False keeps them), else a RowSets with one
    row per basket. eu: [n, d] float32, one row per basket, supplied by the caller (an unseen
    user has no learned embedding); ei: the item table. items: a candidate item set in
    item_candidates' forms -- F[:, C] is gathered and ranked with the exclusions renumbered and
    ei[C], real item ids in the lists. W: a prebuilt spread_hybrid(A, lam) sends the baskets
    through the dense path (_blocks_topk; lam is then not read). stats: a dict that receives
    t_setup_ms / t_pass1_ms / t_pass2_ms / t_topk_ms (HIP events; one synchronize)."""
    k = int(k)
    if k < 1 or k > 1024:
        raise ValueError(f"k={k} not in [1, 1024]")
    if isinstance(items, slice):
        raise ValueError("spread_rows_recommend: items= is a candidate set (ids or a mask)")
    B, ex = _rows_guard(A, rows, excl, drop, eu, ei, W)
    dev = A.k_item.device
    n, I = B.n_rows, A.n_items
    cand = None if items is None else item_candidates(items, I, dev)
    N.require_gpu(A.k_item, "A")
    if W is not None and cand is None:
        return _blocks_topk(B, W, k, _nonempty(ex), drop, eu, ei)
    vals = torch.full((n, k), float("-inf"), dtype=torch.float64, device=dev)
    idxs = torch.full((n, k), -1, dtype=torch.int64, device=dev)
    if n == 0 or I == 0 or (cand is not None and cand.numel() == 0):
        return vals, idxs
    evs = [] if stats is not None else None
    _mark(evs, "setup")
    if cand is not None:
        c64 = cand.to(torch.int64)
        ex = ex.restrict_cols(cand) if ex is not None else None
        eic = None if ei is None else ei[c64]
    ex = _nonempty(ex)
    for b0, b1, Fb in _rows_f_blocks(A, B, lam, W, evs):
        _mark(evs, "topk")
        exb = ex.slice_rows(b0, b1) if ex is not None else None
        eub = None if eu is None else eu[b0:b1]
        if cand is None:
            vals[b0:b1], idxs[b0:b1] = rows_topk(Fb, k, exb, drop, eub, ei)
        else:
            v, i = rows_topk(Fb[:, c64], k, exb, drop, eub, eic)
            vals[b0:b1], idxs[b0:b1] = v, torch.where(i >= 0, c64[i.clamp(min=0)], i)
        _mark(evs, "setup")
    if evs is not None:
        _mark(evs, None)
        _stage_ms(stats, evs, dev, "setup", "pass1", "pass2", "topk")
    return vals, idxs


def spread_rows_rank(A: Interactions, rows, lam: float, targets, excl: RowSets | None = None,
                     drop: bool = True, eu: torch.Tensor | None = None,
                     ei: torch.Tensor | None = None):
    """Where given items stand among ALL items under spread_rows_recommend's scores -- given
    half a basket, where does the other half rank: (rank int64 [nnz], value fp64 [nnz]) aligned
    with the target CSR's col, rows_rank's definitions. For any k <= 1024, rank < k iff
    spread_rows_recommend(A, rows, lam, k, excl, drop, eu, ei) holds the item at [row, rank],
    with a bit-equal value; a dropped target gets -1. targets: anything candidate_rows takes,
    one row per basket."""
    B, ex = _rows_guard(A, rows, excl, drop, eu, ei, None)
    dev = A.k_item.device
    n, I = B.n_rows, A.n_items
    if isinstance(targets, RowSets) and targets.n_rows != n:
        raise ValueError(f"target rows {targets.n_rows} != {n} baskets")
    targets = candidate_rows(targets, n, I, dev)
    N.require_gpu(A.k_item, "A")
    nnz = int(targets.col.numel())
    rank = torch.full((nnz,), -1, dtype=torch.int64, device=dev)
    val = torch.full((nnz,), float("-inf"), dtype=torch.float64, device=dev)
    if n == 0 or nnz == 0 or I == 0:
        return rank, val
    ex = _nonempty(ex)
    for b0, b1, Fb in _rows_f_blocks(A, B, lam, None):
        rows_rank(Fb, targets.slice_rows(b0, b1),
                  ex.slice_rows(b0, b1) if ex is not None else None, drop,
                  None if eu is None else eu[b0:b1], ei, out=(rank, val))
    return rank, val


def spread_related_items(A: Interactions, item_ids, lam: float, k: int, items=None):
    """"Related to this item": spread_rows_recommend for one single-item basket per entry of
    item_ids (any order, duplicates allowed), the item itself dropped."""
    t = torch.as_tensor(item_ids)
    if t.numel() and (t.dtype == torch.bool or t.is_floating_point() or t.is_complex()):
        raise ValueError("item ids must be integers")
    t = t.reshape(-1).to(torch.int64)
    if not t.is_cuda and t.numel() and (int(t.min()) < 0 or int(t.max()) >= A.n_items):
        raise ValueError(f"item id outside [0, {A.n_items})")
    dev = A.k_item.device
    n = int(t.numel())
    B = RowSets(torch.arange(n + 1, dtype=torch.int64, device=dev), t.to(dev, torch.int32), n,
                A.n_items)
    return spread_rows_recommend(A, B, lam, k, items=items)
