"""fp16 layer storage against fp32 propagation on one MI355X: the 3-layer
ops.propagate_mean with and without store=torch.float16, same process, same graph, the two
modes alternating, HIP events around each forward. Prints one JSON line
(profiles/half_storage_propagation.json is this script's output).

Workloads: the C5 uniform graph of bench.py (1M users x 1M items, 100M interactions = 200M
directed nnz, seed 3) at d = 64 and d = 128, and the Zipf(1.1) C5 graph at d = 64
(informational). Per workload: ms per layer of both modes (median, min, max over the
repeats), their ratio, G edge-layers/s, and the float16 mode's byte model with its fraction
of the HBM peak.

Byte model of one float16-storage forward of L layers over N nodes and nnz entries, dim d
(fp32 model beside it: what bench.py prices, nnz (8 + 4 d) + N (4 + 4 d) per layer):
  edges    L nnz (4 B source id + 4 B weight + 2 d B gathered float16 row)
  rows     L N (8 B rowptr + 4 B dis + 4 d B read of e0 or acc + 4 d B write of acc or out)
  operand  (L - 1) N 2 d B   the next layer's float16 rows (the last layer writes none)
  convert  N (4 d + 2 d) B   e0 -> float16, once per forward

Run: python scripts/half_storage_bench.py [--reps R --warmup W --workloads a,b] [--tiny]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "light-graph-convolutional-recommendation-algorithm-based-on-hybrid-spreading_amd")
for _p in (REPO, PKG):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import torch  # noqa: E402

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E (bench.py's)
WORKLOADS = {
    # name: (users, items, interactions, dim, layers, item distribution)
    "c5-d64": (1_000_000, 1_000_000, 100_000_000, 64, 3, "uniform"),
    "c5-d128": (1_000_000, 1_000_000, 100_000_000, 128, 3, "uniform"),
    "c5-zipf-d64": (1_000_000, 1_000_000, 100_000_000, 64, 3, "zipf"),
}
TINY = (20_000, 20_000, 1_000_000)  # --tiny: a rehearsal of the script, not a measurement


def half_bytes(nnz: int, n: int, d: int, L: int) -> dict:
    parts = {"edges": L * nnz * (8 + 2 * d), "rows": L * n * (12 + 8 * d),
             "operand": (L - 1) * n * 2 * d, "convert": n * 6 * d}
    parts["total"] = sum(parts.values())
    return parts


def stats(ms: list, L: int) -> dict:
    per = [t / L for t in ms]
    return {"ms_per_layer": statistics.median(per), "min": min(per), "max": max(per),
            "ms_per_forward": statistics.median(ms)}


def run(name: str, reps: int, warmup: int, tiny: bool, dev) -> dict:
    from lgcnhs import ops
    from lgcnhs.graph import Adjacency
    from lgcnhs.synth import synth_graph_device
    U, I, E, d, L, dist = WORKLOADS[name]
    if tiny:
        U, I, E = TINY
    n = U + I
    rowptr, src, keys = synth_graph_device(U, I, E, 3, dev, dist=dist)
    del keys
    adj = Adjacency(rowptr, src, n, n_users=U, symmetric=True)
    adj.dis(), adj.edge_weight()
    plan = adj.long_plan()
    nnz = adj.nnz
    e0 = torch.randn(n, d, device=dev, generator=torch.Generator(device=dev).manual_seed(43)) * 0.1
    modes = {"fp32": None, "fp16": torch.float16}
    outs = {}
    for _ in range(max(1, warmup)):
        for m, store in modes.items():
            outs[m] = ops.propagate_mean(adj, e0, L, store=store)
    torch.cuda.synchronize()
    diff = float((outs["fp16"] - outs["fp32"]).abs().max())
    outs.clear()
    ms = {m: [] for m in modes}
    for _ in range(reps):  # the two modes alternate: drift of the shared box hits both
        for m, store in modes.items():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            ops.propagate_mean(adj, e0, L, store=store)
            e.record()
            e.synchronize()
            ms[m].append(s.elapsed_time(e))
    f32, f16 = stats(ms["fp32"], L), stats(ms["fp16"], L)
    hb = half_bytes(nnz, n, d, L)
    f32_bytes = L * (nnz * (8 + 4 * d) + n * (4 + 4 * d))
    for st in (f32, f16):
        st["G_edge_layers_per_s"] = nnz * L / st["ms_per_forward"] / 1e6
    f32["alg_bytes_per_forward"] = f32_bytes
    f32["hbm_frac"] = f32_bytes / f32["ms_per_forward"] / 1e6 / HBM_PEAK_GBS
    f16["byte_model_per_forward"] = hb
    f16["hbm_frac"] = hb["total"] / f16["ms_per_forward"] / 1e6 / HBM_PEAK_GBS
    res = {"users": U, "items": I, "nnz": nnz, "dim": d, "layers": L, "dist": dist,
           "long_rows": plan.n_long, "reps": reps, "warmup": max(1, warmup),
           "fp32": f32, "fp16": f16,
           "ratio": f32["ms_per_layer"] / f16["ms_per_layer"],
           "ratio_min_max": [f32["min"] / f16["max"], f32["max"] / f16["min"]],
           "byte_model_ceiling": f32_bytes / hb["total"],
           # faster by more than the run-to-run spread: every float16 repeat beats every fp32 one
           "faster_beyond_spread": f16["max"] < f32["min"],
           "max_abs_diff_fp16_vs_fp32": diff}
    del adj, e0, rowptr, src
    torch.cuda.empty_cache()
    return res


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--workloads", default=",".join(WORKLOADS))
    ap.add_argument("--tiny", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print("half_storage_bench: no GPU visible (nothing is measured on the CPU)",
              file=sys.stderr)
        return 2
    dev = torch.device("cuda:0")
    from lgcnhs import _native as N
    rec = {"what": "3-layer propagate_mean, store=torch.float16 vs fp32, alternating, HIP events",
           "device": torch.cuda.get_device_name(dev), "library": os.path.relpath(N.LIB_PATH, REPO),
           "tiny": a.tiny, "hbm_peak_GBs": HBM_PEAK_GBS, "workloads": {}}
    for name in a.workloads.split(","):
        rec["workloads"][name] = run(name, a.reps, a.warmup, a.tiny, dev)
    print(json.dumps(rec))
    return 0


if __name__ == "__main__":
    sys.exit(main())
