"""Measure the spreading top-K for 128 < k <= 1024 (csrc/rows_topk.hip and the peeled tile
walk of ops.spread_topk_tiled) and write profiles/spread_wide.json.

dense   bench.py's Douban stand-in (600 users x 20,000 items, 60,000 Zipf(1.1) interactions,
        d = 64, lambda = 0.5, the users' own items dropped), with and without the G factor:
        lg_rows_topk_wide_f64 at k = 128 / 129 / 256 / 512 / 1024, lg_rows_topk_f64 at k = 128
        and the reference's op sequence in torch on the same GPU (fp64 G * F, excluded columns
        set to -inf, torch.topk(k); G itself precomputed outside the timed region). One launch
        per HIP-event pair, the variants alternating in one process, median of --reps rounds
        after --warmup.
tiled   bench.py's c4 graph (200,000 x 200,000, 20M interactions, d = 64, tile 2048):
        ops.spread_topk_tiled at k = 128 / 256 / 512, one run each after a warm-up run: wall
        seconds, the ratio to k = 128 and the share spent rebuilding exclusions between the
        peeled passes (stats["t_excl_ms"]).
--resources FILE merges the compiler's per-kernel report (hipcc
-Rpass-analysis=kernel-resource-usage on csrc/rows_topk.hip, stderr saved to FILE) into
the JSON: VGPRs, LDS bytes, scratch bytes per instantiation. No GPU needed for that step.

Usage: python scripts/spread_wide_time.py [--skip-tiled] [--out profiles/spread_wide.json]
       python scripts/spread_wide_time.py --resources report.txt"""
import argparse
import json
import os
import re
import statistics
import sys
import time

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [R, os.path.join(R, "light-graph-convolutional-recommendation-algorithm-based-on-hybrid-spreading_amd")]

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(R, "profiles", "spread_wide.json"))
ap.add_argument("--reps", type=int, default=25)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--skip-tiled", action="store_true")
ap.add_argument("--skip-dense", action="store_true")
ap.add_argument("--resources", default=None)
a = ap.parse_args()

out = json.load(open(a.out)) if os.path.exists(a.out) else {}


def parse_resources(path):
    """{kernel<template arguments>: {vgprs, lds_bytes, scratch_bytes}} from the remarks."""
    res = {}
    for blk in open(path).read().split("Function Name: ")[1:]:
        name = blk.split()[0].rstrip("]")
        # k_rows_topk<lg::LdsList<H>, D, NW> (the register-sorted RegList<M> instantiations are
        # the k <= 128 entry's) and k_lists_merge_wide<CAP, NWB>
        m = re.match(r"_ZN2lg\d+(k_rows_topk|k_lists_merge_wide)I(?:NS_7LdsListI)?((?:Li\d+E)+)", name)
        if not m or (m.group(1) == "k_rows_topk") != ("LdsList" in name):
            continue
        args = [int(x) for x in re.findall(r"Li(\d+)E", name.split("EEv")[0])]
        if m.group(1) == "k_rows_topk":
            key = f"k_rows_topk<LdsList<{args[0]}>, {args[1]}, {args[2]}>"
        else:
            key = f"k_lists_merge_wide<{', '.join(map(str, args))}>"

        def field(label):
            return int(re.search(re.escape(label) + r": (\d+)", blk).group(1))
        res[key] = {"vgprs": field("VGPRs"), "agprs": field("AGPRs"),
                    "lds_bytes": field("LDS Size [bytes/block]"),
                    "scratch_bytes_per_lane": field("ScratchSize [bytes/lane]")}
    return res


if a.resources:
    out["resources"] = {
        "source": "hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage, "
                  "csrc/rows_topk.hip; k_rows_topk<LdsList<H>, D, waves per row> (CAP = 2 H; the record of "
                  "k_rows_topk_wide<CAP, D, waves per row> is the same class), "
                  "k_lists_merge_wide<CAP, rows per block>",
        "kernels": parse_resources(a.resources)}
    assert all(v["scratch_bytes_per_lane"] == 0 for v in out["resources"]["kernels"].values())
    json.dump(out, open(a.out, "w"), indent=1)
    print(f"{len(out['resources']['kernels'])} kernels, scratch 0 in all -> {a.out}")
    sys.exit(0)

import torch  # noqa: E402

from lgcnhs import _native as N  # noqa: E402
from lgcnhs import ops  # noqa: E402

dev = torch.device("cuda:0")


def rows_entry(name, F, k, ex, eu, ei):
    n, m = F.shape
    val = torch.empty((n, k), dtype=torch.float64, device=dev)
    idx = torch.empty((n, k), dtype=torch.int64, device=dev)
    fn = getattr(N.lib(), name)
    args = (N.ptr(F), F.stride(0), n, m, N.ptr(eu), N.ptr(ei), 0 if eu is None else eu.shape[1],
            N.ptr(ex.rowptr), N.ptr(ex.col), N.LG_EXCL_DROP, k, N.ptr(val), N.ptr(idx))

    def run():
        N.check(fn(*args, N.stream_handle(dev)), name)
        return val, idx
    return run


def dense():
    from lgcnhs.synth import synth_interactions
    du, di, de, lam = 600, 20_000, 60_000, 0.5
    users, items = synth_interactions(du, di, de, seed=3, dist="zipf")
    g = torch.Generator(device=dev).manual_seed(42)
    deu = torch.randn(du, 64, device=dev, generator=g) * 0.1
    dei = torch.randn(di, 64, device=dev, generator=g) * 0.1
    A = ops.Interactions.from_pairs(torch.as_tensor(users), torch.as_tensor(items), du, di, dev)
    F = ops.spread_resource(A, ops.spread_hybrid(A, lam))
    ex = A.by_user
    ex_rows = torch.repeat_interleave(torch.arange(du, device=dev), ex.degrees())
    ex_cols = ex.col.to(torch.int64)
    G32 = deu @ dei.T  # (precomputed: the timed sequence starts at G * F)
    ninf = torch.tensor(float("-inf"), dtype=torch.float64, device=dev)
    res = {"shape": {"users": du, "items": di, "interactions": de, "dim": 64, "lambda": lam,
                     "excluded": int(ex.col.numel())}, "reps": a.reps, "warmup": a.warmup}
    for use_g in (False, True):
        eu, ei = (deu, dei) if use_g else (None, None)

        def torch_ref(k):
            def run():
                S = G32.to(torch.float64) * F if use_g else F.clone()
                S.index_put_((ex_rows, ex_cols), ninf)
                return torch.topk(S, k, dim=1)
            return run
        variants = {"narrow_k128": rows_entry("lg_rows_topk_f64", F, 128, ex, eu, ei)}
        for k in (128, 129, 256, 512, 1024):
            variants[f"wide_k{k}"] = rows_entry("lg_rows_topk_wide_f64", F, k, ex, eu, ei)
        for k in (129, 256, 512, 1024):
            variants[f"torch_k{k}"] = torch_ref(k)
        # the lists agree (the twin bit for bit; torch on the item sets except ties at the cut)
        vn, in_ = variants["narrow_k128"]()
        vw, iw = variants["wide_k128"]()
        assert torch.equal(in_, iw) and torch.equal(vn.view(torch.int64), vw.view(torch.int64))
        vt, _ = variants["torch_k1024"]()
        vw, _ = variants["wide_k1024"]()
        if use_g:  # (torch's matmul sums G in another order than the fp32 chain)
            assert torch.allclose(vt, vw, rtol=1e-3, atol=1e-9), "wide k = 1024 vs torch"
        else:
            assert torch.equal(vt, vw), "wide k = 1024 values differ from torch's"
        ms = {n: [] for n in variants}
        for r in range(a.warmup + a.reps):
            for n, fn in variants.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                if r >= a.warmup:
                    ms[n].append(e0.elapsed_time(e1))
        med = {n: statistics.median(v) for n, v in ms.items()}
        leg = {"median_ms": med, "min_ms": {n: min(v) for n, v in ms.items()},
               "wide_over_narrow_k128": {n: med[n] / med["narrow_k128"] for n in med
                                         if n.startswith("wide")},
               "wide_over_torch": {f"k{k}": med[f"wide_k{k}"] / med[f"torch_k{k}"]
                                   for k in (129, 256, 512, 1024)}}
        res["with_G" if use_g else "no_G"] = leg
        print(("with G" if use_g else "no G"), json.dumps(leg["median_ms"]), flush=True)
    return res


def tiled():
    from lgcnhs.synth import synth_graph_device
    U, I, E, d, lam, tile = 200_000, 200_000, 20_000_000, 64, 0.5, 2048
    _, _, keys = synth_graph_device(U, I, E, 3, dev, dist="uniform")
    A = ops.Interactions.from_pairs(keys // I, keys % I, U, I, dev)
    del keys
    g = torch.Generator(device=dev).manual_seed(42)
    eu = torch.randn(U, d, device=dev, generator=g) * 0.1
    ei = torch.randn(I, d, device=dev, generator=g) * 0.1
    res = {"shape": {"users": U, "items": I, "interactions": E, "dim": d, "lambda": lam,
                     "tile": tile, "graph": "bench.py c4 (uniform, seed 3)"}, "runs": {}}
    ops.spread_topk_tiled(A, lam, 128, A.by_user, True, eu, ei, tile=tile)  # warm-up
    torch.cuda.synchronize()
    for k in (128, 256, 512):
        st = {}
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        v, i = ops.spread_topk_tiled(A, lam, k, A.by_user, True, eu, ei, tile=tile, stats=st)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        res["runs"][f"k{k}"] = {
            "seconds": dt, "passes": st.get("peel_passes", 1),
            "excl_rebuild_ms": st.get("t_excl_ms", 0.0),
            "excl_rebuild_share": st.get("t_excl_ms", 0.0) / 1e3 / dt,
            "walk_ms": st["t_walk_ms"], "build_ms": st["t_build_ms"],
            "bounds_ms": st["t_bounds_ms"], "filled_frac": float((i >= 0).float().mean())}
        print(f"tiled k={k}", json.dumps(res["runs"][f"k{k}"]), flush=True)
        del v, i
    base = res["runs"]["k128"]["seconds"]
    res["seconds_over_k128"] = {n: r["seconds"] / base for n, r in res["runs"].items()}
    return res


if not a.skip_dense:
    out["dense"] = dense()
    json.dump(out, open(a.out, "w"), indent=1)
if not a.skip_tiled:
    torch.cuda.empty_cache()
    out["tiled"] = tiled()
    json.dump(out, open(a.out, "w"), indent=1)
print("wrote", a.out)
