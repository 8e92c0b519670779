"""Measure the spreading / LGCNHS top-K over a candidate item set (csrc/rows_topk_items.hip and
the column view of ops.spread_topk_tiled) and write profiles/spread_items.json.

dense   bench.py's Douban stand-in (600 users x 20,000 items, 60,000 Zipf(1.1) interactions,
        d = 64, lambda = 0.5, the users' own items dropped), with and without the G factor,
        W = spread_hybrid(A, lambda) prebuilt. Per case (users 1 / 8 / 16 / all 600, candidate
        share 1.0 / 0.5 / 0.1 / 0.01, k 20 / 100 / 256) the routes
          fused   lg_spread_rows_topk_items_f64 (ops._spread_topk_items(route="fused"))
          gather  lg_spread_resource_f64 + F[:, C] + rows_topk + the id map
                  (route="gather"; every gather inside the timed window)
          full    today's call without items= (share 1.0 only)
        one call per HIP-event pair, the routes alternating in one process, median of --reps
        rounds after --warmup, spread = (max - min) / median recorded. The lists of all routes
        of a case must be equal bit for bit (the run stops otherwise). `fused_wins`: its median
        beats gather's by more than the larger of the two spreads -- what
        ops.SPREAD_ITEMS_FUSED_* is read off ("routing": per user count, the shares won at
        every k, with and without G).
tiled   bench.py's c4 graph (200,000 x 200,000, 20M interactions, d = 64, tile 2048), k = 20:
        ops.spread_topk_tiled without items= and at share 1.0 / 0.1 / 0.01, one run each
        after a warm-up run: wall seconds, build / bounds / walk ms, the ratio to the
        no-items run. No threshold; reported as measured.

Usage: python scripts/spread_items_time.py [--skip-tiled] [--skip-dense] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys
import time

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [R, os.path.join(R, "light-graph-convolutional-recommendation-algorithm-based-on-hybrid-spreading_amd")]

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(R, "profiles", "spread_items.json"))
ap.add_argument("--reps", type=int, default=25)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--skip-tiled", action="store_true")
ap.add_argument("--skip-dense", action="store_true")
a = ap.parse_args()

out = json.load(open(a.out)) if os.path.exists(a.out) else {}
out["script"] = "scripts/spread_items_time.py"

import torch  # noqa: E402

from lgcnhs import ops  # noqa: E402

dev = torch.device("cuda:0")
USERS, SHARES, KS = (1, 8, 16, 600), (1.0, 0.5, 0.1, 0.01), (20, 100, 256)


def stats(ms):
    s = sorted(ms)
    med = statistics.median(s)
    return {"median_ms": med, "min_ms": s[0], "max_ms": s[-1],
            "spread": (s[-1] - s[0]) / med if med > 0 else 0.0, "n": len(s)}


def same(x, y):
    return bool(torch.equal(x[1], y[1]) and
                torch.equal(x[0].view(torch.int64), y[0].view(torch.int64)))


def dense():
    from lgcnhs.synth import synth_interactions
    du, di, de, lam = 600, 20_000, 60_000, 0.5
    users, items = synth_interactions(du, di, de, seed=3, dist="zipf")
    g = torch.Generator(device=dev).manual_seed(42)
    deu = torch.randn(du, 64, device=dev, generator=g) * 0.1
    dei = torch.randn(di, 64, device=dev, generator=g) * 0.1
    A = ops.Interactions.from_pairs(torch.as_tensor(users), torch.as_tensor(items), du, di, dev)
    W = ops.spread_hybrid(A, lam)
    ex = A.by_user
    res = {"shape": {"users": du, "items": di, "interactions": de, "dim": 64, "lambda": lam,
                     "excluded": int(ex.col.numel())}, "reps": a.reps, "warmup": a.warmup,
           "cases": []}
    for use_g in (False, True):
        eu, ei = (deu, dei) if use_g else (None, None)
        for nu in USERS:
            ids = None if nu == du else torch.randperm(du, device=dev, generator=g)[:nu]
            for share in SHARES:
                nc = max(1, int(round(di * share)))
                cand = torch.sort(torch.randperm(di, device=dev, generator=g)[:nc])[0] \
                    .to(torch.int32)
                for k in KS:
                    def route(name):
                        return lambda: ops._spread_topk_items(A, W, ids, cand, k, ex, True, eu,
                                                              ei, route=name)

                    def full():
                        if ids is None:
                            return ops.spread_topk(A, W, k, ex, True, eu, ei)
                        return ops._spread_topk_users(A, W, ids, k, ex, True, eu, ei)
                    routes = {"fused": route("fused"), "gather": route("gather")}
                    if nc == di:
                        routes["full"] = full
                    outs = {n: fn() for n, fn in routes.items()}
                    equal = {n: same(o, outs["fused"]) for n, o in outs.items()}
                    ms = {n: [] for n in routes}
                    for r in range(a.warmup + a.reps):
                        for n, fn in routes.items():
                            e0 = torch.cuda.Event(enable_timing=True)
                            e1 = torch.cuda.Event(enable_timing=True)
                            e0.record()
                            fn()
                            e1.record()
                            e1.synchronize()
                            if r >= a.warmup:
                                ms[n].append(e0.elapsed_time(e1))
                    rec = {"G": use_g, "users": nu, "share": share, "candidates": nc, "k": k,
                           "routes": {n: stats(v) for n, v in ms.items()},
                           "lists_equal": equal}
                    fu, ga = rec["routes"]["fused"], rec["routes"]["gather"]
                    rec["fused_over_gather"] = fu["median_ms"] / ga["median_ms"]
                    if "full" in rec["routes"]:
                        rec["fused_over_full"] = fu["median_ms"] / rec["routes"]["full"]["median_ms"]
                    rec["fused_wins"] = bool(fu["median_ms"] < ga["median_ms"] *
                                             (1.0 - max(fu["spread"], ga["spread"])))
                    res["cases"].append(rec)
                    print("G=%d users=%d share=%g k=%d  " % (use_g, nu, share, k) +
                          "  ".join("%s %.4f" % (n, s["median_ms"])
                                    for n, s in rec["routes"].items()) +
                          "  wins=%s" % rec["fused_wins"], flush=True)
                    if not all(equal.values()):
                        raise SystemExit(f"lists differ: {equal}")
    # per user count, the shares at which fused wins every k, with and without G
    res["routing"] = {str(nu): {str(sh): all(c["fused_wins"] for c in res["cases"]
                                             if c["users"] == nu and c["share"] == sh)
                                for sh in SHARES} for nu in USERS}
    return res


def tiled():
    from lgcnhs.synth import synth_graph_device
    U, I, E, d, lam, tile, k = 200_000, 200_000, 20_000_000, 64, 0.5, 2048, 20
    _, _, keys = synth_graph_device(U, I, E, 3, dev, dist="uniform")
    A = ops.Interactions.from_pairs(keys // I, keys % I, U, I, dev)
    del keys
    g = torch.Generator(device=dev).manual_seed(42)
    eu = torch.randn(U, d, device=dev, generator=g) * 0.1
    ei = torch.randn(I, d, device=dev, generator=g) * 0.1
    res = {"shape": {"users": U, "items": I, "interactions": E, "dim": d, "lambda": lam,
                     "tile": tile, "k": k, "graph": "bench.py c4 (uniform, seed 3)"},
           "runs": {}}
    ops.spread_topk_tiled(A, lam, k, A.by_user, True, eu, ei, tile=tile)  # warm-up
    torch.cuda.synchronize()
    full_ids = None
    for name, share in (("no_items", None), ("share_1", 1.0), ("share_0.1", 0.1),
                        ("share_0.01", 0.01)):
        kw = {}
        if share is not None:
            nc = max(1, int(round(I * share)))
            kw["items"] = torch.sort(torch.randperm(I, device=dev, generator=g)[:nc])[0] \
                .to(torch.int32)
        st = {}
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        v, i = ops.spread_topk_tiled(A, lam, k, A.by_user, True, eu, ei, tile=tile, stats=st,
                                     **kw)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        run = {"seconds": dt, "candidates": I if share is None else nc,
               "tiles": st["walk_launches"], "walk_ms": st["t_walk_ms"],
               "build_ms": st["t_build_ms"], "bounds_ms": st["t_bounds_ms"],
               "filled_frac": float((i >= 0).float().mean())}
        if share is None:
            full_ids = (v, i)
        elif share == 1.0:
            run["bitwise_the_no_items_lists"] = same((v, i), full_ids)
        else:
            c64 = kw["items"].to(torch.int64)
            inside = torch.isin(i[i >= 0], c64)
            run["ids_all_candidates"] = bool(inside.all())
        res["runs"][name] = run
        print(f"tiled {name}", json.dumps(run), flush=True)
        del v, i
    base = res["runs"]["no_items"]["seconds"]
    res["seconds_over_no_items"] = {n: r["seconds"] / base for n, r in res["runs"].items()}
    return res


os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
if not a.skip_dense:
    out["dense"] = dense()
    json.dump(out, open(a.out, "w"), indent=1)
if not a.skip_tiled:
    torch.cuda.empty_cache()
    out["tiled"] = tiled()
    json.dump(out, open(a.out, "w"), indent=1)
print("wrote", a.out)
