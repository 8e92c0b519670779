"""Time ops.spread_rank_tiled (the tile walk's counting finish, MODE_RANK of
csrc/spread_tiled.hip) against the routes a caller had without it, on the C4 shape of
profiles/spread_wide.json's tiled entries: 200,000 x 200,000, 20M interactions (uniform, seed
3), d = 64, lambda 0.5, tile 2048; without and with the G factor. The record -> --out (default
profiles/spread_rank_tiled.json), rewritten after every case.

Cases: all users x 1 target, all users x 10 targets, 16 users x 1 target (random items; the
users' own interactions dropped). Baselines, in the same run and on the same graph:
  topk20    (a) ops.spread_topk_tiled(k = 20): the walk that exists -- the yardstick, since the
            count sweep is one walk with another finish
  topk1024  (b) the peeled ops.spread_topk_tiled(k = 1024) and a torch membership search of
            every target in its row's list: the route to a rank that stops at depth 1,024
Every timing is one whole call between two HIP events on the launch stream (tile builds, score
bounds, host work and the device-side grouping included); per arm one warm-up call, then
--repeats repeats, the arms alternating repeat by repeat; median and [min, max]. `split`: the
stats= event times of one further call (build / bounds / value sweep / count sweep, and the
launches of each sweep). `rank_over_topk20`: ratio of medians; `loses_to_topk20`: the rank's
fastest repeat is slower than (a)'s slowest (beyond the run-to-run spread). `agrees_topk1024`:
the ranks below 1,024 are (b)'s positions, exactly.
  --which noG|G|c5   one leg per process (each GPU step under its own time limit)
  --c5               1,000,000 x 1,000,000, 100M interactions, 1 target per user, no G, once"""
import argparse
import json
import os
import sys

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(R, "light-graph-convolutional-recommendation-algorithm-based-on-hybrid-spreading_amd")


def stats(ms):
    s = sorted(ms)
    return {"median_ms": s[len(s) // 2], "min_ms": s[0], "max_ms": s[-1], "n": len(s)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--which", default="noG", choices=["noG", "G", "c5"])
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--tile", type=int, default=2048)
    ap.add_argument("--skip-topk1024", action="store_true")
    ap.add_argument("--out", default=os.path.join(R, "profiles", "spread_rank_tiled.json"))
    args = ap.parse_args()
    sys.path[:0] = [R, PKG]
    import torch
    from lgcnhs import ops
    from lgcnhs.graph import RowSets
    from lgcnhs.synth import synth_graph_device

    if not torch.cuda.is_available():
        print("no GPU: nothing is measured", file=sys.stderr)
        return 1
    dev = torch.device("cuda:0")
    rec = {}
    if os.path.exists(args.out):
        with open(args.out) as f:
            rec = json.load(f)
    rec.setdefault("script", "scripts/spread_rank_tiled_time.py")
    rec["row_max"] = ops.SPREAD_RANK_ROW_MAX
    rec["cus"] = torch.cuda.get_device_properties(dev).multi_processor_count

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")

    def once(fn):
        e0, e1 = (torch.cuda.Event(enable_timing=True) for _ in range(2))
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), out

    def timed(fns, repeats):
        for fn in fns.values():
            once(fn)  # warm-up
        times = {name: [] for name in fns}
        for _ in range(repeats):
            for name, fn in fns.items():
                times[name].append(once(fn)[0])
        return {n: stats(t) for n, t in times.items()}

    c5 = args.which == "c5"
    U, I, E, d, lam = (1_000_000, 1_000_000, 100_000_000, 64, 0.5) if c5 else \
        (200_000, 200_000, 20_000_000, 64, 0.5)
    tile = args.tile
    _, _, keys = synth_graph_device(U, I, E, 3, dev, dist="uniform")
    A = ops.Interactions.from_pairs(keys // I, keys % I, U, I, dev)
    del keys
    g = torch.Generator(device=dev).manual_seed(42)
    use_g = args.which == "G"
    eu = ei = None
    if use_g:
        eu = torch.randn(U, d, device=dev, generator=g) * 0.1
        ei = torch.randn(I, d, device=dev, generator=g) * 0.1
    leg = {"shape": {"users": U, "items": I, "interactions": E, "dim": d, "lambda": lam,
                     "tile": tile, "graph": "bench.py c4 / c5 (uniform, seed 3)"},
           "G": use_g, "repeats": 1 if c5 else args.repeats, "complete": False, "cases": []}
    rec["c5" if c5 else ("with_G" if use_g else "no_G")] = leg
    save()

    def targets_of(n, per):
        it = torch.randint(0, I, (n * per,), device=dev, generator=g)
        return RowSets.from_pairs(torch.arange(n, device=dev).repeat_interleave(per), it, n, I,
                                  dev)

    for n, per in (((U, 1),) if c5 else ((U, 1), (U, 10), (16, 1))):
        users = None if n == U else torch.arange(n, device=dev) * (U // n)
        tg = targets_of(n, per)
        rowof = torch.arange(n, device=dev).repeat_interleave(tg.degrees())

        def rank():
            return ops.spread_rank_tiled(A, lam, tg, A.by_user, True, eu, ei, users=users,
                                         tile=tile)

        def topk20():
            return ops.spread_topk_tiled(A, lam, 20, A.by_user, True, eu, ei, users=users,
                                         tile=tile)

        def topk1024():
            _, idx = ops.spread_topk_tiled(A, lam, 1024, A.by_user, True, eu, ei, users=users,
                                           tile=tile)
            pos = torch.full((tg.col.numel(),), -1, dtype=torch.int64, device=dev)
            for c0 in range(0, tg.col.numel(), 1 << 18):  # (chunks: [chunk, 1024] compares)
                hit = idx[rowof[c0:c0 + (1 << 18)]] == tg.col[c0:c0 + (1 << 18), None]
                pos[c0:c0 + (1 << 18)] = torch.where(hit.any(1), hit.to(torch.int8).argmax(1), -1)
            return pos

        if c5:
            ms, out = once(rank)
            st = {}
            ops.spread_rank_tiled(A, lam, tg, A.by_user, True, eu, ei, tile=tile, stats=st)
            ms20, _ = once(topk20)
            case = {"users": n, "per_user": per, "rank_ms": ms, "topk20_ms": ms20,
                    "rank_over_topk20": ms / ms20, "split": st,
                    "ranked": int((out[0] >= 0).sum()), "nnz": int(tg.col.numel())}
            leg["cases"].append(case)
            save()
            print(json.dumps(case), flush=True)
            continue
        arms = {"rank": rank, "topk20": topk20}
        t = timed(arms, args.repeats)
        case = {"users": n, "per_user": per, "nnz": int(tg.col.numel()), "arms": t}
        st = {}
        rk = ops.spread_rank_tiled(A, lam, tg, A.by_user, True, eu, ei, users=users, tile=tile,
                                   stats=st)[0]
        case["split"] = st
        case["ranked"] = int((rk >= 0).sum())
        case["median_rank"] = float(rk[rk >= 0].double().median()) if case["ranked"] else None
        case["rank_over_topk20"] = t["rank"]["median_ms"] / t["topk20"]["median_ms"]
        case["loses_to_topk20"] = bool(t["rank"]["min_ms"] > t["topk20"]["max_ms"])
        leg["cases"].append(case)
        save()
        if not args.skip_topk1024:
            # (b): ceil(1024 / 128) whole walks per call -- 3 repeats
            tb = timed({"topk1024": topk1024}, min(3, args.repeats))
            t.update(tb)
            case["rank_over_topk1024"] = t["rank"]["median_ms"] / tb["topk1024"]["median_ms"]
            case["agrees_topk1024"] = bool(torch.equal(
                topk1024(), torch.where((rk >= 0) & (rk < 1024), rk, -1)))
            save()
        print("%d users x %d G=%s  " % (n, per, use_g) +
              "  ".join("%s %.1f [%.1f, %.1f]" % (k, a["median_ms"], a["min_ms"], a["max_ms"])
                        for k, a in t.items()) +
              "  split %s" % json.dumps({k: round(v, 1) for k, v in st.items()}), flush=True)
    leg["complete"] = True
    save()
    print("wrote", args.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
