"""Time ops.spread_rows_recommend (spreading for item baskets outside the graph: the two sweeps
of csrc/spread_rows.hip and rows_topk) against the routes a caller had without it. The record
-> --out (default profiles/spread_rows.json), rewritten after every case.

  --which c4      200,000 x 200,000, 20M interactions (uniform, seed 3; the README's C4 shape),
                  d = 64, lambda 0.5, k = 20: 1 / 8 / 16 / 32 / 64 / 256 baskets of 1 / 10 / 100
                  random items, without and with the G factor; and, for baskets that are the rows
                  of as many users, (a) ops.spread_topk_tiled(users=ids, k=20, tile 2048) -- the
                  only route above the dense limit, and only for rows of A
  --which douban  600 x 20,000, 240,000 interactions: the same baskets against (b)
                  ops.spread_recommend(users=ids, W=W) for baskets that are users' rows
  --which c5      1,000,000 x 1,000,000, 100M interactions: the new path alone (no other route
                  serves a foreign row there)
Every timing is one whole call between two HIP events on the launch stream (host work and the
basket set-up included); per arm one warm-up call, then --repeats repeats, the arms alternating
repeat by repeat; median and [min, max]. `split`: the stats= event times of one further call
(setup = ra / rb / 1/k_u and the buffers, pass1 = the basket words and the sweep of A by user,
pass2 = the sweep of A by item and the F rows, topk = rows_topk). `hbm`: each pass's bytes on the
footprint model -- 4 nnz of ids, the row pointers, the gathered words (8 per item in pass 1, 8
per user in pass 2), ra of the basket items, the T entries of the marked users (written in pass
1, read in pass 2) and the F rows written -- over its time, as a fraction of 8.0 TB/s.
`loses`: the new path's fastest repeat is slower than the baseline's slowest."""
import argparse
import json
import os
import sys

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(R, "light-graph-convolutional-recommendation-algorithm-based-on-hybrid-spreading_amd")
HBM_PEAK = 8.0e12

SHAPES = {"c4": (200_000, 200_000, 20_000_000), "douban": (600, 20_000, 240_000),
          "c5": (1_000_000, 1_000_000, 100_000_000)}


def stats(ms):
    s = sorted(ms)
    return {"median_ms": s[len(s) // 2], "min_ms": s[0], "max_ms": s[-1], "n": len(s)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--which", default="c4", choices=list(SHAPES))
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--tile", type=int, default=2048)
    ap.add_argument("--out", default=os.path.join(R, "profiles", "spread_rows.json"))
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
    rec.setdefault("script", "scripts/spread_rows_time.py")
    rec["block"], rec["seg"] = ops.SPREAD_ROWS_BLOCK, ops.SPREAD_ROWS_SEG
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

    U, I, E = SHAPES[args.which]
    d, lam, k = 64, 0.5, 20
    _, _, keys = synth_graph_device(U, I, E, 3, dev, dist="uniform")
    A = ops.Interactions.from_pairs(keys // I, keys % I, U, I, dev)
    del keys
    nnz = int(A.by_user.col.numel())
    g = torch.Generator(device=dev).manual_seed(42)
    ei = torch.randn(I, d, device=dev, generator=g) * 0.1
    W = ops.spread_hybrid(A, lam) if args.which == "douban" else None
    leg = {"shape": {"users": U, "items": I, "interactions": nnz, "dim": d, "lambda": lam,
                     "k": k, "graph": "uniform, seed 3"},
           "repeats": args.repeats, "complete": False, "cases": []}
    rec[args.which] = leg
    save()

    def hbm(B, st, n):
        """Fractions of the HBM peak of the two passes on the footprint model."""
        calls = -(-n // ops.SPREAD_ROWS_BLOCK)
        nb_items = int(B.col.numel())
        # (the T entries of the marked users: an upper bound from the basket items' degrees)
        reach = int(A.k_item[B.col.to(torch.int64)].sum())
        p1 = calls * (4 * nnz + 8 * (U + 1) + 8 * I + 8 * U) + 8 * nb_items + 8 * reach
        p2 = calls * (4 * nnz + 8 * (I + 1) + 8 * U) + 8 * reach + 8 * n * I
        out = {"pass1_bytes": p1, "pass2_bytes": p2, "t_entries_upper_bound": reach}
        if st.get("t_pass1_ms"):
            out["pass1_of_peak"] = p1 / (st["t_pass1_ms"] * 1e-3) / HBM_PEAK
        if st.get("t_pass2_ms"):
            out["pass2_of_peak"] = p2 / (st["t_pass2_ms"] * 1e-3) / HBM_PEAK
        return out

    sizes = (1, 8, 16, 32, 64, 256)
    for use_g in (False, True):
        for n in sizes:
            eu = torch.randn(n, d, device=dev, generator=g) * 0.1 if use_g else None
            ids = torch.arange(n, device=dev) * (U // n)
            for per in (1, 10, 100, "rows"):
                if per == "rows":
                    B = A.by_user.take(ids)
                else:
                    it = torch.randint(0, I, (n * per,), device=dev, generator=g)
                    B = RowSets.from_pairs(torch.arange(n, device=dev).repeat_interleave(per),
                                           it, n, I, dev)
                e_i = ei if use_g else None

                def rows():
                    return ops.spread_rows_recommend(A, B, lam, k, eu=eu, ei=e_i)

                arms = {"rows": rows}
                base = None
                if per == "rows" and args.which == "c4":
                    base = "topk_tiled"
                    eu_all = None
                    if use_g:  # (the baseline takes eu by user id)
                        eu_all = torch.zeros(U, d, device=dev)
                        eu_all[ids] = eu

                    def topk_tiled():
                        return ops.spread_topk_tiled(A, lam, k, A.by_user, True, eu_all, e_i,
                                                     users=ids, tile=args.tile)
                    arms[base] = topk_tiled
                elif per == "rows" and args.which == "douban":
                    base = "dense_W"
                    eu_all = None
                    if use_g:
                        eu_all = torch.zeros(U, d, device=dev)
                        eu_all[ids] = eu

                    def dense_W():
                        return ops.spread_recommend(A, lam, k, A.by_user, True, eu_all, e_i,
                                                    users=ids, W=W)
                    arms[base] = dense_W
                t = timed(arms, args.repeats)
                st = {}
                got = ops.spread_rows_recommend(A, B, lam, k, eu=eu, ei=e_i, stats=st)
                case = {"baskets": n, "items_per_basket": per, "G": use_g,
                        "basket_items": int(B.col.numel()), "arms": t, "split": st,
                        "hbm": hbm(B, st, n)}
                if base:
                    case["rows_over_" + base] = t["rows"]["median_ms"] / t[base]["median_ms"]
                    case["loses"] = bool(t["rows"]["min_ms"] > t[base]["max_ms"])
                    ref = arms[base]()
                    v, rv = got[0], ref[0]
                    fin = torch.isfinite(rv)
                    case["max_rel_diff_vs_" + base] = float(
                        ((v[fin] - rv[fin]).abs() / rv[fin].abs().clamp(min=1e-300)).max()) \
                        if bool(fin.any()) else 0.0
                    case["same_lists"] = float((got[1] == ref[1]).all(1).double().mean())
                leg["cases"].append(case)
                save()
                print("%s %3d baskets x %-4s G=%d  " % (args.which, n, per, use_g) +
                      "  ".join("%s %.2f [%.2f, %.2f]" % (a, x["median_ms"], x["min_ms"],
                                                         x["max_ms"]) for a, x in t.items()) +
                      "  split %s" % json.dumps({s: round(x, 2) for s, x in st.items()}),
                      flush=True)
    leg["complete"] = True
    save()
    print("wrote", args.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
