"""Time lg_score_topk_batch_items_f32 (K2i, csrc/topk_items.hip) against the routes a caller
has without it, for B users of a 100,000-user table over a candidate item set: B in
{1, 8, 16, 32, 64} x items in {100K, 1M} x candidate share in {1.0, 0.5, 0.1, 0.01} (random,
ascending) x k in {20, 100} x d in {64, 128}, N(0, 0.1^2) embeddings, ~100 excluded items per
user. One JSON record -> --out (default profiles/topk_items.json).

Routes (one child process, all routes of a case alternating window by window):
  new              ops.score_topk_users(items=cand) with ITEMS_BATCH_MAX_USERS lifted: the new
                   entry on the ids, in chunks of 16, nothing gathered
  gather           what a caller has without the entry: ei[cand], eu[ids],
                   excl.take(ids).restrict_cols(cand), ops.score_topk_users on the sub-table
                   and the id map, with the gathers inside the window
  gather_prepared  the same with the sub-table and the renumbered exclusion rows built outside
                   the window (a filter that many requests share)
  full             at share 1.0: lg_score_topk_batch_f32 (K2b) on the whole table -- the cost of
                   the indirection
A window is --calls back-to-back calls between two HIP events (its time per call); per route
the median and (max - min) / median over --windows windows. Every route's lists must equal
`new`'s. The verdict per case: new beats `gather` by more than the larger of the two spreads;
`items_batch_max_users` = the largest B for which that holds at both catalog sizes for every
share, k and d timed, and at every smaller B (0: never) -- the value of
ops.ITEMS_BATCH_MAX_USERS. `gathered_tb_s` is (candidates x (d x 4 + 4) bytes) / new's median:
the rows and ids the kernel has to read, against the 8 TB/s HBM peak in `hbm_frac`.
  --batches 1,8,...  --items 100000,1000000  --shares 1.0,0.5,0.1,0.01  --ks 20,100
  --dims 64,128  --windows 5"""
import argparse
import json
import os
import subprocess
import sys
import threading

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(R, "light-graph-convolutional-recommendation-algorithm-based-on-hybrid-spreading_amd")
HBM_PEAK = 8.0e12  # bytes / s


def stats(ms):
    s = sorted(ms)
    med = s[len(s) // 2]
    return {"median_ms": med, "min_ms": s[0], "max_ms": s[-1],
            "spread": (s[-1] - s[0]) / med if med > 0 else 0.0, "n": len(s)}


def child(args):
    sys.path[:0] = [R, PKG]
    import torch
    from lgcnhs import ops
    from lgcnhs.graph import RowSets

    dev = torch.device("cuda:0")
    ops.ITEMS_BATCH_MAX_USERS = 1 << 30
    batch_max = ops.BATCH_MAX_USERS  # the gather routes dispatch as the product does
    U = args.table_users
    ints = lambda s: [int(x) for x in s.split(",")]
    for d in ints(args.dims):
        for I in ints(args.items):
            g = torch.Generator(device=dev).manual_seed(42)
            eu = torch.randn(U, d, device=dev, generator=g) * 0.1
            ei = torch.randn(I, d, device=dev, generator=g) * 0.1
            ku = torch.unique(torch.randint(0, U, (U * 100,), device=dev, generator=g) * I +
                              torch.randint(0, I, (U * 100,), device=dev, generator=g))
            excl = RowSets.from_pairs(ku // I, ku % I, U, I, dev)
            del ku
            for share in [float(x) for x in args.shares.split(",")]:
                nc = max(1, int(round(I * share)))
                cand = torch.sort(torch.randperm(I, device=dev, generator=g)[:nc])[0] \
                    .to(torch.int32)
                c64 = cand.to(torch.int64)
                sub_p = ei[c64]
                for k in ints(args.ks):
                    for B in ints(args.batches):
                        ids = torch.randint(0, U, (B,), device=dev, generator=g)
                        rows = torch.arange(B, device=dev)
                        # (a request none of whose excluded items is a candidate passes no
                        # exclusion set: an empty tensor has no pointer)
                        some = lambda x: x if x.col.numel() else None
                        eg_p, xg_p = eu[ids], some(excl.take(ids).restrict_cols(cand))

                        def back(vi):
                            v, i = vi
                            return v, torch.where(i >= 0, c64[i.clamp(min=0)], i)

                        def full():
                            ops.BATCH_MAX_USERS = 1 << 30
                            try:
                                return ops.score_topk_users(eu, ei, ids, k, excl)
                            finally:
                                ops.BATCH_MAX_USERS = batch_max

                        routes = {
                            "new": lambda: ops.score_topk_users(eu, ei, ids, k, excl,
                                                                items=cand),
                            "gather": lambda: back(ops.score_topk_users(
                                eu[ids], ei[c64], rows, k,
                                some(excl.take(ids).restrict_cols(cand)))),
                            "gather_prepared": lambda: back(ops.score_topk_users(
                                eg_p, sub_p, rows, k, xg_p)),
                        }
                        if nc == I:
                            routes["full"] = full
                        outs = {}
                        for name, fn in routes.items():  # warm-up + the results
                            fn()
                            outs[name] = fn()
                        torch.cuda.synchronize()
                        nv, ni_ = outs["new"]
                        equal = {name: bool(torch.equal(i, ni_) and torch.equal(
                            v.view(torch.int32), nv.view(torch.int32)))
                            for name, (v, i) in outs.items()}
                        times = {name: [] for name in routes}
                        for _ in range(args.windows):
                            for name, fn in routes.items():
                                e0 = torch.cuda.Event(enable_timing=True)
                                e1 = torch.cuda.Event(enable_timing=True)
                                e0.record()
                                for _c in range(args.calls):
                                    fn()
                                e1.record()
                                e1.synchronize()
                                times[name].append(e0.elapsed_time(e1) / args.calls)
                        rec = {"d": d, "items": I, "share": share, "candidates": nc, "k": k,
                               "B": B, "grid": list(ops.items_topk_grid(min(B, 16), nc, k, dev)),
                               "routes": {n: stats(t) for n, t in times.items()},
                               "lists_equal": equal}
                        new, gat = rec["routes"]["new"], rec["routes"]["gather"]
                        margin = max(new["spread"], gat["spread"])
                        rec["new_over_gather"] = new["median_ms"] / gat["median_ms"]
                        rec["new_over_gather_prepared"] = (
                            new["median_ms"] / rec["routes"]["gather_prepared"]["median_ms"])
                        if "full" in rec["routes"]:
                            rec["new_over_full"] = (new["median_ms"]
                                                    / rec["routes"]["full"]["median_ms"])
                        rec["new_wins"] = bool(
                            new["median_ms"] < gat["median_ms"] * (1.0 - margin))
                        calls = -(-B // 16)  # the table's candidates are read once per call
                        rec["gathered_tb_s"] = (calls * nc * (d * 4 + 4)
                                                / (new["median_ms"] * 1e-3) / 1e12)
                        rec["hbm_frac"] = rec["gathered_tb_s"] * 1e12 / HBM_PEAK
                        print("RECORD " + json.dumps(rec), flush=True)
                        if not all(equal.values()):
                            print("results differ:", equal, file=sys.stderr)
                            return 1
                del sub_p, cand, c64
    return 0


def items_batch_max_users(cases):
    """The largest B such that `new` wins every (items, share, k, d) case timed at that B and at
    every smaller B (the dispatch sends all lists up to it to the new entry); 0: never."""
    best = 0
    for B in sorted({c["B"] for c in cases}):
        if not all(c["new_wins"] for c in cases if c["B"] == B):
            break
        best = B
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,8,16,32,64")
    ap.add_argument("--items", default="100000,1000000")
    ap.add_argument("--shares", default="1.0,0.5,0.1,0.01")
    ap.add_argument("--ks", default="20,100")
    ap.add_argument("--dims", default="64,128")
    ap.add_argument("--table-users", type=int, default=100_000)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--calls", type=int, default=40, help="calls per window")
    ap.add_argument("--out", default=os.path.join(R, "profiles", "topk_items.json"))
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--timeout", type=int, default=840, help="seconds for the whole run")
    args = ap.parse_args()
    if args.child:
        return child(args)
    cmd = [sys.executable, os.path.abspath(__file__), "--child"] + sys.argv[1:]
    # the child's lines are passed on as they come; a run past --timeout keeps what finished
    p = subprocess.Popen(cmd, stdout=subprocess.PIPE, text=True)
    killer = threading.Timer(args.timeout, p.kill)
    killer.start()
    cases = []
    for line in p.stdout:
        if line.startswith("RECORD "):
            c = json.loads(line[7:])
            cases.append(c)
            print("d=%d I=%d share=%g k=%d B=%d  " % (c["d"], c["items"], c["share"], c["k"],
                                                     c["B"]) +
                  "  ".join("%s %.4f" % (n, s["median_ms"]) for n, s in c["routes"].items()) +
                  "  wins=%s" % c["new_wins"], flush=True)
        else:
            sys.stdout.write(line)
            sys.stdout.flush()
    code = p.wait()
    killer.cancel()
    rec = {"script": "scripts/topk_items_time.py", "windows": args.windows,
           "calls_per_window": args.calls, "table_users": args.table_users,
           "complete": code == 0, "items_batch_max_users": items_batch_max_users(cases),
           "cases": cases}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print("wrote", args.out, "items_batch_max_users", rec["items_batch_max_users"])
    return code


if __name__ == "__main__":
    sys.exit(main())
