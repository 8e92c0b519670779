"""Time lg_score_topk_batch_f32 (K2b, csrc/topk_batch.hip) against the routes a caller has
without it, for B users of a 100,000-user table: B in {1, 8, 16, 32, 64, 256} x items in
{100K, 1M} x k in {20, 100} x d in {64, 128}, N(0, 0.1^2) embeddings, ~100 excluded items per
user. One JSON record -> --out (default profiles/topk_batch.json).

Routes (one child process, all routes of a case alternating window by window):
  new        ops.score_topk_users with BATCH_MAX_USERS lifted: the batch entry on the ids, in
             chunks of 64, no gathers
  default    ops.score_topk(eu[ids], ei, k, excl.take(ids)) at its default dispatch, on rows
             gathered once outside the window
  ns64 .. ns4096   the same call with screen=False, n_splits = 64 / 256 / 1024 / 4096: the best
             the existing entry can do
  gathered   `default` with the two gathers (eu[ids], excl.take(ids)) inside the window: what
             a request costs today end to end
A window is --calls back-to-back calls between two HIP events (its time per call); per route
the median and (max - min) / median over --windows windows. Every route's lists and value sums
must equal `new`'s. The verdict per case: new beats the best of default / ns* by more than the
larger of the two spreads; `batch_max_users` = the largest B for which that holds at both
catalog sizes for every k and d timed (0: never) -- the value of ops.BATCH_MAX_USERS.
  --batches 1,8,...  --items 100000,1000000  --ks 20,100  --dims 64,128  --windows 5"""
import argparse
import json
import os
import subprocess
import sys
import threading

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(R, "light-graph-convolutional-recommendation-algorithm-based-on-hybrid-spreading_amd")
SPLITS = (64, 256, 1024, 4096)


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
    ops.BATCH_MAX_USERS = 1 << 30
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
            for k in ints(args.ks):
                for B in ints(args.batches):
                    ids = torch.randint(0, U, (B,), device=dev, generator=g)
                    eg, xg = eu[ids].contiguous(), excl.take(ids)
                    routes = {
                        "new": lambda: ops.score_topk_users(eu, ei, ids, k, excl),
                        "default": lambda: ops.score_topk(eg, ei, k, xg),
                        "gathered": lambda: ops.score_topk(eu[ids], ei, k, excl.take(ids)),
                    }
                    for ns in SPLITS:
                        routes[f"ns{ns}"] = (lambda ns=ns: ops.score_topk(
                            eg, ei, k, xg, n_splits=ns, screen=False))
                    outs = {}
                    for name, fn in routes.items():  # warm-up + the results
                        fn()
                        outs[name] = fn()
                    torch.cuda.synchronize()
                    nv, ni_ = outs["new"]
                    equal = {name: bool(torch.equal(i, ni_) and torch.equal(
                        v.view(torch.int32), nv.view(torch.int32)) and
                        float(v[torch.isfinite(v)].double().sum()) ==
                        float(nv[torch.isfinite(nv)].double().sum()))
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
                    rec = {"d": d, "items": I, "k": k, "B": B,
                           "grid": list(ops.batch_topk_grid(min(B, 64), I, k, dev)),
                           "routes": {n: stats(t) for n, t in times.items()},
                           "lists_and_sums_equal": equal}
                    kern = {n: s for n, s in rec["routes"].items()
                            if n == "default" or n.startswith("ns")}
                    best = min(kern, key=lambda n: kern[n]["median_ms"])
                    new = rec["routes"]["new"]
                    margin = max(new["spread"], kern[best]["spread"])
                    rec["parent_best"] = best
                    rec["new_over_parent_best"] = new["median_ms"] / kern[best]["median_ms"]
                    rec["new_wins"] = bool(
                        new["median_ms"] < kern[best]["median_ms"] * (1.0 - margin))
                    print("RECORD " + json.dumps(rec), flush=True)
                    if not all(equal.values()):
                        print("results differ:", equal, file=sys.stderr)
                        return 1
    return 0


def batch_max_users(cases):
    """The largest B such that `new` wins every (items, k, d) case timed at that B and at every
    smaller B (the dispatch sends all lists up to it to the batch entry); 0: never."""
    best = 0
    for B in sorted({c["B"] for c in cases}):
        if not all(c["new_wins"] for c in cases if c["B"] == B):
            break
        best = B
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,8,16,32,64,256")
    ap.add_argument("--items", default="100000,1000000")
    ap.add_argument("--ks", default="20,100")
    ap.add_argument("--dims", default="64,128")
    ap.add_argument("--table-users", type=int, default=100_000)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--calls", type=int, default=40, help="calls per window")
    ap.add_argument("--out", default=os.path.join(R, "profiles", "topk_batch.json"))
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--timeout", type=int, default=540, help="seconds for the whole run")
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
        sys.stdout.write(line)
        sys.stdout.flush()
        if line.startswith("RECORD "):
            cases.append(json.loads(line[7:]))
    code = p.wait()
    killer.cancel()
    rec = {"script": "scripts/topk_batch_time.py", "windows": args.windows,
           "calls_per_window": args.calls, "table_users": args.table_users,
           "complete": code == 0, "batch_max_users": batch_max_users(cases),
           "cases": cases}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print("wrote", args.out, "batch_max_users", rec["batch_max_users"])
    return code


if __name__ == "__main__":
    sys.exit(main())
