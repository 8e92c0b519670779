"""Time lg_score_rank_f32 (K2k, csrc/rank.hip: the full-catalog rank of held-out items) against
the two routes a caller has without it. Tables: 100,000 users x 1M items, N(0, 0.1^2)
embeddings, d = 64 (the C5 item table). Shapes (users x targets per user): 32768 x 1,
32768 x LG_RANK_ROW_MAX, 4096 x 10 (rows split by ops.rank_rows), 16 x 1 and 64 x 1 (the split
plan); each with and without an exclusion CSR of ~100 items per user.
The record -> --out (default profiles/score_rank.json), rewritten after every case.

Arms (one process, alternating repeat by repeat):
  rank   ops.score_rank, n_splits from ops.rank_splits
  topk   (a) ops.score_topk(screen=False, k=20) on the same users: the same MFMA stream with the
         list work in place of the counting
  torch  (b) the route a user has today: eu[chunk] @ ei.T in chunks of --chunk users, the excluded
         pairs (flat indices built outside the timing) set to the mask value, then per target
         ((S > t) | ((S == t) & (id < i))).sum(1)
A repeat is `calls` back-to-back calls between two HIP events (time per call), calls sized so
that a repeat lasts >= 20 ms; warm-up calls per arm first; per arm the median and [min, max] of
--repeats repeats. Per case `equal_torch64`: the kernel's ranks of the first 64 users equal arm
(b)'s, computed on the library's own dense chain scores (ops.score_dense) so that the comparison
is exact; `rank_over_topk`, `rank_over_torch`: ratios of medians; `loses_to_topk`: the kernel's
fastest repeat is slower than (a)'s slowest (a loss beyond run-to-run spread).
`split_sweep`: every shape (with the exclusion CSR) over n_splits: 61 to 3904 for the few-user
shapes, 1 to 16 for the others.
  --shapes 32768x1,32768x4,4096x10,16x1,64x1  --repeats 7"""
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
    ap.add_argument("--shapes", default="32768x1,32768x4,4096x10,16x1,64x1")
    ap.add_argument("--dim", type=int, default=64)
    ap.add_argument("--items", type=int, default=1_000_000)
    ap.add_argument("--table-users", type=int, default=100_000)
    ap.add_argument("--chunk", type=int, default=512)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(R, "profiles", "score_rank.json"))
    args = ap.parse_args()
    sys.path[:0] = [R, PKG]
    import torch
    from lgcnhs import ops
    from lgcnhs.graph import RowSets

    if not torch.cuda.is_available():
        print("no GPU: nothing is measured", file=sys.stderr)
        return 1
    dev = torch.device("cuda:0")
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    U, I, d = args.table_users, args.items, args.dim
    shapes = [tuple(int(x) for x in s.split("x")) for s in args.shapes.split(",")]
    rec = {"script": "scripts/score_rank_time.py", "repeats": args.repeats,
           "warmup": args.warmup, "items": I, "table_users": U, "d": d, "cus": cus,
           "row_max": ops.RANK_ROW_MAX, "waves_per_cu": ops.RANK_WAVES_PER_CU,
           "min_split": ops.RANK_MIN_SPLIT, "chunk": args.chunk, "complete": False,
           "cases": [], "split_sweep": []}

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")

    def timed(fns):
        """{name: stats}: warm-ups, then the arms alternating repeat by repeat."""
        calls = {}
        for name, fn in fns.items():
            for _ in range(args.warmup - 1):
                fn()
            e0, e1 = (torch.cuda.Event(enable_timing=True) for _ in range(2))
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            calls[name] = max(1, min(100, int(20.0 / max(e0.elapsed_time(e1), 1e-3))))
        times = {name: [] for name in fns}
        for _ in range(args.repeats):
            for name, fn in fns.items():
                e0, e1 = (torch.cuda.Event(enable_timing=True) for _ in range(2))
                e0.record()
                for _c in range(calls[name]):
                    fn()
                e1.record()
                e1.synchronize()
                times[name].append(e0.elapsed_time(e1) / calls[name])
        out = {n: stats(t) for n, t in times.items()}
        for n in out:
            out[n]["calls_per_repeat"] = calls[n]
        return out

    g = torch.Generator(device=dev).manual_seed(42)
    ku = torch.unique(torch.randint(0, U, (U * 100,), device=dev, generator=g) * I +
                      torch.randint(0, I, (U * 100,), device=dev, generator=g))  # (sorted)
    excl_all = RowSets.from_pairs(ku // I, ku % I, U, I, dev)
    eu = torch.randn(U, d, device=dev, generator=g) * 0.1
    ei = torch.randn(I, d, device=dev, generator=g) * 0.1
    item_ids = torch.arange(I, device=dev)

    def torch_ranks(users, tgt, valid, ex_flat, chunk, scores=None):
        """Arm (b): ranks [n, T] (-1 where not valid) of the padded targets tgt [n, T]."""
        n, T = tgt.shape
        out = torch.full((n, T), -1, dtype=torch.int64, device=dev)
        for c0 in range(0, n, chunk):
            c1 = min(c0 + chunk, n)
            S = (eu[users[c0:c1]] @ ei.T) if scores is None else scores(users[c0:c1])
            if ex_flat is not None:
                lo, hi = ex_flat[1][c0], ex_flat[1][c1]
                S.view(-1)[ex_flat[0][lo:hi] - c0 * I] = ops.MASK_VALUE
            for m in range(T):
                i = tgt[c0:c1, m]
                t = S.gather(1, i[:, None])
                b = (S > t) | ((S == t) & (item_ids[None, :] < i[:, None]))
                out[c0:c1, m] = torch.where(valid[c0:c1, m], b.sum(1), out[c0:c1, m])
        return out

    for rows, per in shapes:
        users = torch.randperm(U, device=dev, generator=g)[:rows]
        it = torch.randint(0, I, (rows * per,), device=dev, generator=g)
        tg = RowSets.from_pairs(torch.arange(rows, device=dev).repeat_interleave(per), it, rows,
                                I, dev)
        deg = tg.degrees()
        nnz, T = int(tg.col.numel()), int(deg.max())
        rowof = torch.arange(rows, device=dev).repeat_interleave(deg)
        pos = torch.arange(nnz, device=dev) - tg.rowptr[:-1][rowof]
        pad = torch.zeros((rows, T), dtype=torch.int64, device=dev)
        pad[rowof, pos] = tg.col.to(torch.int64)
        valid = torch.zeros((rows, T), dtype=torch.bool, device=dev)
        valid[rowof, pos] = True
        for with_excl in (True, False):
            excl = excl_all if with_excl else None
            ex_flat = None
            if with_excl:  # flat (row-in-request, item) indices of the users' excluded pairs
                sub = excl_all.take(users)
                r_of = torch.arange(rows, device=dev).repeat_interleave(sub.degrees())
                ex_flat = (r_of * I + sub.col.to(torch.int64), sub.rowptr.tolist())
            kr = int(ops.rank_rows(tg, users)[1].numel())
            ns = ops.rank_splits(ops.rank_plan_rows(rows, nnz), I, dev)  # (score_rank's plan)
            eu_sub = eu[users].contiguous()
            ex_sub = excl_all.take(users) if with_excl else None

            def rank(ns=ns):
                return ops.score_rank(eu, ei, tg, excl, users=users, n_splits=ns)

            def topk():
                return ops.score_topk(eu_sub, ei, 20, ex_sub, screen=False)

            def tch():
                return torch_ranks(users, pad, valid, ex_flat, args.chunk)

            arms = {"rank": rank, "topk": topk, "torch": tch}
            t = timed(arms)
            # exact check on the first 64 users: arm (b)'s arithmetic on the library's chain
            n64 = min(rows, 64)
            want = torch_ranks(users[:n64], pad[:n64], valid[:n64],
                               None if ex_flat is None else (ex_flat[0], ex_flat[1][:n64 + 1]),
                               n64, scores=lambda us: ops.score_dense(eu[us].contiguous(), ei))
            got = torch.full((rows, T), -1, dtype=torch.int64, device=dev)
            got[rowof, pos] = rank()[0]
            case = {"rows": rows, "per_row": per, "nnz": nnz, "excl": with_excl,
                    "kernel_rows": kr, "n_splits": ns, "arms": t,
                    "equal_torch64": bool(torch.equal(got[:n64], want))}
            med = t["rank"]["median_ms"]
            case["rank_over_topk"] = med / t["topk"]["median_ms"]
            case["rank_over_torch"] = med / t["torch"]["median_ms"]
            case["loses_to_topk"] = bool(t["rank"]["min_ms"] > t["topk"]["max_ms"])
            case["loses_to_torch"] = bool(med > t["torch"]["median_ms"])
            case["scores_per_s"] = rows * I / (med * 1e-3)
            rec["cases"].append(case)
            save()
            print("%dx%d excl=%s rows=%d n_splits=%d  " % (rows, per, with_excl, kr, ns) +
                  "  ".join("%s %.3f [%.3f, %.3f]" % (n, a["median_ms"], a["min_ms"], a["max_ms"])
                            for n, a in t.items()) +
                  "  equal %s" % case["equal_torch64"], flush=True)
            if with_excl:
                few = rows <= 64
                sweep = {"n_splits=%d" % n: (lambda n=n: rank(n))
                         for n in ((61, 122, 244, 488, 976, 1952, 3904) if few
                                   else (1, 2, 3, 4, 8, 16))}
                st = timed(sweep)
                rec["split_sweep"].append({"rows": rows, "per_row": per, "kernel_rows": kr,
                                           "planned": ns, "arms": st})
                save()
                print("   sweep " + "  ".join("%s %.3f" % (n, a["median_ms"])
                                              for n, a in st.items()), flush=True)
    rec["complete"] = True
    save()
    print("wrote", args.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
