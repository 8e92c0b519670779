"""Time lg_rows_rank_f64 (K4k, csrc/rows_rank.hip: the rank of held-out items under the spreading
/ LGCNHS scores) against the routes a caller has without it. Shape: the dense Douban shape, 600
users x 20,000 items (--interactions Zipf interactions), F = A @ HybridS(A, 0.5) prepared once,
N(0, 0.1^2) embeddings of d = 64; with and without the G factor; 1 / 10 / 100 / 1,000 targets
per user (random items, sorted and de-duplicated per user); for the first 1 / 16 / 600 users.
The record -> --out (default profiles/spread_rank.json), rewritten after every case.

Arms (one process, alternating repeat by repeat), all on the same prepared F rows, with the
users' own interactions dropped:
  rank     (a) ops.rows_rank
  topk20   (b) ops.rows_topk(k = 20): the cost of one cut-off today
  topk1024 (c) ops.rows_topk(k = 1024) and a torch membership search of every target in its
           row's list: today's route to a rank truncated at 1,024
  torch    (d) V = score_dense(eu, ei).double() * F (or F), the excluded pairs (flat indices built
           outside the timing) set to -inf, the targets gathered, then per user chunk
           ((V > t) | ((V == t) & (id < i))).sum(-1), chunks of at most 2^28 comparisons
A repeat is `calls` back-to-back calls between two HIP events (time per call), calls sized so
that a repeat lasts >= 20 ms; warm-up calls per arm first; per arm the median and [min, max] of
--repeats repeats. Per case `equal_torch64`: (a)'s ranks of the first 64 users equal (d)'s
(exact: (d) runs on the library's own dense chain scores); `rank_over_*`: ratios of medians;
`loses_to_topk20`: (a)'s fastest repeat is slower than (b)'s slowest (beyond run-to-run spread).
`growth`: per (users, G) the median of (a) at 1,000 targets per user over that at 1.
`end_to_end`: ops.spread_rank next to ops.spread_recommend(k = 20) for all 600 users, 10 and
1,000 targets per user, with W prebuilt (what remains is lg_spread_resource_f64 and the
ranking) and with W rebuilt inside the call (the default of both).
  --users 1,16,600  --per 1,10,100,1000  --repeats 7"""
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
    ap.add_argument("--n-users", type=int, default=600)
    ap.add_argument("--items", type=int, default=20_000)
    ap.add_argument("--interactions", type=int, default=60_000)
    ap.add_argument("--dim", type=int, default=64)
    ap.add_argument("--users", default="1,16,600")
    ap.add_argument("--per", default="1,10,100,1000")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(R, "profiles", "spread_rank.json"))
    args = ap.parse_args()
    sys.path[:0] = [R, PKG]
    import torch
    from lgcnhs import ops
    from lgcnhs.graph import RowSets
    from lgcnhs.synth import synth_interactions

    if not torch.cuda.is_available():
        print("no GPU: nothing is measured", file=sys.stderr)
        return 1
    dev = torch.device("cuda:0")
    U, I, d = args.n_users, args.items, args.dim
    rec = {"script": "scripts/spread_rank_time.py", "repeats": args.repeats,
           "warmup": args.warmup, "n_users": U, "items": I, "interactions": args.interactions,
           "d": d, "lam": 0.5, "row_max": ops.ROWS_RANK_ROW_MAX,
           "cus": torch.cuda.get_device_properties(dev).multi_processor_count,
           "complete": False, "cases": [], "growth": [], "end_to_end": []}

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

    pu, pi = synth_interactions(U, I, args.interactions, seed=7, dist="zipf")
    A = ops.Interactions.from_pairs(torch.as_tensor(pu), torch.as_tensor(pi), U, I, dev)
    W = ops.spread_hybrid(A, 0.5)
    F = ops.spread_resource(A, W)
    rec["zero_share_of_F"] = float((F == 0).double().mean())
    g = torch.Generator(device=dev).manual_seed(42)
    eu = torch.randn(U, d, device=dev, generator=g) * 0.1
    ei = torch.randn(I, d, device=dev, generator=g) * 0.1
    item_ids = torch.arange(I, device=dev)
    NEG = float("-inf")

    def torch_ranks(n, pad, valid, ex_flat, G):
        """Arm (d): ranks [n, T] (-1: padding or a target that does not rank)."""
        T = pad.shape[1]
        V = (G(n).double() * F[:n]) if G is not None else F[:n].clone()
        V.view(-1)[ex_flat] = NEG
        out = torch.full((n, T), -1, dtype=torch.int64, device=dev)
        chunk = max(1, min(n, (1 << 28) // (T * I)))
        for c0 in range(0, n, chunk):
            c1 = min(c0 + chunk, n)
            Vc = V[c0:c1, None, :]
            i = pad[c0:c1]
            t = V[c0:c1].gather(1, i)[:, :, None]
            b = (Vc > t) | ((Vc == t) & (item_ids[None, None, :] < i[:, :, None]))
            ok = valid[c0:c1] & (t[:, :, 0] > NEG)
            out[c0:c1] = torch.where(ok, b.sum(-1), out[c0:c1])
        return out

    def targets_of(n, per):
        it = torch.randint(0, I, (n * per,), device=dev, generator=g)
        tg = RowSets.from_pairs(torch.arange(n, device=dev).repeat_interleave(per), it, n, I,
                                dev)
        deg = tg.degrees()
        nnz, T = int(tg.col.numel()), int(deg.max())
        rowof = torch.arange(n, device=dev).repeat_interleave(deg)
        pos = torch.arange(nnz, device=dev) - tg.rowptr[:-1][rowof]
        pad = torch.zeros((n, T), dtype=torch.int64, device=dev)
        pad[rowof, pos] = tg.col.to(torch.int64)
        valid = torch.zeros((n, T), dtype=torch.bool, device=dev)
        valid[rowof, pos] = True
        return tg, rowof, pos, pad, valid

    med_a = {}
    for n in (int(x) for x in args.users.split(",")):
        Fn = F[:n]
        ex = A.by_user.slice_rows(0, n)
        exd = ex.degrees()
        ex_flat = (torch.arange(n, device=dev).repeat_interleave(exd) * I
                   + A.by_user.col[:int(ex.rowptr[-1])].to(torch.int64))
        for per in (int(x) for x in args.per.split(",")):
            tg, rowof, pos, pad, valid = targets_of(n, per)
            nnz = int(tg.col.numel())
            for use_g in (False, True):
                eu_n, ei_n = (eu[:n], ei) if use_g else (None, None)
                G = (lambda m: ops.score_dense(eu[:m].contiguous(), ei)) if use_g else None

                def rank():
                    return ops.rows_rank(Fn, tg, ex, True, eu_n, ei_n)

                def topk20():
                    return ops.rows_topk(Fn, 20, ex, True, eu_n, ei_n)

                def topk1024():
                    _, idx = ops.rows_topk(Fn, 1024, ex, True, eu_n, ei_n)
                    hit = idx[rowof] == tg.col[:, None]
                    return torch.where(hit.any(1), hit.to(torch.int8).argmax(1), -1)

                def tch():
                    return torch_ranks(n, pad, valid, ex_flat, G)

                t = timed({"rank": rank, "topk20": topk20, "topk1024": topk1024, "torch": tch})
                n64 = min(n, 64)
                m64 = int((ex.rowptr[n64] - ex.rowptr[0]))
                want = torch_ranks(n64, pad[:n64], valid[:n64], ex_flat[:m64], G)
                got = torch.full(pad.shape, -1, dtype=torch.int64, device=dev)
                got[rowof, pos] = rank()[0]
                trunc = topk1024()
                rk = rank()[0]
                case = {"users": n, "per_user": per, "nnz": nnz, "G": use_g, "arms": t,
                        "equal_torch64": bool(torch.equal(got[:n64], want)),
                        "equal_topk1024": bool(torch.equal(
                            trunc, torch.where((rk >= 0) & (rk < 1024), rk, -1)))}
                med = t["rank"]["median_ms"]
                for other in ("topk20", "topk1024", "torch"):
                    case["rank_over_" + other] = med / t[other]["median_ms"]
                case["loses_to_topk20"] = bool(t["rank"]["min_ms"] > t["topk20"]["max_ms"])
                med_a[(n, use_g, per)] = med
                rec["cases"].append(case)
                save()
                print("%d users x %d G=%s  " % (n, per, use_g) +
                      "  ".join("%s %.3f [%.3f, %.3f]" % (k, a["median_ms"], a["min_ms"],
                                                          a["max_ms"]) for k, a in t.items()) +
                      "  equal %s %s" % (case["equal_torch64"], case["equal_topk1024"]),
                      flush=True)
    pers = sorted({p for (_, _, p) in med_a})
    for (n, use_g, p) in sorted(med_a):
        if p == pers[-1] and (n, use_g, pers[0]) in med_a:
            rec["growth"].append({"users": n, "G": use_g, "per_lo": pers[0], "per_hi": p,
                                  "rank_hi_over_lo": med_a[(n, use_g, p)] /
                                  med_a[(n, use_g, pers[0])]})
    save()

    for per in (10, 1000):
        tg = targets_of(U, per)[0]
        for use_g in (False, True):
            e_u, e_i = (eu, ei) if use_g else (None, None)
            t = timed({
                "spread_rank_W": lambda: ops.spread_rank(A, 0.5, tg, A.by_user, True, e_u, e_i,
                                                         W=W),
                "spread_recommend20_W": lambda: ops.spread_recommend(A, 0.5, 20, A.by_user, True,
                                                                     e_u, e_i, W=W),
                "resource_only": lambda: ops.spread_resource(A, W),
                "spread_rank": lambda: ops.spread_rank(A, 0.5, tg, A.by_user, True, e_u, e_i,
                                                       tiled=False),
                "spread_recommend20": lambda: ops.spread_recommend(A, 0.5, 20, A.by_user, True,
                                                                   e_u, e_i, tiled=False)})
            rec["end_to_end"].append({"users": U, "per_user": per, "G": use_g, "arms": t})
            save()
            print("end to end x %d G=%s  " % (per, use_g) +
                  "  ".join("%s %.3f" % (k, a["median_ms"]) for k, a in t.items()), flush=True)
    rec["complete"] = True
    save()
    print("wrote", args.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
