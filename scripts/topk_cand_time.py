"""Time lg_score_topk_cand_f32 (K2c, csrc/topk_cand.hip: top-K over every row's own candidate
list) against the routes a caller has without it. Tables: 100,000 users x 1M items, N(0, 0.1^2)
embeddings, d in {64, 128}, k in {20, 100}, ~100 excluded items per user. Shapes (rows x
candidates per row): 32768 x 100 (sampled-negative evaluation), 4096 x 1000 (re-ranking),
64 x 10000, 16 x 100000. Candidates are drawn uniformly (duplicates inside a row collapse, so
the longest rows come out a few per cent short); at d = 64, k = 20 every shape is also timed
with candidates drawn from a Zipf(1.1) popularity, where the popular rows stay in cache.
The record -> --out (default profiles/topk_cand.json), rewritten after every case.

Arms (one process, alternating repeat by repeat):
  k2c    ops.score_topk_cand with max_len given (no host read), n_seg from ops.cand_segments
  loop   (A) one ops.score_topk_users(items=cand_r) call per row -- only up to 64 rows
  torch  (B) the padded route: ei[pad ids] -> [R, L, d], bmm with the users' rows, excluded
         pairs (a searchsorted into the sorted exclusion keys, built outside the timing) set to
         the mask value, padding to -inf, torch.topk
A repeat is `calls` back-to-back calls between two HIP events (time per call), calls sized so
that a repeat lasts >= 20 ms; 3 warm-up calls per arm; per arm the median and [min, max] of
--repeats repeats. Per case: `gathered_frac_hbm` = nnz x 4d bytes / k2c's median over the
8 TB/s peak (the candidate rows the kernel has to read); `n_seg`; `bits_equal_loop16` = K2c's
first 16 rows equal the loop's bit for bit; `k2c_every_repeat_beats_parent` = K2c's slowest
repeat is faster than the median of the fastest other arm.
The `min_seg_sweep` cases time K2c alone at the two few-row shapes with the segments
ops.cand_segments would plan for CAND_MIN_SEG in {128, 256, 512, 1024, 2048, 4096}.
  --shapes 32768x100,4096x1000,64x10000,16x100000  --dims 64,128  --ks 20,100  --repeats 7"""
import argparse
import json
import os
import sys

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(R, "light-graph-convolutional-recommendation-algorithm-based-on-hybrid-spreading_amd")
HBM_PEAK = 8.0e12  # bytes / s
LOOP_MAX_ROWS = 64


def stats(ms):
    s = sorted(ms)
    return {"median_ms": s[len(s) // 2], "min_ms": s[0], "max_ms": s[-1], "n": len(s)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="32768x100,4096x1000,64x10000,16x100000")
    ap.add_argument("--dims", default="64,128")
    ap.add_argument("--ks", default="20,100")
    ap.add_argument("--items", type=int, default=1_000_000)
    ap.add_argument("--table-users", type=int, default=100_000)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(R, "profiles", "topk_cand.json"))
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
    U, I = args.table_users, args.items
    ints = lambda s: [int(x) for x in s.split(",")]
    shapes = [tuple(int(x) for x in s.split("x")) for s in args.shapes.split(",")]
    rec = {"script": "scripts/topk_cand_time.py", "repeats": args.repeats,
           "warmup": args.warmup, "items": I, "table_users": U, "cus": cus,
           "cand_min_seg": ops.CAND_MIN_SEG, "complete": False, "cases": [],
           "min_seg_sweep": []}

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
    excl = RowSets.from_pairs(ku // I, ku % I, U, I, dev)
    zipf_w = (torch.arange(1, I + 1, device=dev, dtype=torch.float64) ** -1.1).float()
    zipf_perm = torch.randperm(I, device=dev, generator=g)  # popularity is not id order

    def draw(rows, per_row, dist):
        n = rows * per_row
        if dist == "uniform":
            it = torch.randint(0, I, (n,), device=dev, generator=g)
        else:
            it = torch.cat([zipf_perm[torch.multinomial(zipf_w, min(1 << 22, n - o), True,
                                                        generator=g)]
                            for o in range(0, n, 1 << 22)])
        r = torch.arange(rows, device=dev).repeat_interleave(per_row)
        return RowSets.from_pairs(r, it, rows, I, dev)

    for d in ints(args.dims):
        eu = torch.randn(U, d, device=dev, generator=g) * 0.1
        ei = torch.randn(I, d, device=dev, generator=g) * 0.1
        for rows, per_row in shapes:
            for dist in ("uniform", "zipf1.1"):
                if dist != "uniform" and not (d == 64 and 20 in ints(args.ks)):
                    continue
                cand = draw(rows, per_row, dist)
                users = torch.randperm(U, device=dev, generator=g)[:rows]
                deg = cand.degrees()
                max_len, nnz = int(deg.max()), int(cand.col.numel())
                # the padded form of arm (B), built outside the timing
                rowof = torch.arange(rows, device=dev).repeat_interleave(deg)
                pos = torch.arange(nnz, device=dev) - cand.rowptr[:-1][rowof]
                pad = torch.zeros((rows, max_len), dtype=torch.int64, device=dev)
                pad[rowof, pos] = cand.col.to(torch.int64)
                valid = torch.zeros((rows, max_len), dtype=torch.bool, device=dev)
                valid[rowof, pos] = True
                rp_host = cand.rowptr[:min(rows, LOOP_MAX_ROWS) + 1].tolist()
                for k in ints(args.ks):
                    if dist != "uniform" and not (d == 64 and k == 20):
                        continue
                    ns = ops.cand_segments(rows, max_len, k, dev)

                    def k2c(ns=ns):
                        return ops.score_topk_cand(eu, ei, cand, k, excl, users=users,
                                                   max_len=max_len, n_seg=ns)

                    def loop(n=rows):
                        rp = rp_host
                        vs = [ops.score_topk_users(eu, ei, users[r:r + 1], k, excl,
                                                   items=cand.col[rp[r]:rp[r + 1]])
                              for r in range(n)]
                        return torch.cat([v for v, _ in vs]), torch.cat([i for _, i in vs])

                    def padded():
                        s = torch.bmm(ei[pad], eu[users].unsqueeze(2)).squeeze(2)
                        key = users.unsqueeze(1) * I + pad
                        hit = torch.searchsorted(ku, key).clamp(max=ku.numel() - 1)
                        s = torch.where(ku[hit] == key, torch.full_like(s, ops.MASK_VALUE), s)
                        s = torch.where(valid, s, torch.full_like(s, float("-inf")))
                        v, j = torch.topk(s, min(k, max_len), dim=1)
                        return v, torch.gather(pad, 1, j)

                    arms = {"k2c": k2c, "torch": padded}
                    if rows <= LOOP_MAX_ROWS:
                        arms["loop"] = loop
                    t = timed(arms)
                    v, i = k2c()
                    lv, li = loop(min(rows, 16))
                    n16 = min(rows, 16)
                    case = {"d": d, "rows": rows, "per_row": per_row, "dist": dist, "k": k,
                            "nnz": nnz, "max_len": max_len, "n_seg": ns, "arms": t,
                            "bits_equal_loop16": bool(
                                torch.equal(i[:n16], li) and
                                torch.equal(v[:n16].view(torch.int32), lv.view(torch.int32)))}
                    med = t["k2c"]["median_ms"]
                    case["gathered_tb_s"] = nnz * 4 * d / (med * 1e-3) / 1e12
                    case["gathered_frac_hbm"] = case["gathered_tb_s"] * 1e12 / HBM_PEAK
                    parent = min((a for n, a in t.items() if n != "k2c"),
                                 key=lambda a: a["median_ms"])
                    case["fastest_parent"] = next(n for n, a in t.items() if a is parent)
                    case["k2c_over_parent"] = med / parent["median_ms"]
                    case["k2c_every_repeat_beats_parent"] = bool(
                        t["k2c"]["max_ms"] < parent["median_ms"])
                    rec["cases"].append(case)
                    save()
                    print("d=%d %dx%d %s k=%d n_seg=%d  " % (d, rows, per_row, dist, k, ns) +
                          "  ".join("%s %.4f [%.4f, %.4f]" % (n, a["median_ms"], a["min_ms"],
                                                              a["max_ms"])
                                    for n, a in t.items()) +
                          "  hbm %.3f  bits %s" % (case["gathered_frac_hbm"],
                                                   case["bits_equal_loop16"]), flush=True)
                    if rows <= LOOP_MAX_ROWS and dist == "uniform":
                        sweep = {}
                        for ms in (128, 256, 512, 1024, 2048, 4096):
                            n_ms = max(1, min(-(-16 * cus // rows), -(-max_len // ms), 4096))
                            sweep["min_seg=%d,n_seg=%d" % (ms, n_ms)] = \
                                (lambda n_ms=n_ms: k2c(n_ms))
                        st = timed(sweep)
                        rec["min_seg_sweep"].append({"d": d, "rows": rows, "per_row": per_row,
                                                     "k": k, "max_len": max_len, "arms": st})
                        save()
                        print("   sweep " + "  ".join("%s %.4f" % (n, a["median_ms"])
                                                      for n, a in st.items()), flush=True)
                del cand, pad, valid, rowof, pos
    rec["complete"] = True
    save()
    print("wrote", args.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
