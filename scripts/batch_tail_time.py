"""Time lg_score_topk_batch_f32 (K2b) and lg_score_topk_batch_items_f32 (K2i) of two builds of
the library against each other: --parent-lib (the parent commit's liblgcnhs.so, built in a
separate worktree) and the tree's own. Only the two C entries are timed (outputs and workspace
allocated once, no Python routing): B users of a 100,000-user table, N(0, 0.1^2) embeddings,
~100 excluded items per user; K2b B in {1, 16, 64}, K2i B in {1, 16} x candidate share in
{1.0, 0.1} (random, ascending); items in {100K, 1M} x k in {20, 100} x d in {64, 128}.

The method of profiles/rows_topk_fold.json: one child process per (library, window), parent
and new alternating, --windows windows each; a window is one HIP-event interval of about
--window-s seconds of back-to-back calls per case (reps calibrated from 20 calls). The lists of
the two libraries must be equal (sha256 of values and ids). A case passes if new / parent
median <= 1 + the parent's own spread, (max - min) / median of its windows. One JSON record ->
--out (default profiles/batch_tail_fold.json); exit status 1 if a case fails or lists differ.
Usage: python scripts/batch_tail_time.py --parent-lib PATH [--parent-commit ID]"""
import argparse
import hashlib
import json
import os
import subprocess
import sys

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(R, "light-graph-convolutional-recommendation-algorithm-based-on-hybrid-spreading_amd")
SOURCES = ("topk_batch.hip", "topk_items.hip", "batch_lists.h", "score_stream.h", "common.h")


def child(args):
    sys.path[:0] = [R, PKG]
    import torch
    from lgcnhs import _native as N
    from lgcnhs.graph import RowSets

    dev = torch.device("cuda:0")
    lib, U = N.lib(), args.table_users
    ints = lambda s: [int(x) for x in s.split(",")]
    for d in ints(args.dims):
        for I in ints(args.items):
            g = torch.Generator(device=dev).manual_seed(42)
            eu = torch.randn(U, d, device=dev, generator=g) * 0.1
            ei = torch.randn(I, d, device=dev, generator=g) * 0.1
            ku = torch.unique(torch.randint(0, U, (U * 100,), device=dev, generator=g) * I +
                              torch.randint(0, I, (U * 100,), device=dev, generator=g))
            ex = RowSets.from_pairs(ku // I, ku % I, U, I, dev)
            del ku
            cands = {}
            for share in (1.0, 0.1):
                nc = int(round(I * share))
                cands[share] = torch.sort(torch.randperm(I, device=dev, generator=g)[:nc])[0] \
                    .to(torch.int32)
            for k in ints(args.ks):
                for B in (1, 16, 64):
                    ids = torch.randint(0, U, (B,), device=dev, generator=g)
                    val = torch.empty((B, k), dtype=torch.float32, device=dev)
                    idx = torch.empty((B, k), dtype=torch.int64, device=dev)
                    for share, cand in [(None, None)] + (list(cands.items()) if B <= 16 else []):
                        if cand is None:
                            name, mid, n = "lg_score_topk_batch", (), I
                        else:
                            name, n = "lg_score_topk_batch_items", int(cand.numel())
                            mid = (N.ptr(cand), n)
                        ws_bytes = getattr(lib, name + "_ws_bytes")(B, n, d, k)
                        ws = torch.empty(max(ws_bytes, 8), dtype=torch.uint8, device=dev)
                        fn = getattr(lib, name + "_f32")
                        argv = (N.ptr(eu), N.ptr(ei), N.ptr(ids), B, U, I, *mid, d,
                                N.ptr(ex.rowptr), N.ptr(ex.col), -1024.0, k, N.ptr(val),
                                N.ptr(idx), N.ptr(ws), ws_bytes, N.stream_handle(dev))

                        def window(reps):
                            e0 = torch.cuda.Event(enable_timing=True)
                            e1 = torch.cuda.Event(enable_timing=True)
                            e0.record()
                            for _ in range(reps):
                                N.check(fn(*argv), name)
                            e1.record()
                            e1.synchronize()
                            return e0.elapsed_time(e1) / reps

                        val.fill_(0), idx.fill_(0)
                        window(5)  # warm-up, and the lists
                        h = hashlib.sha256(val.cpu().numpy().tobytes() +
                                           idx.cpu().numpy().tobytes()).hexdigest()[:16]
                        reps = max(20, int(args.window_s * 1e3 / window(20)))
                        case = "%s_B%d_I%d_k%d_d%d" % ("K2b" if cand is None else
                                                        "K2i_s%g" % share, B, I, k, d)
                        print("RECORD " + json.dumps({"case": case, "ms": window(reps),
                                                      "reps": reps, "lists": h}), flush=True)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", required=True)
    ap.add_argument("--parent-commit", default="")
    ap.add_argument("--items", default="100000,1000000")
    ap.add_argument("--ks", default="20,100")
    ap.add_argument("--dims", default="64,128")
    ap.add_argument("--table-users", type=int, default=100_000)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--window-s", type=float, default=0.15)
    ap.add_argument("--out", default=os.path.join(R, "profiles", "batch_tail_fold.json"))
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--child-timeout", type=int, default=150, help="seconds per child process")
    args = ap.parse_args()
    if args.child:
        return child(args)
    libs = {"parent": os.path.abspath(args.parent_lib),
            "new": os.path.join(PKG, "lib", "liblgcnhs.so")}
    cmd = [sys.executable, os.path.abspath(__file__), "--child"] + sys.argv[1:]
    runs = {"parent": {}, "new": {}}  # library -> case -> [records]
    for w in range(args.windows):
        for which, path in libs.items():
            # a child that fails or runs out of time ends the run: nothing more is started
            p = subprocess.run(cmd, env=dict(os.environ, LGCNHS_LIB_PATH=path), text=True,
                               stdout=subprocess.PIPE, timeout=args.child_timeout)
            if p.returncode != 0:
                print(p.stdout[-2000:])
                print("child failed:", which, "window", w, "status", p.returncode)
                return 2
            for line in p.stdout.splitlines():
                if line.startswith("RECORD "):
                    r = json.loads(line[7:])
                    runs[which].setdefault(r["case"], []).append(r)
            print("window", w, which, "done", flush=True)
    cases, ok = {}, True
    for case, pr in runs["parent"].items():
        nr = runs["new"][case]
        pm, nm = sorted(r["ms"] for r in pr), sorted(r["ms"] for r in nr)
        pmed, nmed = pm[len(pm) // 2], nm[len(nm) // 2]
        spread = (pm[-1] - pm[0]) / pmed
        c = {"parent_ms": [round(r["ms"], 6) for r in pr],
             "new_ms": [round(r["ms"], 6) for r in nr],
             "reps_per_window": [pr[0]["reps"], nr[0]["reps"]],
             "parent_median_ms": round(pmed, 6), "new_median_ms": round(nmed, 6),
             "parent_spread": round(spread, 5), "new_over_parent": round(nmed / pmed, 5),
             "within_parent_spread": bool(nmed / pmed <= 1.0 + spread),
             "lists_equal": len({r["lists"] for r in pr + nr}) == 1}
        ok = ok and c["within_parent_spread"] and c["lists_equal"]
        cases[case] = c
        print("%-32s parent %.5f new %.5f ratio %.4f spread %.4f %s" % (
            case, pmed, nmed, nmed / pmed, spread,
            "ok" if c["within_parent_spread"] and c["lists_equal"] else "FAIL"), flush=True)
    worst = max(cases, key=lambda c: cases[c]["new_over_parent"] - cases[c]["parent_spread"])
    sha = lambda f: hashlib.sha256(open(os.path.join(PKG, "csrc", f), "rb").read()).hexdigest()[:16]
    rec = {"what": __doc__.split("\n\n")[0].replace("\n", " "),
           "script": "scripts/batch_tail_time.py", "parent_commit": args.parent_commit,
           "new": {"note": "the measured sources, named by content", "sha256_16":
                   {f: sha(f) for f in SOURCES}},
           "windows": args.windows, "window_s": args.window_s, "all_pass": ok,
           "worst_case": worst, "cases": cases}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print("wrote", args.out, "all_pass", ok, "worst", worst)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
