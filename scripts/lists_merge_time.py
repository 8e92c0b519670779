"""Time lg_topk_lists_merge_f64 and lg_topk_lists_merge_wide_f64 of two builds of the library
against each other: --parent-lib (the parent commit's liblgcnhs.so, built in a separate
worktree) and the tree's own. Only the two C entries are timed (inputs and outputs allocated
once, no Python routing): L = 8 sorted lists of 131072 rows, uniform random fp64 values,
distinct ids; k in {20, 64, 100, 128} for the first entry, {129, 1024} for the wide one.

The method of scripts/batch_tail_time.py: one child process per (library, window), parent
and new alternating, --windows windows each; a window is one HIP-event interval of about
--window-s seconds of back-to-back calls per case (reps calibrated from 20 calls). The lists of
the two libraries must be equal (sha256 of values and ids). A case passes if new / parent
median <= 1 + the parent's own spread, (max - min) / median of its windows. One JSON record ->
--out (default profiles/lists_merge_fold.json); exit status 1 if a case fails or lists differ.
Usage: python scripts/lists_merge_time.py --parent-lib PATH [--parent-commit ID]"""
import argparse
import hashlib
import json
import os
import subprocess
import sys

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(R, "light-graph-convolutional-recommendation-algorithm-based-on-hybrid-spreading_amd")
SOURCES = ("rows_topk.hip", "wave_list.h", "common.h")


def child(args):
    sys.path[:0] = [R, PKG]
    import torch
    from lgcnhs import _native as N

    dev = torch.device("cuda:0")
    lib, L, n = N.lib(), args.lists, args.rows
    for k in [int(x) for x in args.ks.split(",")]:
        g = torch.Generator(device=dev).manual_seed(42 + k)
        val = torch.rand((L, n, k), dtype=torch.float64, device=dev, generator=g)
        val = torch.sort(val, dim=-1, descending=True)[0].contiguous()
        # list l holds the ids l k .. l k + k - 1 in every row: distinct over a row's lists
        idx = (torch.arange(L, device=dev).view(L, 1, 1) * k +
               torch.arange(k, device=dev).view(1, 1, k)).expand(L, n, k).contiguous()
        ov = torch.empty((n, k), dtype=torch.float64, device=dev)
        oi = torch.empty((n, k), dtype=torch.int64, device=dev)
        name = "lg_topk_lists_merge_f64" if k <= 128 else "lg_topk_lists_merge_wide_f64"
        fn = getattr(lib, name)
        argv = (N.ptr(val), N.ptr(idx), L, n, k, N.ptr(ov), N.ptr(oi), N.stream_handle(dev))

        def window(reps):
            e0 = torch.cuda.Event(enable_timing=True)
            e1 = torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                N.check(fn(*argv), name)
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1) / reps

        ov.fill_(0), oi.fill_(0)
        window(5)  # warm-up, and the lists
        h = hashlib.sha256(ov.cpu().numpy().tobytes() + oi.cpu().numpy().tobytes()).hexdigest()[:16]
        reps = max(20, int(args.window_s * 1e3 / window(20)))
        print("RECORD " + json.dumps({"case": "%s_L%d_n%d_k%d" % (name[8:-4], L, n, k),
                                      "ms": window(reps), "reps": reps, "lists": h}), flush=True)
        del val, idx, ov, oi
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", required=True)
    ap.add_argument("--parent-commit", default="")
    ap.add_argument("--ks", default="20,64,100,128,129,1024")
    ap.add_argument("--lists", type=int, default=8)
    ap.add_argument("--rows", type=int, default=131072)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--window-s", type=float, default=0.15)
    ap.add_argument("--out", default=os.path.join(R, "profiles", "lists_merge_fold.json"))
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
        print("%-36s parent %.5f new %.5f ratio %.4f spread %.4f %s" % (
            case, pmed, nmed, nmed / pmed, spread,
            "ok" if c["within_parent_spread"] and c["lists_equal"] else "FAIL"), flush=True)
    worst = max(cases, key=lambda c: cases[c]["new_over_parent"] - cases[c]["parent_spread"])
    sha = lambda f: hashlib.sha256(open(os.path.join(PKG, "csrc", f), "rb").read()).hexdigest()[:16]
    rec = {"what": __doc__.split("\n\n")[0].replace("\n", " "),
           "script": "scripts/lists_merge_time.py", "parent_commit": args.parent_commit,
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
