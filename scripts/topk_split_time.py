"""Time lg_score_topk_screened_f32 at d = 128, 32 < k <= 64 -- the main pass
k_topk_ring<128, 2, 8, 2, 32, 13, 7, 1, false, true>, the one kernel whose code hipcc emitted
differently once topk.hip held the ring alone (profiles/topk_split_asm.txt) -- of two builds of
the library against each other: --parent-lib (the parent commit's liblgcnhs.so, built in a
separate worktree) and the tree's own. Only the C entry is timed (bf16 operands, margins,
outputs and workspace prepared once; the splits ops.score_topk would take): N(0, 0.1^2)
embeddings, ~100 excluded items per user (the differing instructions are in the exclusion
search), users x items in {32768 x 1M, 4096 x 200K}, k in {33, 50, 64}.

The method of scripts/batch_tail_time.py: one child process per (library, window), parent and
new alternating, --windows windows each; a window is one HIP-event interval of about --window-s
seconds of back-to-back calls per case (reps calibrated from 5 calls). The lists of the two
libraries must be equal (sha256 of values and ids). A case passes if new / parent median <=
1 + the parent's own spread, (max - min) / median of its windows. One JSON record -> --out
(default profiles/topk_split_time.json); exit status 1 if a case fails or lists differ.
Usage: python scripts/topk_split_time.py --parent-lib PATH [--parent-commit ID]"""
import argparse
import hashlib
import json
import os
import subprocess
import sys

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(R, "light-graph-convolutional-recommendation-algorithm-based-on-hybrid-spreading_amd")
SOURCES = ("topk.hip", "topk_plain.hip", "score_stream.h", "common.h")
SHAPES = ((32768, 1_000_000), (4096, 200_000))
KS = (33, 50, 64)
D = 128


def child(args):
    sys.path[:0] = [R, PKG]
    import torch
    from lgcnhs import _native as N
    from lgcnhs import ops
    from lgcnhs.graph import RowSets

    dev = torch.device("cuda:0")
    lib = N.lib()
    for U, I in SHAPES:
        g = torch.Generator(device=dev).manual_seed(42)
        eu = torch.randn(U, D, device=dev, generator=g) * 0.1
        ei = torch.randn(I, D, device=dev, generator=g) * 0.1
        ku = torch.unique(torch.randint(0, U, (U * 100,), device=dev, generator=g) * I +
                          torch.randint(0, I, (U * 100,), device=dev, generator=g))
        ex = RowSets.from_pairs(ku // I, ku % I, U, I, dev)
        del ku
        ub, un, ue = ops.bound_operands(eu, with_err=True)
        ib, inorm, ierr = ops.bound_operands(ei, with_err=True)
        umarg = ops.screen_margins(un, ue, inorm, ierr, D)
        for k in KS:
            ns = ops._splits_for(U, I, k, ops._resident_blocks(dev, k, True), True, D)
            ws_bytes = lib.lg_score_topk_screened_ws_bytes(U, I, D, k, ns)
            ws = torch.empty(max(ws_bytes, 8), dtype=torch.uint8, device=dev)
            val = torch.zeros((U, k), dtype=torch.float32, device=dev)
            idx = torch.zeros((U, k), dtype=torch.int64, device=dev)
            argv = (N.ptr(eu), N.ptr(ei), N.ptr(ub), N.ptr(ib), N.ptr(umarg), U, I, D,
                    N.ptr(ex.rowptr), N.ptr(ex.col), -1024.0, k, ns, N.ptr(val), N.ptr(idx),
                    N.ptr(ws), ws_bytes, N.stream_handle(dev))

            def window(reps):
                e0 = torch.cuda.Event(enable_timing=True)
                e1 = torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(reps):
                    N.check(lib.lg_score_topk_screened_f32(*argv), "lg_score_topk_screened_f32")
                e1.record()
                e1.synchronize()
                return e0.elapsed_time(e1) / reps

            window(3)  # warm-up, and the lists
            h = hashlib.sha256(val.cpu().numpy().tobytes() +
                               idx.cpu().numpy().tobytes()).hexdigest()[:16]
            reps = max(5, int(args.window_s * 1e3 / window(5)))
            print("RECORD " + json.dumps({"case": "U%d_I%d_k%d_d%d_ns%d" % (U, I, k, D, ns),
                                          "ms": window(reps), "reps": reps, "lists": h}),
                  flush=True)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", required=True)
    ap.add_argument("--parent-commit", default="")
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--window-s", type=float, default=0.3)
    ap.add_argument("--out", default=os.path.join(R, "profiles", "topk_split_time.json"))
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--child-timeout", type=int, default=120, help="seconds per child process")
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
    sha = lambda f: hashlib.sha256(open(os.path.join(PKG, "csrc", f), "rb").read()).hexdigest()[:16]
    rec = {"what": __doc__.split("\n\n")[0].replace("\n", " "),
           "script": "scripts/topk_split_time.py", "parent_commit": args.parent_commit,
           "new": {"note": "the measured sources, named by content", "sha256_16":
                   {f: sha(f) for f in SOURCES}},
           "windows": args.windows, "window_s": args.window_s, "all_pass": ok, "cases": cases}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print("wrote", args.out, "all_pass", ok)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
