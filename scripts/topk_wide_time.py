"""Time lg_score_topk_wide_f32 (K2w, 128 < k <= 1024) on the bench's top-K shape: 32,768 users
x 1M items, N(0, 0.1^2) embeddings, 100 excluded items per user; d = 64 at k in {129, 256,
512, 1024} and d = 128 at k = 256. One JSON record -> --out (default profiles/topk_wide.json).

Per case one child process (this driver never opens the GPU), HIP events, a warm-up, the
median and range over --reps repeats with the kernels alternating:
  wide   ops.score_topk(k)                       the new kernel
  A      ops.score_topk(128, screen=False)       the same MFMA stream with the smallest lists
  B      torch.matmul + -1024 index_put + torch.topk in 2,048-user blocks over 8,192 users,
         scaled to the user count: what a caller does today
and, on B's 8,192 users, tests/_compare.py::compare_topk_sets counts of the wide lists against
B's (identical / tie-affected / mismatched). k = 1024 also times the user-chunked path
(WIDE_WS_CAP_BYTES lowered to a quarter of the slabs). A measurement build of the library
(-DLG_TOPK_COUNT, selected with LGCNHS_LIB_PATH) adds insertions and compactions per user.
  --cases 64:129,64:256,...   --users 32768   --items 1000000   --reps 7   --no-b"""
import argparse
import json
import os
import subprocess
import sys

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(R, "light-graph-convolutional-recommendation-algorithm-based-on-hybrid-spreading_amd")
PEAK_F32_MFMA = 157.3e12  # MI355X fp32 matrix peak, FLOP/s


def stats(ms):
    s = sorted(ms)
    return {"median_ms": s[len(s) // 2], "min_ms": s[0], "max_ms": s[-1], "n": len(s)}


def child(args, d, k):
    sys.path[:0] = [R, PKG, os.path.join(R, "tests")]
    import ctypes
    import numpy as np
    import torch
    from _compare import compare_topk_sets
    from lgcnhs import _native as N
    from lgcnhs import ops
    from lgcnhs.graph import RowSets

    dev = torch.device("cuda:0")
    U, I = args.users, args.items
    g = torch.Generator(device=dev).manual_seed(42)
    eu = torch.randn(U, d, device=dev, generator=g) * 0.1
    ei = torch.randn(I, d, device=dev, generator=g) * 0.1
    ku = torch.unique(torch.randint(0, U, (U * 100,), device=dev, generator=g) * I +
                      torch.randint(0, I, (U * 100,), device=dev, generator=g))
    excl = RowSets.from_pairs(ku // I, ku % I, U, I, dev)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), out

    def wide():
        return ops.score_topk(eu, ei, k, excl)

    def plain128():
        return ops.score_topk(eu, ei, 128, excl, screen=False)

    counts = getattr(N.lib(), "lg_topk_wide_counts", None)  # (-DLG_TOPK_COUNT builds)
    buf = (ctypes.c_ulonglong * 4)()
    if counts is not None:
        counts.argtypes, counts.restype = [ctypes.c_void_p], ctypes.c_int
    blk, ns = ops._wide_plan(U, I, d, k, ops._wide_resident_blocks(dev, k, d),
                             ops.WIDE_WS_CAP_BYTES)
    rec = {"d": d, "k": k, "users": U, "items": I, "n_splits": ns, "user_block": blk}
    wide(), plain128()  # warm-up (allocator, code objects)
    torch.cuda.synchronize()
    if counts is not None:
        counts(buf)
        wide()
        counts(buf)
        rec["counts_per_user"] = {"inserted": buf[0] / U, "compactions": buf[1] / U,
                                  "users_finished": buf[2] / U}
    tw, ta = [], []
    for _ in range(args.reps):
        t, (v, i) = timed(wide)
        tw.append(t)
        t, (va, ia) = timed(plain128)
        ta.append(t)
    rec["wide"], rec["A_plain_k128"] = stats(tw), stats(ta)
    rec["wide_over_A"] = rec["wide"]["median_ms"] / rec["A_plain_k128"]["median_ms"]
    rec["mfma_fraction"] = 2.0 * U * I * d / (rec["wide"]["median_ms"] * 1e-3) / PEAK_F32_MFMA
    rec["prefix_128_equals_A"] = bool(torch.equal(i[:, :128], ia) and torch.equal(
        v[:, :128].view(torch.int32), va.view(torch.int32)))
    if args.chunked and k == 1024:
        full = N.lib().lg_score_topk_wide_ws_bytes(U, I, d, k, rec["n_splits"])
        keep = ops.WIDE_WS_CAP_BYTES
        rec["unchunked_ws_bytes"], rec["wide_chunked"] = full, []
        for div in (2, 4):  # the slabs of half and of a quarter of the users
            ops.WIDE_WS_CAP_BYTES = max(full // div, 1)
            blk, ns = ops._wide_plan(U, I, d, k, ops._wide_resident_blocks(dev, k, d),
                                     ops.WIDE_WS_CAP_BYTES)
            wide()
            tc = []
            for _ in range(args.reps):
                t, (vc, ic) = timed(wide)
                tc.append(t)
            rec["wide_chunked"].append(dict(
                stats(tc), cap_bytes=ops.WIDE_WS_CAP_BYTES, user_block=blk, n_splits=ns,
                equals_unchunked=bool(torch.equal(ic, i) and torch.equal(
                    vc.view(torch.int32), v.view(torch.int32)))))
        ops.WIDE_WS_CAP_BYTES = keep
    if not args.no_b:
        UB, BLK = min(8192, U), 2048
        rows = torch.repeat_interleave(torch.arange(U, device=dev), excl.degrees())
        cols = excl.col.to(torch.int64)

        def b_pass(kk):
            outs = []
            for u0 in range(0, UB, BLK):
                u1 = min(UB, u0 + BLK)
                score = torch.matmul(eu[u0:u1], ei.T)
                m = (rows >= u0) & (rows < u1)
                score[rows[m] - u0, cols[m]] = -(1 << 10)
                outs.append(torch.topk(score, kk))
                del score
            return outs
        ref = b_pass(k + 1)  # (untimed; warm-up) the lists and the (v_k, v_k+1) gaps
        rv = torch.cat([o[0] for o in ref]).cpu().numpy()
        ri = torch.cat([o[1] for o in ref]).cpu().numpy()
        del ref
        tb = []
        for _ in range(args.reps):
            t, _ = timed(lambda: b_pass(k))
            tb.append(t * (U / UB))
        rec["B_torch_blocks"] = stats(tb)
        rec["B_over_wide"] = rec["B_torch_blocks"]["median_ms"] / rec["wide"]["median_ms"]
        got, gv = i[:UB].cpu().numpy(), v[:UB].cpu().numpy()
        tol = args.tol
        identical = int(sum(set(got[u].tolist()) == set(ri[u, :k].tolist()) for u in range(UB)))
        try:
            ties = compare_topk_sets(got, ri[:, :k], rv[:, k - 1:k + 1], tol=tol,
                                     max_tie_frac=1.0, got_vals=gv)
            mismatched = UB - identical - ties
        except AssertionError as e:
            ties, mismatched = None, str(e)[:300]
        rec["vs_B"] = {"users": UB, "identical": identical, "tie_affected": ties,
                       "mismatched": mismatched, "tol": tol}
    print("RECORD " + json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="64:129,64:256,64:512,64:1024,128:256")
    ap.add_argument("--users", type=int, default=32768)
    ap.add_argument("--items", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--tol", type=float, default=2e-6,
                    help="|v_k - v_k+1| of B at or below this: a tie-affected user")
    ap.add_argument("--no-b", action="store_true")
    ap.add_argument("--no-chunked", dest="chunked", action="store_false")
    ap.add_argument("--out", default=os.path.join(R, "profiles", "topk_wide.json"))
    ap.add_argument("--child", default=None)
    ap.add_argument("--timeout", type=int, default=280, help="seconds per case")
    args = ap.parse_args()
    if args.child:
        d, k = (int(x) for x in args.child.split(":"))
        return child(args, d, k)
    cases = []
    for case in args.cases.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", case] + \
            [a for a in sys.argv[1:] if not a.startswith("--child")]
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=args.timeout)
        sys.stdout.write(p.stdout)
        if p.returncode != 0:  # a failed case ends the run: nothing more starts on the GPU
            sys.stderr.write(p.stderr[-3000:])
            return p.returncode
        cases += [json.loads(l[7:]) for l in p.stdout.splitlines() if l.startswith("RECORD ")]
    rec = {"script": "scripts/topk_wide_time.py", "peak_f32_mfma_tflops": PEAK_F32_MFMA / 1e12,
           "reps": args.reps, "cases": cases}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print("wrote", args.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
