"""One C5 layer (FIRST mode, with the next operand written) of lg_spmm_layer_f16 across builds
of csrc/spmm.hip with different numbers of gathered loads in flight, beside the product build
and lg_spmm_layer_f32 on the widened operand; the builds alternate, HIP events, median / min /
max ms over 8 repeats per d in {64, 128}. Prints one JSON line
(profiles/half_storage_unroll.json).

The measurement builds are lib/ab/liblgcnhs_u<A>_<B>.so, made with
  scripts/build_flags.sh u<A>_<B> "-DLG_F16_UNROLL_64=<A> -DLG_F16_UNROLL_HI=<B>" spmm
(A: loads in flight at d = 64, B: at d >= 128)."""
import ctypes, glob, json, os, statistics, sys
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))  # scripts/..
PKG = os.path.join(REPO, "light-graph-convolutional-recommendation-algorithm-based-on-hybrid-spreading_amd")
sys.path[:0] = [REPO, PKG]
import torch
from lgcnhs import _native as N
from lgcnhs.graph import Adjacency
from lgcnhs.synth import synth_graph_device
dev = torch.device("cuda:0")
U = I = 1_000_000
rowptr, src, keys = synth_graph_device(U, I, 100_000_000, 3, dev)
del keys
adj = Adjacency(rowptr, src, U + I, n_users=U, symmetric=True)
dis, w = adj.dis(), adj.edge_weight()
libs = {"product": N.lib()}
for p in sorted(glob.glob(os.path.join(PKG, "lib", "ab", "liblgcnhs_u*.so"))):
    l = ctypes.CDLL(p)
    for name in ("lg_spmm_layer_f16", "lg_spmm_layer_f32"):
        f = getattr(l, name); f.restype, f.argtypes = N.SIGNATURES[name]
    libs[os.path.basename(p)[10:-3]] = l  # "u<A>_<B>"
n = U + I
strm = N.stream_handle(dev)
res = {"what": "one C5 layer (1M x 1M users x items, 200M nnz, FIRST mode, next operand written): "
               "ms [median, min, max] of 8 alternating repeats; fp16 builds keyed by gathered "
               "loads in flight per lane group", "source": "scripts/half_storage_unroll.py"}
for d in (64, 128):
    x0 = torch.randn(n, d, device=dev) * 0.1
    xh = x0.to(torch.float16); yh = torch.empty_like(xh)
    x32 = xh.float(); y32 = torch.empty_like(x32); acc = torch.empty_like(x0)
    def call(lib, half):
        fn = lib.lg_spmm_layer_f16 if half else lib.lg_spmm_layer_f32
        x, y = (xh, yh) if half else (x32, y32)
        st = fn(N.ptr(adj.rowptr), N.ptr(adj.src), N.ptr(dis), N.ptr(w), N.ptr(x), N.ptr(y), N.ptr(x0),
                N.ptr(acc), None, n, 0, d, N.LG_ACC_FIRST, 4.0, 0, strm)
        assert st == 0, st
    def key(k):  # the build's loads in flight at this d
        return "fp16_product" if k == "product" else "fp16_unroll_" + k[1:].split("_")[d > 64]
    runs = [("lg_spmm_layer_f32", libs["product"], False)] + [(key(k), l, True)
                                                              for k, l in libs.items()]
    for _, l, h in runs:
        call(l, h); call(l, h)
    torch.cuda.synchronize()
    ms = {k: [] for k, _, _ in runs}
    for _ in range(8):
        for k, l, h in runs:
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record(); call(l, h); e.record(); e.synchronize()
            ms[k].append(s.elapsed_time(e))
    res[f"d{d}"] = {k: [round(statistics.median(v), 3), round(min(v), 3), round(max(v), 3)] for k, v in ms.items()}
    print(d, res[f"d{d}"], file=sys.stderr, flush=True)
print(json.dumps(res))
