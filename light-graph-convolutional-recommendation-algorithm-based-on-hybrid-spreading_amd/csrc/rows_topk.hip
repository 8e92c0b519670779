// K4: top-K over dense fp64 rows (the spreading / LGCNHS recommendation) and the merge of
// top-K lists (lg_topk_lists_merge_f64, k <= 128; _wide_f64, k <= 1024), gfx950.
//
// Reference: model/SpreadMethod/recommend.py:31-50 and model/SpreadLightGCN/recommend.py: per
// user argsort(F[u])[::-1], drop train|val items, [:k] -- any RECOMMEND["k"] -- with
// F = G * F for LGCNHS (model/SpreadLightGCN/model.py:151, fp32 G promoted to fp64). Here:
// the candidate-list selection of common.h, 64 columns per step, admission v > tau, an
// exclusion cursor over the row's sorted exclusions, order (value desc, column asc), output
// padded with {-inf, -1}.
//
// One kernel text, two candidate lists (wave_list.h):
//   lg_rows_topk_f64       k <= 64 / 128:        RegList<2> / <4>, sorted in registers
//   lg_rows_topk_wide_f64  k <= 256 / 512 / 1024: LdsList<256> / <512> / <1024>, two halves in
//                          LDS (it serves k <= 128 too, bit for bit the first entry's lists)
// LDS per wave = 12 CAP bytes: 1.5 / 3 KiB for the register-sorted lists, 6 / 12 / 24 KiB for
// the LDS ones. Rows of >= kSplitCols columns get 8 waves each (register-sorted lists) or
// 8 / 4 / 2 (LDS lists: 48 KiB per block in every class, three blocks per CU of 160 KiB),
// shorter rows one wave.
#include "common.h"
#include "wave_list.h"

namespace lg {

// fp32 score in the chain order of lg_score_topk_f32 (see topk_plain.hip header).
template <int D>
__device__ __forceinline__ float chain_score(const float *__restrict__ us,
                                             const float *__restrict__ it) {
  constexpr int Q = D / 4;
  float r[D];
  const float4 *p4 = reinterpret_cast<const float4 *>(it);
#pragma unroll
  for (int t = 0; t < D / 4; ++t) {
    const float4 q = p4[t];
    r[4 * t] = q.x;
    r[4 * t + 1] = q.y;
    r[4 * t + 2] = q.z;
    r[4 * t + 3] = q.w;
  }
  float acc = 0.f;
#pragma unroll
  for (int s = 0; s < Q; ++s)
#pragma unroll
    for (int g = 0; g < 4; ++g) acc = __builtin_fmaf(us[g * Q + s], r[g * Q + s], acc);
  return acc;
}

// NW waves per row (one row per block), D == 0: no G factor. Wave w scans the row's w-th
// column range (whole 64-column steps) in ascending order into its own candidate list --
// at the C3 Douban shape (600 rows x 20,000 columns) one wave per row left the chip mostly
// idle behind each step's load -> 64-FMA chain latency -- then the waves' top-k lists merge
// pairwise in log2(NW) rounds (each merge: the partner's <= k entries appended, the list
// compacted; the (value desc, column asc) order is total, so the result is the single
// scan's). Columns arrive in ascending order within a wave, so a tie with tau loses.
template <typename List, int D, int NW>
__global__ __launch_bounds__(64 * NW) void k_rows_topk(
    const double *__restrict__ F, int64_t ldf, int64_t n_rows, int64_t n_cols,
    const float *__restrict__ eu, const float *__restrict__ ei,
    const int64_t *__restrict__ ex_rowptr, const int32_t *__restrict__ ex_col, int excl_mode,
    int k, double *__restrict__ out_val, int64_t *__restrict__ out_idx) {
  constexpr int CAP = List::CAP;
  constexpr int DU = D > 0 ? D : 1;
  static_assert((NW & (NW - 1)) == 0, "the waves' lists merge pairwise");
  __shared__ double cs[NW][CAP];
  __shared__ int ci[NW][CAP];
  __shared__ float us[DU];
  __shared__ int s_n[NW];
  const int wave = threadIdx.x / 64;
  const int lane = lane_id();
  const int64_t r = blockIdx.x;  // (< n_rows: one block per row)
  if (D > 0) {
    for (int t = threadIdx.x; t < D; t += 64 * NW) us[t] = eu[r * D + t];
    __syncthreads();
  }
  int64_t lo = 0, hi = 0;
  if (ex_rowptr && excl_mode == LG_EXCL_DROP) {
    lo = ex_rowptr[r];
    hi = ex_rowptr[r + 1];
  }
  const int64_t span = ((n_cols + NW - 1) / NW + 63) / 64 * 64;
  const int64_t c0 = wave * span, c1 = c0 + span < n_cols ? c0 + span : n_cols;
  List list;
  double tau = neg_inf<double>();
  int tau_id = kPadId;
  if constexpr (List::kPadded) list.init(cs[wave], ci[wave]);
  const double *row = F + r * ldf;
  // no G: two 64-column steps per round (both loads in flight; the candidates of the first
  // step are taken before the second's, so columns still reach the list in ascending order):
  // 0.141 -> 0.119 ms at the C3 shape. With G one step: two interleaved score chains measured
  // slower (0.52 -> 0.59 ms: 186 instead of 125 VGPRs, half the waves per SIMD)
  constexpr int STEPS = D > 0 ? 1 : 2;
  for (int64_t j00 = c0; j00 < c1; j00 += 64 * STEPS) {
    double v2[STEPS];
#pragma unroll
    for (int h = 0; h < STEPS; ++h) {
      const int64_t j = j00 + 64 * h + lane;
      v2[h] = j < c1 ? row[j] : neg_inf<double>();
    }
    if constexpr (D > 0) {
      if (j00 + lane < c1) v2[0] = (double)chain_score<DU>(us, ei + (j00 + lane) * D) * v2[0];
    }
#pragma unroll
    for (int h = 0; h < STEPS; ++h) {
      const int64_t j0 = j00 + 64 * h;
      if (j0 >= c1) break;  // (wave-uniform)
      const int64_t j = j0 + lane;
      const bool valid = j < c1;
      const double v = v2[h];
      bool cand = valid && v > tau;
      if (__ballot(cand)) {
        if (cand && lo < hi) {
          const int64_t p = lower_bound_i32(ex_col, lo, hi, (int32_t)j);
          lo = p;
          if (p < hi && ex_col[p] == (int32_t)j) cand = false;
        }
        const uint64_t bal = __ballot(cand);
        const int pos = list.slot(__popcll(bal & lanemask_lt()));
        if (cand) {
          cs[wave][pos] = v;
          ci[wave][pos] = (int)j;
        }
        list.add(__popcll(bal));
        if (list.full()) {
          wave_sync();
          list.compact(cs[wave], ci[wave], k, tau, tau_id);
        }
      }
    }
  }
  wave_sync();
  int nc = list.compact(cs[wave], ci[wave], k, tau, tau_id);
  if (lane == 0) s_n[wave] = nc;
#pragma unroll
  for (int st = 1; st < NW; st <<= 1) {
    __syncthreads();
    if (wave % (2 * st) == 0) {  // (wave + st < NW: NW is a power of two)
      nc = list.append(cs[wave], ci[wave], cs[wave + st], ci[wave + st], s_n[wave + st], k,
                       tau, tau_id);
      if (lane == 0) s_n[wave] = nc;
    }
  }
  if (wave == 0) {
    for (int e = lane; e < k; e += 64) {
      out_val[r * k + e] = e < nc ? cs[0][e] : neg_inf<double>();
      out_idx[r * k + e] = e < nc ? ci[0][e] : -1;
    }
  }
}

// rows of at least this many columns get several waves each, shorter ones one
constexpr int64_t kSplitCols = 4096;

// what both rows entries take
struct RowsArgs {
  const double *F;
  int64_t ldf, n_rows, n_cols;
  const float *eu, *ei;
  int dim;
  const int64_t *ex_rowptr;
  const int32_t *ex_col;
  int excl_mode, k;
  double *out_val;
  int64_t *out_idx;
  hipStream_t s;
};

template <typename List, int NW>
static void launch_rows_topk_nw(const RowsArgs &a) {
  auto kern = k_rows_topk<List, 0, NW>;
  switch (a.eu ? a.dim : 0) {
    case 0: break;
    case 32: kern = k_rows_topk<List, 32, NW>; break;
    case 64: kern = k_rows_topk<List, 64, NW>; break;
    default: kern = k_rows_topk<List, 128, NW>; break;
  }
  kern<<<dim3((unsigned)a.n_rows), dim3(64 * NW), 0, a.s>>>(
      a.F, a.ldf, a.n_rows, a.n_cols, a.eu, a.ei, a.ex_rowptr, a.ex_col, a.excl_mode, a.k,
      a.out_val, a.out_idx);
}

// NW waves per long row
template <typename List, int NW>
static void launch_rows_topk(const RowsArgs &a) {
  if (a.n_cols >= kSplitCols) launch_rows_topk_nw<List, NW>(a);
  else launch_rows_topk_nw<List, 1>(a);
}

// the checks of both rows entries: `who` is the entry's name, k in [1, kmax]
static int check_rows_args(const char *who, int kmax, const RowsArgs &a) {
  LG_REQUIRE(a.F && a.out_val && a.out_idx && a.n_rows >= 0 && a.n_cols >= 0 &&
                 a.ldf >= a.n_cols && a.n_cols < 0x7fffffff,
             "%s: bad arguments", who);
  LG_REQUIRE(a.k >= 1 && a.k <= kmax, "%s: k=%d not in [1,%d]", who, a.k, kmax);
  LG_REQUIRE(!a.eu == !a.ei, "%s: eu/ei must both be set or both NULL", who);
  LG_REQUIRE(!a.eu || a.dim == 32 || a.dim == 64 || a.dim == 128,
             "%s: dim %d not in {32,64,128}", who, a.dim);
  LG_REQUIRE(a.excl_mode == LG_EXCL_DROP || a.excl_mode == LG_EXCL_NONE,
             "%s: bad excl_mode %d", who, a.excl_mode);
  LG_REQUIRE(!a.ex_rowptr == !a.ex_col, "%s: ex_rowptr/ex_col must both be set", who);
  LG_REQUIRE(!(a.eu && a.excl_mode == LG_EXCL_NONE && a.ex_rowptr),
             "%s: a G factor with exclusions requires LG_EXCL_DROP", who);
  return LG_OK;
}

// Merge n_lists sorted top-K lists per row ([n_lists][n_rows][k], index -1 = empty) into one
// ([n_rows][k]): the item-range shards of a multi-GPU spreading run. One wave per row, the
// candidate list in LDS (CAP = 64*M >= k + 64), compacted by the wave-wide bitonic sort.
// (A twin of k_lists_merge_wide below: as one k_lists_merge<List, NWB> this one compiled to
// another instruction order, k = 64 slower than the parent's spread: DESIGN.md.)
template <int M>
__global__ __launch_bounds__(256) void k_lists_merge_f64(const double *__restrict__ in_val,
                                                         const int64_t *__restrict__ in_idx,
                                                         int n_lists, int64_t n_rows, int k,
                                                         double *__restrict__ out_val,
                                                         int64_t *__restrict__ out_idx) {
  constexpr int CAP = 64 * M;
  __shared__ double cs[4][CAP];
  __shared__ int ci[4][CAP];
  const int wave = threadIdx.x / 64;
  const int lane = lane_id();
  const int64_t row = (int64_t)blockIdx.x * 4 + wave;
  if (row >= n_rows) return;
  int cnt = 0;
  double tau = neg_inf<double>();
  int tau_id = kPadId;
  for (int s = 0; s < n_lists; ++s) {
    const int64_t base = ((int64_t)s * n_rows + row) * k;
    for (int e0 = 0; e0 < k; e0 += 64) {
      const int e = e0 + lane;
      double v = neg_inf<double>();
      int id = -1;
      if (e < k) {
        const int64_t x = in_idx[base + e];
        if (x >= 0) {
          v = in_val[base + e];
          id = (int)x;
        }
      }
      const bool cand = id >= 0 && before(v, id, tau, tau_id);
      const uint64_t bal = __ballot(cand);
      const int pos = cnt + __popcll(bal & lanemask_lt());
      if (cand) {
        cs[wave][pos] = v;
        ci[wave][pos] = id;
      }
      cnt += __popcll(bal);
      if (cnt > CAP - 64) {
        wave_sync();
        cnt = wave_compact<double, M>(cs[wave], ci[wave], cnt, k, tau, tau_id);
      }
    }
  }
  wave_sync();
  const int nc = wave_compact<double, M>(cs[wave], ci[wave], cnt, k, tau, tau_id);
  for (int e = lane; e < k; e += 64) {
    out_val[row * k + e] = e < nc ? cs[wave][e] : neg_inf<double>();
    out_idx[row * k + e] = e < nc ? ci[wave][e] : -1;
  }
}

// k_lists_merge_f64 with the list (k <= CAP / 2) in LDS: one wave per row, NWB rows per
// block.
template <int CAP, int NWB>
__global__ __launch_bounds__(64 * NWB) void k_lists_merge_wide(
    const double *__restrict__ in_val, const int64_t *__restrict__ in_idx, int n_lists,
    int64_t n_rows, int k, double *__restrict__ out_val, int64_t *__restrict__ out_idx) {
  using List = LdsList<CAP / 2>;
  __shared__ double cs[NWB][List::CAP];
  __shared__ int ci[NWB][List::CAP];
  const int wave = threadIdx.x / 64;
  const int lane = lane_id();
  const int64_t row = (int64_t)blockIdx.x * NWB + wave;
  if (row >= n_rows) return;  // (no block-wide barrier below)
  List list;
  double tau = neg_inf<double>();
  int tau_id = kPadId;
  list.init(cs[wave], ci[wave]);
  for (int s = 0; s < n_lists; ++s) {
    const int64_t base = ((int64_t)s * n_rows + row) * k;
    for (int e0 = 0; e0 < k; e0 += 64) {
      const int e = e0 + lane;
      double v = neg_inf<double>();
      int id = -1;
      if (e < k) {
        const int64_t x = in_idx[base + e];
        if (x >= 0) {
          v = in_val[base + e];
          id = (int)x;
        }
      }
      const bool cand = id >= 0 && before(v, id, tau, tau_id);
      const uint64_t bal = __ballot(cand);
      const int pos = list.slot(__popcll(bal & lanemask_lt()));
      if (cand) {
        cs[wave][pos] = v;
        ci[wave][pos] = id;
      }
      list.add(__popcll(bal));
      if (list.full()) {
        wave_sync();
        list.compact(cs[wave], ci[wave], k, tau, tau_id);
      }
    }
  }
  wave_sync();
  const int nc = list.compact(cs[wave], ci[wave], k, tau, tau_id);
  for (int e = lane; e < k; e += 64) {
    out_val[row * k + e] = e < nc ? cs[wave][e] : neg_inf<double>();
    out_idx[row * k + e] = e < nc ? ci[wave][e] : -1;
  }
}

template <int CAP, int NWB>
static void launch_merge_wide(const double *in_val, const int64_t *in_idx, int n_lists,
                              int64_t n_rows, int k, double *out_val, int64_t *out_idx,
                              hipStream_t s) {
  k_lists_merge_wide<CAP, NWB><<<dim3((unsigned)((n_rows + NWB - 1) / NWB)), dim3(64 * NWB), 0,
                                 s>>>(in_val, in_idx, n_lists, n_rows, k, out_val, out_idx);
}

}  // namespace lg

using namespace lg;

extern "C" int lg_rows_topk_f64(const double *F, int64_t ldf, int64_t n_rows,
                                int64_t n_cols, const float *eu, const float *ei,
                                int32_t dim, const int64_t *ex_rowptr,
                                const int32_t *ex_col, int32_t excl_mode, int32_t k,
                                double *out_val, int64_t *out_idx, lg_stream_t stream) {
  const RowsArgs a{F, ldf, n_rows, n_cols, eu, ei, dim, ex_rowptr, ex_col, excl_mode, k,
                   out_val, out_idx, (hipStream_t)stream};
  if (const int rc = check_rows_args("lg_rows_topk_f64", 128, a)) return rc;
  if (n_rows == 0) return LG_OK;
  if (k <= 64) launch_rows_topk<RegList<2>, 8>(a);
  else launch_rows_topk<RegList<4>, 8>(a);
  return launch_status("lg_rows_topk_f64");
}

extern "C" int lg_rows_topk_wide_f64(const double *F, int64_t ldf, int64_t n_rows,
                                     int64_t n_cols, const float *eu, const float *ei,
                                     int32_t dim, const int64_t *ex_rowptr,
                                     const int32_t *ex_col, int32_t excl_mode, int32_t k,
                                     double *out_val, int64_t *out_idx, lg_stream_t stream) {
  const RowsArgs a{F, ldf, n_rows, n_cols, eu, ei, dim, ex_rowptr, ex_col, excl_mode, k,
                   out_val, out_idx, (hipStream_t)stream};
  if (const int rc = check_rows_args("lg_rows_topk_wide_f64", 1024, a)) return rc;
  if (n_rows == 0) return LG_OK;
  if (k <= 256) launch_rows_topk<LdsList<256>, 8>(a);
  else if (k <= 512) launch_rows_topk<LdsList<512>, 4>(a);
  else launch_rows_topk<LdsList<1024>, 2>(a);
  return launch_status("lg_rows_topk_wide_f64");
}

extern "C" int lg_topk_lists_merge_f64(const double *in_val, const int64_t *in_idx,
                                       int32_t n_lists, int64_t n_rows, int32_t k,
                                       double *out_val, int64_t *out_idx, lg_stream_t stream) {
  LG_REQUIRE(n_lists >= 1 && n_rows >= 0, "lg_topk_lists_merge_f64: bad sizes");
  LG_REQUIRE(k >= 1 && k <= 128, "lg_topk_lists_merge_f64: k=%d not in [1,128]", k);
  LG_REQUIRE(n_rows == 0 || (in_val && in_idx && out_val && out_idx),
             "lg_topk_lists_merge_f64: NULL argument");
  if (n_rows == 0) return LG_OK;
  const dim3 grid((unsigned)((n_rows + 3) / 4));
  hipStream_t s = (hipStream_t)stream;
  if (k <= 64)
    k_lists_merge_f64<2><<<grid, dim3(256), 0, s>>>(in_val, in_idx, n_lists, n_rows, k, out_val,
                                                    out_idx);
  else
    k_lists_merge_f64<4><<<grid, dim3(256), 0, s>>>(in_val, in_idx, n_lists, n_rows, k, out_val,
                                                    out_idx);
  return launch_status("lg_topk_lists_merge_f64");
}

extern "C" int lg_topk_lists_merge_wide_f64(const double *in_val, const int64_t *in_idx,
                                            int32_t n_lists, int64_t n_rows, int32_t k,
                                            double *out_val, int64_t *out_idx,
                                            lg_stream_t stream) {
  LG_REQUIRE(n_lists >= 1 && n_rows >= 0, "lg_topk_lists_merge_wide_f64: bad sizes");
  LG_REQUIRE(k >= 1 && k <= 1024, "lg_topk_lists_merge_wide_f64: k=%d not in [1,1024]", k);
  LG_REQUIRE(n_rows == 0 || (in_val && in_idx && out_val && out_idx),
             "lg_topk_lists_merge_wide_f64: NULL argument");
  if (n_rows == 0) return LG_OK;
  hipStream_t s = (hipStream_t)stream;
  if (k <= 256)
    launch_merge_wide<512, 4>(in_val, in_idx, n_lists, n_rows, k, out_val, out_idx, s);
  else if (k <= 512)
    launch_merge_wide<1024, 4>(in_val, in_idx, n_lists, n_rows, k, out_val, out_idx, s);
  else
    launch_merge_wide<2048, 2>(in_val, in_idx, n_lists, n_rows, k, out_val, out_idx, s);
  return launch_status("lg_topk_lists_merge_wide_f64");
}
