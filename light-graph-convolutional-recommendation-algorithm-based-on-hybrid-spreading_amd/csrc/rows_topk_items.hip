// K4i: the spreading / LGCNHS recommendation over a CANDIDATE ITEM SET (strictly ascending
// ids into the full catalog), dense path, gfx950: getResource's F = A @ W summed for the
// candidates' columns only and reduced to per-user top-K in the same pass.
//
// Row u of the output is the first k of {(v(u, j), j) : j in item_ids, j not dropped by u's
// exclusions} under (value desc, item id asc), v(u, j) = (G[u][j] *) F[u][j] with
//   F[u][j] = sum_{i in items(u), ascending} W[i][j]     k_spread_resource's fp64 chain
//   G[u][j] = the fp32 chain score of lg_score_topk_f32, promoted to fp64 (K4's product)
// W is the full I x I HybridS matrix: a candidate set restricts the columns that are ranked,
// never the paths u -> i -> v -> j behind them. It equals lg_rows_topk_f64 / _wide_f64 on the
// gathered columns lg_spread_resource_f64(...)[:, item_ids] with ei[item_ids], the exclusion
// columns renumbered and the ids mapped back, bit for bit -- but no F is written, nothing is
// gathered and only the candidates' columns of W are read: the work is E_rows x |C| adds
// instead of E_rows x I.
//
// It is K4's scan (k_rows_topk, csrc/rows_topk.hip) turned onto candidate POSITIONS: one
// block per row, the row's waves take consecutive position ranges in whole 64-position
// steps, the lane of position p reads j = item_ids[p], sums its column over the row's items
// (four loads in flight per position, as k_spread_resource; without G two positions per lane:
// eight), admits on v > tau, checks the exclusion cursor in item-id space (lower_bound on j:
// monotone, the candidates ascend), stores {v, j}. The lists are wave_list.h's and the waves'
// lists merge pairwise as in K4. No workspace.
//
// Any input is memory-safe: a position past the range never enters a list; an id outside
// [0, n_items) reads column 0 and never ranks; a list that is not ascending gives
// unspecified lists, no out-of-bounds access (the cursor stays inside the row's exclusions).
#include "common.h"
#include "wave_list.h"

namespace lg {
namespace {

// fp32 score in the chain order of lg_score_topk_f32: a copy of rows_topk.hip's chain_score
// (that file's instantiations keep their text).
template <int D>
__device__ __forceinline__ float items_chain_score(const float *__restrict__ us,
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

// rows of at least this many candidates get several waves each, shorter ones one. (K4 splits
// at 4096 columns of one load each; a position here is a chain of the row's degree loads.)
constexpr int64_t kSplitCand = 512;

template <typename List, int D, int NW>
__global__ __launch_bounds__(64 * NW) void k_rows_topk_items(
    const int64_t *__restrict__ user_rowptr, const int32_t *__restrict__ user_items,
    const double *__restrict__ W, int64_t n_items, const int32_t *__restrict__ item_ids,
    int64_t n_cand, const float *__restrict__ eu, const float *__restrict__ ei,
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
  const int64_t pb = user_rowptr[r], pe = user_rowptr[r + 1];
  const int64_t span = ((n_cand + NW - 1) / NW + 63) / 64 * 64;
  const int64_t c0 = wave * span, c1 = c0 + span < n_cand ? c0 + span : n_cand;
  List list;
  double tau = neg_inf<double>();
  int tau_id = kPadId;
  if constexpr (List::kPadded) list.init(cs[wave], ci[wave]);
  // no G: two 64-position steps per round (eight loads in flight per lane; the candidates of
  // the first step are taken before the second's, so ids reach the list in ascending order).
  // With G one step: K4 measured two interleaved score chains slower (rows_topk.hip).
  constexpr int STEPS = D > 0 ? 1 : 2;
  for (int64_t p00 = c0; p00 < c1; p00 += 64 * STEPS) {
    int jd[STEPS];        // the position's item id (-1: none, or outside the catalog)
    const double *col[STEPS];
#pragma unroll
    for (int h = 0; h < STEPS; ++h) {
      const int64_t p = p00 + 64 * h + lane;
      int j = p < c1 ? item_ids[p] : -1;
      if (j < 0 || j >= n_items) j = -1;
      jd[h] = j;
      col[h] = W + (j < 0 ? 0 : j);  // (column 0 is read instead; it never ranks)
    }
    double s[STEPS];
#pragma unroll
    for (int h = 0; h < STEPS; ++h) s[h] = 0.0;
    int64_t q = pb;
    for (; q + 4 <= pe; q += 4) {
      const int64_t i0 = user_items[q], i1 = user_items[q + 1], i2 = user_items[q + 2],
                    i3 = user_items[q + 3];
      double w[STEPS][4];
#pragma unroll
      for (int h = 0; h < STEPS; ++h) {
        w[h][0] = col[h][i0 * n_items];
        w[h][1] = col[h][i1 * n_items];
        w[h][2] = col[h][i2 * n_items];
        w[h][3] = col[h][i3 * n_items];
      }
#pragma unroll
      for (int h = 0; h < STEPS; ++h) s[h] = (((s[h] + w[h][0]) + w[h][1]) + w[h][2]) + w[h][3];
    }
    for (; q < pe; ++q) {
      const int64_t i = user_items[q];
#pragma unroll
      for (int h = 0; h < STEPS; ++h) s[h] += col[h][i * n_items];
    }
    if constexpr (D > 0) {
      if (jd[0] >= 0)
        s[0] = (double)items_chain_score<DU>(us, ei + (int64_t)jd[0] * D) * s[0];
    }
#pragma unroll
    for (int h = 0; h < STEPS; ++h) {
      if (p00 + 64 * h >= c1) break;  // (wave-uniform)
      const int j = jd[h];
      const double v = s[h];
      bool cand = j >= 0 && v > tau;
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
          ci[wave][pos] = j;
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

struct ItemsArgs {
  const int64_t *user_rowptr;
  const int32_t *user_items;
  const double *W;
  int64_t n_rows, n_items;
  const int32_t *item_ids;
  int64_t n_cand;
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
void launch_items_nw(const ItemsArgs &a) {
  auto kern = k_rows_topk_items<List, 0, NW>;
  switch (a.eu ? a.dim : 0) {
    case 0: break;
    case 32: kern = k_rows_topk_items<List, 32, NW>; break;
    case 64: kern = k_rows_topk_items<List, 64, NW>; break;
    default: kern = k_rows_topk_items<List, 128, NW>; break;
  }
  kern<<<dim3((unsigned)a.n_rows), dim3(64 * NW), 0, a.s>>>(
      a.user_rowptr, a.user_items, a.W, a.n_items, a.item_ids, a.n_cand, a.eu, a.ei,
      a.ex_rowptr, a.ex_col, a.excl_mode, a.k, a.out_val, a.out_idx);
}

// NW waves per row of at least kSplitCand candidates
template <typename List, int NW>
void launch_items(const ItemsArgs &a) {
  if (a.n_cand >= kSplitCand) launch_items_nw<List, NW>(a);
  else launch_items_nw<List, 1>(a);
}

}  // namespace
}  // namespace lg

using namespace lg;

extern "C" int lg_spread_rows_topk_items_f64(
    const int64_t *user_rowptr, const int32_t *user_items, const double *W, int64_t n_rows,
    int64_t n_items, const int32_t *item_ids, int64_t n_cand, const float *eu, const float *ei,
    int32_t dim, const int64_t *ex_rowptr, const int32_t *ex_col, int32_t excl_mode, int32_t k,
    double *out_val, int64_t *out_idx, lg_stream_t stream) {
  const char *who = "lg_spread_rows_topk_items_f64";
  LG_REQUIRE(user_rowptr && user_items && W && item_ids && out_val && out_idx,
             "%s: null argument", who);
  LG_REQUIRE(n_rows >= 0 && n_rows < 0x7fffffff && n_items >= 0 && n_items < 0x7fffffff,
             "%s: bad sizes (n_rows %lld, n_items %lld)", who, (long long)n_rows,
             (long long)n_items);
  LG_REQUIRE(n_cand >= 0 && n_cand <= n_items, "%s: n_cand %lld not in [0, n_items = %lld]",
             who, (long long)n_cand, (long long)n_items);
  LG_REQUIRE(k >= 1 && k <= 1024, "%s: k=%d not in [1,%d]", who, k, 1024);
  LG_REQUIRE(!eu == !ei, "%s: eu/ei must both be set or both NULL", who);
  LG_REQUIRE(!eu || dim == 32 || dim == 64 || dim == 128, "%s: dim %d not in {32,64,128}", who,
             dim);
  LG_REQUIRE(excl_mode == LG_EXCL_DROP || excl_mode == LG_EXCL_NONE, "%s: bad excl_mode %d",
             who, excl_mode);
  LG_REQUIRE(!ex_rowptr == !ex_col, "%s: ex_rowptr/ex_col must both be set", who);
  LG_REQUIRE(!(eu && excl_mode == LG_EXCL_NONE && ex_rowptr),
             "%s: a G factor with exclusions requires LG_EXCL_DROP", who);
  if (n_rows == 0) return LG_OK;
  const ItemsArgs a{user_rowptr, user_items, W, n_rows, n_items, item_ids, n_cand, eu, ei, dim,
                    ex_rowptr, ex_col, excl_mode, k, out_val, out_idx, (hipStream_t)stream};
  if (k <= 64) launch_items<RegList<2>, 8>(a);
  else if (k <= 128) launch_items<RegList<4>, 8>(a);
  else if (k <= 256) launch_items<LdsList<256>, 8>(a);
  else if (k <= 512) launch_items<LdsList<512>, 4>(a);
  else launch_items<LdsList<1024>, 2>(a);
  return launch_status(who);
}
