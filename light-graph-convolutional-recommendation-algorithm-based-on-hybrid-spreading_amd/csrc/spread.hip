// K3: hybrid spreading (mass diffusion / heat conduction mix) in fp64, gfx950.
//
// Reference (model/SpreadMethod/model.py), all dense numpy fp64 on the host:
//   getSpreadingGeneralMat :14-27   k_u = A.sum(1) (0 -> 1); general_W = (A.T / k_u) @ A
//   HybridS                :63-85   k_i = A.sum(0); den = k_i^(1-l) (x) k_j^l; den==0 -> 1;
//                                    W = general_W / den
//   getResource            :88-99   F = A @ W
//
// A is 0/1 and sparse, so the GEMMs are replaced by sparse row sums with a deterministic
// ascending summation order:
//   general_W[i][j] = sum_{v in users(i)} [j in items(v)] * fl(1/k_v)   (one block per i)
//   F[u][j]         = sum_{i in items(u)} W[i][j]                        (one block per u)
// which cost E*avg_deg and E*I instead of 2*U*I^2 each. The top-K over the rows of F (K4) is
// rows_topk.hip.
#include "common.h"

namespace lg {

__global__ __launch_bounds__(256) void k_spread_general(
    const int64_t *__restrict__ item_rowptr, const int32_t *__restrict__ item_users,
    const int64_t *__restrict__ user_rowptr, const int32_t *__restrict__ user_items,
    int64_t n_items, double *__restrict__ gW) {
  const int64_t i = blockIdx.x;
  double *row = gW + i * n_items;
  for (int64_t j = threadIdx.x; j < n_items; j += blockDim.x) row[j] = 0.0;
  __syncthreads();
  const int64_t eb = item_rowptr[i], ee = item_rowptr[i + 1];
  for (int64_t e = eb; e < ee; ++e) {
    const int32_t v = item_users[e];
    const int64_t pb = user_rowptr[v], pe = user_rowptr[v + 1];
    // (A.T / k_u)[i][v] = 1.0 / k_v, correctly rounded; times A[v][j] = 1 is exact.
    const double wv = 1.0 / (double)(pe - pb);
    for (int64_t p = pb + threadIdx.x; p < pe; p += blockDim.x) row[user_items[p]] += wv;
    __syncthreads();  // the next user may hit the same columns from other threads
  }
}

// The two factors of HybridS's denominator per item: alpha = k^(1-l), beta = k^l (the pow()
// calls of k_hybrid_weight).
__global__ __launch_bounds__(256) void k_hybrid_factors(const double *__restrict__ k_item,
                                                        int64_t n, double lambda,
                                                        double *__restrict__ alpha,
                                                        double *__restrict__ beta) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  alpha[i] = pow(k_item[i], 1.0 - lambda);
  beta[i] = pow(k_item[i], lambda);
}

// general_W and HybridS in one pass, W = general_W / den without general_W in memory. One
// block per (item row i, range of kSpreadCols columns): the range of the row is summed in an
// LDS accumulator with the same fp64 adds in the same order as k_spread_general (users of i
// ascending, one fl(1/k_v) per item of v in the range), then written as
// fl(acc / fl(alpha_i beta_j)) (den == 0 -> 1), k_hybrid_weight's arithmetic. general_W is
// exactly symmetric, so its transposed form gives the same W. Where each user's items enter
// each range comes from a table built once (k_user_range_starts). Users are taken kSpreadG at
// a time: their row bounds and range starts, then every thread's item of each of them, are
// loaded together (one round trip per kind, not one per user), and the adds follow user by
// user (a barrier between users: two may share a column). Rows of hub items (hundreds of
// users) spread over the ranges' blocks instead of one block's chain. At the C3 shape this
// writes one I x I matrix instead of writing general_W, reading it back and writing W.
constexpr int kSpreadCols = 4096;
constexpr int kSpreadG = 8;

// starts[v][r] = the position (relative to v's row) of v's first item >= r kSpreadCols, for
// r = 0 .. n_ranges (the last: the row's length)
__global__ __launch_bounds__(256) void k_user_range_starts(const int64_t *__restrict__ user_rowptr,
                                                           const int32_t *__restrict__ user_items,
                                                           int64_t n_users, int n_ranges,
                                                           int32_t *__restrict__ starts) {
  const int64_t x = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (x >= n_users * (n_ranges + 1)) return;
  const int64_t v = x / (n_ranges + 1);
  const int r = (int)(x - v * (n_ranges + 1));
  const int64_t pb = user_rowptr[v], pe = user_rowptr[v + 1];
  const int64_t c = (int64_t)r * kSpreadCols;
  const int64_t p = r == n_ranges ? pe : lower_bound_i32(user_items, pb, pe, (int32_t)(c < 0x7fffffff ? c : 0x7fffffff));
  starts[x] = (int32_t)(p - pb);
}

__global__ __launch_bounds__(256) void k_spread_hybrid(
    const int64_t *__restrict__ item_rowptr, const int32_t *__restrict__ item_users,
    const int64_t *__restrict__ user_rowptr, const int32_t *__restrict__ user_items,
    const int32_t *__restrict__ starts, int n_ranges, int64_t n_items,
    const double *__restrict__ alpha, const double *__restrict__ beta,
    double *__restrict__ W) {
  __shared__ double acc[kSpreadCols];
  const int64_t i = blockIdx.x / n_ranges;
  const int r = (int)(blockIdx.x - i * n_ranges);
  const int64_t c0 = (int64_t)r * kSpreadCols;
  const int64_t c1 = c0 + kSpreadCols < n_items ? c0 + kSpreadCols : n_items;
  const int tid = threadIdx.x;
  for (int t = tid; t < kSpreadCols; t += blockDim.x) acc[t] = 0.0;
  __syncthreads();
  const int64_t eb = item_rowptr[i], ee = item_rowptr[i + 1];
  for (int64_t g0 = eb; g0 < ee; g0 += kSpreadG) {
    const int ng = ee - g0 < kSpreadG ? (int)(ee - g0) : kSpreadG;
    int64_t pb[kSpreadG];
    int32_t sb[kSpreadG], se[kSpreadG];
    int32_t deg[kSpreadG];
#pragma unroll
    for (int g = 0; g < kSpreadG; ++g) {
      const int32_t v = item_users[g0 + (g < ng ? g : 0)];
      pb[g] = user_rowptr[v];
      deg[g] = (int32_t)(user_rowptr[v + 1] - pb[g]);
      sb[g] = starts[(int64_t)v * (n_ranges + 1) + r];
      se[g] = starts[(int64_t)v * (n_ranges + 1) + r + 1];
    }
    int32_t x[kSpreadG];  // this thread's first item of each user in the range (-1: none)
#pragma unroll
    for (int g = 0; g < kSpreadG; ++g)
      x[g] = g < ng && sb[g] + tid < se[g] ? user_items[pb[g] + sb[g] + tid] : -1;
#pragma unroll
    for (int g = 0; g < kSpreadG; ++g) {
      if (g >= ng) break;
      const double wv = 1.0 / (double)deg[g];  // k_spread_general's fl(1/k_v)
      if (x[g] >= 0) acc[x[g] - c0] += wv;
      for (int32_t q = sb[g] + tid + (int32_t)blockDim.x; q < se[g]; q += blockDim.x)
        acc[user_items[pb[g] + q] - c0] += wv;  // (users with > 256 items in the range)
      __syncthreads();  // the next user may hit the same columns from other threads
    }
  }
  double *row = W + i * n_items;
  const double ai = alpha[i];
  for (int64_t j = c0 + tid; j < c1; j += blockDim.x) {
    double den = ai * beta[j];
    if (den == 0.0) den = 1.0;
    row[j] = acc[j - c0] / den;
  }
}

// 32x32 tiles; the transposed source is staged through LDS for coalesced reads. The
// tile's 32 row factors k_i^(1-l) and 32 column factors k_j^l are computed once per tile
// (np.power(item_degrees, 1 - Lambda) / np.power(item_degrees, Lambda)).
__global__ __launch_bounds__(256) void k_hybrid_weight(const double *__restrict__ gW,
                                                       const double *__restrict__ k_item,
                                                       double lambda, int64_t n, int transpose,
                                                       double *__restrict__ W) {
  __shared__ double tile[32][33];
  __shared__ double alpha[32], beta[32];
  const int64_t bi = blockIdx.y * 32, bj = blockIdx.x * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8
  if (threadIdx.x < 32) {
    const int64_t i = bi + threadIdx.x;
    alpha[threadIdx.x] = i < n ? pow(k_item[i], 1.0 - lambda) : 1.0;
  } else if (threadIdx.x < 64) {
    const int64_t j = bj + threadIdx.x - 32;
    beta[threadIdx.x - 32] = j < n ? pow(k_item[j], lambda) : 1.0;
  }
  if (transpose) {
    for (int yy = ty; yy < 32; yy += 8) {
      const int64_t si = bj + yy, sj = bi + tx;  // source row = output column
      tile[yy][tx] = (si < n && sj < n) ? gW[si * n + sj] : 0.0;
    }
  }
  __syncthreads();
  for (int yy = ty; yy < 32; yy += 8) {
    const int64_t i = bi + yy, j = bj + tx;
    if (i >= n || j >= n) continue;
    const double src = transpose ? tile[tx][yy] : gW[i * n + j];
    double den = alpha[yy] * beta[tx];
    if (den == 0.0) den = 1.0;
    W[i * n + j] = src / den;
  }
}

__global__ __launch_bounds__(256) void k_spread_resource(
    const int64_t *__restrict__ user_rowptr, const int32_t *__restrict__ user_items,
    const double *__restrict__ W, int64_t n_items, double *__restrict__ F, int64_t ldf) {
  const int64_t u = blockIdx.y;
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n_items) return;
  const int64_t pb = user_rowptr[u], pe = user_rowptr[u + 1];
  double s = 0.0;
  int64_t p = pb;
  for (; p + 4 <= pe; p += 4) {
    const double w0 = W[(int64_t)user_items[p] * n_items + j];
    const double w1 = W[(int64_t)user_items[p + 1] * n_items + j];
    const double w2 = W[(int64_t)user_items[p + 2] * n_items + j];
    const double w3 = W[(int64_t)user_items[p + 3] * n_items + j];
    s = (((s + w0) + w1) + w2) + w3;
  }
  for (; p < pe; ++p) s += W[(int64_t)user_items[p] * n_items + j];
  F[u * ldf + j] = s;
}

}  // namespace lg

using namespace lg;

extern "C" int lg_spread_general_f64(const int64_t *item_rowptr, const int32_t *item_users,
                                     const int64_t *user_rowptr, const int32_t *user_items,
                                     int64_t n_users, int64_t n_items, double *gW,
                                     lg_stream_t stream) {
  LG_REQUIRE(item_rowptr && item_users && user_rowptr && user_items && gW && n_users >= 0 &&
                 n_items >= 0,
             "lg_spread_general_f64: bad arguments");
  if (n_items == 0) return LG_OK;
  k_spread_general<<<dim3((unsigned)n_items), dim3(256), 0, (hipStream_t)stream>>>(
      item_rowptr, item_users, user_rowptr, user_items, n_items, gW);
  return launch_status("lg_spread_general_f64");
}

static int spread_ranges(int64_t n_items) { return (int)((n_items + kSpreadCols - 1) / kSpreadCols); }

extern "C" size_t lg_spread_hybrid_ws_bytes(int64_t n_items, int64_t n_users) {
  if (n_items <= 0) return 0;
  return (size_t)n_items * 2 * sizeof(double) +
         (size_t)(n_users > 0 ? n_users : 0) * (spread_ranges(n_items) + 1) * sizeof(int32_t);
}

extern "C" int lg_spread_hybrid_f64(const int64_t *item_rowptr, const int32_t *item_users,
                                    const int64_t *user_rowptr, const int32_t *user_items,
                                    const double *k_item, int64_t n_users, int64_t n_items,
                                    double lambda, double *W, void *ws, size_t ws_bytes,
                                    lg_stream_t stream) {
  LG_REQUIRE(item_rowptr && item_users && user_rowptr && user_items && k_item && W &&
                 n_users >= 0 && n_items >= 0 && n_items < 0x7fffffff,
             "lg_spread_hybrid_f64: bad arguments");
  if (n_items == 0) return LG_OK;
  const size_t need = lg_spread_hybrid_ws_bytes(n_items, n_users);
  if (!ws || ws_bytes < need) {
    set_error("lg_spread_hybrid_f64: workspace %zu < %zu bytes", ws_bytes, need);
    return LG_ERR_WORKSPACE;
  }
  const int nr = spread_ranges(n_items);
  LG_REQUIRE((int64_t)nr * n_items < 0x7fffffff, "lg_spread_hybrid_f64: %lld items: too many",
             (long long)n_items);
  hipStream_t s = (hipStream_t)stream;
  double *alpha = (double *)ws, *beta = alpha + n_items;
  int32_t *starts = (int32_t *)(beta + n_items);
  k_hybrid_factors<<<dim3((unsigned)((n_items + 255) / 256)), dim3(256), 0, s>>>(
      k_item, n_items, lambda, alpha, beta);
  const int64_t ns = n_users * (nr + 1);
  if (ns > 0)
    k_user_range_starts<<<dim3((unsigned)((ns + 255) / 256)), dim3(256), 0, s>>>(
        user_rowptr, user_items, n_users, nr, starts);
  k_spread_hybrid<<<dim3((unsigned)(nr * n_items)), dim3(256), 0, s>>>(
      item_rowptr, item_users, user_rowptr, user_items, starts, nr, n_items, alpha, beta, W);
  return launch_status("lg_spread_hybrid_f64");
}

extern "C" int lg_hybrid_weight_f64(const double *gW, const double *k_item, int64_t n_items,
                                    double lambda, int32_t transpose_gw, double *W,
                                    lg_stream_t stream) {
  LG_REQUIRE(gW && k_item && W && n_items >= 0, "lg_hybrid_weight_f64: bad arguments");
  LG_REQUIRE(gW != W || !transpose_gw, "lg_hybrid_weight_f64: transposed source cannot alias W");
  if (n_items == 0) return LG_OK;
  const unsigned t = (unsigned)((n_items + 31) / 32);
  k_hybrid_weight<<<dim3(t, t), dim3(256), 0, (hipStream_t)stream>>>(gW, k_item, lambda, n_items,
                                                                    transpose_gw, W);
  return launch_status("lg_hybrid_weight_f64");
}

extern "C" int lg_spread_resource_f64(const int64_t *user_rowptr, const int32_t *user_items,
                                      const double *W, int64_t n_users, int64_t n_items,
                                      double *F, int64_t ldf, lg_stream_t stream) {
  LG_REQUIRE(user_rowptr && user_items && W && F && n_users >= 0 && n_items >= 0 &&
                 ldf >= n_items,
             "lg_spread_resource_f64: bad arguments");
  if (n_users == 0 || n_items == 0) return LG_OK;
  hipStream_t s = (hipStream_t)stream;
  // grid.y is limited to 65535: walk users in slabs
  for (int64_t u0 = 0; u0 < n_users; u0 += 65535) {
    const int64_t nu = (n_users - u0) < 65535 ? (n_users - u0) : 65535;
    k_spread_resource<<<dim3((unsigned)((n_items + 255) / 256), (unsigned)nu), dim3(256), 0,
                        s>>>(user_rowptr + u0, user_items, W, n_items, F + u0 * ldf, ldf);
  }
  return launch_status("lg_spread_resource_f64");
}
