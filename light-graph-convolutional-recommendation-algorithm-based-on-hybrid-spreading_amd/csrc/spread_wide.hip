// K4w: the dense spreading top-K and the list merge for 128 < k <= 1024, fp64, gfx950.
//
// Reference: model/SpreadMethod/recommend.py:31-50 and model/SpreadLightGCN/recommend.py
// slice [:k] off an argsort of F[u] (G * F, model/SpreadLightGCN/model.py:151), so they take
// any RECOMMEND["k"]. spread.hip's k_rows_topk and spread_tiled.hip's k_lists_merge_f64 sort
// their candidate lists in registers (wave_compact<K, M>, CAP = 64 M <= 256), which stops
// at k = 128. Their wide twins here keep the same scan, admission rule (v > tau), exclusion
// cursor, order (value desc, column asc) and {-inf, -1} padding, with the candidate list of
// CAP = 512 / 1024 / 2048 {double, int} entries (k <= 256 / 512 / 1024) in wave-owned LDS.
//
// The list is two halves of H = CAP / 2 >= k entries: A, always sorted, and B, the entries
// admitted since the last compaction. A compaction sorts B alone, takes the better of
// A[H - 1 - j] and B[j] into A (which leaves the H best of both there, as a bitonic
// sequence) and runs the log2(H) merge stages over A: about 0.45 of sorting A and B
// together. Two waves' lists merge the same way without any sort. Sorting works on
// 256-entry chunks: a chunk is loaded into registers (4 entries per lane), every bitonic stage
// of stride < 256 runs there (register swaps and wave shuffles, as wave_bitonic_sort of
// common.h), and only the strides >= 256 are compare-exchanges through LDS.
//
// LDS per wave = 12 CAP bytes: 6 / 12 / 24 KiB. Rows of >= 4096 columns get 8 / 4 / 2 waves
// per class (48 KiB per block in every class, three blocks per CU of 160 KiB), shorter rows
// one wave.
#include "common.h"

namespace lg {

constexpr int kChunk = 256;  // entries a wave sorts in registers: 4 per lane
constexpr int kChunkM = kChunk / 64;

// Bitonic stages (size; stride = S0, S0 / 2, .. 1) on one chunk in registers. S0 < kChunk.
// Entry j of a lane is global element base + 64 j + lane (base a multiple of kChunk).
template <int S0>
__device__ __forceinline__ void chunk_stages(double (&k)[kChunkM], int (&id)[kChunkM], int base,
                                             int size) {
  const int lane = lane_id();
#pragma unroll
  for (int stride = S0; stride > 0; stride >>= 1) {
    if (stride >= 64) {
      const int js = stride / 64;
#pragma unroll
      for (int j = 0; j < kChunkM; ++j) {
        if (j & js) continue;
        const int e = base + j * 64 + lane;  // lower element of the pair
        const bool desc = (e & size) == 0;   // this block sorts best-first
        const int p = j | js;
        const bool lo_better = before(k[j], id[j], k[p], id[p]);
        if (lo_better != desc) {
          const double tk = k[j]; k[j] = k[p]; k[p] = tk;
          const int ti = id[j]; id[j] = id[p]; id[p] = ti;
        }
      }
    } else {
#pragma unroll
      for (int j = 0; j < kChunkM; ++j) {
        const int e = base + j * 64 + lane;
        const double ok = __shfl_xor(k[j], stride);
        const int oi = __shfl_xor(id[j], stride);
        const bool lower = (e & stride) == 0;
        const bool desc = (e & size) == 0;
        const bool mine_better = before(k[j], id[j], ok, oi);
        const bool keep_mine = (lower == desc) ? mine_better : !mine_better;
        if (!keep_mine) { k[j] = ok; id[j] = oi; }
      }
    }
  }
}

__device__ __forceinline__ void chunk_load(const double *ks, const int *ids, int base,
                                           double (&k)[kChunkM], int (&id)[kChunkM]) {
  const int lane = lane_id();
#pragma unroll
  for (int j = 0; j < kChunkM; ++j) {
    k[j] = ks[base + j * 64 + lane];
    id[j] = ids[base + j * 64 + lane];
  }
}

__device__ __forceinline__ void chunk_store(double *ks, int *ids, int base,
                                            const double (&k)[kChunkM],
                                            const int (&id)[kChunkM]) {
  const int lane = lane_id();
#pragma unroll
  for (int j = 0; j < kChunkM; ++j) {
    ks[base + j * 64 + lane] = k[j];
    ids[base + j * 64 + lane] = id[j];
  }
}

// The bitonic stages (size; stride = size / 2 .. 1) over the entries [0, P) of a wave-owned LDS
// list (P a multiple of kChunk): the strides >= kChunk as compare-exchanges through LDS (P / 2
// disjoint pairs per stage, two per lane per trip with their reads issued together; p < half
// is wave-uniform: half % 128 == 0 whenever such a stride exists), the rest chunk by chunk in
// registers. The caller has synchronised the wave's LDS writes.
__device__ __forceinline__ void lds_size_stages(double *ks, int *ids, int P, int size) {
  const int lane = lane_id();
  const int half = P >> 1;
  for (int stride = size >> 1; stride >= kChunk; stride >>= 1) {
    for (int p0 = lane; p0 < half; p0 += 128) {
      double a[2], b[2];
      int ia[2], ib[2], lo[2];
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const int p = p0 + 64 * q;
        lo[q] = ((p & ~(stride - 1)) << 1) | (p & (stride - 1));
        a[q] = ks[lo[q]];
        ia[q] = ids[lo[q]];
        b[q] = ks[lo[q] + stride];
        ib[q] = ids[lo[q] + stride];
      }
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const bool desc = (lo[q] & size) == 0;
        const bool swap = before(a[q], ia[q], b[q], ib[q]) != desc;
        if (swap) {
          ks[lo[q]] = b[q];
          ids[lo[q]] = ib[q];
          ks[lo[q] + stride] = a[q];
          ids[lo[q] + stride] = ia[q];
        }
      }
    }
    wave_sync();
  }
  double k[kChunkM];
  int id[kChunkM];
  for (int base = 0; base < P; base += kChunk) {
    chunk_load(ks, ids, base, k, id);
    chunk_stages<128>(k, id, base, size);
    chunk_store(ks, ids, base, k, id);
  }
  wave_sync();
}

// Bitonic sort of the P entries (ks, ids)[0, P) of a wave-owned LDS list (P a power of two,
// a multiple of kChunk) into the output order: entry 0 is the best by (value desc, id asc).
// The callers pad with {-inf, kPadId}, which sorts last.
__device__ __forceinline__ void lds_chunk_sort(double *ks, int *ids, int P) {
  double k[kChunkM];
  int id[kChunkM];
  // every chunk sorted on its own: the stages of size <= kChunk
  for (int base = 0; base < P; base += kChunk) {
    chunk_load(ks, ids, base, k, id);
    chunk_stages<1>(k, id, base, 2);
    chunk_stages<2>(k, id, base, 4);
    chunk_stages<4>(k, id, base, 8);
    chunk_stages<8>(k, id, base, 16);
    chunk_stages<16>(k, id, base, 32);
    chunk_stages<32>(k, id, base, 64);
    chunk_stages<64>(k, id, base, 128);
    chunk_stages<128>(k, id, base, 256);
    chunk_store(ks, ids, base, k, id);
  }
  wave_sync();
  for (int size = 2 * kChunk; size <= P; size <<= 1) lds_size_stages(ks, ids, P, size);
}

// A wave's candidate list of CAP = 2 H entries: A = [0, H), always sorted best-first with
// {-inf, kPadId} behind its entries, and B = [H, H + m), the m <= H entries admitted since
// the last compaction (or a partner wave's sorted list). list_init pads A.
template <int H>
__device__ __forceinline__ void list_init(double *ks, int *ids) {
  for (int e = lane_id(); e < H; e += 64) {
    ks[e] = neg_inf<double>();
    ids[e] = kPadId;
  }
  wave_sync();
}

// Merge B into A and keep A's best `keep` <= H as the list: B is sorted (unless it already
// is) over the next power of two >= m, then one flip stage -- A[H - 1 - j] takes the better
// of itself and B[j]; of two best-first sequences that leaves the H best of both in A, as a
// bitonic sequence -- and the log2(H) stages of a bitonic merge of A alone. About 0.45 of a
// full sort of A and B at m = H, less for a short B, no sort at all for a sorted one.
// wave_compact's contract (common.h): returns the new count (of the `keep` that rank), tau =
// the last kept entry when the list is full. The caller has synchronised B's writes.
template <int H>
__device__ __forceinline__ int list_compact(double *ks, int *ids, int cnt, int m, bool sorted,
                                            int keep, double &tau, int &tau_id) {
  const int lane = lane_id();
  if (m == 0) return cnt;  // (wave-uniform; tau stands)
  double *kb = ks + H;
  int *ib = ids + H;
  if (!sorted) {
    int P = kChunk;
    while (P < m) P <<= 1;
    for (int e = m + lane; e < P; e += 64) {
      kb[e] = neg_inf<double>();
      ib[e] = kPadId;
    }
    wave_sync();
    lds_chunk_sort(kb, ib, P);
  }
  for (int j = lane; j < m; j += 64) {  // (B's entries past m are padding: no exchange)
    const int i = H - 1 - j;
    const double vb = kb[j];
    const int xb = ib[j];
    if (before(vb, xb, ks[i], ids[i])) {
      ks[i] = vb;
      ids[i] = xb;
    }
  }
  wave_sync();
  lds_size_stages(ks, ids, H, H);
  cnt = cnt + m < keep ? cnt + m : keep;
  if (cnt == keep && keep > 0) { tau = ks[keep - 1]; tau_id = ids[keep - 1]; }
  else { tau = neg_inf<double>(); tau_id = kPadId; }
  wave_sync();
  return cnt;
}

// fp32 score in the chain order of chain_score<D> of spread.hip (lg_score_topk_f32's).
template <int D>
__device__ __forceinline__ float chain_score_w(const float *__restrict__ us,
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

// k_rows_topk of spread.hip with the lists (CAP / 2 >= k, see above) in LDS: NW waves per row
// (one row per block), wave w scans the row's w-th column range (whole 64-column steps) in
// ascending order into its own list, then the waves' top-k lists merge pairwise in log2(NW)
// rounds (the partner's <= k entries appended, the list compacted; the order is total, so
// the result is the single ascending scan's and ties go to the smaller column).
template <int CAP, int D, int NW>
__global__ __launch_bounds__(64 * NW) void k_rows_topk_wide(
    const double *__restrict__ F, int64_t ldf, int64_t n_rows, int64_t n_cols,
    const float *__restrict__ eu, const float *__restrict__ ei,
    const int64_t *__restrict__ ex_rowptr, const int32_t *__restrict__ ex_col, int excl_mode,
    int k, double *__restrict__ out_val, int64_t *__restrict__ out_idx) {
  constexpr int DU = D > 0 ? D : 1;
  constexpr int H = CAP / 2;
  static_assert(H >= kChunk && (CAP & (CAP - 1)) == 0 && (NW & (NW - 1)) == 0,
                "the list and its new entries: k <= CAP / 2 each");
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
  int cnt = 0, m = 0;  // entries of the sorted list, new entries behind it
  double tau = neg_inf<double>();
  int tau_id = kPadId;
  list_init<H>(cs[wave], ci[wave]);
  const double *row = F + r * ldf;
  constexpr int STEPS = D > 0 ? 1 : 2;  // (as k_rows_topk: two loads in flight without G)
  for (int64_t j00 = c0; j00 < c1; j00 += 64 * STEPS) {
    double v2[STEPS];
#pragma unroll
    for (int h = 0; h < STEPS; ++h) {
      const int64_t j = j00 + 64 * h + lane;
      v2[h] = j < c1 ? row[j] : neg_inf<double>();
    }
    if constexpr (D > 0) {
      if (j00 + lane < c1) v2[0] = (double)chain_score_w<DU>(us, ei + (j00 + lane) * D) * v2[0];
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
        const int pos = H + m + __popcll(bal & lanemask_lt());  // (< CAP: m <= H - 64)
        if (cand) {
          cs[wave][pos] = v;
          ci[wave][pos] = (int)j;
        }
        m += __popcll(bal);
        if (m > H - 64) {
          wave_sync();
          cnt = list_compact<H>(cs[wave], ci[wave], cnt, m, false, k, tau, tau_id);
          m = 0;
        }
      }
    }
  }
  wave_sync();
  int nc = list_compact<H>(cs[wave], ci[wave], cnt, m, false, k, tau, tau_id);
  if (lane == 0) s_n[wave] = nc;
#pragma unroll
  for (int st = 1; st < NW; st <<= 1) {
    __syncthreads();
    if (wave % (2 * st) == 0) {  // (wave + st < NW: NW is a power of two)
      const int n1 = s_n[wave + st];
      for (int e = lane; e < n1; e += 64) {  // (n1 <= k <= H)
        cs[wave][H + e] = cs[wave + st][e];
        ci[wave][H + e] = ci[wave + st][e];
      }
      wave_sync();
      nc = list_compact<H>(cs[wave], ci[wave], nc, n1, true, k, tau, tau_id);
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

// rows of at least this many columns get several waves each (spread.hip's threshold)
constexpr int64_t kWideSplitCols = 4096;

template <int CAP, int NW>
static void launch_rows_wide_nw(int dim, const double *F, int64_t ldf, int64_t n_rows,
                                int64_t n_cols, const float *eu, const float *ei,
                                const int64_t *ex_rowptr, const int32_t *ex_col, int excl_mode,
                                int k, double *out_val, int64_t *out_idx, hipStream_t s) {
  dim3 grid((unsigned)n_rows), block(64 * NW);
  switch (eu ? dim : 0) {
    case 0: k_rows_topk_wide<CAP, 0, NW><<<grid, block, 0, s>>>(F, ldf, n_rows, n_cols, eu, ei, ex_rowptr, ex_col, excl_mode, k, out_val, out_idx); break;
    case 32: k_rows_topk_wide<CAP, 32, NW><<<grid, block, 0, s>>>(F, ldf, n_rows, n_cols, eu, ei, ex_rowptr, ex_col, excl_mode, k, out_val, out_idx); break;
    case 64: k_rows_topk_wide<CAP, 64, NW><<<grid, block, 0, s>>>(F, ldf, n_rows, n_cols, eu, ei, ex_rowptr, ex_col, excl_mode, k, out_val, out_idx); break;
    default: k_rows_topk_wide<CAP, 128, NW><<<grid, block, 0, s>>>(F, ldf, n_rows, n_cols, eu, ei, ex_rowptr, ex_col, excl_mode, k, out_val, out_idx); break;
  }
}

// NW waves per long row: 48 KiB of lists per block in every class
template <int CAP, int NW>
static void launch_rows_wide(int dim, const double *F, int64_t ldf, int64_t n_rows,
                             int64_t n_cols, const float *eu, const float *ei,
                             const int64_t *ex_rowptr, const int32_t *ex_col, int excl_mode,
                             int k, double *out_val, int64_t *out_idx, hipStream_t s) {
  if (n_cols >= kWideSplitCols)
    launch_rows_wide_nw<CAP, NW>(dim, F, ldf, n_rows, n_cols, eu, ei, ex_rowptr, ex_col,
                                 excl_mode, k, out_val, out_idx, s);
  else
    launch_rows_wide_nw<CAP, 1>(dim, F, ldf, n_rows, n_cols, eu, ei, ex_rowptr, ex_col,
                                excl_mode, k, out_val, out_idx, s);
}

// k_lists_merge_f64 of spread_tiled.hip with the list (CAP / 2 >= k) in LDS: one wave
// per row, NWB rows per block.
template <int CAP, int NWB>
__global__ __launch_bounds__(64 * NWB) void k_lists_merge_wide(
    const double *__restrict__ in_val, const int64_t *__restrict__ in_idx, int n_lists,
    int64_t n_rows, int k, double *__restrict__ out_val, int64_t *__restrict__ out_idx) {
  __shared__ double cs[NWB][CAP];
  __shared__ int ci[NWB][CAP];
  const int wave = threadIdx.x / 64;
  const int lane = lane_id();
  const int64_t row = (int64_t)blockIdx.x * NWB + wave;
  if (row >= n_rows) return;  // (no block-wide barrier below)
  constexpr int H = CAP / 2;
  static_assert(H >= kChunk && (CAP & (CAP - 1)) == 0, "k <= CAP / 2");
  int cnt = 0, m = 0;
  double tau = neg_inf<double>();
  int tau_id = kPadId;
  list_init<H>(cs[wave], ci[wave]);
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
      const int pos = H + m + __popcll(bal & lanemask_lt());  // (< CAP: m <= H - 64)
      if (cand) {
        cs[wave][pos] = v;
        ci[wave][pos] = id;
      }
      m += __popcll(bal);
      if (m > H - 64) {
        wave_sync();
        cnt = list_compact<H>(cs[wave], ci[wave], cnt, m, false, k, tau, tau_id);
        m = 0;
      }
    }
  }
  wave_sync();
  const int nc = list_compact<H>(cs[wave], ci[wave], cnt, m, false, k, tau, tau_id);
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

extern "C" int lg_rows_topk_wide_f64(const double *F, int64_t ldf, int64_t n_rows,
                                     int64_t n_cols, const float *eu, const float *ei,
                                     int32_t dim, const int64_t *ex_rowptr,
                                     const int32_t *ex_col, int32_t excl_mode, int32_t k,
                                     double *out_val, int64_t *out_idx, lg_stream_t stream) {
  LG_REQUIRE(F && out_val && out_idx && n_rows >= 0 && n_cols >= 0 && ldf >= n_cols &&
                 n_cols < 0x7fffffff,
             "lg_rows_topk_wide_f64: bad arguments");
  LG_REQUIRE(k >= 1 && k <= 1024, "lg_rows_topk_wide_f64: k=%d not in [1,1024]", k);
  LG_REQUIRE(!eu == !ei, "lg_rows_topk_wide_f64: eu/ei must both be set or both NULL");
  LG_REQUIRE(!eu || dim == 32 || dim == 64 || dim == 128,
             "lg_rows_topk_wide_f64: dim %d not in {32,64,128}", dim);
  LG_REQUIRE(excl_mode == LG_EXCL_DROP || excl_mode == LG_EXCL_NONE,
             "lg_rows_topk_wide_f64: bad excl_mode %d", excl_mode);
  LG_REQUIRE(!ex_rowptr == !ex_col,
             "lg_rows_topk_wide_f64: ex_rowptr/ex_col must both be set");
  LG_REQUIRE(!(eu && excl_mode == LG_EXCL_NONE && ex_rowptr),
             "lg_rows_topk_wide_f64: a G factor with exclusions requires LG_EXCL_DROP");
  if (n_rows == 0) return LG_OK;
  hipStream_t s = (hipStream_t)stream;
  if (k <= 256)
    launch_rows_wide<512, 8>(dim, F, ldf, n_rows, n_cols, eu, ei, ex_rowptr, ex_col, excl_mode,
                             k, out_val, out_idx, s);
  else if (k <= 512)
    launch_rows_wide<1024, 4>(dim, F, ldf, n_rows, n_cols, eu, ei, ex_rowptr, ex_col, excl_mode,
                              k, out_val, out_idx, s);
  else
    launch_rows_wide<2048, 2>(dim, F, ldf, n_rows, n_cols, eu, ei, ex_rowptr, ex_col, excl_mode,
                              k, out_val, out_idx, s);
  return launch_status("lg_rows_topk_wide_f64");
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
