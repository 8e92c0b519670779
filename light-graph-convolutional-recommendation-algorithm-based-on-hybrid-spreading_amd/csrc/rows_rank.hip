// K4k: the rank of given (row, column) targets over dense fp64 rows -- where a user's held-out
// items stand among ALL items under the spreading / LGCNHS scores -- gfx950.
//
// Reference: model/SpreadMethod/recommend.py:31-50 orders a user's row by argsort(F[u])[::-1]
// with the train|val items filtered out, F = G * F for LGCNHS (model/SpreadLightGCN/model.py:151,
// fp32 G promoted to fp64); an evaluation on held-out items asks for the position of given items
// in that order, at any depth. With v(r, j) = F[r][j], or (double)chain(eu[r], ei[j]) * F[r][j]
// (K4's product, k_rows_topk of csrc/rows_topk.hip, the same expression), a column j RANKS for
// row r iff v(r, j) > -inf (NaN and -inf never rank) and, under LG_EXCL_DROP, j is not in r's
// exclusion row. For a target i of row r
//     out_val  = v(r, i)
//     out_rank = #{ ranked j != i : before(v(r, j), j, v(r, i), i) }   if i ranks, else -1
// before = (value desc, column asc), the order of every K4 list: rank < k iff
// lg_rows_topk_(wide_)f64's row holds i at position rank, with a bit-equal value.
//
// One block per KERNEL ROW: a run of at most LG_ROWS_RANK_ROW_MAX targets of one F row (the host
// cuts longer target rows; several kernel rows may name the same F row). NW waves per block by
// n_cols, as K4 splits its rows. No workspace, no global atomics:
//
//   1. the block computes the targets' values, writes out_val, and puts the ranking ones as
//      keys (v, id) into LDS, padded with {-inf, kPadId} to P = 64 / 256 / 512 / 1024; wave 0
//      sorts the keys best-first (in registers for P = 64, lds_chunk_sort above).
//   2. each wave streams its column range 64 columns per step with K4's loads. A column is of
//      interest only when it is `before` the WORST ranking target: a wave-uniform ballot skips
//      every other step. A surviving lane binary-searches the sorted keys for the first
//      position q with before((v, j), key_q) and adds 1 to hist[q] in LDS (one key: the wave
//      sums its ballots and adds once). A column that is itself a target is not before itself
//      and lands behind its own key(s). Excluded columns are counted here like any other and
//      taken out again in 2b: the block walks the row's exclusion run (DROP) and subtracts
//      every excluded column that is before the worst target at the key the stream found for
//      it -- the same value, bit for bit -- so the stream carries no exclusion search (K4's
//      cursor is a binary search in global memory per surviving lane; K4 admits few lanes,
//      a count admits most: K2k's correction, csrc/rank.hip, for the same reason).
//   3. an inclusive prefix sum over hist gives every sorted key its rank (equal keys -- a
//      target named twice -- get the same: nothing lands between them); every target finds its
//      own key by binary search and writes out_rank. A target that does not rank (value, or
//      excluded: its id is then not among the keys) keeps step 1's -1.
// The counts are integers: nothing depends on NW or on timing. The row is read once whatever
// the number of targets; a step that survives costs a binary search (<= 10 LDS reads) and one
// LDS atomic per surviving lane (measured at 600 x 20,000 without G: 0.028 ms for one target
// per row, 0.12 ms for 10 or 100, 0.21 ms for 1,000).
//
// LDS per block: keys 8 KiB + ids 4 KiB + hist 4 KiB (+ the user's embedding row, <= 512 B).
//
// Any input is memory-safe: a kernel row longer than LG_ROWS_RANK_ROW_MAX is clamped to it (the
// entries past it keep the caller's initial values); a target id outside [0, n_cols) gets
// {-1, -inf}; a kernel row whose F row is outside [0, n_f_rows) gets {-1, -inf} throughout.
#include "common.h"
#include "wave_list.h"

namespace lg {
namespace {

constexpr int kRankMax = LG_ROWS_RANK_ROW_MAX;
static_assert(kRankMax == 1024, "P's classes and the prefix sum assume 1024");

// fp32 score in the chain order of lg_score_topk_f32: a copy of rows_topk.hip's chain_score
// (that file's instantiations keep their text).
template <int D>
__device__ __forceinline__ float rank_chain_score(const float *__restrict__ us,
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

// rows of at least this many columns get several waves each, shorter ones one (K4's split)
constexpr int64_t kRankSplitCols = 4096;

template <int D, int NW>
__global__ __launch_bounds__(64 * NW) void k_rows_rank(
    const double *__restrict__ F, int64_t ldf, int64_t n_f_rows, int64_t n_cols,
    const float *__restrict__ eu, const float *__restrict__ ei,
    const int64_t *__restrict__ ex_rowptr, const int32_t *__restrict__ ex_col, int excl_mode,
    const int64_t *__restrict__ krow_f, const int64_t *__restrict__ t_rowptr,
    const int32_t *__restrict__ t_col, int64_t *__restrict__ out_rank,
    double *__restrict__ out_val) {
  constexpr int DU = D > 0 ? D : 1;
  constexpr int NT = 64 * NW;
  __shared__ double ks[kRankMax];
  __shared__ int ki[kRankMax];
  __shared__ int hist[kRankMax];
  __shared__ float us[DU];
  __shared__ int s_nr;
  const int wave = threadIdx.x / 64;
  const int lane = lane_id();
  const int64_t kr = blockIdx.x;  // (< n_krows: one block per kernel row)
  const int64_t t0 = t_rowptr[kr];
  const int64_t full = t_rowptr[kr + 1] - t0;
  const int n = full < 0 ? 0 : (full > kRankMax ? kRankMax : (int)full);
  if (n == 0) return;  // (block-uniform, as every early return below)
  const int64_t r = krow_f[kr];
  if (r < 0 || r >= n_f_rows) {
    for (int e = threadIdx.x; e < n; e += NT) {
      out_rank[t0 + e] = -1;
      out_val[t0 + e] = neg_inf<double>();
    }
    return;
  }
  if (D > 0)
    for (int t = threadIdx.x; t < D; t += NT) us[t] = eu[r * D + t];
  if (threadIdx.x == 0) s_nr = 0;
  int64_t xlo = 0, xhi = 0;
  if (ex_rowptr && excl_mode == LG_EXCL_DROP) {
    xlo = ex_rowptr[r];
    xhi = ex_rowptr[r + 1];
  }
  const double *row = F + r * ldf;
  const int P = n <= 64 ? 64 : (n <= 256 ? 256 : (n <= 512 ? 512 : 1024));
  __syncthreads();

  // ---- 1. the targets' values; the ranking ones become keys
  for (int e = threadIdx.x; e < P; e += NT) {
    double kv = neg_inf<double>();
    int kid = kPadId;
    if (e < n) {
      const int id = t_col[t0 + e];
      double v = neg_inf<double>();
      bool ranks = false;
      if ((unsigned)id < (unsigned)n_cols) {
        v = row[id];
        if constexpr (D > 0) v = (double)rank_chain_score<DU>(us, ei + (int64_t)id * D) * v;
        ranks = v > neg_inf<double>();
        if (ranks && xlo < xhi) {
          const int64_t p = lower_bound_i32(ex_col, xlo, xhi, (int32_t)id);
          if (p < xhi && ex_col[p] == (int32_t)id) ranks = false;
        }
      }
      out_val[t0 + e] = v;
      if (ranks) {
        kv = v;
        kid = id;
        atomicAdd(&s_nr, 1);
      } else {
        out_rank[t0 + e] = -1;
      }
    }
    ks[e] = kv;
    ki[e] = kid;
    hist[e] = 0;
  }
  __syncthreads();
  const int nr = s_nr;  // ranking targets: the keys [0, nr) once sorted
  if (nr == 0) return;
  if (wave == 0) {
    if (P == 64) {
      double k1[1] = {ks[lane]};
      int i1[1] = {ki[lane]};
      wave_bitonic_sort<double, 1>(k1, i1);
      ks[lane] = k1[0];
      ki[lane] = i1[0];
    } else {
      lds_chunk_sort(ks, ki, P);
    }
  }
  __syncthreads();

  // ---- 2. the stream: count every column whose value ranks at the first key it is before
  // (the row's excluded columns too: 2b takes them out again, which keeps the exclusion search
  // -- a binary search in global memory per surviving lane -- out of this loop)
  const double wv = ks[nr - 1];  // the worst ranking target
  const int wi = ki[nr - 1];
  {
    int one = 0;  // nr == 1: this wave's count, added to hist[0] once
    const int64_t span = ((n_cols + NW - 1) / NW + 63) / 64 * 64;
    const int64_t c0 = wave * span, c1 = c0 + span < n_cols ? c0 + span : n_cols;
    // no G: two 64-column steps per round, both loads in flight (k_rows_topk's loop)
    constexpr int STEPS = D > 0 ? 1 : 2;
    for (int64_t j00 = c0; j00 < c1; j00 += 64 * STEPS) {
      double v2[STEPS];
#pragma unroll
      for (int h = 0; h < STEPS; ++h) {
        const int64_t j = j00 + 64 * h + lane;
        v2[h] = j < c1 ? row[j] : neg_inf<double>();
      }
      if constexpr (D > 0) {
        if (j00 + lane < c1)
          v2[0] = (double)rank_chain_score<DU>(us, ei + (j00 + lane) * D) * v2[0];
      }
#pragma unroll
      for (int h = 0; h < STEPS; ++h) {
        const int64_t j0 = j00 + 64 * h;
        if (j0 >= c1) break;  // (wave-uniform)
        const int64_t j = j0 + lane;
        const double v = v2[h];
        // (before the worst target: v >= wv > -inf, so the value ranks)
        const bool cand = j < c1 && before(v, (int)j, wv, wi);
        const uint64_t bal = __ballot(cand);
        if (bal) {
          if (nr == 1) {  // (block-uniform) one key: every surviving lane lands on it
            one += __popcll(bal);
          } else if (cand) {
            int a = 0, b = nr - 1;  // before(., key_b) holds
            while (a < b) {
              const int mid = (a + b) >> 1;
              if (before(v, (int)j, ks[mid], ki[mid])) b = mid;
              else a = mid + 1;
            }
            atomicAdd(&hist[a], 1);
          }
        }
      }
    }
    if (lane == 0 && one) atomicAdd(&hist[0], one);
  }
  // ---- 2b. the row's excluded columns do not rank (DROP): those the stream counted come out
  // again, each at the key the stream put it (the same value expression, bit for bit). An id
  // outside the columns is skipped, an entry equal to the one before it counts once.
  for (int64_t p = xlo + threadIdx.x; p < xhi; p += NT) {
    const int j = ex_col[p];
    if ((unsigned)j >= (unsigned)n_cols) continue;
    if (p > xlo && ex_col[p - 1] == j) continue;
    double v = row[j];
    if constexpr (D > 0) v = (double)rank_chain_score<DU>(us, ei + (int64_t)j * D) * v;
    if (!before(v, j, wv, wi)) continue;
    int a = 0, b = nr - 1;
    while (a < b) {
      const int mid = (a + b) >> 1;
      if (before(v, j, ks[mid], ki[mid])) b = mid;
      else a = mid + 1;
    }
    atomicSub(&hist[a], 1);
  }
  __syncthreads();

  // ---- 3. ranks: the inclusive prefix sum of hist, P / 64 consecutive entries per lane
  if (wave == 0) {
    const int per = P / 64;
    const int base = lane * per;
    int s = 0;
    for (int t = 0; t < per; ++t) s += hist[base + t];
    int inc = s;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int up = __shfl_up(inc, o);
      if (lane >= o) inc += up;
    }
    int run = inc - s;  // the lanes below
    for (int t = 0; t < per; ++t) {
      run += hist[base + t];
      hist[base + t] = run;
    }
  }
  __syncthreads();
  for (int e = threadIdx.x; e < n; e += NT) {
    const int id = t_col[t0 + e];
    if ((unsigned)id >= (unsigned)n_cols) continue;
    const double v = out_val[t0 + e];  // (this thread's own store of step 1)
    if (!(v > neg_inf<double>())) continue;
    // the first key that is not before (v, id): the target's own, unless it is excluded
    int a = 0, b = nr;
    while (a < b) {
      const int mid = (a + b) >> 1;
      if (before(ks[mid], ki[mid], v, id)) a = mid + 1;
      else b = mid;
    }
    if (a < nr && ks[a] == v && ki[a] == id) out_rank[t0 + e] = hist[a];
  }
}

struct RankArgs {
  const double *F;
  int64_t ldf, n_f_rows, n_cols;
  const float *eu, *ei;
  int dim;
  const int64_t *ex_rowptr;
  const int32_t *ex_col;
  int excl_mode;
  int64_t n_krows;
  const int64_t *krow_f, *t_rowptr;
  const int32_t *t_col;
  int64_t *out_rank;
  double *out_val;
  hipStream_t s;
};

template <int NW>
void launch_rows_rank_nw(const RankArgs &a) {
  auto kern = k_rows_rank<0, NW>;
  switch (a.eu ? a.dim : 0) {
    case 0: break;
    case 32: kern = k_rows_rank<32, NW>; break;
    case 64: kern = k_rows_rank<64, NW>; break;
    default: kern = k_rows_rank<128, NW>; break;
  }
  kern<<<dim3((unsigned)a.n_krows), dim3(64 * NW), 0, a.s>>>(
      a.F, a.ldf, a.n_f_rows, a.n_cols, a.eu, a.ei, a.ex_rowptr, a.ex_col, a.excl_mode,
      a.krow_f, a.t_rowptr, a.t_col, a.out_rank, a.out_val);
}

}  // namespace
}  // namespace lg

using namespace lg;

extern "C" int lg_rows_rank_f64(const double *F, int64_t ldf, int64_t n_f_rows, int64_t n_cols,
                                const float *eu, const float *ei, int32_t dim,
                                const int64_t *ex_rowptr, const int32_t *ex_col,
                                int32_t excl_mode, int64_t n_krows, const int64_t *krow_f,
                                const int64_t *t_rowptr, const int32_t *t_col,
                                int64_t *out_rank, double *out_val, lg_stream_t stream) {
  const char *who = "lg_rows_rank_f64";
  LG_REQUIRE(F && krow_f && t_rowptr && t_col && out_rank && out_val, "%s: null argument", who);
  LG_REQUIRE(n_f_rows >= 0 && n_cols >= 0 && ldf >= n_cols && n_cols < 0x7fffffff,
             "%s: bad sizes (n_f_rows %lld, n_cols %lld, ldf %lld)", who, (long long)n_f_rows,
             (long long)n_cols, (long long)ldf);
  LG_REQUIRE(n_krows >= 0 && n_krows < 0x7fffffff, "%s: n_krows %lld not in [0, 2^31-1)", who,
             (long long)n_krows);
  LG_REQUIRE(!eu == !ei, "%s: eu/ei must both be set or both NULL", who);
  LG_REQUIRE(!eu || dim == 32 || dim == 64 || dim == 128, "%s: dim %d not in {32,64,128}", who,
             dim);
  LG_REQUIRE(excl_mode == LG_EXCL_DROP || excl_mode == LG_EXCL_NONE, "%s: bad excl_mode %d",
             who, excl_mode);
  LG_REQUIRE(!ex_rowptr == !ex_col, "%s: ex_rowptr/ex_col must both be set", who);
  LG_REQUIRE(!(eu && excl_mode == LG_EXCL_NONE && ex_rowptr),
             "%s: a G factor with exclusions requires LG_EXCL_DROP", who);
  if (n_krows == 0) return LG_OK;
  const RankArgs a{F, ldf, n_f_rows, n_cols, eu, ei, dim, ex_rowptr, ex_col, excl_mode,
                   n_krows, krow_f, t_rowptr, t_col, out_rank, out_val, (hipStream_t)stream};
  if (n_cols >= kRankSplitCols) launch_rows_rank_nw<8>(a);
  else launch_rows_rank_nw<1>(a);
  return launch_status(who);
}
