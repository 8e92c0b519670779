// K3r: hybrid spreading for item baskets that are not rows of A -- a new visitor's cart, a
// session, "related to this item" -- in two sweeps of the interaction lists, gfx950.
//
// Reference (model/SpreadMethod/model.py): getSpreadingGeneralMat :14-27, HybridS :63-85 and
// getResource :88-99 give F = B @ (general_W / den) for any 0/1 row B over the items, a user of
// A or not. With ra_i = 1/k_i^(1-l), rb_j = 1/k_j^l (lg_hybrid_recip_f64) and inv_v = fl(1/k_v)
// (lg_inv_degree_f64) the sum regroups as
//     T[v] = inv_v * sum_{i in items(v), i in B} ra_i        pass 1: one sweep of A by user
//     F[j] = rb_j  * sum_{v in users(j)}         T[v]        pass 2: one sweep of A by item
// with no I x I object and no tile: 4 nnz bytes of ids per pass for a whole block of baskets,
// whatever the catalog size.
//
// A block is at most LG_SPREAD_ROWS_BLOCK = 64 baskets: one wave sweeps one list, 64 positions
// per step, and LANE b OWNS BASKET b. Pass 1 turns the block's baskets (a CSR) into one 64-bit
// word per item, bit b = "item in basket b" (integer atomic OR); a lane gathers the word of its
// position's item, and only where a ballot finds a non-zero word does the wave visit the hit
// positions, ascending, one at a time: the hit's word and ra are broadcast and lane b adds ra
// iff bit b is set. Pass 2 does the same over users(j) with the users' mark words (bit b =
// "T[v, b] != 0", written by pass 1) and lane b's load of T[v, b].
//
// THE ORDER OF EVERY SUM is therefore a function of the one list alone: the terms of basket b
// are added one by one in ascending position, into a sum that starts at +0.0. A list longer
// than LG_SPREAD_ROWS_SEG = 4096 positions is cut at multiples of 4096 (one wave, "unit", per
// segment, so that a hub item's 10^5-10^6 users do not serialise one wave); every segment is
// summed as above from +0.0 and the partial sums are added in segment order by one lane.
// Nothing depends on the grid, the CU count, the block's other baskets (another basket's hit
// adds nothing to lane b), where the basket sits in the call (bit b only names the lane) or
// timing. There is no floating-point atomic, global or LDS. Users whose T row is zero are
// skipped BY TEST (their mark word is 0), never by compacting positions: adding +0.0 to a
// non-negative sum is exact, so the skip leaves every bit as it is.
//
// T is dense, [n_users, n_baskets] fp64, but only its non-zero entries are ever written or
// read: pass 1 writes T[v, b] iff bit b of v's mark word is set and pass 2 reads under the
// same test, so T needs no clearing and the traffic is that of the marked users' lines only.
//
// Which lists are long is the caller's table (long_ids ascending list ids, long_ptr the
// exclusive prefix sum of their segment counts): it depends on A alone and is built once.
#include "common.h"

namespace lg {
namespace {

constexpr int kSeg = LG_SPREAD_ROWS_SEG;
constexpr int kBlk = LG_SPREAD_ROWS_BLOCK;
static_assert(kBlk == 64, "lane b owns basket b: one wave");
static_assert(kSeg % 64 == 0, "segments are whole steps");
constexpr int kWaves = 4;         // per workgroup
constexpr int kWaveLists = 4;     // consecutive lists per wave
constexpr int kTile = kWaves * kWaveLists;  // lists per workgroup: pass 2 writes 128-byte runs
constexpr int kUnits = 4;         // long-list segments per workgroup, one wave each

__device__ __forceinline__ uint64_t read_lane(uint64_t x, int l) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)x, l);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(x >> 32), l);
  return ((uint64_t)hi << 32) | lo;
}
__device__ __forceinline__ double read_lane(double x, int l) {
  return __longlong_as_double((long long)read_lane((uint64_t)__double_as_longlong(x), l));
}

// Pass 1 over positions [p0, p1) of one user's items: this lane's basket's sum of ra, the
// terms in ascending position from +0.0.
__device__ __forceinline__ double weight_segment(const int32_t *__restrict__ items, int64_t p0,
                                                 int64_t p1, const uint64_t *__restrict__ mask,
                                                 const double *__restrict__ ra,
                                                 int64_t n_items) {
  const int lane = lane_id();
  double acc = 0.0;
  for (int64_t p = p0; p < p1; p += 64) {
    const int64_t q = p + lane;
    uint64_t m = 0;
    double r = 0.0;
    if (q < p1) {
      const int32_t i = items[q];
      if ((uint32_t)i < (uint64_t)n_items) {
        m = mask[i];
        if (m) r = ra[i];
      }
    }
    uint64_t hits = __ballot(m != 0);
    while (hits) {  // (wave-uniform) the hit positions, ascending
      const int l = __ffsll((unsigned long long)hits) - 1;
      hits &= hits - 1;
      const uint64_t ml = read_lane(m, l);
      const double rl = read_lane(r, l);
      if ((ml >> lane) & 1) acc += rl;
    }
  }
  return acc;
}

// Pass 2 over positions [p0, p1) of one item's users: this lane's basket's sum of T[v, lane],
// the terms in ascending position from +0.0; users without a mark are skipped by test. The
// loads of up to four hits are issued together, the adds follow in position order.
__device__ __forceinline__ double resource_segment(const int32_t *__restrict__ users, int64_t p0,
                                                   int64_t p1, const uint64_t *__restrict__ umask,
                                                   const double *__restrict__ T, int nb,
                                                   int64_t n_users) {
  const int lane = lane_id();
  double acc = 0.0;
  for (int64_t p = p0; p < p1; p += 64) {
    const int64_t q = p + lane;
    uint64_t m = 0;
    int32_t v = 0;
    if (q < p1) {
      v = users[q];
      if ((uint32_t)v < (uint64_t)n_users) m = umask[v];
    }
    uint64_t hits = __ballot(m != 0);
    while (hits) {  // (wave-uniform)
      bool mine[4];
      double t[4];
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        mine[g] = false;
        t[g] = 0.0;
        if (hits) {
          const int l = __ffsll((unsigned long long)hits) - 1;
          hits &= hits - 1;
          const uint64_t ml = read_lane(m, l);
          const int64_t vl = __builtin_amdgcn_readlane(v, l);
          // (a mark bit at or above nb has no T entry: never read)
          mine[g] = ((ml >> lane) & 1) && lane < nb;
          if (mine[g]) t[g] = T[vl * nb + lane];
        }
      }
#pragma unroll
      for (int g = 0; g < 4; ++g)
        if (mine[g]) acc += t[g];
    }
  }
  return acc;
}

__global__ __launch_bounds__(256) void k_rows_clear(uint64_t *__restrict__ mask, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) mask[i] = 0;
}

// bit b of mask[i] for every item i of basket b (an id outside the catalog is skipped, an item
// named twice sets its bit twice)
__global__ __launch_bounds__(256) void k_rows_mask(const int64_t *__restrict__ b_rowptr,
                                                   const int32_t *__restrict__ b_col, int nb,
                                                   int64_t n_items, uint64_t *__restrict__ mask) {
  const int b = blockIdx.y;
  if (b >= nb) return;
  const int64_t p0 = b_rowptr[b], p1 = b_rowptr[b + 1];
  for (int64_t p = p0 + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < p1;
       p += (int64_t)gridDim.x * blockDim.x) {
    const int32_t i = b_col[p];
    if ((uint32_t)i < (uint64_t)n_items)
      atomicOr((unsigned long long *)&mask[i], 1ull << b);
  }
}

// Pass 1, the users of at most kSeg items: T[v, b] where it is not zero, and v's mark word.
__global__ __launch_bounds__(64 * kWaves) void k_rows_weight(
    const int64_t *__restrict__ user_rowptr, const int32_t *__restrict__ user_items,
    int64_t n_users, int64_t n_items, const double *__restrict__ ra,
    const double *__restrict__ inv_ku, const uint64_t *__restrict__ mask, int nb,
    double *__restrict__ T, uint64_t *__restrict__ umask) {
  const int wave = threadIdx.x / 64, lane = lane_id();
  const int64_t v0 = ((int64_t)blockIdx.x * kWaves + wave) * kWaveLists;
  for (int t = 0; t < kWaveLists; ++t) {
    const int64_t v = v0 + t;
    if (v >= n_users) break;  // (wave-uniform)
    const int64_t pb = user_rowptr[v], pe = user_rowptr[v + 1];
    if (pe - pb > kSeg) {
      // a long list: k_rows_unit / k_rows_weight_long, later in stream order, write its T row
      // and mark word; one the caller's table omits stays unmarked (a zero T row)
      if (lane == 0) umask[v] = 0;
      continue;
    }
    const double acc = weight_segment(user_items, pb, pe, mask, ra, n_items);
    const uint64_t um = __ballot(acc != 0.0);
    if (acc != 0.0 && lane < nb) T[v * nb + lane] = inv_ku[v] * acc;
    if (lane == 0) umask[v] = um;
  }
}

// One segment of a long list per wave: part[unit, lane] = the segment's sum (zeros included).
template <bool RES>
__global__ __launch_bounds__(64 * kUnits) void k_rows_unit(
    const int64_t *__restrict__ rowptr, const int32_t *__restrict__ col, int64_t n_lists,
    int64_t n_other, const int32_t *__restrict__ long_ids, const int64_t *__restrict__ long_ptr,
    int64_t n_long, int64_t n_units, const uint64_t *__restrict__ mask,
    const double *__restrict__ x, int nb, double *__restrict__ part) {
  const int wave = threadIdx.x / 64, lane = lane_id();
  const int64_t unit = (int64_t)blockIdx.x * kUnits + wave;
  if (unit >= n_units) return;
  int64_t lo = 0, hi = n_long;  // the last q with long_ptr[q] <= unit
  while (hi - lo > 1) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (long_ptr[mid] <= unit) lo = mid;
    else hi = mid;
  }
  const int64_t id = long_ids[lo], seg = unit - long_ptr[lo];
  double acc = 0.0;
  if (id >= 0 && id < n_lists && seg >= 0) {
    const int64_t pb = rowptr[id], pe = rowptr[id + 1];
    const int64_t p0 = pb + seg * kSeg;
    const int64_t p1 = pe - p0 > kSeg ? p0 + kSeg : pe;
    if (p0 < p1) {
      if (RES) acc = resource_segment(col, p0, p1, mask, x, nb, n_other);
      else acc = weight_segment(col, p0, p1, mask, x, n_other);
    }
  }
  part[unit * 64 + lane] = acc;
}

// The partial sums of long list q in segment order, one wave per list, lane b = basket b.
__device__ __forceinline__ double long_sum(const double *__restrict__ part,
                                           const int64_t *__restrict__ long_ptr, int64_t q) {
  const int lane = lane_id();
  const int64_t u0 = long_ptr[q], u1 = long_ptr[q + 1];
  double s = 0.0;
  for (int64_t u = u0; u < u1; ++u) s += part[u * 64 + lane];
  return s;
}

__global__ __launch_bounds__(64 * kUnits) void k_rows_weight_long(
    const int32_t *__restrict__ long_ids, const int64_t *__restrict__ long_ptr, int64_t n_long,
    int64_t n_users, const double *__restrict__ part, const double *__restrict__ inv_ku, int nb,
    double *__restrict__ T, uint64_t *__restrict__ umask) {
  const int lane = lane_id();
  const int64_t q = (int64_t)blockIdx.x * kUnits + threadIdx.x / 64;
  if (q >= n_long) return;
  const int64_t v = long_ids[q];
  if (v < 0 || v >= n_users) return;
  const double acc = long_sum(part, long_ptr, q);
  const uint64_t um = __ballot(acc != 0.0);
  if (acc != 0.0 && lane < nb) T[v * nb + lane] = inv_ku[v] * acc;
  if (lane == 0) umask[v] = um;
}

__global__ __launch_bounds__(64 * kUnits) void k_rows_resource_long(
    const int32_t *__restrict__ long_ids, const int64_t *__restrict__ long_ptr, int64_t n_long,
    int64_t n_items, const double *__restrict__ part, const double *__restrict__ rb, int nb,
    double *__restrict__ F, int64_t ldf) {
  const int lane = lane_id();
  const int64_t q = (int64_t)blockIdx.x * kUnits + threadIdx.x / 64;
  if (q >= n_long) return;
  const int64_t j = long_ids[q];
  if (j < 0 || j >= n_items) return;
  const double acc = long_sum(part, long_ptr, q);
  if (lane < nb) F[lane * ldf + j] = rb[j] * acc;
}

// Pass 2, the items of at most kSeg users: kTile consecutive columns per workgroup, staged in
// LDS so that every basket row of F gets one 128-byte run.
__global__ __launch_bounds__(64 * kWaves) void k_rows_resource(
    const int64_t *__restrict__ item_rowptr, const int32_t *__restrict__ item_users,
    int64_t n_items, int64_t n_users, const uint64_t *__restrict__ umask,
    const double *__restrict__ T, const double *__restrict__ rb, int nb, double *__restrict__ F,
    int64_t ldf) {
  __shared__ double tile[kTile][65];
  __shared__ int skip[kTile];
  const int wave = threadIdx.x / 64, lane = lane_id();
  const int64_t j0 = (int64_t)blockIdx.x * kTile;
  for (int t = 0; t < kWaveLists; ++t) {
    const int jl = wave * kWaveLists + t;
    const int64_t j = j0 + jl;
    double val = 0.0;
    bool s = true;  // outside the catalog, or a long list (k_rows_resource_long writes it)
    if (j < n_items) {
      const int64_t pb = item_rowptr[j], pe = item_rowptr[j + 1];
      if (pe - pb <= kSeg) {
        val = rb[j] * resource_segment(item_users, pb, pe, umask, T, nb, n_users);
        s = false;
      }
    }
    tile[jl][lane] = val;
    if (lane == 0) skip[jl] = s;
  }
  __syncthreads();
  const int jl = threadIdx.x % kTile;
  if (skip[jl]) return;
  for (int b = threadIdx.x / kTile; b < nb; b += 64 * kWaves / kTile)
    F[b * ldf + j0 + jl] = tile[jl][b];
}

bool long_table_ok(const char *who, const int32_t *long_ids, const int64_t *long_ptr,
                   int64_t n_long, int64_t n_long_units) {
  if (n_long < 0 || n_long_units < 0 || n_long >= 0x7fffffff || n_long_units >= 0x7fffffff ||
      (n_long == 0) != (n_long_units == 0) || n_long_units < n_long) {
    set_error("%s: bad long-list table sizes (n_long %lld, n_long_units %lld)", who,
              (long long)n_long, (long long)n_long_units);
    return false;
  }
  if (n_long > 0 && (!long_ids || !long_ptr)) {
    set_error("%s: null long_ids / long_ptr with n_long %lld", who, (long long)n_long);
    return false;
  }
  return true;
}

}  // namespace
}  // namespace lg

using namespace lg;

extern "C" size_t lg_spread_rows_weight_ws_bytes(int64_t n_items, int64_t n_long_units) {
  return (size_t)(n_items > 0 ? n_items : 0) * sizeof(uint64_t) +
         (size_t)(n_long_units > 0 ? n_long_units : 0) * 64 * sizeof(double);
}

extern "C" size_t lg_spread_rows_resource_ws_bytes(int64_t n_long_units) {
  return (size_t)(n_long_units > 0 ? n_long_units : 0) * 64 * sizeof(double);
}

extern "C" int lg_spread_rows_weight_f64(
    const int64_t *user_rowptr, const int32_t *user_items, int64_t n_users, int64_t n_items,
    const double *ra, const double *inv_ku, const int64_t *basket_rowptr,
    const int32_t *basket_items, int32_t n_baskets, const int32_t *long_ids,
    const int64_t *long_ptr, int64_t n_long, int64_t n_long_units, double *T,
    uint64_t *user_marks, void *ws, size_t ws_bytes, lg_stream_t stream) {
  const char *who = "lg_spread_rows_weight_f64";
  LG_REQUIRE(user_rowptr && user_items && ra && inv_ku && basket_rowptr && basket_items && T &&
                 user_marks,
             "%s: null argument", who);
  LG_REQUIRE(n_baskets >= 1 && n_baskets <= kBlk, "%s: n_baskets %d not in [1, %d]", who,
             n_baskets, kBlk);
  LG_REQUIRE(n_users >= 0 && n_items >= 0 && n_users < 0x7fffffff && n_items < 0x7fffffff,
             "%s: bad sizes (n_users %lld, n_items %lld)", who, (long long)n_users,
             (long long)n_items);
  if (!long_table_ok(who, long_ids, long_ptr, n_long, n_long_units)) return LG_ERR_ARG;
  const size_t need = lg_spread_rows_weight_ws_bytes(n_items, n_long_units);
  LG_REQUIRE(need == 0 || (ws && ws_bytes >= need), "%s: ws_bytes %zu < %zu (or ws null)", who,
             ws_bytes, need);
  if (n_users == 0) return LG_OK;
  hipStream_t s = (hipStream_t)stream;
  uint64_t *mask = (uint64_t *)ws;
  double *part = (double *)(mask + n_items);
  if (n_items > 0) {
    k_rows_clear<<<dim3((unsigned)((n_items + 255) / 256)), dim3(256), 0, s>>>(mask, n_items);
    k_rows_mask<<<dim3(8, (unsigned)n_baskets), dim3(256), 0, s>>>(basket_rowptr, basket_items,
                                                                    n_baskets, n_items, mask);
  }
  const int64_t per = (int64_t)kWaves * kWaveLists;
  k_rows_weight<<<dim3((unsigned)((n_users + per - 1) / per)), dim3(64 * kWaves), 0, s>>>(
      user_rowptr, user_items, n_users, n_items, ra, inv_ku, mask, n_baskets, T, user_marks);
  if (n_long > 0) {
    k_rows_unit<false><<<dim3((unsigned)((n_long_units + kUnits - 1) / kUnits)),
                         dim3(64 * kUnits), 0, s>>>(user_rowptr, user_items, n_users, n_items,
                                                    long_ids, long_ptr, n_long, n_long_units,
                                                    mask, ra, n_baskets, part);
    k_rows_weight_long<<<dim3((unsigned)((n_long + kUnits - 1) / kUnits)), dim3(64 * kUnits), 0,
                         s>>>(long_ids, long_ptr, n_long, n_users, part, inv_ku, n_baskets, T,
                              user_marks);
  }
  return launch_status(who);
}

extern "C" int lg_spread_rows_resource_f64(
    const int64_t *item_rowptr, const int32_t *item_users, int64_t n_items, int64_t n_users,
    const double *T, const uint64_t *user_marks, const double *rb, int32_t n_baskets,
    const int32_t *long_ids, const int64_t *long_ptr, int64_t n_long, int64_t n_long_units,
    double *F, int64_t ldf, void *ws, size_t ws_bytes, lg_stream_t stream) {
  const char *who = "lg_spread_rows_resource_f64";
  LG_REQUIRE(item_rowptr && item_users && T && user_marks && rb && F, "%s: null argument", who);
  LG_REQUIRE(n_baskets >= 1 && n_baskets <= kBlk, "%s: n_baskets %d not in [1, %d]", who,
             n_baskets, kBlk);
  LG_REQUIRE(n_users >= 0 && n_items >= 0 && n_users < 0x7fffffff && n_items < 0x7fffffff,
             "%s: bad sizes (n_users %lld, n_items %lld)", who, (long long)n_users,
             (long long)n_items);
  LG_REQUIRE(ldf >= n_items, "%s: ldf %lld < n_items %lld", who, (long long)ldf,
             (long long)n_items);
  if (!long_table_ok(who, long_ids, long_ptr, n_long, n_long_units)) return LG_ERR_ARG;
  const size_t need = lg_spread_rows_resource_ws_bytes(n_long_units);
  LG_REQUIRE(need == 0 || (ws && ws_bytes >= need), "%s: ws_bytes %zu < %zu (or ws null)", who,
             ws_bytes, need);
  if (n_items == 0) return LG_OK;
  hipStream_t s = (hipStream_t)stream;
  double *part = (double *)ws;
  k_rows_resource<<<dim3((unsigned)((n_items + kTile - 1) / kTile)), dim3(64 * kWaves), 0, s>>>(
      item_rowptr, item_users, n_items, n_users, user_marks, T, rb, n_baskets, F, ldf);
  if (n_long > 0) {
    k_rows_unit<true><<<dim3((unsigned)((n_long_units + kUnits - 1) / kUnits)),
                        dim3(64 * kUnits), 0, s>>>(item_rowptr, item_users, n_items, n_users,
                                                   long_ids, long_ptr, n_long, n_long_units,
                                                   user_marks, T, n_baskets, part);
    k_rows_resource_long<<<dim3((unsigned)((n_long + kUnits - 1) / kUnits)), dim3(64 * kUnits),
                           0, s>>>(long_ids, long_ptr, n_long, n_items, part, rb, n_baskets, F,
                                   ldf);
  }
  return launch_status(who);
}
