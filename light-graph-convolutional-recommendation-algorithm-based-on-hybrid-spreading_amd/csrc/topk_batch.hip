// K2b: full-catalog scoring + exclusion mask + top-K for a short list of users (<= 64 ids
// into the full tables), gfx950 f32 MFMA.
//
// The request form of model/LightGCN/recommend.py:83-114: the same score, mask and top-k as
// K2 (csrc/topk_plain.hip), for the rows user_ids[0 .. n_batch) of users_emb only. Row b of the
// output is lg_score_topk_f32's row user_ids[b] bit for bit: the score is k_score_topk's
// chain (v_mfma_f32_16x16x4_f32, D/4 dependent steps from a zero accumulator, lane l = item
// row l & 15 as A, user column l & 15 as B, k-slot l >> 4), admission is strict (NaN and -inf
// never rank), an excluded item takes mask_value when its list is compacted, the order is
// (score desc, item asc), the padding {-inf, -1}.
//
// Shape of the work. K2 gives every wave its own users and streams the whole catalog (or one of
// <= 64 splits) past them; with a handful of users that is a handful of waves. Here every wave
// holds ALL the users of the request (NG <= 4 groups of 16, the B fragments) and the ITEMS are
// divided over every wave of a grid that fills the device: wave w of the grid scores the items
// [w ipw, (w + 1) ipw). A wave keeps one candidate list per user in LDS (CAP = 64 M entries,
// M = 1 / 2 / 4 for k <= 32 / 64 / 128), exclusion applied lazily at compaction exactly as in
// k_score_topk (the exclusion CSR is the full table's, indexed by the user id; the routine, the
// loads, the filter and the threshold rule are the one text of score_stream.h). At the end the
// waves of a workgroup merge their lists pairwise in LDS (a tree: log2(WAVES) steps), so the
// workspace holds one sorted partial list per (workgroup, user); k_topk_batch_merge then
// merges a user's R partial lists with 16 waves, each taking every 16th list, and the same
// tree over the waves. Every list order is total (item ids are distinct), so the result does
// not depend on how the items were divided.
//
// The host side behind the stream is shared with K2i (csrc/topk_items.hip) through
// batch_lists.h: the grid plan, the workspace bound and split, the argument checks. This file
// holds the one definition of k_topk_batch_merge, of its launcher launch_batch_merge and of
// device_cus. The workgroup tail of the scoring kernel (the pairwise tree and the store) is
// the same text in both kernels: as one inlined function it kept every register count but
// not hipcc's instruction stream, and missed the timing rule (CHANGELOG.md).
//
// LDS per workgroup: WAVES NG M x 8 KiB of lists; WAVES = min(4, 16 / (NG M)) keeps that within
// 128 KiB (one workgroup per CU at NG M = 16, two where the lists take <= 64 KiB).
#include "batch_lists.h"
#include "score_stream.h"

namespace lg {
namespace {

constexpr int kBatchMax = 64;  // users per call

// One wave: all the request's users (NG groups of 16; slot b = 16 g + (lane & 15) is row b of
// the request), the items [w ipw, (w + 1) ipw) of the catalog, w = the wave's index in the grid.
// The loop is k_score_topk's software pipeline: MFMAs of tile t + 1 interleaved with the
// one-max-one-compare filter of tile t, loads two to three tiles ahead, all compiler-visible.
template <int D, int NG, int M, int WAVES>
__global__ __launch_bounds__(64 * WAVES) void k_score_topk_batch(
    const float *__restrict__ eu, const float *__restrict__ ei,
    const int64_t *__restrict__ user_ids, int n_batch, int64_t n_table_users, int64_t n_items,
    const int64_t *__restrict__ ex_rowptr, const int32_t *__restrict__ ex_col,
    float mask_value, int k, int64_t items_per_wave, float *__restrict__ out_val,
    int64_t *__restrict__ out_idx, float *__restrict__ part_val,
    int32_t *__restrict__ part_idx) {
  constexpr int Q = D / 4;
  constexpr int LT = Q / 4;  // buffer loads per tile per lane
  constexpr int CAP = 64 * M;
  constexpr int NU = 16 * NG;
  __shared__ float cs[WAVES][NU][CAP];
  __shared__ int ci[WAVES][NU][CAP];
  __shared__ int exs[WAVES][64];
  __shared__ int ncs[WAVES][NU];  // entries of each final list

  const int wave = threadIdx.x / 64;
  const int lane = lane_id();
  const int ul = lane & 15;
  const int gq = lane >> 4;
  // the wave's items (every wave stays to the end: the workgroup's barriers below)
  int64_t i0 = ((int64_t)blockIdx.x * WAVES + wave) * items_per_wave;
  if (i0 > n_items) i0 = n_items;
  int64_t i1 = i0 + items_per_wave;
  if (i1 > n_items) i1 = n_items;
  const int n_valid = (int)(i1 - i0);   // items of this wave
  const int n_t = (n_valid + 15) / 16;  // tiles of this wave

  float uf[NG][Q];
  bool uvalid[NG];
  int64_t ex_pos[NG], ex_hi[NG];
  int cnt[NG], chk[NG];
  float thr[NG];
#pragma unroll
  for (int g = 0; g < NG; ++g) {
    const int b = g * 16 + ul;
    // an id outside the table is clamped (row 0 is read instead) and its list stays empty
    int64_t u = 0;
    uvalid[g] = b < n_batch;
    if (uvalid[g]) {
      u = user_ids ? user_ids[b] : (int64_t)b;
      uvalid[g] = u >= 0 && u < n_table_users;
      if (!uvalid[g]) u = 0;
    }
    load_piece<Q>(eu + u * D + gq * Q, uf[g]);
    ex_pos[g] = 0;
    ex_hi[g] = 0;
    if (ex_rowptr && uvalid[g]) {
      ex_hi[g] = ex_rowptr[u + 1];
      // the user's first excluded item inside the wave's range
      ex_pos[g] = lower_bound_i32(ex_col, ex_rowptr[u], ex_hi[g], (int32_t)i0);
    }
    cnt[g] = 0;
    chk[g] = 0;
    thr[g] = uvalid[g] ? neg_inf<float>() : __builtin_huge_valf();
  }
  const uint64_t same_user = 0x0001000100010001ull << ul;

  // Compact user u of group g, all of whose items so far are below lim: the entries [chk, n)
  // added since its last compaction get the lazy exclusion (mask_excluded_run; ex_pos starts
  // at the user's first excluded item inside the wave's range), then the best k stay, sorted.
  auto compact_user = [&](int g, int u, int lim) __attribute__((always_inline)) {
    const int n = __shfl(cnt[g], u);
    const int c0 = __shfl(chk[g], u);
    int64_t pos = __shfl(ex_pos[g], u);
    const int64_t hi = __shfl(ex_hi[g], u);
    float *ks = &cs[wave][g * 16 + u][0];
    int *is = &ci[wave][g * 16 + u][0];
    pos = mask_excluded_run(
        ex_col, pos, hi, lim, exs, wave, c0, n, [&](int j) { return is[j]; },
        [&](int j) { ks[j] = mask_value; });
    float t;
    int tid;
    const int nc = wave_compact<float, M>(ks, is, n, k, t, tid);
    if (ul == u) {
      cnt[g] = nc;
      chk[g] = nc;
      ex_pos[g] = pos;
      thr[g] = entry_thr(uvalid[g], mask_value, t);
    }
  };

  // acc[g][r] = score(user slot 16g + ul, item i0 + 16t + 4gq + r)
  auto mfma_tile = [&](const f32x4(&af)[LT], f32x4 (&acc)[NG]) __attribute__((always_inline)) {
#pragma unroll
    for (int g = 0; g < NG; ++g) acc[g] = f32x4{0.f, 0.f, 0.f, 0.f};
    // s outer / g inner: NG independent accumulation chains interleave on the MFMA pipe
#pragma unroll
    for (int s = 0; s < Q; ++s)
#pragma unroll
      for (int g = 0; g < NG; ++g)
        acc[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[s / 4][s % 4], uf[g][s], acc[g], 0,
                                                      0, 0);
  };

  auto any_cand = [&](const f32x4 (&acc)[NG]) __attribute__((always_inline)) {
    bool any = false;
#pragma unroll
    for (int g = 0; g < NG; ++g) any |= above(max4(acc[g]), thr[g]);
    return __ballot(any) != 0;
  };

  // Slow path, taken when some lane of the wave has a candidate in tile t.
  auto insert_tile = [&](int t, const f32x4 (&acc)[NG]) __attribute__((always_inline)) {
    const int rel = t * 16 + gq * 4;
#pragma unroll
    for (int g = 0; g < NG; ++g) {
      if (__ballot(above(max4(acc[g]), thr[g])) == 0) continue;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float sc = acc[g][r];
        const bool cand = rel + r < n_valid && sc > thr[g];
        const uint64_t bal = __ballot(cand);
        if (bal) {
          const int pos = cnt[g] + __popcll(bal & same_user & lanemask_lt());
          if (cand) {
            cs[wave][g * 16 + ul][pos] = sc;
            ci[wave][g * 16 + ul][pos] = (int)i0 + rel + r;
          }
          cnt[g] += __popcll(bal & same_user);
        }
      }
    }
  };

  // compact every user whose list could overflow on the next tile (+16 max per tile)
  auto maybe_compact = [&](int lim) __attribute__((always_inline)) {
    bool over = false;
#pragma unroll
    for (int g = 0; g < NG; ++g) over |= cnt[g] > CAP - 16;
    if (__ballot(over) == 0) return;
#pragma unroll
    for (int g = 0; g < NG; ++g) {
      uint64_t need = __ballot(cnt[g] > CAP - 16) & 0xffffull;
      if (need) {
        wave_sync();
        while (need) {
          const int u = __ffsll((long long)need) - 1;
          need &= need - 1;
          compact_user(g, u, lim);
        }
      }
    }
  };

  const int voff = (ul * D + gq * Q) * 4;
  const int lim_end = (int)i1;
  auto step_lim = [&](int t) __attribute__((always_inline)) {
    const int l = (int)i0 + (t + 1) * 16;
    return l < lim_end ? l : lim_end;
  };
  // retire the prologue loads with a wait hipcc sees (vmcnt(0)), as k_score_topk does
  __builtin_amdgcn_s_waitcnt(0x0F70);
  if (n_t > 0) {
    f32x4 afA[LT], afB[LT];
    f32x4 accA[NG], accB[NG];
    load_item_tile<D, true>(ei, i1, i0, voff, afA);
    load_item_tile<D, true>(ei, i1, i0 + 16, voff, afB);
    mfma_tile(afA, accA);
    load_item_tile<D, true>(ei, i1, i0 + 32, voff, afA);
    // invariant at step t: acc[t%2] = tile t; buffer (t+1)%2 = tile t+1 (landed or in
    // flight); buffer t%2 = tile t+2 in flight
    for (int t = 0;; t += 2) {
      // ---- even step: tile t in accA, tile t+1 in afB
      mfma_tile(afB, accB);
      bool hit = any_cand(accA);
      load_item_tile<D, true>(ei, i1, i0 + (int64_t)(t + 3) * 16, voff, afB);
      if (hit) insert_tile(t, accA);
      maybe_compact(step_lim(t));
      if (t + 1 >= n_t) break;
      // ---- odd step: tile t+1 in accB, tile t+2 in afA
      mfma_tile(afA, accA);
      hit = any_cand(accB);
      load_item_tile<D, true>(ei, i1, i0 + (int64_t)(t + 4) * 16, voff, afA);
      if (hit) insert_tile(t + 1, accB);
      maybe_compact(step_lim(t + 1));
      if (t + 2 >= n_t) break;
    }
  }

  // the wave's final lists: the best k of each user, sorted, ncs entries
  wave_sync();
#pragma unroll
  for (int g = 0; g < NG; ++g) {
    for (int u = 0; u < 16; ++u) {
      const int b = g * 16 + u;
      if (b >= n_batch) break;
      compact_user(g, u, lim_end);
      const int nc = __shfl(cnt[g], u);
      if (lane == 0) ncs[wave][b] = nc;
    }
  }

  // the workgroup's waves merge pairwise in LDS: wave w takes wave w + s's lists behind its
  // own (n0 + n1 <= 2k <= CAP) and keeps the best k
  for (int s = 1; s < WAVES; s <<= 1) {
    __syncthreads();
    if ((wave & (2 * s - 1)) == 0 && wave + s < WAVES) {
      for (int b = 0; b < n_batch; ++b) {
        const int n0 = ncs[wave][b];
        const int n1 = ncs[wave + s][b];
        if (n1 == 0) continue;  // (wave-uniform)
        float *ks = &cs[wave][b][0];
        int *is = &ci[wave][b][0];
        for (int e = lane; e < n1; e += 64) {
          ks[n0 + e] = cs[wave + s][b][e];
          is[n0 + e] = ci[wave + s][b][e];
        }
        wave_sync();
        float t;
        int tid;
        const int nc = wave_compact<float, M>(ks, is, n0 + n1, k, t, tid);
        if (lane == 0) ncs[wave][b] = nc;
      }
    }
  }
  __syncthreads();
  // wave 0 holds the workgroup's lists; every wave writes a share of the users
  for (int b = wave; b < n_batch; b += WAVES) {
    const int nc = ncs[0][b];
    for (int e = lane; e < k; e += 64) {
      const float v = e < nc ? cs[0][b][e] : neg_inf<float>();
      const int id = e < nc ? ci[0][b][e] : -1;
      if (gridDim.x == 1) {
        out_val[(int64_t)b * k + e] = v;
        out_idx[(int64_t)b * k + e] = id;
      } else {
        const int64_t o = ((int64_t)blockIdx.x * n_batch + b) * k + e;
        part_val[o] = v;
        part_idx[o] = id;
      }
    }
  }
}

// Merge the R partial lists of user blockIdx.x (each sorted, at most k entries, padded with
// id -1): wave w of the 16 takes the lists w, w + 16, .. (k_topk_merge's loop: an entry
// enters only if it beats the wave's running k-th best), then the waves merge pairwise in LDS.
// R <= 16: one list per wave, the tree alone.
template <int M>
__global__ __launch_bounds__(64 * kMergeWaves) void k_topk_batch_merge(
    const float *__restrict__ part_val, const int32_t *__restrict__ part_idx, int n_batch,
    int k, int n_lists, float *__restrict__ out_val, int64_t *__restrict__ out_idx) {
  constexpr int CAP = 64 * M;
  __shared__ float cs[kMergeWaves][CAP];
  __shared__ int ci[kMergeWaves][CAP];
  __shared__ int ncs[kMergeWaves];
  const int wave = threadIdx.x / 64;
  const int lane = lane_id();
  const int b = blockIdx.x;
  int cnt = 0;
  float tau = neg_inf<float>();
  int tau_id = kPadId;
  for (int r = wave; r < n_lists; r += kMergeWaves) {
    const int64_t base = ((int64_t)r * n_batch + b) * k;
    for (int e0 = 0; e0 < k; e0 += 64) {
      const int e = e0 + lane;
      float v = neg_inf<float>();
      int id = -1;
      if (e < k) {
        v = part_val[base + e];
        id = part_idx[base + e];
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
        cnt = wave_compact<float, M>(cs[wave], ci[wave], cnt, k, tau, tau_id);
      }
    }
  }
  wave_sync();
  cnt = wave_compact<float, M>(cs[wave], ci[wave], cnt, k, tau, tau_id);
  if (lane == 0) ncs[wave] = cnt;
  for (int s = 1; s < kMergeWaves; s <<= 1) {
    __syncthreads();
    if ((wave & (2 * s - 1)) == 0) {
      const int n0 = ncs[wave];
      const int n1 = ncs[wave + s];
      if (n1 > 0) {  // (wave-uniform; n0 + n1 <= 2k <= CAP)
        for (int e = lane; e < n1; e += 64) {
          cs[wave][n0 + e] = cs[wave + s][e];
          ci[wave][n0 + e] = ci[wave + s][e];
        }
        wave_sync();
        const int nc = wave_compact<float, M>(cs[wave], ci[wave], n0 + n1, k, tau, tau_id);
        if (lane == 0) ncs[wave] = nc;
      }
    }
  }
  __syncthreads();
  const int nc = ncs[0];
  for (int e = threadIdx.x; e < k; e += 64 * kMergeWaves) {
    out_val[(int64_t)b * k + e] = e < nc ? cs[0][e] : neg_inf<float>();
    out_idx[(int64_t)b * k + e] = e < nc ? ci[0][e] : -1;
  }
}

int batch_groups(int64_t n_batch) { return n_batch <= 16 ? 1 : (n_batch <= 32 ? 2 : 4); }
// waves per workgroup: the lists (NG M x 8 KiB per wave) within 128 KiB
int batch_waves(int ng, int m) { return ng * m >= 16 ? 1 : (ng * m >= 8 ? 2 : 4); }

template <int D, int NG, int M>
void launch_batch(int blocks, const float *eu, const float *ei, const int64_t *user_ids,
                  int n_batch, int64_t n_table_users, int64_t n_items,
                  const int64_t *ex_rowptr, const int32_t *ex_col, float mask_value, int k,
                  int64_t ipw, float *out_val, int64_t *out_idx, float *part_val,
                  int32_t *part_idx, hipStream_t stream) {
  constexpr int WAVES = NG * M >= 16 ? 1 : (NG * M >= 8 ? 2 : 4);
  k_score_topk_batch<D, NG, M, WAVES><<<dim3((unsigned)blocks), dim3(64 * WAVES), 0, stream>>>(
      eu, ei, user_ids, n_batch, n_table_users, n_items, ex_rowptr, ex_col, mask_value, k, ipw,
      out_val, out_idx, part_val, part_idx);
}

template <int D>
void dispatch_batch(int ng, int m, int blocks, const float *eu, const float *ei,
                    const int64_t *user_ids, int n_batch, int64_t n_table_users,
                    int64_t n_items, const int64_t *ex_rowptr, const int32_t *ex_col,
                    float mask_value, int k, int64_t ipw, float *out_val, int64_t *out_idx,
                    float *part_val, int32_t *part_idx, hipStream_t stream) {
#define LG_BATCH_CASE(NG, MM)                                                                 \
  if (ng == NG && m == MM)                                                                    \
    return launch_batch<D, NG, MM>(blocks, eu, ei, user_ids, n_batch, n_table_users, n_items, \
                                   ex_rowptr, ex_col, mask_value, k, ipw, out_val, out_idx,   \
                                   part_val, part_idx, stream);
  LG_BATCH_CASE(1, 1) LG_BATCH_CASE(1, 2) LG_BATCH_CASE(1, 4)
  LG_BATCH_CASE(2, 1) LG_BATCH_CASE(2, 2) LG_BATCH_CASE(2, 4)
  LG_BATCH_CASE(4, 1) LG_BATCH_CASE(4, 2) LG_BATCH_CASE(4, 4)
#undef LG_BATCH_CASE
}

}  // namespace
}  // namespace lg

using namespace lg;

extern "C" size_t lg_score_topk_batch_ws_bytes(int64_t n_batch, int64_t n_items, int32_t dim,
                                               int32_t k) {
  if (n_batch < 1 || n_batch > kBatchMax || n_items < 1 || n_items >= 0x7fffffff || k < 1 ||
      k > 128 || !(dim == 32 || dim == 64 || dim == 128))
    return 0;
  return list_ws_bytes(n_items, n_batch, k);
}

extern "C" int lg_score_topk_batch_f32(const float *eu, const float *ei, const int64_t *user_ids,
                                       int64_t n_batch, int64_t n_table_users, int64_t n_items,
                                       int32_t dim, const int64_t *ex_rowptr,
                                       const int32_t *ex_col, float mask_value, int32_t k,
                                       float *out_val, int64_t *out_idx, void *ws,
                                       size_t ws_bytes, lg_stream_t stream) {
  const char *me = "lg_score_topk_batch_f32";
  const int st0 = check_list_args(me, eu && ei && out_val && out_idx, n_batch, kBatchMax,
                                  n_table_users, n_items, dim, k, ex_rowptr, ex_col, ws, ws_bytes,
                                  lg_score_topk_batch_ws_bytes(n_batch, n_items, dim, k));
  if (st0 != LG_OK) return st0;
  const int cus = device_cus();
  if (cus <= 0) {
    set_error("%s: no device", me);
    return LG_ERR_ARG;
  }
  const int ng = batch_groups(n_batch), m = list_cap_m(k), waves = batch_waves(ng, m);
  const ListGrid grid = plan_list_grid(n_items, cus, waves, waves * ng * m);
  const int64_t blocks = grid.blocks, ipw = grid.per_wave;
  const ListParts part = split_list_ws(ws, blocks, n_batch, k);
  hipStream_t s = (hipStream_t)stream;
  switch (dim) {
    case 32: dispatch_batch<32>(ng, m, (int)blocks, eu, ei, user_ids, (int)n_batch, n_table_users, n_items, ex_rowptr, ex_col, mask_value, k, ipw, out_val, out_idx, part.val, part.idx, s); break;
    case 64: dispatch_batch<64>(ng, m, (int)blocks, eu, ei, user_ids, (int)n_batch, n_table_users, n_items, ex_rowptr, ex_col, mask_value, k, ipw, out_val, out_idx, part.val, part.idx, s); break;
    default: dispatch_batch<128>(ng, m, (int)blocks, eu, ei, user_ids, (int)n_batch, n_table_users, n_items, ex_rowptr, ex_col, mask_value, k, ipw, out_val, out_idx, part.val, part.idx, s); break;
  }
  const int st = launch_status(me);
  if (st != LG_OK || blocks == 1) return st;
  return launch_batch_merge(part.val, part.idx, (int)n_batch, k, (int)blocks, out_val, out_idx, s,
                            "lg_score_topk_batch_f32(merge)");
}

namespace lg {

// (behind the entry: the kernels are emitted in the order of their first launch in this file)
int device_cus() {
  static int cus[64];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 0;
  if (cus[dev] == 0) {
    int n = 0;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
      return 0;
    cus[dev] = n;
  }
  return cus[dev];
}

int launch_batch_merge(const float *part_val, const int32_t *part_idx, int n_batch, int k,
                       int n_lists, float *out_val, int64_t *out_idx, hipStream_t s,
                       const char *what) {
  if (k <= 64)
    k_topk_batch_merge<2><<<dim3((unsigned)n_batch), dim3(64 * kMergeWaves), 0, s>>>(
        part_val, part_idx, n_batch, k, n_lists, out_val, out_idx);
  else
    k_topk_batch_merge<4><<<dim3((unsigned)n_batch), dim3(64 * kMergeWaves), 0, s>>>(
        part_val, part_idx, n_batch, k, n_lists, out_val, out_idx);
  return launch_status(what);
}

}  // namespace lg
