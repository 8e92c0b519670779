// K2w: full-catalog scoring + exclusion mask + streaming top-K for every k <= 1024, gfx950
// f32 MFMA. The wide twin of K2 (csrc/topk_plain.hip, k <= 128).
//
// Replaces model/LightGCN/recommend.py:83-114 (identical in LightGCNOpti/recommend.py and
// LightGCN/evaluation.py:31-51) for any RECOMMEND["k"] up to 1024:
//     score = torch.matmul(users_emb.weight, items_emb.weight.T)       # [U, I] fp32
//     score[train positives] = -(1 << 10); score[val positives] = -(1 << 10)
//     _, recommendations = torch.topk(score, k)
//
// The score, the software pipeline, the one-max-one-compare filter and the admission rule are
// k_score_topk's (see the head of topk_plain.hip; the loads, the filter, the threshold rule and the
// lazy exclusion are the one text of score_stream.h): 16 users per wave as MFMA B fragments,
// 16-item tiles as A fragments through raw buffer loads, the v_mfma_f32_16x16x4_f32 chain
//     acc = 0; for s < Q: for g < 4: acc = fmaf(u[g*Q+s], i[g*Q+s], acc),
// and a score enters a user's list on sc > thr, thr = the running k-th value (-inf while
// mask_value would itself enter, +inf for padding users). NaN and -inf never rank.
//
// What differs is where the lists live. K2 keeps CAP <= 256 entries per user in LDS; 16 users
// per wave at CAP = 2048 would be 256 KiB. Here each (split, user) owns a slab of CAP = 64 M
// 8-byte entries {float score, int32 item} in the caller's workspace (M = 8 / 16 / 32 for
// k <= 256 / 512 / 1024). A candidate lane stores its entry straight to
// slab[cnt + its rank among the user's candidates of the ballot]. A user whose count passes
// CAP - 16 is compacted by its wave: the slab is loaded into a per-wave LDS scratch of CAP
// entries, the entries added since the last compaction get the lazy exclusion (K2's cursor
// over the sorted exclusion row, 64 excluded ids at a time, binary-searched; an excluded
// entry takes mask_value), a looped bitonic sort orders the scratch by (score desc, item
// asc), and the best k go back to the slab sorted; tau / thr come from entry k - 1.
//
// Store-to-load visibility inside the wave: the slab is written by plain vector stores and
// read back by the same wave only, so s_waitcnt vmcnt(0) precedes each slab read and the reads
// are agent-scope loads (the vector L1 may hold the slab's lines from the previous
// compaction's reads). Nothing crosses waves: no fences, no flags.
//
// Several splits: every (split, user) slab ends with its best k entries sorted (padded with
// {-inf, -1}), and k_topk_wide_merge reads the slabs' first k entries.
#include "common.h"
#include "score_stream.h"

namespace lg {
namespace wide {

// A list entry: x = the score's bits, y = the item (kPadId / -1 for padding).
__device__ __forceinline__ uint2 make_entry(float v, int id) {
  return make_uint2(__builtin_bit_cast(uint32_t, v), (uint32_t)id);
}
__device__ __forceinline__ float entry_val(uint2 e) { return __builtin_bit_cast(float, e.x); }
__device__ __forceinline__ int entry_id(uint2 e) { return (int)e.y; }

// the slab's entry e as its owner wave sees it after s_waitcnt vmcnt(0): past the vector L1
__device__ __forceinline__ uint2 slab_load(const uint2 *p) {
  const uint64_t e = __hip_atomic_load(reinterpret_cast<uint64_t *>(const_cast<uint2 *>(p)),
                                       __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return make_uint2((uint32_t)e, (uint32_t)(e >> 32));
}

// Looped bitonic sort of the P entries sc[0, P) (P a power of two >= 128, wave-owned LDS) into
// the output order: entry 0 is the best by (score desc, item asc). P / 2 compare-exchanges per
// stage, 64 at a time; the callers pad with {-inf, kPadId}, which sorts last. W = the
// compare-exchanges a lane keeps in flight (4 for the 2048-entry slabs, where the sort is a
// fifth of the kernel's time and LDS bounds the occupancy anyway; 1 below: 24 fewer VGPRs).
template <int W>
__device__ __forceinline__ void lds_bitonic_sort(uint2 *sc, int P) {
  const int lane = lane_id();
  for (int size = 2; size <= P; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      // W compare-exchanges per lane per trip, their reads issued together: a stage's pairs
      // are disjoint, and the stage is LDS-latency bound (p < half is wave-uniform)
      const int half = P >> 1;
      for (int p0 = lane; p0 < half; p0 += 64 * W) {
        uint2 a[W], b[W];
        int lo[W];
#pragma unroll
        for (int q = 0; q < W; ++q) {
          const int p = p0 + 64 * q;
          lo[q] = ((p & ~(stride - 1)) << 1) | (p & (stride - 1));
          if (p < half) {
            a[q] = sc[lo[q]];
            b[q] = sc[lo[q] + stride];
          }
        }
#pragma unroll
        for (int q = 0; q < W; ++q) {
          if (p0 + 64 * q < half) {
            const bool desc = (lo[q] & size) == 0;  // this block sorts best-first
            const bool lo_better =
                before(entry_val(a[q]), entry_id(a[q]), entry_val(b[q]), entry_id(b[q]));
            const bool swap = lo_better != desc;
            sc[lo[q]] = swap ? b[q] : a[q];
            sc[lo[q] + stride] = swap ? a[q] : b[q];
          }
        }
      }
      wave_sync();
    }
  }
}

// the smallest power of two >= n, at least 128
__device__ __forceinline__ int sort_span(int n) {
  int P = 128;
  while (P < n) P <<= 1;
  return P;
}

#ifdef LG_TOPK_COUNT  // measurement builds only: 0 inserted entries, 1 compactions, 2 users
__device__ unsigned long long g_topk_wide_counts[4];
#define LGW_COUNT(i, v) (cnt_ev[i] += (v))
#else
#define LGW_COUNT(i, v) ((void)0)
#endif

// One wave: 16 users; the block's waves work independently (no block-level barrier).
// LDS: WAVES x CAP x 8 B of sort scratch + WAVES x 256 B (64 KiB + 1 KiB at M = 32, WAVES = 4).
template <int D, int M, int WAVES>
__global__ __launch_bounds__(64 * WAVES) void k_score_topk_wide(
    const float *__restrict__ eu, const float *__restrict__ ei, int64_t n_users,
    int64_t n_items, const int64_t *__restrict__ ex_rowptr,
    const int32_t *__restrict__ ex_col, float mask_value, int k, int n_splits,
    int64_t items_per_split, float *__restrict__ out_val, int64_t *__restrict__ out_idx,
    uint2 *__restrict__ slabs) {
  constexpr int Q = D / 4;
  constexpr int LT = Q / 4;  // buffer loads per tile per lane
  constexpr int CAP = 64 * M;
  __shared__ uint2 sc[WAVES][CAP];
  __shared__ int exs[WAVES][64];

  const int wave = threadIdx.x / 64;
  const int lane = lane_id();
  const int ul = lane & 15;
  const int gq = lane >> 4;
  const int64_t tile = blockIdx.x / n_splits;
  const int split = blockIdx.x % n_splits;
  const int64_t ubase = (tile * WAVES + wave) * 16;
  if (ubase >= n_users) return;  // wave-uniform
  const int64_t i0 = (int64_t)split * items_per_split;
  int64_t i1 = i0 + items_per_split;
  if (i1 > n_items) i1 = n_items;
  const int n_valid = i1 > i0 ? (int)(i1 - i0) : 0;  // items of this split
  const int n_t = (n_valid + 15) / 16;                // tiles of this split

  float uf[Q];
  const int64_t u_l = ubase + ul;
  const bool uvalid = u_l < n_users;
  const int64_t uu = uvalid ? u_l : n_users - 1;
  load_piece<Q>(eu + uu * D + gq * Q, uf);
  int64_t ex_pos = 0, ex_hi = 0;
  if (ex_rowptr && uvalid) {
    ex_pos = ex_rowptr[u_l];
    ex_hi = ex_rowptr[u_l + 1];
  }
  int cnt = 0, chk = 0;
  float thr = uvalid ? neg_inf<float>() : __builtin_huge_valf();
  // this lane's user's slab (padding users never insert; theirs is the last valid user's)
  uint2 *const my_slab = slabs + ((int64_t)split * n_users + uu) * CAP;
  const uint64_t same_user = 0x0001000100010001ull << ul;
  uint2 *const ws = &sc[wave][0];
#ifdef LG_TOPK_COUNT
  unsigned long long cnt_ev[4] = {};
#endif

  // Compact user u (0..15) of this wave, all of whose items so far are below lim. Entries
  // [chk, n) were added since the last compaction on their raw scores and get the lazy
  // exclusion (mask_excluded_run; ex_pos starts at the row start). Leaves the best min(n, k)
  // entries sorted in ws[0 ..) and returns their number; unless `fin`, writes them back to the
  // slab.
  auto compact_user = [&](int u, int lim, bool fin) __attribute__((always_inline)) {
    const int n = __shfl(cnt, u);
    const int c0 = __shfl(chk, u);
    int64_t pos = __shfl(ex_pos, u);
    const int64_t hi = __shfl(ex_hi, u);
    uint2 *slab = slabs + ((int64_t)split * n_users + ubase + u) * CAP;
    const int P = sort_span(n);  // <= CAP: n <= CAP and CAP is a power of two >= 512
    // the insertions' and the last compaction's stores have completed (in L2) before the slab
    // is read, and the reads bypass the vector L1
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    for (int e = lane; e < P; e += 64)
      ws[e] = e < n ? slab_load(slab + e) : make_entry(neg_inf<float>(), kPadId);
    wave_sync();
    pos = mask_excluded_run(
        ex_col, pos, hi, lim, exs, wave, c0, n, [&](int j) { return (int)ws[j].y; },
        [&](int j) { ws[j].x = __builtin_bit_cast(uint32_t, mask_value); });
    lds_bitonic_sort<(M >= 32 ? 4 : 1)>(ws, P);
    const int nc = n < k ? n : k;
    const float t = nc == k ? entry_val(ws[k - 1]) : neg_inf<float>();
    if (!fin)
      for (int e = lane; e < nc; e += 64) slab[e] = ws[e];
    LGW_COUNT(1, 1);
    if (ul == u) {
      cnt = nc;
      chk = nc;
      ex_pos = pos;
      thr = entry_thr(uvalid, mask_value, t);
    }
    return nc;
  };

  // acc[r] = score(user ubase + ul, item i0 + 16t + 4gq + r)
  auto mfma_tile = [&](const f32x4(&af)[LT], f32x4 &acc) __attribute__((always_inline)) {
    acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < Q; ++s)
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(af[s / 4][s % 4], uf[s], acc, 0, 0, 0);
  };

  // Slow path, taken when some lane of the wave has a candidate in tile t. A user gains at
  // most 16 entries per tile and enters the tile with cnt <= CAP - 16: pos < CAP.
  auto insert_tile = [&](int t, const f32x4 &acc) __attribute__((always_inline)) {
    const int rel = t * 16 + gq * 4;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float s = acc[r];
      const bool cand = rel + r < n_valid && s > thr;
      const uint64_t bal = __ballot(cand);
      if (bal) {
        const int pos = cnt + __popcll(bal & same_user & lanemask_lt());
        if (cand) my_slab[pos] = make_entry(s, (int)i0 + rel + r);
        cnt += __popcll(bal & same_user);
        LGW_COUNT(0, __popcll(bal));
      }
    }
  };

  // compact every user whose list could overflow on the next tile (+16 max per tile)
  auto maybe_compact = [&](int lim) __attribute__((always_inline)) {
    uint64_t need = __ballot(cnt > CAP - 16) & 0xffffull;
    if (need == 0) return;
    wave_sync();
    while (need) {
      const int u = __ffsll((long long)need) - 1;
      need &= need - 1;
      compact_user(u, lim, false);
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
    f32x4 accA, accB;
    load_item_tile<D>(ei, n_items, i0, voff, afA);
    load_item_tile<D>(ei, n_items, i0 + 16, voff, afB);
    mfma_tile(afA, accA);
    load_item_tile<D>(ei, n_items, i0 + 32, voff, afA);
    // invariant at step t: acc[t%2] = tile t; buffer (t+1)%2 = tile t+1 (landed or in
    // flight); buffer t%2 = tile t+2 in flight
    for (int t = 0;; t += 2) {
      // ---- even step: tile t in accA, tile t+1 in afB
      mfma_tile(afB, accB);
      bool hit = __ballot(above(max4(accA), thr)) != 0;
      load_item_tile<D>(ei, n_items, i0 + (int64_t)(t + 3) * 16, voff, afB);
      if (hit) insert_tile(t, accA);
      maybe_compact(step_lim(t));
      if (t + 1 >= n_t) break;
      // ---- odd step: tile t+1 in accB, tile t+2 in afA
      mfma_tile(afA, accA);
      hit = __ballot(above(max4(accB), thr)) != 0;
      load_item_tile<D>(ei, n_items, i0 + (int64_t)(t + 4) * 16, voff, afA);
      if (hit) insert_tile(t + 1, accB);
      maybe_compact(step_lim(t + 1));
      if (t + 2 >= n_t) break;
    }
  }

  // final lists: one split writes the outputs; several leave k padded entries in each slab
  wave_sync();
  for (int u = 0; u < 16; ++u) {
    const int64_t user = ubase + u;
    if (user >= n_users) break;
    const int nc = compact_user(u, lim_end, true);
    LGW_COUNT(2, 1);
    if (n_splits == 1) {
      for (int e = lane; e < k; e += 64) {
        out_val[user * k + e] = e < nc ? entry_val(ws[e]) : neg_inf<float>();
        out_idx[user * k + e] = e < nc ? (int64_t)entry_id(ws[e]) : -1;
      }
    } else {
      uint2 *slab = slabs + ((int64_t)split * n_users + user) * CAP;
      for (int e = lane; e < k; e += 64) slab[e] = e < nc ? ws[e] : make_entry(neg_inf<float>(), -1);
    }
    wave_sync();
  }
#ifdef LG_TOPK_COUNT
  if (lane == 0)
    for (int i = 0; i < 4; ++i)
      if (cnt_ev[i]) __hip_atomic_fetch_add(&g_topk_wide_counts[i], cnt_ev[i], __ATOMIC_RELAXED,
                                            __HIP_MEMORY_SCOPE_AGENT);
#endif
}

// Merge the n_splits slabs of a user (each: its best k sorted, padded with id -1; item ranges
// ascending by split): one wave per user, k_topk_merge's logic on a CAP-entry LDS list.
// CAP >= 2 k and CAP >= 512, so a compacted list (k entries) always has room for 64 more.
template <int M, int WAVES>
__global__ __launch_bounds__(64 * WAVES) void k_topk_wide_merge(
    const uint2 *__restrict__ slabs, int64_t n_users, int k, int n_splits,
    float *__restrict__ out_val, int64_t *__restrict__ out_idx) {
  constexpr int CAP = 64 * M;
  __shared__ uint2 sc[WAVES][CAP];
  const int wave = threadIdx.x / 64;
  const int lane = lane_id();
  const int64_t user = (int64_t)blockIdx.x * WAVES + wave;
  if (user >= n_users) return;
  uint2 *const ws = &sc[wave][0];
  int cnt = 0;
  float tau = neg_inf<float>();
  int tau_id = kPadId;
  auto compact = [&]() __attribute__((always_inline)) {
    const int P = sort_span(cnt);
    wave_sync();
    for (int e = cnt + lane; e < P; e += 64) ws[e] = make_entry(neg_inf<float>(), kPadId);
    wave_sync();
    lds_bitonic_sort<4>(ws, P);
    if (cnt >= k) {
      cnt = k;
      tau = entry_val(ws[k - 1]);
      tau_id = entry_id(ws[k - 1]);
    }
    wave_sync();
  };
  for (int s = 0; s < n_splits; ++s) {
    const uint2 *slab = slabs + ((int64_t)s * n_users + user) * CAP;
    for (int e0 = 0; e0 < k; e0 += 64) {
      const int e = e0 + lane;
      uint2 en = make_entry(neg_inf<float>(), -1);
      if (e < k) en = slab[e];
      const bool cand =
          entry_id(en) >= 0 && before(entry_val(en), entry_id(en), tau, tau_id);
      const uint64_t bal = __ballot(cand);
      if (cand) ws[cnt + __popcll(bal & lanemask_lt())] = en;
      cnt += __popcll(bal);
      if (cnt > CAP - 64) compact();
    }
  }
  compact();
  for (int e = lane; e < k; e += 64) {
    out_val[user * k + e] = e < cnt ? entry_val(ws[e]) : neg_inf<float>();
    out_idx[user * k + e] = e < cnt ? (int64_t)entry_id(ws[e]) : -1;
  }
}

constexpr int kWideWaves = 4;  // 64 users per block

static int wide_m(int k) { return k <= 256 ? 8 : (k <= 512 ? 16 : 32); }

static size_t wide_slab_bytes(int64_t n_users, int k, int ns) {
  return (size_t)ns * (size_t)n_users * 64 * (size_t)wide_m(k) * sizeof(uint2);
}

template <int D, int M>
static void launch_wide(const float *eu, const float *ei, int64_t n_users, int64_t n_items,
                        const int64_t *ex_rowptr, const int32_t *ex_col, float mask_value,
                        int k, int ns, int64_t per, float *out_val, int64_t *out_idx,
                        uint2 *slabs, hipStream_t s) {
  const int64_t upb = 16 * kWideWaves;
  const int64_t tiles = (n_users + upb - 1) / upb;
  k_score_topk_wide<D, M, kWideWaves><<<dim3((unsigned)(tiles * ns)), dim3(64 * kWideWaves), 0,
                                        s>>>(eu, ei, n_users, n_items, ex_rowptr, ex_col,
                                             mask_value, k, ns, per, out_val, out_idx, slabs);
}

template <int D>
static void dispatch_wide(int M, const float *eu, const float *ei, int64_t n_users,
                          int64_t n_items, const int64_t *ex_rowptr, const int32_t *ex_col,
                          float mask_value, int k, int ns, int64_t per, float *out_val,
                          int64_t *out_idx, uint2 *slabs, hipStream_t s) {
  if (M == 8)
    launch_wide<D, 8>(eu, ei, n_users, n_items, ex_rowptr, ex_col, mask_value, k, ns, per,
                      out_val, out_idx, slabs, s);
  else if (M == 16)
    launch_wide<D, 16>(eu, ei, n_users, n_items, ex_rowptr, ex_col, mask_value, k, ns, per,
                       out_val, out_idx, slabs, s);
  else
    launch_wide<D, 32>(eu, ei, n_users, n_items, ex_rowptr, ex_col, mask_value, k, ns, per,
                       out_val, out_idx, slabs, s);
}

}  // namespace wide
}  // namespace lg

using namespace lg;
using namespace lg::wide;

extern "C" size_t lg_score_topk_wide_ws_bytes(int64_t n_users, int64_t n_items, int32_t dim,
                                              int32_t k, int32_t n_splits) {
  (void)dim;
  if (n_users <= 0 || n_items <= 0 || n_items >= 0x7fffffff || k < 1 || k > 1024 ||
      n_splits < 1 || n_splits > 4096)
    return 0;
  const int64_t per = split_len(n_items, n_splits);
  const int ns = (int)((n_items + per - 1) / per);
  return wide_slab_bytes(n_users, k, ns);
}

extern "C" int lg_score_topk_wide_f32(const float *eu, const float *ei, int64_t n_users,
                                      int64_t n_items, int32_t dim, const int64_t *ex_rowptr,
                                      const int32_t *ex_col, float mask_value, int32_t k,
                                      int32_t n_splits, float *out_val, int64_t *out_idx,
                                      void *ws, size_t ws_bytes, lg_stream_t stream) {
  LG_REQUIRE(eu && ei && out_val && out_idx, "lg_score_topk_wide_f32: null pointer");
  LG_REQUIRE(n_users >= 0 && n_items > 0 && n_items < 0x7fffffff,
             "lg_score_topk_wide_f32: n_items must be in [1, 2^31-1)");
  LG_REQUIRE(dim == 32 || dim == 64 || dim == 128,
             "lg_score_topk_wide_f32: dim %d not in {32,64,128}", dim);
  LG_REQUIRE(k >= 1 && k <= 1024, "lg_score_topk_wide_f32: k=%d not in [1,1024]", k);
  LG_REQUIRE(n_splits >= 1 && n_splits <= 4096, "lg_score_topk_wide_f32: bad n_splits %d",
             n_splits);
  LG_REQUIRE(!ex_rowptr == !ex_col, "lg_score_topk_wide_f32: ex_rowptr/ex_col must both be set");
  LG_REQUIRE(((uintptr_t)ws & 7) == 0, "lg_score_topk_wide_f32: workspace not 8-byte aligned");
  if (n_users == 0) return LG_OK;
  const int64_t per = split_len(n_items, n_splits);
  const int ns = (int)((n_items + per - 1) / per);
  const size_t need = wide_slab_bytes(n_users, k, ns);
  if (!ws || ws_bytes < need) {
    set_error("lg_score_topk_wide_f32: workspace %zu < %zu bytes", ws_bytes, need);
    return LG_ERR_WORKSPACE;
  }
  hipStream_t s = (hipStream_t)stream;
  const int M = wide_m(k);
  uint2 *slabs = (uint2 *)ws;
  switch (dim) {
    case 32: dispatch_wide<32>(M, eu, ei, n_users, n_items, ex_rowptr, ex_col, mask_value, k, ns, per, out_val, out_idx, slabs, s); break;
    case 64: dispatch_wide<64>(M, eu, ei, n_users, n_items, ex_rowptr, ex_col, mask_value, k, ns, per, out_val, out_idx, slabs, s); break;
    default: dispatch_wide<128>(M, eu, ei, n_users, n_items, ex_rowptr, ex_col, mask_value, k, ns, per, out_val, out_idx, slabs, s); break;
  }
  int st = launch_status("lg_score_topk_wide_f32");
  if (st != LG_OK || ns == 1) return st;
  const unsigned blocks = (unsigned)((n_users + kWideWaves - 1) / kWideWaves);
  if (M == 8)
    k_topk_wide_merge<8, kWideWaves><<<dim3(blocks), dim3(64 * kWideWaves), 0, s>>>(
        slabs, n_users, k, ns, out_val, out_idx);
  else if (M == 16)
    k_topk_wide_merge<16, kWideWaves><<<dim3(blocks), dim3(64 * kWideWaves), 0, s>>>(
        slabs, n_users, k, ns, out_val, out_idx);
  else
    k_topk_wide_merge<32, kWideWaves><<<dim3(blocks), dim3(64 * kWideWaves), 0, s>>>(
        slabs, n_users, k, ns, out_val, out_idx);
  return launch_status("lg_score_topk_wide_f32(merge)");
}

#ifdef LG_TOPK_COUNT
// measurement builds only: reads and clears the event counts (inserted entries, compactions,
// users finished) of k_score_topk_wide
extern "C" int lg_topk_wide_counts(unsigned long long *host4) {
  if (hipDeviceSynchronize() != hipSuccess) return LG_ERR_HIP;
  if (hipMemcpyFromSymbol(host4, HIP_SYMBOL(g_topk_wide_counts), 32) != hipSuccess) return LG_ERR_HIP;
  const unsigned long long z[4] = {};
  if (hipMemcpyToSymbol(HIP_SYMBOL(g_topk_wide_counts), z, 32) != hipSuccess) return LG_ERR_HIP;
  return LG_OK;
}
#endif
