// The shared pieces of the K2 stream -- score a range of items against a wave's users, 16
// items per step, and keep each user's best k -- for k_score_topk (topk_plain.hip), k_topk_ring
// (topk.hip), k_score_topk_wide (topk_wide.hip) and k_score_topk_batch (topk_batch.hip):
//
//   load_piece, load_item_tile  the MFMA operand loads
//   max4, above, entry_thr      the one-max-one-compare filter and the admission threshold
//   mask_excluded_run           the lazy exclusion of a list's new entries, for lists in LDS
//   split_len, screened_splits, list_cap_m, launch_topk_merge
//                               the split and list arithmetic of the launchers; the split merge
//
// Each kernel keeps its own text of the software pipeline (the loop of k_score_topk, described
// there): written once over a list policy, hipcc allocated more registers in some
// instantiations of every kernel. What is here compiles to the code the kernels
// had with their own copies.
#pragma once

#include "common.h"

namespace lg {

typedef float f32x4 __attribute__((ext_vector_type(4)));

template <int Q>
__device__ __forceinline__ void load_piece(const float *__restrict__ p, float (&v)[Q]) {
  const float4 *p4 = reinterpret_cast<const float4 *>(p);
#pragma unroll
  for (int t = 0; t < Q / 4; ++t) {
    const float4 q = p4[t];
    v[4 * t + 0] = q.x;
    v[4 * t + 1] = q.y;
    v[4 * t + 2] = q.z;
    v[4 * t + 3] = q.w;
  }
}

// Item-tile loads: raw buffer loads through a per-tile descriptor whose base is the tile's
// first row and whose record count is the bytes left below `end` (the table's end, or the
// wave's range end; 0 past it), so rows beyond `end` read as 0 and every tile issues the same
// D / 16 loads with no branch and no per-lane address arithmetic. Compiler-visible
// (__builtin_amdgcn_raw_buffer_load_b128): hipcc counts these loads itself and places each
// s_waitcnt vmcnt before the first use. CLAMP: `it` may run far past `end` (a range that is a
// small part of the table), so the 64-bit remainder is clamped before it is narrowed and a
// tile past the end takes row 0 as its base; without it end - it must fit an int (the clamp
// costs the loop a 64-bit compare and two selects per tile).
template <int D, bool CLAMP = false>
__device__ __forceinline__ void load_item_tile(const float *ei, int64_t end, int64_t it,
                                               int voff, f32x4 (&v)[D / 16]) {
  constexpr int TB = 16 * D * 4;  // bytes of one 16-item tile
  const int64_t rem64 = end - it;
  const int rem = CLAMP && rem64 > 16 ? 16 : (int)rem64;  // items left below `end` (end < 2^31)
  const int num = rem >= 16 ? TB : (rem > 0 ? rem * (D * 4) : 0);
  const __amdgpu_buffer_rsrc_t r = __builtin_amdgcn_make_buffer_rsrc(
      (void *)(ei + (!CLAMP || rem > 0 ? it : 0) * D), 0, num, 0x00020000);
#pragma unroll
  for (int t = 0; t < D / 16; ++t)
    v[t] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r, voff + 16 * t, 0, 0));
}

// max of the four scores of an MFMA result: two v_maximum3_f32 (gfx950), compiler-visible, so
// hipcc pads the MFMA-result wait states itself. NaN-propagating: callers test
// !(max4(a) <= thr), which sends a NaN score to the exact per-element test (sc > thr) instead
// of hiding the tile's other scores behind it.
__device__ __forceinline__ float max4(f32x4 a) {
  return __builtin_elementwise_maximum(__builtin_elementwise_maximum(a[0], a[1]),
                                       __builtin_elementwise_maximum(a[2], a[3]));
}
__device__ __forceinline__ bool above(float m, float thr) { return !(m <= thr); }

// The entry threshold of a user whose list's k-th value is t (-inf while the list is short):
// a masked (excluded) item would enter with mask_value, so everything is admitted while that
// beats t; a padding user admits nothing.
__device__ __forceinline__ float entry_thr(bool valid, float mask_value, float t) {
  return !valid ? __builtin_huge_valf() : (mask_value > t ? neg_inf<float>() : t);
}

// items per split: a multiple of 16, at least 16
inline int64_t split_len(int64_t n_items, int n_splits) {
  int64_t per = (n_items + n_splits - 1) / n_splits;
  per = (per + 15) / 16 * 16;
  return per < 16 ? 16 : per;
}

// the screened kernel's splits: at least one per 2^20 items (k_topk_ring's 16-bit tile
// indices); split_len of it is then <= 2^20 (a multiple of 16)
constexpr int kTileBits = 16;  // tile index field: splits of at most 2^20 items
inline int screened_splits(int64_t n_items, int n_splits) {
  const int64_t need = (n_items + ((int64_t)1 << (kTileBits + 4)) - 1) >> (kTileBits + 4);
  return n_splits > need ? n_splits : (int)need;
}

// list capacity CAP = 64 M entries per (wave, user) at this k (2k <= CAP for the pairwise merges
// of K2b and K2i)
inline int list_cap_m(int k) { return k <= 32 ? 1 : (k <= 64 ? 2 : 4); }

// Merge the n_splits partial lists of each user (k_topk_merge; <2> for k <= 64, else <4>; four
// users per block) for lg_score_topk_f32 and lg_score_topk_screened_f32: defined once, in
// topk_plain.hip.
void launch_topk_merge(const float *part_val, const int32_t *part_idx, int64_t n_users, int k,
                       int n_splits, float *out_val, int64_t *out_idx, hipStream_t stream);

// Exclusion is applied lazily: a candidate enters on its raw score (or on the mask value when
// that alone beats tau), and the entries [c0, n) added since the user's last compaction are
// checked when the list is compacted. Their items all lie in [previous limit, lim), and pos is
// the user's first excluded item not yet passed (>= the previous limit, or where the kernel
// started it: items below i0 are harmless), so the excluded items to test are one ascending
// run ex_col[pos .. hi) read 64 at a time, coalesced, parked in the wave's exs[wave][64] and
// binary-searched there. item_of(j) is entry j's item and mask(j) gives entry j the mask
// value. Exact: an excluded item would enter with mask_value, and mask_value > tau admits
// every item. Returns the advanced pos. By one wave, its LDS writes synchronised.
// (exs and the wave's index, not the wave's row: with the row's address formed by the caller
// hipcc scheduled k_score_topk_batch differently, as wave_list.h records for its lists.)
template <class ItemOf, class Mask>
__device__ __forceinline__ int64_t mask_excluded_run(const int32_t *ex_col, int64_t pos,
                                                     int64_t hi, int lim, int (*exs)[64], int wave,
                                                     int c0, int n, ItemOf item_of, Mask mask) {
  const int lane = lane_id();
  if (n > c0) {
    while (pos < hi) {
      const int64_t e = pos + lane;
      const int32_t x = e < hi ? ex_col[e] : 0x7fffffff;
      const int nin = __popcll(__ballot(x < lim));  // ascending: a prefix of the lanes
      if (nin == 0) break;
      exs[wave][lane] = x;
      wave_sync();
      for (int j = c0 + lane; j < n; j += 64) {
        const int item = item_of(j);
        int a = 0, b = nin;  // first index with exs[] >= item
        while (a < b) {
          const int mid = (a + b) >> 1;
          if (exs[wave][mid] < item) a = mid + 1;
          else b = mid;
        }
        if (a < nin && exs[wave][a] == item) mask(j);
      }
      wave_sync();
      pos += nin;
      if (nin < 64) break;
    }
  }
  return pos;
}

}  // namespace lg
