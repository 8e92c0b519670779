// What K2b (csrc/topk_batch.hip) and K2i (csrc/topk_items.hip) share behind their streams: the
// scoring grid divides n items (K2b) or candidate positions (K2i) over every wave of a grid
// that fills the device, a workgroup's waves merge their per-user lists pairwise in LDS, the
// workspace holds one sorted partial list per (workgroup, user), and k_topk_batch_merge
// (csrc/topk_batch.hip, the one device copy) merges a user's partial lists.
//
// - the grid plan, the workspace bound and its split, the argument checks of both entries
// - launch_batch_merge: defined once, in csrc/topk_batch.hip (as is common.h's device_cus)
#pragma once

#include "common.h"

namespace lg {

constexpr int kMaxBlocks = 512;  // workgroups of the scoring grid: partial lists per user
constexpr int kMergeWaves = 16;  // waves of k_topk_batch_merge's workgroup (one per user)

// Merge the n_lists partial lists of each of n_batch users (part_val / part_idx: list r of
// user b at ((r n_batch + b) k), sorted, padded with id -1) into out_val / out_idx.
int launch_batch_merge(const float *part_val, const int32_t *part_idx, int n_batch, int k,
                       int n_lists, float *out_val, int64_t *out_idx, hipStream_t s,
                       const char *what);

// One partial list per (workgroup, user): the grid never has more than kMaxBlocks workgroups,
// nor more than one per 16-entry tile of the n items or candidates. (The bound does not depend
// on the device.)
inline size_t list_ws_bytes(int64_t n, int64_t n_batch, int k) {
  const int64_t tiles = (n + 15) / 16;
  const int64_t lists = tiles < kMaxBlocks ? tiles : kMaxBlocks;
  return (size_t)lists * (size_t)n_batch * (size_t)k * (sizeof(float) + sizeof(int32_t));
}

struct ListGrid {
  int64_t blocks;    // workgroups = partial lists per user
  int64_t per_wave;  // items or candidate positions of one wave, a multiple of 16
};

// A grid that fills the device: two workgroups per CU where a workgroup's lists
// (lists_units = waves x user groups x M, 8 KiB each) take <= 64 KiB, else one; at least one
// 16-entry tile per wave; the tiles divided evenly over the grid's waves.
inline ListGrid plan_list_grid(int64_t n, int cus, int waves, int lists_units) {
  const int64_t tiles = (n + 15) / 16;
  int64_t blocks = (int64_t)cus * (lists_units <= 8 ? 2 : 1);
  if (blocks > kMaxBlocks) blocks = kMaxBlocks;
  if (blocks > (tiles + waves - 1) / waves) blocks = (tiles + waves - 1) / waves;
  const int64_t per_wave = (tiles + blocks * waves - 1) / (blocks * waves) * 16;
  blocks = ((n + per_wave - 1) / per_wave + waves - 1) / waves;  // (no workgroup without items)
  return {blocks, per_wave};
}

struct ListParts {
  float *val;
  int32_t *idx;
};

// the workspace as the grid's partial lists: blocks x n_batch x k values, then as many ids
inline ListParts split_list_ws(void *ws, int64_t blocks, int64_t n_batch, int k) {
  return {(float *)ws, (int32_t *)((char *)ws + (size_t)blocks * n_batch * k * sizeof(float))};
}

// The checks both entries make, under the entry's name `me`: ptrs = every required pointer is
// set, n_batch within the entry's own bound batch_max, need = the entry's *_ws_bytes.
inline int check_list_args(const char *me, bool ptrs, int64_t n_batch, int batch_max,
                           int64_t n_table_users, int64_t n_items, int32_t dim, int32_t k,
                           const int64_t *ex_rowptr, const int32_t *ex_col, const void *ws,
                           size_t ws_bytes, size_t need) {
  LG_REQUIRE(ptrs, "%s: null pointer", me);
  LG_REQUIRE(n_batch >= 1 && n_batch <= batch_max, "%s: n_batch=%lld not in [1,%d]", me,
             (long long)n_batch, batch_max);
  LG_REQUIRE(n_table_users >= 1, "%s: n_table_users must be >= 1", me);
  LG_REQUIRE(n_items > 0 && n_items < 0x7fffffff, "%s: n_items must be in [1, 2^31-1)", me);
  LG_REQUIRE(dim == 32 || dim == 64 || dim == 128, "%s: dim %d not in {32,64,128}", me, dim);
  LG_REQUIRE(k >= 1 && k <= 128, "%s: k=%d not in [1,128]", me, k);
  LG_REQUIRE(!ex_rowptr == !ex_col, "%s: ex_rowptr/ex_col must both be set", me);
  if (!ws || ws_bytes < need) {
    set_error("%s: workspace %zu < %zu bytes", me, ws_bytes, need);
    return LG_ERR_WORKSPACE;
  }
  return LG_OK;
}

}  // namespace lg
