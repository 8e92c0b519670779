// K3s: factored hybrid spreading for catalogs whose I x I matrices do not fit (SURVEY.md §8
// a9 "K3s", C5: 1M x 1M, 100M interactions -> general_W and W would be 8 TB each).
//
// Reference (dense numpy fp64, model/SpreadMethod/model.py):
//   general_W = (A.T / k_u) @ A            :14-27
//   W = general_W / (k_i^(1-l) (x) k_j^l)   :63-85   (den == 0 -> 1)
//   F = A @ W                               :88-99
//   F_new = G * F; per user argsort desc, drop train|val, [:k]
//                       model/SpreadLightGCN/model.py:151, recommend.py:18-52
//
// Factored: W[i][j] = general_W[i][j] * ra_i * rb_j with ra = 1/alpha, rb = 1/beta (alpha_i =
// k_i^(1-l), beta_j = k_j^l; a zero factor -> 1, the reference's den == 0 rule), so
//   F[u][j] = rb_j * sum_{i in items(u)} ra_i * sum_{v in users(i) and users(j)} fl(1/k_v)
//           = rb_j * sum over the 3-hop paths u -> i -> v -> j of fl(1/k_v) * ra_i.
// The items are processed in column tiles [j0, j0 + T). Per tile:
//   cursor   end[v] = first position of user v's (ascending) item row with item >= j0 + T;
//            cur[v] (the previous tile's end) marks the first item >= j0, so
//            items(v) inside the tile = user_items[cur[v] .. end[v])
//   bound    bound[i] = sum_{v in users(i)} (end[v] - cur[v]) = the (user, item) pairs
//            behind row i of W in the tile (its paths)
//   rows     row i of general_W restricted to the tile, in the line format below
//   walk     per user (one wave): the paths of its rows added into an LDS accumulator, then
//            scaled by rb_j and either written out (F mode) or merged straight into the
//            user's running top-K list (top-K mode: (G *) F, G = the fp32 e0 score chain,
//            candidates screened by per-(user, 64-column chunk) score bounds).
// Work: the rows pass costs sum_i deg(i) lookups + the 2-hop pairs once per tile (not per
// user); the walk reads one 128-byte line per (user, item) and tile (~5e10 lines at C5) and
// adds ~1e12 paths (one LDS atomic each); F never leaves LDS.
//
// Rounding: every path contributes fl(fl(1/k_v) * ra_i) (P rows) or fl(general_W[i][j] * ra_i)
// (V rows); the sum order is the walk's (fixed: deterministic, but not the dense path's
// ascending-i order), then one multiply by rb_j. Against the reference's
// general_W / (alpha (x) beta) summed by BLAS this is a few ulp per term (tests: 1e-12
// relative), the reference's own BLAS order being unspecified.
//
// This header: the tile line format and the helpers more than one of these files uses.
//   spread_build.hip  the build passes (k_group_*, k_hub_list, k_tile_seek, the reciprocals)
//   spread_tiled.hip  the fused walk (k_tile_walk) alone: its traffic record is keyed on the file
//   spread_ref.hip    the per-tile reference paths of include/lgcnhs_ref.h (tests only)
#pragma once

#include "common.h"

namespace lg {

// A W tile is one 128-byte LINE per item row i at lines[i * 32 ..] (32 words) plus, for rows
// that do not fit, a run of 16-byte units in an overflow array. Word 0 of the line is the
// header: bit 31 = V format, bit 30 = overflow, bit 29 = slow (a V row, or a P row with a
// degree class >= kInvTab: the walk's general decode), bits 0-28 = the overflow run's first
// unit (ovf[u].x = the number of data units that follow it). No per-row metadata: the walk
// reads the line of every item of its user straight from i * 128. Line I (one past the last
// item) is all zero: the walk's padding rows read it.
//
// P rows (<= the hub threshold's pairs, the common case): one 4-byte slot per (user v,
//   item j) PAIR behind the row (v in users(i), j in items(v) inside the tile), in pair order
//   (users ascending, each user's items ascending):
//     bits 0-15  j - item_begin
//     bits 16-30 the 1-based class of v's degree k_v (fl(1 / k_v) = inv[class]; classes
//                < kInvTab are cached in LDS); bit 31 clear (it marks V entries); a zero
//                word is padding
//   line words 1..31 hold the first 31 slots, the overflow units 4 slots each.
// V rows (hub items, more pairs than the threshold; merged while building): one 16-byte
//   entry per distinct column, ascending: {0x80000000 | (j - item_begin), fp64
//   general_W[i][j] (lo, hi), 0}; line units 1..7 hold the first 7, the overflow units one
//   each.
//   A V row with more than width / 2 + 8 entries (hub items held by a large share of the
//   users: nearly every column) is DENSE instead: its line holds only the header, and its
//   overflow run (header x = kRunDense | n, n = ceil(width / 2) data units) holds the row's
//   general_W of columns 2q and 2q + 1 in unit q as two fp64 (zeros included) -- 8 bytes per
//   column instead of 16 per entry, read with no column index (the walk's hub rows are bound
//   by these reads). The sparse run's allocation (1 + min(pairs, width) - 7 units) covers it.
// Neither format depends on lambda (ra / rb are applied by the walk), so a lambda sweep
// reuses the built tiles.
constexpr uint32_t kHdrV = 0x80000000u;
constexpr uint32_t kHdrOvf = 0x40000000u;
constexpr uint32_t kHdrSlow = 0x20000000u;
constexpr uint32_t kHdrPtr = 0x1FFFFFFFu;
constexpr uint32_t kEntV = 0x80000000u;
constexpr uint32_t kRunDense = 0x80000000u;  // overflow run header: a dense V row
constexpr int kLineSlots = 31;  // P slots in a line (word 0 is the header)
constexpr int kLineEnts = 7;    // V entries in a line (unit 0 holds the header)
constexpr int kInvTab = 512;    // degree classes whose fl(1/k) is cached in LDS

// Slot p of a row: line word 1 + p for p < 31, else word (p - 31) of the overflow run's
// data units (the run's unit 0 is its header).
__device__ __forceinline__ void put_slot(uint32_t *__restrict__ line, uint32_t *__restrict__ ovf,
                                         int64_t ou, int64_t p, uint32_t w) {
  if (p < kLineSlots) line[1 + p] = w;
  else ovf[(ou + 1) * 4 + (p - kLineSlots)] = w;
}

// The dense form of a V row from its accumulator acc[0 .. width) (threads t = t0 .. of a
// stride-ts group write): the line's header and zero words, the run header, the data units.
__device__ __forceinline__ bool hub_row_dense(int nz, int width) { return nz > width / 2 + 8; }
__device__ inline void write_hub_row_dense(const double *acc, int width, uint32_t *line, uint32_t *ov,
                                    int64_t ou, int t0, int ts) {
  const int nd = (width + 1) / 2;
  for (int t = t0; t < 32; t += ts) line[t] = t == 0 ? (kHdrV | kHdrSlow | kHdrOvf | (uint32_t)ou) : 0u;
  for (int t = t0; t < 4; t += ts) ov[ou * 4 + t] = t == 0 ? (kRunDense | (uint32_t)nd) : 0u;
  for (int q = t0; q < nd; q += ts) {
    const uint64_t a = (uint64_t)__double_as_longlong(acc[2 * q]);
    const uint64_t b = 2 * q + 1 < width ? (uint64_t)__double_as_longlong(acc[2 * q + 1]) : 0ull;
    *reinterpret_cast<uint4 *>(ov + 4 * (ou + 1 + q)) =
        uint4{(uint32_t)a, (uint32_t)(a >> 32), (uint32_t)b, (uint32_t)(b >> 32)};
  }
}

__device__ __forceinline__ void lds_add(double *acc, uint32_t col, double v) {
  __hip_atomic_fetch_add(&acc[col], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// hub_rows[0 .. *n_hub) = the rows i < n with bound[i] > vthr, in no particular order (*n_hub
// zeroed by the caller): k_hub_list, defined in spread_build.hip
void launch_hub_list(const int64_t *bound, int64_t n, int64_t vthr, int64_t *n_hub,
                     int64_t *hub_rows, hipStream_t s);

}  // namespace lg
