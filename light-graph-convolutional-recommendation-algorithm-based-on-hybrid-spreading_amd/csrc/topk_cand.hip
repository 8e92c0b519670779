// K2c: scoring + exclusion mask + top-K where every row has ITS OWN candidate list, gfx950 f32
// MFMA; and the same gather and chain with no lists (lg_score_cand_f32: "predict these pairs").
//
// The request form of model/LightGCN/recommend.py:83-114 behind a per-user retrieval stage, and
// the sampled-negative evaluation protocol (rank a held-out positive among sampled negatives):
// row r of the output is the first k of {(v(u_r, i), i) : i in candidate row r} under (value
// desc, item id asc), u_r = user_ids[r] (or r), v the fp32 chain score of lg_score_topk_f32
// (k_score_topk's chain: v_mfma_f32_16x16x4_f32, D/4 dependent steps from a zero accumulator) or
// mask_value where i is in u_r's exclusion row. It equals lg_score_topk_f32 on the one-user
// sub-problem (eu[u_r], ei[cand_r]) with the exclusion columns renumbered and the ids mapped
// back, bit for bit -- but nothing is gathered into memory.
//
// The candidates are a CSR (lgcnhs.graph.RowSets): cand_rowptr int64 [n_rows + 1], cand_col
// int32, strictly ascending inside a row. A row's candidates at positions >= max_len are ignored.
//
// One wave per work unit (row r, segment s) = positions [s seg, min((s + 1) seg, len_r)) of row
// r, seg = split_len(max_len, n_seg); 4 independent waves per workgroup, no block barrier: a
// wave whose unit is empty writes its padding and leaves. With n_seg == 1 a unit writes the
// output row itself, else a k-entry partial list at ((s n_rows + r) k), merged by
// launch_topk_merge (k_topk_merge, csrc/topk_plain.hip).
//
//   * The user's row is the B operand, the same user in all 16 columns (as exact_entries of
//     csrc/topk.hip); a 16-candidate tile is 16 gathered item rows as the A operand: lane
//     (ul, gq) reads piece gq of row cand_col[p + ul]. Every column of the result holds the same
//     16 scores (lane (ul, gq): rows 4 gq + r in acc[r]), so lane (ul < 4, gq) takes acc[ul]: 16
//     lanes own one score each for the compare and the insert.
//   * Tiles go in PAIRS: the two chains of a pair are interleaved (step s of both before step
//     s + 1), since one chain alone leaves the MFMA pipe idle between its dependent steps. The
//     rows of pair q + 1 and q + 2 are in flight while pair q is scored, ids are fetched two
//     pairs ahead of the rows that need them (K2i's stream, csrc/topk_items.hip, over pairs).
//   * One list per wave in LDS, CAP = 64 M entries (M = list_cap_m(k)), the one-max-one-compare
//     filter, entry_thr, wave_compact and the lazy exclusion of score_stream.h in item-id space:
//     the cursor starts at lower_bound(the user's exclusion row, the unit's first candidate),
//     the limit at a compaction is the id of the first candidate not yet streamed.
//   * Any input is memory-safe: a position past the unit's end is read as the unit's last
//     candidate and never enters the list; an id outside [0, n_items) reads row 0 and never
//     enters; a user id outside the table reads row 0 and its row is all padding. A row that is
//     not ascending gives unspecified lists, no out-of-bounds access.
//
// LDS per workgroup: 4 waves x M x 512 B of lists + 1 KiB = 3 / 5 / 9 KiB.
#include "score_stream.h"

namespace lg {
namespace {

constexpr int kCandWaves = 4;      // waves (= work units) per workgroup
constexpr int kCandSegMax = 4096;  // segments per row
constexpr int kPairSeg = 256;      // lg_score_cand_f32: positions per unit step
constexpr int kPairUnitsMax = 1024;  // ... and units per row

template <int D, int M>
__global__ __launch_bounds__(64 * kCandWaves) void k_score_topk_cand(
    const float *__restrict__ eu, const float *__restrict__ ei,
    const int64_t *__restrict__ user_ids, int64_t n_rows, int64_t n_table_users, int n_items,
    const int64_t *__restrict__ cand_rowptr, const int32_t *__restrict__ cand_col,
    int64_t max_len, int64_t seg, int n_seg, const int64_t *__restrict__ ex_rowptr,
    const int32_t *__restrict__ ex_col, float mask_value, int k, float *__restrict__ out_val,
    int64_t *__restrict__ out_idx, float *__restrict__ part_val,
    int32_t *__restrict__ part_idx) {
  constexpr int Q = D / 4;
  constexpr int LT = Q / 4;  // 16-byte loads per tile per lane
  constexpr int CAP = 64 * M;
  constexpr int WAVES = kCandWaves;
  __shared__ float cs[WAVES][CAP];
  __shared__ int ci[WAVES][CAP];
  __shared__ int exs[WAVES][64];

  // (readfirstlane: the unit, its range and its tile count are then scalar to hipcc and the
  // loop's exits uniform branches, as in k_score_topk_items)
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / 64);
  const int lane = lane_id();
  const int ul = lane & 15;
  const int gq = lane >> 4;
  const int64_t unit = (int64_t)blockIdx.x * WAVES + wave;
  if (unit >= n_rows * n_seg) return;  // wave-uniform; no block-level barriers below
  const int64_t r = unit / n_seg;
  const int s = (int)(unit % n_seg);

  // a user id outside the table is clamped (row 0 is read instead) and its row is padding
  int64_t u = user_ids ? user_ids[r] : r;
  const bool uvalid = u >= 0 && u < n_table_users;
  if (!uvalid) u = 0;
  // the unit's candidate positions: [p0, p1) of the row's first min(len, max_len)
  const int64_t c0 = cand_rowptr[r];
  int64_t len = cand_rowptr[r + 1] - c0;
  if (len > max_len) len = max_len;
  const int64_t p0 = (int64_t)s * seg;
  int64_t p1 = p0 + seg;
  if (p1 > len) p1 = len;
  const int n_valid =
      __builtin_amdgcn_readfirstlane(uvalid && p1 > p0 ? (int)(p1 - p0) : 0);  // (< 2^31)
  const int n_t = (n_valid + 15) / 16;  // tiles of this unit
  const int n_q = (n_t + 1) / 2;        // pairs of tiles

  int cnt = 0;
  if (n_valid > 0) {
    const int32_t *__restrict__ ids = cand_col + c0 + p0;
    float uf[Q];
    load_piece<Q>(eu + u * D + gq * Q, uf);
    int64_t ex_pos = 0, ex_hi = 0;
    if (ex_rowptr) {
      ex_hi = ex_rowptr[u + 1];
      // the user's first excluded item at or past the unit's first candidate
      ex_pos = lower_bound_i32(ex_col, ex_rowptr[u], ex_hi, ids[0]);
    }
    int chk = 0;
    float thr = neg_inf<float>();

    // Compact the list, all of whose items so far are below lim (an item id): the entries
    // [chk, cnt) added since the last compaction get the lazy exclusion, then the best k stay.
    auto compact = [&](int lim) __attribute__((always_inline)) {
      float *ks = &cs[wave][0];
      int *is = &ci[wave][0];
      ex_pos = mask_excluded_run(
          ex_col, ex_pos, ex_hi, lim, exs, wave, chk, cnt, [&](int j) { return is[j]; },
          [&](int j) { ks[j] = mask_value; });
      float t;
      int tid;
      cnt = wave_compact<float, M>(ks, is, cnt, k, t, tid);
      chk = cnt;
      thr = entry_thr(true, mask_value, t);
    };

    // this lane's item of tile t; past the unit's end the unit's last candidate again (no
    // branch: its scores are dropped by the position test of insert_pair)
    const unsigned last = (unsigned)(n_valid - 1);
    auto id_at = [&](int t) __attribute__((always_inline)) {
      const unsigned p = (unsigned)t * 16u + (unsigned)ul;
      return ids[p < last ? p : last];
    };
    // piece gq of row `id` (row 0 for an id outside the table): 64-bit address
    auto load_rows = [&](int id, f32x4(&af)[LT]) __attribute__((always_inline)) {
      const int64_t row = (unsigned)id < (unsigned)n_items ? id : 0;
      const f32x4 *rp = reinterpret_cast<const f32x4 *>(ei + row * D + gq * Q);
#pragma unroll
      for (int t = 0; t < LT; ++t) af[t] = rp[t];
    };
    auto load_pair = [&](const int (&id)[2], f32x4(&af)[2][LT]) __attribute__((always_inline)) {
      load_rows(id[0], af[0]);
      load_rows(id[1], af[1]);
    };
    auto ids_of_pair = [&](int q, int (&id)[2]) __attribute__((always_inline)) {
      id[0] = id_at(2 * q);
      id[1] = id_at(2 * q + 1);
    };

    // acc[j][r] = score(user, position 16 (2q + j) + 4 gq + r), the same in every column ul;
    // s outer / j inner: the two chains interleave on the MFMA pipe
    auto mfma_pair = [&](const f32x4(&af)[2][LT], f32x4(&acc)[2]) __attribute__((always_inline)) {
      acc[0] = f32x4{0.f, 0.f, 0.f, 0.f};
      acc[1] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int st = 0; st < Q; ++st)
#pragma unroll
        for (int j = 0; j < 2; ++j)
          acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[j][st / 4][st % 4], uf[st], acc[j], 0,
                                                        0, 0);
    };
    auto any_cand = [&](const f32x4(&acc)[2]) __attribute__((always_inline)) {
      return __ballot(above(max4(acc[0]), thr) || above(max4(acc[1]), thr)) != 0;
    };

    // Slow path, taken when some score of pair q passes the filter: lane (ul < 4, gq) owns the
    // score of position 16 t + 4 gq + ul, whose id another lane loaded; it re-reads it here.
    auto insert_pair = [&](int q, const f32x4(&acc)[2]) __attribute__((always_inline)) {
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const unsigned rel = (unsigned)(2 * q + j) * 16u + (unsigned)(gq * 4 + (ul & 3));
        const float sc = (ul & 2) ? ((ul & 1) ? acc[j][3] : acc[j][2])
                                  : ((ul & 1) ? acc[j][1] : acc[j][0]);
        bool cand = ul < 4 && rel < (unsigned)n_valid && sc > thr;
        int id = 0;
        if (cand) {
          id = ids[rel];
          cand = (unsigned)id < (unsigned)n_items;
        }
        const uint64_t bal = __ballot(cand);
        if (bal) {
          const int pos = cnt + __popcll(bal & lanemask_lt());
          if (cand) {
            cs[wave][pos] = sc;
            ci[wave][pos] = id;
          }
          cnt += __popcll(bal);
        }
      }
    };

    // compact when the list could overflow on the next pair (+32 max per pair); the limit is
    // the id of the first candidate behind pair q
    auto maybe_compact = [&](int q) __attribute__((always_inline)) {
      if (cnt <= CAP - 32) return;
      const unsigned nxt = (unsigned)(q + 1) * 32u;
      const int lim = nxt < (unsigned)n_valid ? ids[nxt] : n_items;
      wave_sync();
      compact(lim);
    };

    f32x4 afA[2][LT], afB[2][LT];
    f32x4 accA[2], accB[2];
    int id0[2], id1[2], id2[2], idA[2], idB[2];
    ids_of_pair(0, id0);
    ids_of_pair(1, id1);
    ids_of_pair(2, id2);
    ids_of_pair(3, idB);
    ids_of_pair(4, idA);
    load_pair(id0, afA);
    load_pair(id1, afB);
    mfma_pair(afA, accA);
    load_pair(id2, afA);
    // Retire the prologue's loads with a wait hipcc sees (vmcnt(0)), as k_score_topk_items does:
    // otherwise its waitcnt pass merges their pending state into the loop header.
    __builtin_amdgcn_s_waitcnt(0x0F70);
    // invariant at step q: acc[q%2] = pair q; buffer (q+1)%2 = pair q+1 (landed or in flight);
    // buffer q%2 = pair q+2 in flight; id[(q+1)%2] = pair q+3's, id[q%2] = pair q+4's. Pairs go
    // two to a trip and the loop has ONE exit (k_score_topk_items: see there): an odd pair
    // count is rounded up, the extra pair repeats the unit's last candidate and inserts nothing.
    for (int q = 0; q < n_q; q += 2) {
      // ---- even step: pair q in accA, pair q+1 in afB
      mfma_pair(afB, accB);
      bool hit = any_cand(accA);
      load_pair(idB, afB);
      ids_of_pair(q + 5, idB);
      if (hit) insert_pair(q, accA);
      maybe_compact(q);
      // ---- odd step: pair q+1 in accB, pair q+2 in afA
      mfma_pair(afA, accA);
      hit = q + 1 < n_q && any_cand(accB);
      load_pair(idA, afA);
      ids_of_pair(q + 6, idA);
      if (hit) insert_pair(q + 1, accB);
      maybe_compact(q + 1);
    }
    // the unit's final list: the best k, sorted
    wave_sync();
    compact(n_items);
  }

  // every unit writes k entries, empty ones all padding
  const int64_t o = n_seg == 1 ? r * k : ((int64_t)s * n_rows + r) * k;
  for (int e = lane; e < k; e += 64) {
    const float v = e < cnt ? cs[wave][e] : neg_inf<float>();
    const int id = e < cnt ? ci[wave][e] : -1;
    if (n_seg == 1) {
      out_val[o + e] = v;
      out_idx[o + e] = id;
    } else {
      part_val[o + e] = v;
      part_idx[o + e] = id;
    }
  }
}

// The chain scores of every candidate position, no lists: out[c0_r + p] = v(u_r, cand_col[c0_r
// + p]) or mask_value where excluded; -inf at positions >= max_len of their row, for an id
// outside [0, n_items) and in the rows of a user id outside the table. Wave (row r, slot s0) of
// `units` per row takes the 256-position steps s0, s0 + units, .. of the row, 16 positions per
// MFMA chain (the user in every column, lane (ul < 4, gq) owns position 4 gq + ul of the tile),
// each owner searching its id in the user's exclusion row; many light waves hide the gather.
template <int D>
__global__ __launch_bounds__(64 * kCandWaves) void k_score_cand(
    const float *__restrict__ eu, const float *__restrict__ ei,
    const int64_t *__restrict__ user_ids, int64_t n_rows, int64_t n_table_users, int n_items,
    const int64_t *__restrict__ cand_rowptr, const int32_t *__restrict__ cand_col,
    int64_t max_len, int units, const int64_t *__restrict__ ex_rowptr,
    const int32_t *__restrict__ ex_col, float mask_value, float *__restrict__ out) {
  constexpr int Q = D / 4;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / 64);
  const int lane = lane_id();
  const int ul = lane & 15;
  const int gq = lane >> 4;
  const int64_t unit = (int64_t)blockIdx.x * kCandWaves + wave;
  if (unit >= n_rows * units) return;
  const int64_t r = unit / units;
  const int s0 = (int)(unit % units);
  int64_t u = user_ids ? user_ids[r] : r;
  const bool uvalid = u >= 0 && u < n_table_users;
  if (!uvalid) u = 0;
  const int64_t c0 = cand_rowptr[r];
  const int64_t full = cand_rowptr[r + 1] - c0;  // the row's positions, all written
  const int64_t len = !uvalid ? 0 : (full < max_len ? full : max_len);  // ... and those scored
  const int32_t *__restrict__ ids = cand_col + c0;
  float *__restrict__ o = out + c0;
  // positions that are not scored: -inf
  for (int64_t p = len + (int64_t)s0 * 64 + lane; p < full; p += (int64_t)units * 64)
    o[p] = neg_inf<float>();
  if ((int64_t)s0 * kPairSeg >= len) return;
  float uf[Q];
  load_piece<Q>(eu + u * D + gq * Q, uf);
  int64_t ex_lo = 0, ex_hi = 0;
  if (ex_rowptr) {
    ex_lo = ex_rowptr[u];
    ex_hi = ex_rowptr[u + 1];
  }
  for (int64_t b = (int64_t)s0 * kPairSeg; b < len; b += (int64_t)units * kPairSeg) {
    const int64_t e = b + kPairSeg < len ? b + kPairSeg : len;
    for (int64_t t = b; t < e; t += 16) {
      // this lane's row of the tile (past the end: the row's last scored candidate again)
      const int64_t pl = t + ul < len ? t + ul : len - 1;
      const int idl = ids[pl];
      const int64_t row = (unsigned)idl < (unsigned)n_items ? idl : 0;
      float af[Q];
      load_piece<Q>(ei + row * D + gq * Q, af);
      f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int st = 0; st < Q; ++st)
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(af[st], uf[st], acc, 0, 0, 0);
      const int64_t p = t + gq * 4 + (ul & 3);
      if (ul < 4 && p < len) {
        float sc = (ul & 2) ? ((ul & 1) ? acc[3] : acc[2]) : ((ul & 1) ? acc[1] : acc[0]);
        const int id = ids[p];
        if ((unsigned)id >= (unsigned)n_items) {
          sc = neg_inf<float>();
        } else if (ex_lo < ex_hi) {
          const int64_t x = lower_bound_i32(ex_col, ex_lo, ex_hi, id);
          if (x < ex_hi && ex_col[x] == id) sc = mask_value;
        }
        o[p] = sc;
      }
    }
  }
}

template <int D>
void dispatch_cand(int m, unsigned blocks, const float *eu, const float *ei,
                   const int64_t *user_ids, int64_t n_rows, int64_t n_table_users, int n_items,
                   const int64_t *cand_rowptr, const int32_t *cand_col, int64_t max_len,
                   int64_t seg, int n_seg, const int64_t *ex_rowptr, const int32_t *ex_col,
                   float mask_value, int k, float *out_val, int64_t *out_idx, float *part_val,
                   int32_t *part_idx, hipStream_t stream) {
#define LG_CAND_CASE(MM)                                                                       \
  if (m == MM)                                                                                 \
    return k_score_topk_cand<D, MM><<<dim3(blocks), dim3(64 * kCandWaves), 0, stream>>>(       \
        eu, ei, user_ids, n_rows, n_table_users, n_items, cand_rowptr, cand_col, max_len, seg, \
        n_seg, ex_rowptr, ex_col, mask_value, k, out_val, out_idx, part_val, part_idx);
  LG_CAND_CASE(1) LG_CAND_CASE(2) LG_CAND_CASE(4)
#undef LG_CAND_CASE
}

// workgroups of n_rows x units work units, 0 when past the grid limit
int64_t cand_blocks(int64_t n_rows, int64_t units) {
  if (n_rows < 1 || units < 1 || n_rows > (int64_t)0x7fffffff * kCandWaves / units) return 0;
  const int64_t blocks = (n_rows * units + kCandWaves - 1) / kCandWaves;
  return blocks <= 0x7fffffff ? blocks : 0;
}

// the checks both entries make, under the entry's name `me`
int check_cand_args(const char *me, bool ptrs, int64_t n_rows, int64_t units,
                    int64_t n_table_users, int64_t n_items, int64_t max_len, int32_t dim,
                    const int64_t *ex_rowptr, const int32_t *ex_col) {
  LG_REQUIRE(ptrs, "%s: null pointer", me);
  LG_REQUIRE(n_rows >= 1, "%s: n_rows=%lld must be >= 1", me, (long long)n_rows);
  LG_REQUIRE(n_table_users >= 1, "%s: n_table_users must be >= 1", me);
  LG_REQUIRE(n_items > 0 && n_items < 0x7fffffff, "%s: n_items must be in [1, 2^31-1)", me);
  LG_REQUIRE(max_len >= 1 && max_len <= 0x7fffffff, "%s: max_len=%lld not in [1, 2^31)", me,
             (long long)max_len);
  LG_REQUIRE(dim == 32 || dim == 64 || dim == 128, "%s: dim %d not in {32,64,128}", me, dim);
  LG_REQUIRE(!ex_rowptr == !ex_col, "%s: ex_rowptr/ex_col must both be set", me);
  LG_REQUIRE(cand_blocks(n_rows, units) > 0,
             "%s: n_rows=%lld x %lld units per row is past the grid limit", me,
             (long long)n_rows, (long long)units);
  return LG_OK;
}

}  // namespace
}  // namespace lg

using namespace lg;

extern "C" size_t lg_score_topk_cand_ws_bytes(int64_t n_rows, int32_t dim, int32_t k,
                                              int32_t n_seg) {
  if (k < 1 || k > 128 || n_seg < 1 || n_seg > kCandSegMax ||
      !(dim == 32 || dim == 64 || dim == 128) || cand_blocks(n_rows, n_seg) == 0)
    return 0;
  if (n_seg == 1) return 0;
  return (size_t)n_seg * (size_t)n_rows * (size_t)k * (sizeof(float) + sizeof(int32_t));
}

extern "C" int lg_score_topk_cand_f32(
    const float *eu, const float *ei, const int64_t *user_ids, int64_t n_rows,
    int64_t n_table_users, int64_t n_items, const int64_t *cand_rowptr, const int32_t *cand_col,
    int64_t max_len, int32_t dim, const int64_t *ex_rowptr, const int32_t *ex_col,
    float mask_value, int32_t k, int32_t n_seg, float *out_val, int64_t *out_idx, void *ws,
    size_t ws_bytes, lg_stream_t stream) {
  const char *me = "lg_score_topk_cand_f32";
  LG_REQUIRE(k >= 1 && k <= 128, "%s: k=%d not in [1,128]", me, k);
  LG_REQUIRE(n_seg >= 1 && n_seg <= kCandSegMax, "%s: n_seg=%d not in [1,%d]", me, n_seg,
             kCandSegMax);
  const int st0 =
      check_cand_args(me, eu && ei && cand_rowptr && cand_col && out_val && out_idx, n_rows,
                      n_seg, n_table_users, n_items, max_len, dim, ex_rowptr, ex_col);
  if (st0 != LG_OK) return st0;
  // the segments in use: seg a multiple of 16, no segment past max_len
  const int64_t seg = split_len(max_len, n_seg);
  const int ns = (int)((max_len + seg - 1) / seg);
  float *part_val = nullptr;
  int32_t *part_idx = nullptr;
  if (ns > 1) {
    const size_t need = lg_score_topk_cand_ws_bytes(n_rows, dim, k, ns);
    if (!ws || ws_bytes < need) {
      set_error("%s: workspace %zu < %zu bytes", me, ws_bytes, need);
      return LG_ERR_WORKSPACE;
    }
    part_val = (float *)ws;
    part_idx = (int32_t *)((char *)ws + (size_t)ns * n_rows * k * sizeof(float));
  }
  const unsigned blocks = (unsigned)cand_blocks(n_rows, ns);
  const int m = list_cap_m(k);
  hipStream_t s = (hipStream_t)stream;
  switch (dim) {
    case 32: dispatch_cand<32>(m, blocks, eu, ei, user_ids, n_rows, n_table_users, (int)n_items, cand_rowptr, cand_col, max_len, seg, ns, ex_rowptr, ex_col, mask_value, k, out_val, out_idx, part_val, part_idx, s); break;
    case 64: dispatch_cand<64>(m, blocks, eu, ei, user_ids, n_rows, n_table_users, (int)n_items, cand_rowptr, cand_col, max_len, seg, ns, ex_rowptr, ex_col, mask_value, k, out_val, out_idx, part_val, part_idx, s); break;
    default: dispatch_cand<128>(m, blocks, eu, ei, user_ids, n_rows, n_table_users, (int)n_items, cand_rowptr, cand_col, max_len, seg, ns, ex_rowptr, ex_col, mask_value, k, out_val, out_idx, part_val, part_idx, s); break;
  }
  const int st = launch_status(me);
  if (st != LG_OK || ns == 1) return st;
  launch_topk_merge(part_val, part_idx, n_rows, k, ns, out_val, out_idx, s);
  return launch_status("lg_score_topk_cand_f32(merge)");
}

extern "C" int lg_score_cand_f32(const float *eu, const float *ei, const int64_t *user_ids,
                                 int64_t n_rows, int64_t n_table_users, int64_t n_items,
                                 const int64_t *cand_rowptr, const int32_t *cand_col,
                                 int64_t max_len, int32_t dim, const int64_t *ex_rowptr,
                                 const int32_t *ex_col, float mask_value, float *out,
                                 lg_stream_t stream) {
  const char *me = "lg_score_cand_f32";
  // 256-position steps of a row are dealt to at most 1024 waves
  int64_t units = max_len >= 1 ? (max_len + kPairSeg - 1) / kPairSeg : 1;
  if (units > kPairUnitsMax) units = kPairUnitsMax;
  const int st0 = check_cand_args(me, eu && ei && cand_rowptr && cand_col && out, n_rows, units,
                                  n_table_users, n_items, max_len, dim, ex_rowptr, ex_col);
  if (st0 != LG_OK) return st0;
  const dim3 grid((unsigned)cand_blocks(n_rows, units)), block(64 * kCandWaves);
  hipStream_t s = (hipStream_t)stream;
  switch (dim) {
    case 32: k_score_cand<32><<<grid, block, 0, s>>>(eu, ei, user_ids, n_rows, n_table_users, (int)n_items, cand_rowptr, cand_col, max_len, (int)units, ex_rowptr, ex_col, mask_value, out); break;
    case 64: k_score_cand<64><<<grid, block, 0, s>>>(eu, ei, user_ids, n_rows, n_table_users, (int)n_items, cand_rowptr, cand_col, max_len, (int)units, ex_rowptr, ex_col, mask_value, out); break;
    default: k_score_cand<128><<<grid, block, 0, s>>>(eu, ei, user_ids, n_rows, n_table_users, (int)n_items, cand_rowptr, cand_col, max_len, (int)units, ex_rowptr, ex_col, mask_value, out); break;
  }
  return launch_status(me);
}
