// K2i: scoring + exclusion mask + top-K for a short list of users (<= 16 ids into the full
// tables) over a CANDIDATE ITEM SET (strictly ascending ids into the full item table), gfx950
// f32 MFMA.
//
// The request form of model/LightGCN/recommend.py:83-114 with a catalog filter (the in-stock
// items, one category, a retrieval stage's output): row b of the output is the first k of
// {(v(user_ids[b], i), i) : i in item_ids} under (value desc, item id asc), v the fp32 chain
// score of lg_score_topk_f32 (k_score_topk's chain: v_mfma_f32_16x16x4_f32, D/4 dependent steps
// from a zero accumulator) or mask_value where i is in the user's exclusion row. It equals
// lg_score_topk_f32 on the gathered sub-table ei[item_ids] with the exclusion columns
// renumbered and the ids mapped back, bit for bit -- but nothing is gathered, and only the
// candidates' rows are read.
//
// It is K2b (csrc/topk_batch.hip) with the division turned onto candidate POSITIONS: wave w of
// the grid scores the positions [w ppw, (w + 1) ppw) of item_ids, ppw a multiple of 16. One
// user group (n_batch <= 16) per wave, one list per user in LDS (CAP = 64 M entries), the
// lazy exclusion of score_stream.h, the pairwise merge of a workgroup's waves (K2b's tail
// text, see there), one partial list per (workgroup, user), and on the host K2b's own code
// through batch_lists.h: the grid plan, the workspace bound and split, the argument checks and
// k_topk_batch_merge (launch_batch_merge) for the final lists. What differs is the stream:
//
//   * The A tiles are row gathers: lane (ul, gq) of tile t reads piece gq of row
//     item_ids[p0 + 16 t + ul] by a global load with a 64-bit address (the table may pass
//     4 GiB). The id is a dependent load, so each lane fetches its tile's id two tiles before
//     the rows that need it are issued (two id registers, one per tile parity). In issue order
//     id(t + 3) follows rows(t + 1), which the MFMAs of step t wait for anyway: the pipeline
//     never waits on an id alone.
//   * Entries hold real item ids. The lane that inserts score r of tile t owns position
//     p0 + 16 t + 4 gq + r, whose id another lane loaded; it re-reads it on the slow path only.
//   * The lazy exclusion runs in item-id space: a user's cursor starts at
//     lower_bound(its exclusion row, item_ids[p0]); the limit at a compaction is the id of the
//     first candidate not yet streamed (n_items at the wave's end).
//   * Any input is memory-safe: a position past the wave's end is read as the wave's last
//     candidate and never enters a list; an id outside [0, n_items) reads row 0 and never
//     enters a list. A list that is not ascending gives unspecified lists, no out-of-bounds
//     access.
//
// LDS per workgroup: 4 waves x 16 users x M x 512 B of lists = 32 / 64 / 128 KiB.
#include "batch_lists.h"
#include "score_stream.h"

namespace lg {
namespace {

constexpr int kItemsBatchMax = 16;  // users per call: one group of 16 per wave
constexpr int kItemsWaves = 4;      // waves per workgroup

template <int D, int M>
__global__ __launch_bounds__(64 * kItemsWaves) void k_score_topk_items(
    const float *__restrict__ eu, const float *__restrict__ ei,
    const int64_t *__restrict__ user_ids, int n_batch, int64_t n_table_users, int n_items,
    const int32_t *__restrict__ item_ids, int64_t n_cand,
    const int64_t *__restrict__ ex_rowptr, const int32_t *__restrict__ ex_col,
    float mask_value, int k, int64_t pos_per_wave, float *__restrict__ out_val,
    int64_t *__restrict__ out_idx, float *__restrict__ part_val,
    int32_t *__restrict__ part_idx) {
  constexpr int Q = D / 4;
  constexpr int LT = Q / 4;  // 16-byte loads per tile per lane
  constexpr int CAP = 64 * M;
  constexpr int WAVES = kItemsWaves;
  __shared__ float cs[WAVES][16][CAP];
  __shared__ int ci[WAVES][16][CAP];
  __shared__ int exs[WAVES][64];
  __shared__ int ncs[WAVES][16];  // entries of each final list

  // (readfirstlane: the wave's range and tile count are then scalar to hipcc, the loop's exits
  // uniform branches. With a per-lane count the exits are exec masks, the control-flow graph
  // has an edge from the even step straight to the loop header, and hipcc's wait for that
  // path -- every load in flight, the ids two tiles ahead included -- lands in each even step.)
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / 64);
  const int lane = lane_id();
  const int ul = lane & 15;
  const int gq = lane >> 4;
  // the wave's candidate positions (every wave stays to the end: the workgroup's barriers)
  int64_t p0 = ((int64_t)blockIdx.x * WAVES + wave) * pos_per_wave;
  if (p0 > n_cand) p0 = n_cand;
  int64_t p1 = p0 + pos_per_wave;
  if (p1 > n_cand) p1 = n_cand;
  const int n_valid = (int)(p1 - p0);   // candidates of this wave
  const int n_t = (n_valid + 15) / 16;  // tiles of this wave
  const int32_t *__restrict__ ids = item_ids + p0;

  float uf[Q];
  // an id outside the table is clamped (row 0 is read instead) and its list stays empty
  int64_t u = 0;
  bool uvalid = ul < n_batch;
  if (uvalid) {
    u = user_ids ? user_ids[ul] : (int64_t)ul;
    uvalid = u >= 0 && u < n_table_users;
    if (!uvalid) u = 0;
  }
  load_piece<Q>(eu + u * D + gq * Q, uf);
  int64_t ex_pos = 0, ex_hi = 0;
  if (ex_rowptr && uvalid && n_valid > 0) {
    ex_hi = ex_rowptr[u + 1];
    // the user's first excluded item at or past the wave's first candidate
    ex_pos = lower_bound_i32(ex_col, ex_rowptr[u], ex_hi, ids[0]);
  }
  int cnt = 0, chk = 0;
  float thr = uvalid ? neg_inf<float>() : __builtin_huge_valf();
  const uint64_t same_user = 0x0001000100010001ull << ul;

  // Compact user b, all of whose items so far are below lim (an item id): the entries
  // [chk, n) added since its last compaction get the lazy exclusion, then the best k stay.
  auto compact_user = [&](int b, int lim) __attribute__((always_inline)) {
    const int n = __shfl(cnt, b);
    const int c0 = __shfl(chk, b);
    int64_t pos = __shfl(ex_pos, b);
    const int64_t hi = __shfl(ex_hi, b);
    float *ks = &cs[wave][b][0];
    int *is = &ci[wave][b][0];
    pos = mask_excluded_run(
        ex_col, pos, hi, lim, exs, wave, c0, n, [&](int j) { return is[j]; },
        [&](int j) { ks[j] = mask_value; });
    float t;
    int tid;
    const int nc = wave_compact<float, M>(ks, is, n, k, t, tid);
    if (ul == b) {
      cnt = nc;
      chk = nc;
      ex_pos = pos;
      thr = entry_thr(uvalid, mask_value, t);
    }
  };

  // this lane's item of tile t; past the wave's end the wave's last candidate again (no
  // branch: its scores are dropped by the position test of insert_tile). Needs n_valid > 0.
  const int last = n_valid - 1;
  auto id_at = [&](int t) __attribute__((always_inline)) {
    const int p = t * 16 + ul;
    return ids[p < last ? p : last];
  };
  // piece gq of row `id` (row 0 for an id outside the table): 64-bit address
  auto load_rows = [&](int id, f32x4(&af)[LT]) __attribute__((always_inline)) {
    const int64_t row = (unsigned)id < (unsigned)n_items ? id : 0;
    const f32x4 *rp = reinterpret_cast<const f32x4 *>(ei + row * D + gq * Q);
#pragma unroll
    for (int t = 0; t < LT; ++t) af[t] = rp[t];
  };

  // acc[r] = score(user slot ul, candidate position p0 + 16t + 4gq + r)
  auto mfma_tile = [&](const f32x4(&af)[LT], f32x4 &acc) __attribute__((always_inline)) {
    acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < Q; ++s)
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(af[s / 4][s % 4], uf[s], acc, 0, 0, 0);
  };

  // Slow path, taken when some lane of the wave has a candidate in tile t.
  auto insert_tile = [&](int t, const f32x4 &acc) __attribute__((always_inline)) {
    const int rel = t * 16 + gq * 4;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float sc = acc[r];
      bool cand = rel + r < n_valid && sc > thr;
      int id = 0;
      if (cand) {
        id = ids[rel + r];
        cand = (unsigned)id < (unsigned)n_items;
      }
      const uint64_t bal = __ballot(cand);
      if (bal) {
        const int pos = cnt + __popcll(bal & same_user & lanemask_lt());
        if (cand) {
          cs[wave][ul][pos] = sc;
          ci[wave][ul][pos] = id;
        }
        cnt += __popcll(bal & same_user);
      }
    }
  };

  // compact every user whose list could overflow on the next tile (+16 max per tile); the
  // limit is the id of the first candidate behind tile t
  auto maybe_compact = [&](int t) __attribute__((always_inline)) {
    uint64_t need = __ballot(cnt > CAP - 16) & 0xffffull;
    if (need == 0) return;
    const int nxt = (t + 1) * 16;
    const int lim = nxt < n_valid ? ids[nxt] : n_items;
    wave_sync();
    while (need) {
      const int b = __ffsll((long long)need) - 1;
      need &= need - 1;
      compact_user(b, lim);
    }
  };

  if (n_t > 0) {
    f32x4 afA[LT], afB[LT];
    f32x4 accA, accB;
    const int id0 = id_at(0), id1 = id_at(1), id2 = id_at(2);
    int idB = id_at(3), idA = id_at(4);
    load_rows(id0, afA);
    load_rows(id1, afB);
    mfma_tile(afA, accA);
    load_rows(id2, afA);
    // Retire the prologue's loads with a wait hipcc sees (vmcnt(0)): it issues tile 2's loads
    // before tile 1's here, and merging that order with the loop's own at the loop header it
    // would wait in every even step as if tile t + 1 were the youngest load in flight.
    __builtin_amdgcn_s_waitcnt(0x0F70);
    // invariant at step t: acc[t%2] = tile t; buffer (t+1)%2 = tile t+1 (landed or in
    // flight); buffer t%2 = tile t+2 in flight; id[(t+1)%2] = tile t+3's, id[t%2] = tile t+4's.
    // Tiles go in pairs and the loop has ONE exit: an odd tile count is rounded up (the extra
    // tile repeats the wave's last candidate and inserts nothing). With K2b's exit after each
    // step the structured control-flow graph has an edge from the even step back to the loop
    // header, and hipcc's wait for that path -- vmcnt(0): every load in flight, the ids two
    // tiles ahead included -- lands in every even step.
    for (int t = 0; t < n_t; t += 2) {
      // ---- even step: tile t in accA, tile t+1 in afB
      mfma_tile(afB, accB);
      bool hit = __ballot(above(max4(accA), thr)) != 0;
      load_rows(idB, afB);
      idB = id_at(t + 5);
      if (hit) insert_tile(t, accA);
      maybe_compact(t);
      // ---- odd step: tile t+1 in accB, tile t+2 in afA
      mfma_tile(afA, accA);
      hit = t + 1 < n_t && __ballot(above(max4(accB), thr)) != 0;
      load_rows(idA, afA);
      idA = id_at(t + 6);
      if (hit) insert_tile(t + 1, accB);
      maybe_compact(t + 1);
    }
  }

  // the wave's final lists: the best k of each user, sorted, ncs entries
  wave_sync();
  for (int b = 0; b < n_batch; ++b) {
    compact_user(b, n_items);
    const int nc = __shfl(cnt, b);
    if (lane == 0) ncs[wave][b] = nc;
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

template <int D>
void dispatch_items(int m, int blocks, const float *eu, const float *ei, const int64_t *user_ids,
                    int n_batch, int64_t n_table_users, int n_items, const int32_t *item_ids,
                    int64_t n_cand, const int64_t *ex_rowptr, const int32_t *ex_col,
                    float mask_value, int k, int64_t ppw, float *out_val, int64_t *out_idx,
                    float *part_val, int32_t *part_idx, hipStream_t stream) {
#define LG_ITEMS_CASE(MM)                                                                      \
  if (m == MM)                                                                                 \
    return k_score_topk_items<D, MM>                                                           \
        <<<dim3((unsigned)blocks), dim3(64 * kItemsWaves), 0, stream>>>(                       \
            eu, ei, user_ids, n_batch, n_table_users, n_items, item_ids, n_cand, ex_rowptr,    \
            ex_col, mask_value, k, ppw, out_val, out_idx, part_val, part_idx);
  LG_ITEMS_CASE(1) LG_ITEMS_CASE(2) LG_ITEMS_CASE(4)
#undef LG_ITEMS_CASE
}

}  // namespace
}  // namespace lg

using namespace lg;

extern "C" size_t lg_score_topk_batch_items_ws_bytes(int64_t n_batch, int64_t n_cand,
                                                     int32_t dim, int32_t k) {
  if (n_batch < 1 || n_batch > kItemsBatchMax || n_cand < 1 || n_cand >= 0x7fffffff || k < 1 ||
      k > 128 || !(dim == 32 || dim == 64 || dim == 128))
    return 0;
  return list_ws_bytes(n_cand, n_batch, k);
}

extern "C" int lg_score_topk_batch_items_f32(
    const float *eu, const float *ei, const int64_t *user_ids, int64_t n_batch,
    int64_t n_table_users, int64_t n_items, const int32_t *item_ids, int64_t n_cand, int32_t dim,
    const int64_t *ex_rowptr, const int32_t *ex_col, float mask_value, int32_t k, float *out_val,
    int64_t *out_idx, void *ws, size_t ws_bytes, lg_stream_t stream) {
  const char *me = "lg_score_topk_batch_items_f32";
  LG_REQUIRE(n_cand >= 1 && n_cand <= n_items, "%s: n_cand=%lld not in [1, n_items=%lld]", me,
             (long long)n_cand, (long long)n_items);
  const int st0 = check_list_args(me, eu && ei && item_ids && out_val && out_idx, n_batch,
                                  kItemsBatchMax, n_table_users, n_items, dim, k, ex_rowptr,
                                  ex_col, ws, ws_bytes,
                                  lg_score_topk_batch_items_ws_bytes(n_batch, n_cand, dim, k));
  if (st0 != LG_OK) return st0;
  const int cus = device_cus();
  if (cus <= 0) {
    set_error("%s: no device", me);
    return LG_ERR_ARG;
  }
  // K2b's grid over the candidate positions
  const int m = list_cap_m(k), waves = kItemsWaves;
  const ListGrid grid = plan_list_grid(n_cand, cus, waves, waves * m);
  const int64_t blocks = grid.blocks, ppw = grid.per_wave;
  const ListParts part = split_list_ws(ws, blocks, n_batch, k);
  hipStream_t s = (hipStream_t)stream;
  switch (dim) {
    case 32: dispatch_items<32>(m, (int)blocks, eu, ei, user_ids, (int)n_batch, n_table_users, (int)n_items, item_ids, n_cand, ex_rowptr, ex_col, mask_value, k, ppw, out_val, out_idx, part.val, part.idx, s); break;
    case 64: dispatch_items<64>(m, (int)blocks, eu, ei, user_ids, (int)n_batch, n_table_users, (int)n_items, item_ids, n_cand, ex_rowptr, ex_col, mask_value, k, ppw, out_val, out_idx, part.val, part.idx, s); break;
    default: dispatch_items<128>(m, (int)blocks, eu, ei, user_ids, (int)n_batch, n_table_users, (int)n_items, item_ids, n_cand, ex_rowptr, ex_col, mask_value, k, ppw, out_val, out_idx, part.val, part.idx, s); break;
  }
  const int st = launch_status(me);
  if (st != LG_OK || blocks == 1) return st;
  return launch_batch_merge(part.val, part.idx, (int)n_batch, k, (int)blocks, out_val, out_idx, s,
                            "lg_score_topk_batch_items_f32(merge)");
}
