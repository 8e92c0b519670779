// K2k: the rank of given (user, item) pairs over the FULL catalog, gfx950 f32 MFMA.
//
// What an evaluation asks first and no top-K list answers past position k: where does a user's
// held-out item stand among all items? For a target pair (u, i)
//     rank(u, i) = #{ j in [0, n_items), j != i : better(v(u, j), j, v(u, i), i) }   (0 = first)
// with v(u, j) = mask_value where j is in u's exclusion row, else the fp32 chain score of
// lg_score_topk_f32 (k_score_topk's chain, csrc/topk_plain.hip; oracle/score_chain.c), and
// better(a, ja, b, jb) = a > b || (a == b && ja < jb), the order of every top-K list here: for
// finite scores rank < k iff lg_score_topk_f32's list holds i at position rank.
//
// Three launches, no list, no LDS, no atomics:
//
//   1. k_rank_targets   one wave per row: the row's (at most LG_RANK_ROW_MAX) target scores by
//                       K2c's pair chain (k_score_cand, csrc/topk_cand.hip: the user in every MFMA
//                       column, the target rows gathered as the A operand). out_score gets v(u, i);
//                       the workspace gets, per (row, slot), the threshold t = v(u, i) -- NaN for a
//                       slot that does not rank, which no score is above or equal to -- and the id.
//   2. k_rank_count     k_score_topk's stream with another consumer: 16 rows per MFMA column group,
//                       NG groups per wave, the load_item_tile double buffer, items in n_splits
//                       ranges. The count runs on RAW scores (no exclusion load in the loop): per
//                       (score s, threshold t) cnt += (s > t), one compare and one carry-add in the
//                       MFMA shadow; s == t anywhere in the wave (rare; the target's own item is
//                       one) takes a ballot-guarded slow path that applies j < i with the real ids.
//                       j == i counts only where raw(u, i) > t, i.e. for an excluded target, and
//                       step 3 takes it out again. A wave keeps 1, 2 or 4 thresholds per row,
//                       the fewest that hold its rows' last ranking slot. Lane counts are int32,
//                       summed over the four k-slot lanes of a column and written per (split,
//                       row, slot).
//   3. k_rank_finish    one wave per row: sums the splits' counts (integers: the result does not
//                       depend on n_splits) and walks the row's exclusion run, 16 excluded items
//                       per pair-chain tile: for an excluded e and a target (t, i)
//                         rank += [e != i] better(mask_value, e, t, i) - better(raw(u, e), e, t, i)
//                       where raw(u, e) is the same chain as the stream's, bit for bit (tested with
//                       an excluded duplicate of a target's embedding row). Exact; it keeps every
//                       exclusion load out of step 2.
//
// Any input is memory-safe: a user id outside the table reads row 0 and its row is all {-1,
// -inf}; a target id outside [0, n_items) reads row 0 and gets {-1, -inf}; positions >=
// max_targets of a row get {-1, -inf}; an excluded id outside [0, n_items) is skipped.
//
// Like every K2 kernel this one keeps its own text of the pipeline (score_stream.h says why).
#include <type_traits>

#include "score_stream.h"

namespace lg {
namespace {

constexpr int kRankWaves = 4;        // waves per workgroup of k_rank_count
constexpr int kRankNG = 2;           // 16-row groups per wave
constexpr int kRankRowWaves = 4;     // rows (one wave each) per workgroup of steps 1 and 3
constexpr int kRankSplitsMax = 4096;

// the workspace: thr f32 [slots], tid i32 [slots], part i32 [n_splits][slots]; slots = n_rows x
// max_targets, slot (r, m) at r max_targets + m
struct RankWs {
  float *thr;
  int32_t *tid;
  int32_t *part;
};

__device__ __forceinline__ bool better(float a, int ja, float b, int jb) {
  return a > b || (a == b && ja < jb);
}

// Pair chain of one 16-position tile: acc[r] = score(user, row 4 gq + r of the tile), the same in
// every column; lane (ul < 4, gq) takes position 4 gq + ul (k_score_cand's layout).
template <int D>
__device__ __forceinline__ float pair_tile_score(const float *__restrict__ ei, int64_t row,
                                                 const float (&uf)[D / 4], int ul, int gq) {
  constexpr int Q = D / 4;
  float af[Q];
  load_piece<Q>(ei + row * D + gq * Q, af);
  f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int st = 0; st < Q; ++st)
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(af[st], uf[st], acc, 0, 0, 0);
  return (ul & 2) ? ((ul & 1) ? acc[3] : acc[2]) : ((ul & 1) ? acc[1] : acc[0]);
}

__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// Step 1. One wave per row; the row's first min(len, max_targets) targets are one tile.
template <int D>
__global__ __launch_bounds__(64 * kRankRowWaves) void k_rank_targets(
    const float *__restrict__ eu, const float *__restrict__ ei,
    const int64_t *__restrict__ user_ids, int64_t n_rows, int64_t n_table_users, int n_items,
    const int64_t *__restrict__ tgt_rowptr, const int32_t *__restrict__ tgt_col, int max_targets,
    const int64_t *__restrict__ ex_rowptr, const int32_t *__restrict__ ex_col, float mask_value,
    float *__restrict__ out_score, RankWs ws) {
  constexpr int Q = D / 4;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / 64);
  const int lane = lane_id();
  const int ul = lane & 15;
  const int gq = lane >> 4;
  const int64_t r = (int64_t)blockIdx.x * kRankRowWaves + wave;
  if (r >= n_rows) return;
  int64_t u = user_ids ? user_ids[r] : r;
  const bool uvalid = u >= 0 && u < n_table_users;
  if (!uvalid) u = 0;
  const int64_t c0 = tgt_rowptr[r];
  int64_t full = tgt_rowptr[r + 1] - c0;  // the row's positions, all written
  if (full < 0) full = 0;
  const int len = (int)(full < max_targets ? full : max_targets);  // ... and those ranked
  const int32_t *__restrict__ ids = tgt_col + c0;
  // positions past max_targets: -inf (their rank, -1, is k_rank_finish's)
  for (int64_t p = len + lane; p < full; p += 64) out_score[c0 + p] = neg_inf<float>();
  // this lane's slot of the row: lane m < max_targets
  float thr = __builtin_nanf("");
  int tid = -1;
  if (len > 0) {
    float uf[Q];
    load_piece<Q>(eu + u * D + gq * Q, uf);
    // this lane's row of the tile (past the end: the last target again)
    const int idl = ids[ul < len ? ul : len - 1];
    const int64_t row = (unsigned)idl < (unsigned)n_items ? idl : 0;
    float sc = pair_tile_score<D>(ei, row, uf, ul, gq);
    // lane (ul < 4, gq = 0) owns position ul: the slot's lane itself (LG_RANK_ROW_MAX <= 4)
    if (lane < len) {
      const int id = ids[lane];
      if (uvalid && (unsigned)id < (unsigned)n_items) {
        if (ex_rowptr) {
          const int64_t lo = ex_rowptr[u], hi = ex_rowptr[u + 1];
          const int64_t x = lower_bound_i32(ex_col, lo, hi, id);
          if (x < hi && ex_col[x] == id) sc = mask_value;
        }
        thr = sc;
        tid = id;
        out_score[c0 + lane] = sc;
      } else {
        out_score[c0 + lane] = neg_inf<float>();
      }
    }
  }
  if (lane < max_targets) {
    ws.thr[r * max_targets + lane] = thr;
    ws.tid[r * max_targets + lane] = tid;
  }
}

// Step 2. One wave: NG groups of 16 rows against the items [i0, i1) of its split; the block's
// waves work independently. The software pipeline is k_score_topk's (one 16-item tile per step:
// the MFMAs of tile t + 1 interleave with the count of tile t, each tile's loads are in flight
// for two steps, all loads compiler-visible). The loop exists for MT = 1, 2 and 4 thresholds per
// row; a wave takes the narrowest that holds its rows' last ranking slot, so rows of one target
// (leave-one-out evaluation) pay one compare per score whatever max_targets is.
template <int D>
__global__ __launch_bounds__(64 * kRankWaves) void k_rank_count(
    const float *__restrict__ eu, const float *__restrict__ ei,
    const int64_t *__restrict__ user_ids, int64_t n_rows, int64_t n_table_users, int64_t n_items,
    int max_targets, int n_splits, int64_t items_per_split, RankWs ws) {
  constexpr int Q = D / 4;
  constexpr int LT = Q / 4;  // buffer loads per tile per lane
  constexpr int NG = kRankNG;
  constexpr int MTX = LG_RANK_ROW_MAX;
  const int wave = threadIdx.x / 64;
  const int lane = lane_id();
  const int ul = lane & 15;
  const int gq = lane >> 4;
  const int64_t tile = blockIdx.x / n_splits;
  const int split = blockIdx.x % n_splits;
  const int64_t rbase = (tile * kRankWaves + wave) * (16 * NG);
  if (rbase >= n_rows) return;  // wave-uniform; no block-level barriers below
  const int64_t i0 = (int64_t)split * items_per_split;
  int64_t i1 = i0 + items_per_split;
  if (i1 > n_items) i1 = n_items;
  const int n_valid = i1 > i0 ? (int)(i1 - i0) : 0;  // items of this split
  const int n_full = n_valid / 16;                    // full tiles of this split

  // thresholds: NaN (nothing is above or equal to it) for padding rows and unused slots
  float thr_x[NG][MTX];
  int cnt_x[NG][MTX];
  int64_t slot0[NG];
  bool rvalid[NG];
  int live = 0;  // this lane's last live slot + 1
#pragma unroll
  for (int g = 0; g < NG; ++g) {
    const int64_t r = rbase + g * 16 + ul;
    rvalid[g] = r < n_rows;
    slot0[g] = (rvalid[g] ? r : 0) * max_targets;
#pragma unroll
    for (int m = 0; m < MTX; ++m) {
      thr_x[g][m] = rvalid[g] && m < max_targets ? ws.thr[slot0[g] + m] : __builtin_nanf("");
      cnt_x[g][m] = 0;
      if (thr_x[g][m] == thr_x[g][m] && live <= m) live = m + 1;
    }
  }
  // the wave's last live slot + 1; 0: none of its rows has a ranking target (rows without
  // targets, the padding rows of a split plan) and it streams nothing
  const int need = __ballot(live > 2) ? 4 : (__ballot(live > 1) ? 2 : (__ballot(live > 0) ? 1 : 0));

  if (need > 0 && n_valid > 0) {
    float uf[NG][Q];
#pragma unroll
    for (int g = 0; g < NG; ++g) {
      const int64_t r = rbase + g * 16 + ul;
      int64_t u = !rvalid[g] ? 0 : (user_ids ? user_ids[r] : r);
      if (u < 0 || u >= n_table_users) u = 0;  // (its thresholds are NaN)
      load_piece<Q>(eu + u * D + gq * Q, uf[g]);
    }

    const int voff = (ul * D + gq * Q) * 4;
    // retire the prologue loads with a wait hipcc sees (vmcnt(0)), as k_score_topk does
    __builtin_amdgcn_s_waitcnt(0x0F70);

    // acc[g][r] = score(row rbase + 16g + ul, item i0 + 16t + 4gq + r)
    auto mfma_tile = [&](const f32x4(&af)[LT], f32x4(&acc)[NG]) __attribute__((always_inline)) {
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

    // The stream with MT thresholds per row (mt: std::integral_constant<int, MT>).
    auto run = [&](auto mt) __attribute__((always_inline)) {
      constexpr int MT = decltype(mt)::value;
      float thr[NG][MT];
      int cnt[NG][MT];
#pragma unroll
      for (int g = 0; g < NG; ++g)
#pragma unroll
        for (int m = 0; m < MT; ++m) {
          thr[g][m] = thr_x[g][m];
          cnt[g][m] = 0;
        }

      // The count of a full tile: a compare and a carry-add per (score, threshold), no branch (the
      // step stays one basic block beside the MFMAs of the next tile); true when some score of
      // the wave equals a threshold.
      auto count_tile = [&](const f32x4(&acc)[NG]) __attribute__((always_inline)) {
        bool eq = false;
#pragma unroll
        for (int g = 0; g < NG; ++g)
#pragma unroll
          for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              cnt[g][m] += acc[g][r] > thr[g][m] ? 1 : 0;
              eq |= acc[g][r] == thr[g][m];
            }
        return __ballot(eq) != 0;
      };

      // A hint to hipcc's scheduler for one step: after every MFMA of the next tile its share of
      // the count's vector instructions (8 register reads of the result, 2.5 per (score, threshold)
      // for the two compares, the select and the carry-add). Left alone it issues the MFMAs back to
      // back and the whole count behind them, every carry-add one wait state after its compare.
      // Only for MT = 4: with one threshold the hinted order measured 5 % slower than hipcc's own
      // (it puts dependent MFMAs back to back), with four 4 % faster
      // (profiles/score_rank_hint_ab.json).
      auto interleave = [&]() __attribute__((always_inline)) {
        if constexpr (MT < 4) return;
        constexpr int kValu = (8 * NG + 10 * NG * MT + Q * NG - 1) / (Q * NG);
#pragma unroll
        for (int i = 0; i < Q * NG; ++i) {
          __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);      // one MFMA
          __builtin_amdgcn_sched_group_barrier(0x002, kValu, 0);  // kValu VALU
        }
      };

      // Slow path: an item whose score equals a threshold is above the target when its id is lower.
      auto count_ties = [&](int t, const f32x4(&acc)[NG]) __attribute__((always_inline)) {
        const int rel = t * 16 + gq * 4;
#pragma unroll
        for (int g = 0; g < NG; ++g)
#pragma unroll
          for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int r = 0; r < 4; ++r)
              if (acc[g][r] == thr[g][m] && rel + r < n_valid) {
                const int item = (int)i0 + rel + r;
                cnt[g][m] += item < ws.tid[slot0[g] + m] ? 1 : 0;  // (a live slot: m < max_targets)
              }
      };

      if (n_full > 0) {
        f32x4 afA[LT], afB[LT];
        f32x4 accA[NG], accB[NG];
        load_item_tile<D>(ei, n_items, i0, voff, afA);
        load_item_tile<D>(ei, n_items, i0 + 16, voff, afB);
        mfma_tile(afA, accA);
        load_item_tile<D>(ei, n_items, i0 + 32, voff, afA);
        // invariant at step t: acc[t%2] = tile t; buffer (t+1)%2 = tile t+1 (landed or in flight);
        // buffer t%2 = tile t+2 in flight
        for (int t = 0;; t += 2) {
          // ---- even step: tile t in accA, tile t+1 in afB
          mfma_tile(afB, accB);
          bool hit = count_tile(accA);
          load_item_tile<D>(ei, n_items, i0 + (int64_t)(t + 3) * 16, voff, afB);
          interleave();
          if (hit) count_ties(t, accA);
          if (t + 1 >= n_full) break;
          // ---- odd step: tile t+1 in accB, tile t+2 in afA
          mfma_tile(afA, accA);
          hit = count_tile(accB);
          load_item_tile<D>(ei, n_items, i0 + (int64_t)(t + 4) * 16, voff, afA);
          interleave();
          if (hit) count_ties(t + 1, accB);
          if (t + 2 >= n_full) break;
        }
      }
      // The table's last tile may be partial (splits are multiples of 16 items): its rows past the
      // end load as zeros and take -inf here, outside the loop (count_ties checks the position).
      if (n_valid & 15) {
        f32x4 af[LT];
        f32x4 acc[NG];
        load_item_tile<D>(ei, n_items, i0 + (int64_t)n_full * 16, voff, af);
        mfma_tile(af, acc);
        const int left = (n_valid & 15) - gq * 4;  // valid scores of this lane
#pragma unroll
        for (int g = 0; g < NG; ++g)
#pragma unroll
          for (int r = 0; r < 4; ++r)
            if (r >= left) acc[g][r] = neg_inf<float>();
        if (count_tile(acc)) count_ties(n_full, acc);
      }
#pragma unroll
      for (int g = 0; g < NG; ++g)
#pragma unroll
        for (int m = 0; m < MT; ++m) cnt_x[g][m] = cnt[g][m];
    };  // run

    if (need == 1) run(std::integral_constant<int, 1>{});
    else if (need == 2) run(std::integral_constant<int, 2>{});
    else run(std::integral_constant<int, MTX>{});
  }

  // the split's counts: summed over the four k-slot lanes of a column, one writer per slot
  int32_t *__restrict__ part = ws.part + (int64_t)split * n_rows * max_targets;
#pragma unroll
  for (int g = 0; g < NG; ++g)
#pragma unroll
    for (int m = 0; m < MTX; ++m) {
      int c = cnt_x[g][m];
      c += __shfl_xor(c, 16);
      c += __shfl_xor(c, 32);
      if (gq == 0 && rvalid[g] && m < max_targets) part[slot0[g] + m] = c;
    }
}

// Step 3. One wave per row: ranks = the splits' counts + the exclusion correction.
template <int D>
__global__ __launch_bounds__(64 * kRankRowWaves) void k_rank_finish(
    const float *__restrict__ eu, const float *__restrict__ ei,
    const int64_t *__restrict__ user_ids, int64_t n_rows, int64_t n_table_users, int n_items,
    const int64_t *__restrict__ tgt_rowptr, int max_targets,
    const int64_t *__restrict__ ex_rowptr, const int32_t *__restrict__ ex_col, float mask_value,
    int n_splits, int64_t *__restrict__ out_rank, RankWs ws) {
  constexpr int Q = D / 4;
  constexpr int MT = LG_RANK_ROW_MAX;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / 64);
  const int lane = lane_id();
  const int ul = lane & 15;
  const int gq = lane >> 4;
  const int64_t r = (int64_t)blockIdx.x * kRankRowWaves + wave;
  if (r >= n_rows) return;
  int64_t u = user_ids ? user_ids[r] : r;
  if (u < 0 || u >= n_table_users) u = 0;  // (its slots do not rank)
  const int64_t c0 = tgt_rowptr[r];
  int64_t full = tgt_rowptr[r + 1] - c0;
  if (full < 0) full = 0;
  const int len = (int)(full < max_targets ? full : max_targets);
  for (int64_t p = len + lane; p < full; p += 64) out_rank[c0 + p] = -1;
  if (len == 0) return;

  // the row's thresholds (wave-uniform values) and whether any slot ranks
  float thr[MT];
  int tid[MT];
  int d[MT];
  bool any = false;
#pragma unroll
  for (int m = 0; m < MT; ++m) {
    thr[m] = m < len ? ws.thr[r * max_targets + m] : __builtin_nanf("");
    tid[m] = m < len ? ws.tid[r * max_targets + m] : -1;
    d[m] = 0;
    any |= tid[m] >= 0;
  }
  if (any && ex_rowptr) {
    const int64_t lo = ex_rowptr[u], hi = ex_rowptr[u + 1];
    if (lo < hi) {
      float uf[Q];
      load_piece<Q>(eu + u * D + gq * Q, uf);
      for (int64_t t = lo; t < hi; t += 16) {
        // this lane's row of the tile (past the end: the run's last item again)
        const int el = ex_col[t + ul < hi ? t + ul : hi - 1];
        const int64_t row = (unsigned)el < (unsigned)n_items ? el : 0;
        const float sc = pair_tile_score<D>(ei, row, uf, ul, gq);
        const int64_t p = t + gq * 4 + (ul & 3);
        if (ul < 4 && p < hi) {
          const int e = ex_col[p];
          if ((unsigned)e < (unsigned)n_items) {
#pragma unroll
            for (int m = 0; m < MT; ++m)
              if (tid[m] >= 0)
                d[m] += (e != tid[m] && better(mask_value, e, thr[m], tid[m]) ? 1 : 0) -
                        (better(sc, e, thr[m], tid[m]) ? 1 : 0);
          }
        }
      }
    }
  }
#pragma unroll
  for (int m = 0; m < MT; ++m) {
    if (m >= len) break;  // (uniform)
    int c = d[m];
    if (tid[m] >= 0)
      for (int s = lane; s < n_splits; s += 64)
        c += ws.part[((int64_t)s * n_rows + r) * max_targets + m];
    c = wave_sum(c);
    if (lane == 0) out_rank[c0 + m] = tid[m] >= 0 ? (int64_t)c : -1;
  }
}

// workgroups of k_rank_count, 0 when past the grid limit
int64_t rank_blocks(int64_t n_rows, int64_t n_splits) {
  constexpr int64_t per = (int64_t)kRankWaves * kRankNG * 16;
  if (n_rows < 1 || n_splits < 1 || n_rows > ((int64_t)1 << 40)) return 0;
  const int64_t tiles = (n_rows + per - 1) / per;
  if (tiles > (int64_t)0x7fffffff / n_splits) return 0;
  // (steps 1 and 3: one wave per row, kRankRowWaves per workgroup)
  if ((n_rows + kRankRowWaves - 1) / kRankRowWaves > 0x7fffffff) return 0;
  return tiles * n_splits;
}

template <int D>
void launch_rank(const float *eu, const float *ei, const int64_t *user_ids, int64_t n_rows,
                 int64_t n_table_users, int64_t n_items, const int64_t *tgt_rowptr,
                 const int32_t *tgt_col, int max_targets, const int64_t *ex_rowptr,
                 const int32_t *ex_col, float mask_value, int ns, int64_t per, int64_t *out_rank,
                 float *out_score, RankWs ws, hipStream_t s) {
  const dim3 rows((unsigned)((n_rows + kRankRowWaves - 1) / kRankRowWaves));
  const dim3 rblock(64 * kRankRowWaves);
  k_rank_targets<D><<<rows, rblock, 0, s>>>(eu, ei, user_ids, n_rows, n_table_users,
                                            (int)n_items, tgt_rowptr, tgt_col, max_targets,
                                            ex_rowptr, ex_col, mask_value, out_score, ws);
  const dim3 grid((unsigned)rank_blocks(n_rows, ns)), block(64 * kRankWaves);
  k_rank_count<D><<<grid, block, 0, s>>>(eu, ei, user_ids, n_rows, n_table_users, n_items,
                                         max_targets, ns, per, ws);
  k_rank_finish<D><<<rows, rblock, 0, s>>>(eu, ei, user_ids, n_rows, n_table_users, (int)n_items,
                                           tgt_rowptr, max_targets, ex_rowptr, ex_col, mask_value,
                                           ns, out_rank, ws);
}

}  // namespace
}  // namespace lg

using namespace lg;

static_assert(LG_RANK_ROW_MAX == 4, "k_rank_targets and k_rank_count's cases assume 4");

extern "C" size_t lg_score_rank_ws_bytes(int64_t n_rows, int64_t n_targets, int32_t dim,
                                         int32_t n_splits) {
  if (n_targets < 1 || n_targets > ((int64_t)1 << 42) || n_splits < 1 ||
      n_splits > kRankSplitsMax || !(dim == 32 || dim == 64 || dim == 128) ||
      rank_blocks(n_rows, n_splits) == 0)
    return 0;
  return (size_t)n_targets * (sizeof(float) + sizeof(int32_t) + (size_t)n_splits * sizeof(int32_t));
}

extern "C" int lg_score_rank_f32(const float *eu, const float *ei, const int64_t *user_ids,
                                 int64_t n_rows, int64_t n_table_users, int64_t n_items,
                                 const int64_t *tgt_rowptr, const int32_t *tgt_col,
                                 int32_t max_targets, int32_t dim, const int64_t *ex_rowptr,
                                 const int32_t *ex_col, float mask_value, int32_t n_splits,
                                 int64_t *out_rank, float *out_score, void *ws, size_t ws_bytes,
                                 lg_stream_t stream) {
  const char *me = "lg_score_rank_f32";
  LG_REQUIRE(eu && ei && tgt_rowptr && tgt_col && out_rank && out_score, "%s: null pointer", me);
  LG_REQUIRE(n_rows >= 1, "%s: n_rows=%lld must be >= 1", me, (long long)n_rows);
  LG_REQUIRE(n_table_users >= 1, "%s: n_table_users must be >= 1", me);
  LG_REQUIRE(n_items > 0 && n_items < 0x7fffffff, "%s: n_items must be in [1, 2^31-1)", me);
  LG_REQUIRE(max_targets >= 1 && max_targets <= LG_RANK_ROW_MAX, "%s: max_targets=%d not in [1,%d]",
             me, max_targets, LG_RANK_ROW_MAX);
  LG_REQUIRE(dim == 32 || dim == 64 || dim == 128, "%s: dim %d not in {32,64,128}", me, dim);
  LG_REQUIRE(n_splits >= 1 && n_splits <= kRankSplitsMax, "%s: n_splits=%d not in [1,%d]", me,
             n_splits, kRankSplitsMax);
  LG_REQUIRE(!ex_rowptr == !ex_col, "%s: ex_rowptr/ex_col must both be set", me);
  LG_REQUIRE(rank_blocks(n_rows, n_splits) > 0,
             "%s: n_rows=%lld x %d splits is past the grid limit", me, (long long)n_rows,
             n_splits);
  // the splits in use: a multiple of 16 items each, none empty
  const int64_t per = split_len(n_items, n_splits);
  const int ns = (int)((n_items + per - 1) / per);
  const int64_t slots = n_rows * max_targets;
  const size_t need = lg_score_rank_ws_bytes(n_rows, slots, dim, ns);
  if (!ws || ws_bytes < need) {
    set_error("%s: workspace %zu < %zu bytes", me, ws_bytes, need);
    return LG_ERR_WORKSPACE;
  }
  RankWs w;
  w.thr = (float *)ws;
  w.tid = (int32_t *)(w.thr + slots);
  w.part = w.tid + slots;
  hipStream_t s = (hipStream_t)stream;
  switch (dim) {
    case 32: launch_rank<32>(eu, ei, user_ids, n_rows, n_table_users, n_items, tgt_rowptr, tgt_col, max_targets, ex_rowptr, ex_col, mask_value, ns, per, out_rank, out_score, w, s); break;
    case 64: launch_rank<64>(eu, ei, user_ids, n_rows, n_table_users, n_items, tgt_rowptr, tgt_col, max_targets, ex_rowptr, ex_col, mask_value, ns, per, out_rank, out_score, w, s); break;
    default: launch_rank<128>(eu, ei, user_ids, n_rows, n_table_users, n_items, tgt_rowptr, tgt_col, max_targets, ex_rowptr, ex_col, mask_value, ns, per, out_rank, out_score, w, s); break;
  }
  return launch_status(me);
}
