// K3s, the test-reference paths (include/lgcnhs_ref.h; lib/liblgcnhs_ref.so only, loaded by
// tests/_ref_paths.py): the per-tile build passes, the F-writing walk and the two-kernel
// top-K merge, kept as bitwise references for the product's group build (spread_build.hip)
// and fused walk (spread_tiled.hip). The product library does not carry them.
//
// The F-writing walk is k_tile_walk<MODE_F, 0, 1> of the product's kernel template, so this
// file includes the walk's source and the reference library links this object in place of
// spread_tiled.o. The other routes are worse: MODE_F instantiated in spread_tiled.hip puts a
// kernel no product path launches into the product library, and the template in a header
// leaves the file whose sha256 the walk's traffic record (profiles/pmc_traffic.json) is keyed on.
#include "spread_tiled.hip"

#include "lgcnhs_ref.h"

namespace lg {

__global__ __launch_bounds__(256) void k_tile_cursor(const int64_t *__restrict__ user_rowptr,
                                                     const int32_t *__restrict__ user_items,
                                                     int64_t n_users, int32_t item_end,
                                                     const int64_t *__restrict__ cur,
                                                     int64_t *__restrict__ end,
                                                     uint16_t *__restrict__ count) {
  const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= n_users) return;
  const int64_t p0 = cur[v];
  int64_t p = p0;
  const int64_t pe = user_rowptr[v + 1];
  while (p < pe && user_items[p] < item_end) ++p;
  end[v] = p;
  count[v] = (uint16_t)(p - p0);  // <= tile <= 8192
}

// one wave per item row
__global__ __launch_bounds__(256) void k_tile_bound(const int64_t *__restrict__ item_rowptr,
                                                    const int32_t *__restrict__ item_users,
                                                    int64_t n_items,
                                                    const uint16_t *__restrict__ count,
                                                    int64_t *__restrict__ bound) {
  const int64_t i = (int64_t)blockIdx.x * 4 + threadIdx.x / 64;
  if (i >= n_items) return;
  const int lane = lane_id();
  int64_t s = 0;
  for (int64_t e = item_rowptr[i] + lane; e < item_rowptr[i + 1]; e += 64)
    s += count[item_users[e]];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
  if (lane == 0) bound[i] = s;
}

// P rows: one wave per item row with bound[i] <= vthr pairs. Every word of the line and of
// the overflow run is written exactly once (header, pairs, zero padding), so no stale data
// of an earlier tile survives and no two stores of the wave hit one word.
__global__ __launch_bounds__(256) void k_tile_rows(
    const int64_t *__restrict__ item_rowptr, const int32_t *__restrict__ item_users,
    const int32_t *__restrict__ user_items, const uint16_t *__restrict__ user_cls,
    int64_t n_items, const int64_t *__restrict__ cur, const uint16_t *__restrict__ count,
    int32_t item_begin, const int64_t *__restrict__ bound, int64_t vthr,
    const int64_t *__restrict__ ovf_ptr, uint32_t *__restrict__ lines,
    uint32_t *__restrict__ ovf, int32_t *__restrict__ row_len) {
  const int64_t i = (int64_t)blockIdx.x * 4 + threadIdx.x / 64;
  if (i >= n_items) return;
  const int lane = lane_id();
  const int64_t nb = bound[i];
  if (nb > vthr) return;  // hub row: k_tile_rows_hub
  uint32_t *line = lines + i * 32;
  const bool has_ovf = nb > kLineSlots;
  const int64_t ou = has_ovf ? ovf_ptr[i] : 0;
  const int64_t n_units = has_ovf ? (nb - kLineSlots + 3) / 4 : 0;
  const int64_t cap = kLineSlots + 4 * n_units;
  if (has_ovf && lane < 4) ovf[ou * 4 + lane] = lane == 0 ? (uint32_t)n_units : 0u;
  for (int64_t p = nb + lane; p < cap; p += 64) put_slot(line, ovf, ou, p, 0u);
  // the pairs: users of i ascending, each user's items in the tile ascending
  int64_t n = 0;
  bool far = false;
  const int64_t e1 = item_rowptr[i + 1];
  for (int64_t e0 = item_rowptr[i]; e0 < e1; e0 += 64) {
    const int64_t e = e0 + lane;
    int32_t v = 0;
    int c = 0;
    if (e < e1) {
      v = item_users[e];
      c = count[v];
    }
    int pre = c;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int y = __shfl_up(pre, o);
      if (lane >= o) pre += y;
    }
    const int total = __shfl(pre, 63);
    pre -= c;
    if (c) {
      const int64_t s0 = cur[v];
      const uint32_t cl = (uint32_t)user_cls[v];
      far |= cl >= (uint32_t)kInvTab;
      for (int q = 0; q < c; ++q)
        put_slot(line, ovf, ou, n + pre + q,
                 (cl << 16) | (uint32_t)(user_items[s0 + q] - item_begin));
    }
    n += total;
  }
  const bool slow = __ballot(far) != 0;
  if (lane == 0) {
    line[0] = (has_ovf ? (kHdrOvf | (uint32_t)ou) : 0u) | (slow ? kHdrSlow : 0u);
    if (row_len) row_len[i] = (int32_t)nb;
  }
}

// V rows (bound > vthr pairs, hub items): one 256-thread block per row (grid-stride over the
// hub list), the tile as a dense LDS accumulator of general_W, users walked in ascending
// order as in k_spread_general, then the touched columns written as ascending entries.
__global__ __launch_bounds__(256) void k_tile_rows_hub(
    const int64_t *__restrict__ hub_rows, const int64_t *__restrict__ n_hub,
    const int64_t *__restrict__ item_rowptr, const int32_t *__restrict__ item_users,
    const int32_t *__restrict__ user_items, const double *__restrict__ inv_deg,
    const int64_t *__restrict__ cur, const uint16_t *__restrict__ count, int32_t item_begin,
    int32_t tile, const int64_t *__restrict__ ovf_ptr, uint32_t *__restrict__ lines,
    uint32_t *__restrict__ ovf, int32_t *__restrict__ row_len) {
  extern __shared__ double acc[];  // tile doubles
  __shared__ int wsum[4];
  const int64_t nh = *n_hub;
  for (int64_t h = blockIdx.x; h < nh; h += gridDim.x) {
    const int64_t i = hub_rows[h];
    for (int j = threadIdx.x; j < tile; j += blockDim.x) acc[j] = 0.0;
    __syncthreads();
    for (int64_t e = item_rowptr[i]; e < item_rowptr[i + 1]; ++e) {
      const int32_t v = item_users[e];
      const int c = count[v];
      if (c == 0) continue;  // uniform across the block: no barrier skipped unevenly
      const double wv = inv_deg[v];
      const int64_t s0 = cur[v];
      for (int q = threadIdx.x; q < c; q += blockDim.x) acc[user_items[s0 + q] - item_begin] += wv;
      __syncthreads();  // the next user may hit the same columns from other threads
    }
    uint32_t *line = lines + i * 32;
    const int64_t ou = ovf_ptr[i];
    if (threadIdx.x == 0) wsum[0] = 0;
    __syncthreads();
    {
      int c = 0;
      for (int j = threadIdx.x; j < tile; j += blockDim.x) c += acc[j] != 0.0;
      atomicAdd(&wsum[0], c);
    }
    __syncthreads();
    const int nzr = wsum[0];
    __syncthreads();
    if (hub_row_dense(nzr, tile)) {  // (tile = this tile's width here)
      write_hub_row_dense(acc, tile, line, ovf, ou, threadIdx.x, blockDim.x);
      if (threadIdx.x == 0 && row_len) row_len[i] = nzr;
      __syncthreads();
      continue;
    }
    int base = 0;
    for (int j0 = 0; j0 < tile; j0 += blockDim.x) {
      const int j = j0 + threadIdx.x;
      const bool nz = j < tile && acc[j] != 0.0;
      const uint64_t b = __ballot(nz);
      const int w = threadIdx.x / 64;
      if (lane_id() == 0) wsum[w] = __popcll(b);
      __syncthreads();
      int before_w = 0, total = 0;
      for (int q = 0; q < 4; ++q) {
        if (q < w) before_w += wsum[q];
        total += wsum[q];
      }
      if (nz) {
        const uint64_t bits = (uint64_t)__double_as_longlong(acc[j]);
        const int64_t e = base + before_w + __popcll(b & lanemask_lt());
        uint32_t *u4 = e < kLineEnts ? line + 4 * (1 + e) : ovf + 4 * (ou + 1 + (e - kLineEnts));
        *reinterpret_cast<uint4 *>(u4) =
            uint4{kEntV | (uint32_t)j, (uint32_t)bits, (uint32_t)(bits >> 32), 0u};
      }
      base += total;
      __syncthreads();
    }
    // header, the unused line units, the overflow run's header
    const bool has_ovf = base > kLineEnts;
    if (threadIdx.x < 32) {
      const int t = threadIdx.x;  // line word t
      const int unit = t / 4;
      if (t == 0) line[0] = kHdrV | kHdrSlow | (has_ovf ? (kHdrOvf | (uint32_t)ou) : 0u);
      else if (unit == 0 || unit > base) line[t] = 0u;
    }
    if (has_ovf && threadIdx.x < 4)
      ovf[ou * 4 + threadIdx.x] = threadIdx.x == 0 ? (uint32_t)(base - kLineEnts) : 0u;
    if (threadIdx.x == 0 && row_len) row_len[i] = base;
    __syncthreads();
  }
}

// Merge the tile's columns of (G *) F into running per-user top-K lists (io_val/io_idx,
// sorted, index -1 = empty). D = 0: no G factor. One wave = NG groups of 16 users (rows);
// lane (ul, gq) holds user ul of each group and items 4gq..4gq+3 of each 16-item step.
// S = the per-user list stride in LDS (entries): 40 for k <= 24 after a walk's first span
// (30 KiB blocks: 8 waves per CU, VGPR-limited), else 64*M. (A 3-slot load ring under a
// 3-waves-per-SIMD register budget spilled and ran 40 % slower.)
template <int D, int NG, int M, bool VEC, int S>
__global__ __launch_bounds__(128) void k_tile_topk(
    const double *__restrict__ F, int64_t ldf, int64_t n_rows, int32_t item_begin,
    int32_t n_cols, const float *__restrict__ eu, const float *__restrict__ ei,
    const int64_t *__restrict__ ex_rowptr, const int32_t *__restrict__ ex_col, int drop,
    int k, int first, double *__restrict__ io_val, int64_t *__restrict__ io_idx) {
  static_assert(S >= 32 && S <= 64 * M, "list stride");
  constexpr int Q = D > 0 ? D / 4 : 1;
  __shared__ double cs[2][NG][16][S];
  __shared__ int ci[2][NG][16][S];
  __shared__ int exs[2][64];
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / 64);  // uniform: SGPR bases
  const int lane = lane_id();
  const int ul = lane & 15, gq = lane >> 4;
  const int64_t ubase = ((int64_t)blockIdx.x * 2 + wave) * (16 * NG);
  if (ubase >= n_rows) return;

  float uf[NG][Q];
  bool uvalid[NG];
  int cnt[NG], chk[NG];
  bool dirty[NG];  // the user's list gained an entry in this call (first call: always)
  double thr[NG];
  int64_t ex_pos[NG], ex_hi[NG];
  const int lim_end = item_begin + n_cols;
#pragma unroll
  for (int g = 0; g < NG; ++g) {
    const int64_t r = ubase + g * 16 + ul;
    uvalid[g] = r < n_rows;
    const int64_t rr = uvalid[g] ? r : n_rows - 1;
    if (D > 0) load_piece<Q>(eu + rr * D + gq * Q, uf[g]);
    ex_pos[g] = 0;
    ex_hi[g] = 0;
    if (drop && ex_rowptr && uvalid[g]) {
      ex_pos[g] = ex_rowptr[r];
      ex_hi[g] = ex_rowptr[r + 1];
    }
    cnt[g] = 0;
    chk[g] = 0;
    dirty[g] = first != 0;
    thr[g] = uvalid[g] ? neg_inf<double>() : __builtin_huge_val();
  }
  // exclusion cursors: first excluded item >= item_begin, all groups' searches in lockstep
  // so their loads overlap; ex_next caches the item under the cursor (INT_MAX = none left)
  int32_t ex_next[NG];
  {
    int64_t lo[NG], hi[NG];
#pragma unroll
    for (int g = 0; g < NG; ++g) {
      lo[g] = ex_pos[g];
      hi[g] = ex_hi[g];
    }
    for (;;) {
      bool busy = false;
      int32_t x[NG];
#pragma unroll
      for (int g = 0; g < NG; ++g) x[g] = lo[g] < hi[g] ? ex_col[(lo[g] + hi[g]) >> 1] : 0;
#pragma unroll
      for (int g = 0; g < NG; ++g) {
        if (lo[g] < hi[g]) {
          const int64_t mid = (lo[g] + hi[g]) >> 1;
          if (x[g] < item_begin) lo[g] = mid + 1;
          else hi[g] = mid;
        }
        busy |= lo[g] < hi[g];
      }
      if (!__ballot(busy)) break;
    }
#pragma unroll
    for (int g = 0; g < NG; ++g) {
      ex_pos[g] = lo[g];
      ex_next[g] = lo[g] < ex_hi[g] ? ex_col[lo[g]] : 0x7fffffff;
    }
  }
  // running lists -> LDS (already sorted and exclusion-checked): the wave's NG*16 lists are
  // contiguous in io_*, so they are read in one pass with 8 loads per lane in flight
  if (!first) {
    const int64_t base = ubase * k;
    const int64_t lim = (n_rows - ubase) * k;
    const int total = NG * 16 * k;
    for (int t0 = 0; t0 < total; t0 += 64 * 8) {
      int64_t id[8];
      double vv[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const int t = t0 + q * 64 + lane;
        const bool in = t < total && t < lim;
        id[q] = in ? io_idx[base + t] : -1;
        vv[q] = in ? io_val[base + t] : neg_inf<double>();
      }
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const int t = t0 + q * 64 + lane;
        if (t < total) {
          const int uu = t / k, e = t - uu * k;
          cs[wave][uu >> 4][uu & 15][e] = vv[q];
          ci[wave][uu >> 4][uu & 15][e] = id[q] >= 0 ? (int)id[q] : -1;
        }
      }
    }
    wave_sync();
    // valid entries form a prefix (lists are sorted, drops written as -1 at the end): the
    // 4 lanes of a user count a quarter each
#pragma unroll
    for (int g = 0; g < NG; ++g) {
      const int *is = &ci[wave][g][ul][0];
      int nv = 0;
      for (int e = gq; e < k; e += 4) nv += is[e] >= 0;
      nv += __shfl_xor(nv, 16);
      nv += __shfl_xor(nv, 32);
      if (uvalid[g]) {
        cnt[g] = nv;
        chk[g] = nv;
        thr[g] = nv == k ? cs[wave][g][ul][k - 1] : neg_inf<double>();
      }
    }
  }
  const uint64_t same_user = 0x0001000100010001ull << ul;

  auto compact_user = [&](int g, int u, int lim) __attribute__((always_inline)) {
    const int n = __shfl(cnt[g], u);
    const int c0 = __shfl(chk[g], u);
    int64_t pos = __shfl(ex_pos[g], u);
    const int64_t hi = __shfl(ex_hi[g], u);
    int32_t nx = __shfl(ex_next[g], u);
    double *ks = &cs[wave][g][u][0];
    int *is = &ci[wave][g][u][0];
    if (n > c0 && nx < lim) {  // the cached next exclusion decides without a load
      while (pos < hi) {  // excluded items in [previous limit, lim): drop their entries
        const int64_t e = pos + lane;
        const int32_t x = e < hi ? ex_col[e] : 0x7fffffff;
        const int nin = __popcll(__ballot(x < lim));
        if (nin < 64) nx = __shfl(x, nin & 63);
        if (nin == 0) break;
        exs[wave][lane] = x;
        wave_sync();
        for (int j = c0 + lane; j < n; j += 64) {
          const int item = is[j];
          int a = 0, b = nin;
          while (a < b) {
            const int mid = (a + b) >> 1;
            if (exs[wave][mid] < item) a = mid + 1;
            else b = mid;
          }
          if (a < nin && exs[wave][a] == item) ks[j] = neg_inf<double>();
        }
        wave_sync();
        pos += nin;
        if (nin < 64) break;
      }
      if (pos >= hi) nx = 0x7fffffff;
    }
    double t;
    int tid;
    const int nc = wave_compact<double, M>(ks, is, n, k, t, tid);
    if (ul == u) {
      cnt[g] = nc;
      chk[g] = nc;
      ex_pos[g] = pos;
      ex_next[g] = nx;
      thr[g] = !uvalid[g] ? __builtin_huge_val() : t;
    }
  };

  // One 16-column step: the item fragment and the F values (clamped to valid memory, so
  // every step issues the same loads) are loaded one step ahead.
  // VEC: ldf >= n_cols rounded up to 16, so a step's 16 columns are always inside the row:
  // the step start is clamped to the last step and each lane reads its 4 columns as two
  // 16-byte loads (columns past n_cols are never inserted: process() checks c < n_cols).
  const int last_step = ((n_cols - 1) / 16) * 16;
  auto load_step = [&](int it, float(&af)[Q], double(&f)[NG][4]) __attribute__((always_inline)) {
    if constexpr (D > 0) {
      const int jc = it + ul < n_cols ? item_begin + it + ul : item_begin + n_cols - 1;
      load_piece<Q>(ei + (int64_t)jc * D + gq * Q, af);
    }
#pragma unroll
    for (int g = 0; g < NG; ++g) {
      const int64_t row = ubase + g * 16 + ul;
      const double *fr = F + (row < n_rows ? row : n_rows - 1) * ldf;
      if constexpr (VEC) {
        const int c0 = (it < last_step ? it : last_step) + gq * 4;
        const double2 a = *reinterpret_cast<const double2 *>(fr + c0);
        const double2 b = *reinterpret_cast<const double2 *>(fr + c0 + 2);
        f[g][0] = a.x;
        f[g][1] = a.y;
        f[g][2] = b.x;
        f[g][3] = b.y;
      } else {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int c = it + gq * 4 + r;
          f[g][r] = fr[c < n_cols ? c : n_cols - 1];
        }
      }
    }
  };
  auto process = [&](int it, const float(&af)[Q], const double(&f)[NG][4]) __attribute__((always_inline)) {
    double v[NG][4];
    if constexpr (D > 0) {
      f32x4 acc[NG];
#pragma unroll
      for (int g = 0; g < NG; ++g) acc[g] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int s = 0; s < Q; ++s)
#pragma unroll
        for (int g = 0; g < NG; ++g)
          acc[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[s], uf[g][s], acc[g], 0, 0, 0);
#pragma unroll
      for (int g = 0; g < NG; ++g)
#pragma unroll
        for (int r = 0; r < 4; ++r) v[g][r] = (double)acc[g][r] * f[g][r];
    } else {
#pragma unroll
      for (int g = 0; g < NG; ++g)
#pragma unroll
        for (int r = 0; r < 4; ++r) v[g][r] = f[g][r];
    }
    // fast filter: one ballot per step; the exact per-column insertion only on a hit
    const int c0 = it + gq * 4;
    bool any = false;
#pragma unroll
    for (int g = 0; g < NG; ++g)
#pragma unroll
      for (int r = 0; r < 4; ++r) any |= v[g][r] > thr[g];
    if (__ballot(any)) {
#pragma unroll
      for (int g = 0; g < NG; ++g) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const bool cand = c0 + r < n_cols && v[g][r] > thr[g];
          const uint64_t bal = __ballot(cand);
          if (bal) {
            const int p = cnt[g] + __popcll(bal & same_user & lanemask_lt());
            if (cand) {
              cs[wave][g][ul][p] = v[g][r];
              ci[wave][g][ul][p] = item_begin + c0 + r;
            }
            cnt[g] += __popcll(bal & same_user);
            dirty[g] |= (bal & same_user) != 0;
          }
        }
      }
    }
    bool over = false;
#pragma unroll
    for (int g = 0; g < NG; ++g) over |= cnt[g] > S - 16;
    if (__ballot(over)) {
      const int lim = item_begin + (it + 16 < n_cols ? it + 16 : n_cols);
#pragma unroll
      for (int g = 0; g < NG; ++g) {
        uint64_t need = __ballot(cnt[g] > S - 16) & 0xffffull;
        if (need) {
          wave_sync();
          while (need) {
            const int u = __ffsll((long long)need) - 1;
            need &= need - 1;
            compact_user(g, u, lim);
          }
        }
      }
    }
  };

  // ring of 4 register buffers: the loads of step t+3 are in flight while step t is
  // processed (F comes from HBM and is not shared between waves, so the wave needs its
  // own memory-level parallelism); past the end the loads are clamped and harmless
  float af0[Q], af1[Q], af2[Q], af3[Q];
  double f0[NG][4], f1[NG][4], f2[NG][4], f3[NG][4];
  load_step(0, af0, f0);
  load_step(16, af1, f1);
  load_step(32, af2, f2);
  for (int it = 0;; it += 64) {
    load_step(it + 48, af3, f3);
    process(it, af0, f0);
    if (it + 16 >= n_cols) break;
    load_step(it + 64, af0, f0);
    process(it + 16, af1, f1);
    if (it + 32 >= n_cols) break;
    load_step(it + 80, af1, f1);
    process(it + 32, af2, f2);
    if (it + 48 >= n_cols) break;
    load_step(it + 96, af2, f2);
    process(it + 48, af3, f3);
    if (it + 64 >= n_cols) break;
  }

  wave_sync();
#pragma unroll
  for (int g = 0; g < NG; ++g) {
    for (int u = 0; u < 16; ++u) {
      const int64_t r = ubase + g * 16 + u;
      if (r >= n_rows) break;
      if (!__shfl((int)dirty[g], u)) continue;  // list as loaded: nothing to compact or store
      compact_user(g, u, lim_end);
      const int nc = __shfl(cnt[g], u);
      for (int e = lane; e < k; e += 64) {
        const double v = e < nc ? cs[wave][g][u][e] : neg_inf<double>();
        const bool ok = e < nc && v != neg_inf<double>();  // dropped entries never surface
        io_val[r * k + e] = ok ? v : neg_inf<double>();
        io_idx[r * k + e] = ok ? ci[wave][g][u][e] : -1;
      }
      wave_sync();
    }
  }
}

template <int D, bool VEC>
static void launch_tile_topk_v(int M, const double *F, int64_t ldf, int64_t n_rows, int32_t j0,
                               int32_t n_cols, const float *eu, const float *ei,
                               const int64_t *ex_rowptr, const int32_t *ex_col, int drop,
                               int k, int first, double *io_val, int64_t *io_idx,
                               hipStream_t s) {
  // LDS per block (2 waves): 2 * NG * 16 * S * 12 B (+ 512 B) = 48 KiB (M=1, NG=2, S=64;
  // 3 blocks = 6 waves per CU), 30 KiB at S=40 (k <= 24: 8 waves per CU, VGPR-limited; the
  // list is compacted once it holds more than S-16 entries, so the first span of a walk,
  // where most columns enter, keeps S=64), 48 KiB (M=2), 96 KiB (M=4). Measured per 4096-
  // column span at 1M users: S=40 8.4-8.6 ms vs S=64 8.8-9.1 ms after the first spans,
  // 26.4 vs 16.7 ms on the first.
  if (M == 1 && k <= 24 && !first) {
    const unsigned b = (unsigned)((n_rows + 63) / 64);
    k_tile_topk<D, 2, 1, VEC, 40><<<b, 128, 0, s>>>(F, ldf, n_rows, j0, n_cols, eu, ei,
                                                    ex_rowptr, ex_col, drop, k, first, io_val,
                                                    io_idx);
  } else if (M == 1) {
    const unsigned b = (unsigned)((n_rows + 63) / 64);
    k_tile_topk<D, 2, 1, VEC, 64><<<b, 128, 0, s>>>(F, ldf, n_rows, j0, n_cols, eu, ei,
                                                    ex_rowptr, ex_col, drop, k, first, io_val,
                                                    io_idx);
  } else if (M == 2) {
    const unsigned b = (unsigned)((n_rows + 31) / 32);
    k_tile_topk<D, 1, 2, VEC, 128><<<b, 128, 0, s>>>(F, ldf, n_rows, j0, n_cols, eu, ei,
                                                     ex_rowptr, ex_col, drop, k, first, io_val,
                                                     io_idx);
  } else {
    const unsigned b = (unsigned)((n_rows + 31) / 32);
    k_tile_topk<D, 1, 4, VEC, 256><<<b, 128, 0, s>>>(F, ldf, n_rows, j0, n_cols, eu, ei,
                                                     ex_rowptr, ex_col, drop, k, first, io_val,
                                                     io_idx);
  }
}

template <int D>
static void launch_tile_topk(int M, const double *F, int64_t ldf, int64_t n_rows, int32_t j0,
                             int32_t n_cols, const float *eu, const float *ei,
                             const int64_t *ex_rowptr, const int32_t *ex_col, int drop, int k,
                             int first, double *io_val, int64_t *io_idx, hipStream_t s) {
  // 16-byte F reads need rows padded to whole steps. (An inline-asm buffer-load form of the
  // ring with hand-counted waits was measured no faster: 9.2 vs 8.9 ms per 4096-column span.)
  const bool vec = ldf >= ((int64_t)n_cols + 15) / 16 * 16 && (ldf % 2) == 0 &&
                   ((uintptr_t)F % 16) == 0;
  if (vec)
    launch_tile_topk_v<D, true>(M, F, ldf, n_rows, j0, n_cols, eu, ei, ex_rowptr, ex_col, drop, k,
                             first, io_val, io_idx, s);
  else
    launch_tile_topk_v<D, false>(M, F, ldf, n_rows, j0, n_cols, eu, ei, ex_rowptr, ex_col, drop, k,
                             first, io_val, io_idx, s);
}

}  // namespace lg

extern "C" int lg_spread_tile_cursor(const int64_t *user_rowptr, const int32_t *user_items,
                                     int64_t n_users, int32_t item_end, const int64_t *cur,
                                     int64_t *end, uint16_t *count, lg_stream_t stream) {
  LG_REQUIRE(user_rowptr && cur && end && count && n_users >= 0 && cur != end,
             "lg_spread_tile_cursor: bad arguments");
  if (n_users == 0) return LG_OK;
  k_tile_cursor<<<dim3((unsigned)((n_users + 255) / 256)), dim3(256), 0,
                  (hipStream_t)stream>>>(user_rowptr, user_items, n_users, item_end, cur, end,
                                         count);
  return launch_status("lg_spread_tile_cursor");
}

extern "C" int lg_spread_tile_bound(const int64_t *item_rowptr, const int32_t *item_users,
                                    int64_t n_items, const uint16_t *count, int64_t *bound,
                                    lg_stream_t stream) {
  LG_REQUIRE(item_rowptr && count && bound && n_items >= 0,
             "lg_spread_tile_bound: bad arguments");
  if (n_items == 0) return LG_OK;
  k_tile_bound<<<dim3((unsigned)((n_items + 3) / 4)), dim3(256), 0, (hipStream_t)stream>>>(
      item_rowptr, item_users, n_items, count, bound);
  return launch_status("lg_spread_tile_bound");
}

extern "C" size_t lg_spread_tile_rows_ws_bytes(int64_t n_items) {
  return (size_t)(n_items + 1) * sizeof(int64_t);  // hub count + hub row list
}

extern "C" int lg_spread_tile_rows_f64(const int64_t *item_rowptr, const int32_t *item_users,
                                       const int32_t *user_items, const uint16_t *user_cls,
                                       const double *inv_deg, int64_t n_items,
                                       const int64_t *cur, const uint16_t *count,
                                       int32_t item_begin, int32_t tile, const int64_t *bound,
                                       int64_t vthr, const int64_t *ovf_ptr, void *lines,
                                       void *ovf, int32_t *row_len, void *ws, size_t ws_bytes,
                                       lg_stream_t stream) {
  LG_REQUIRE(item_rowptr && user_cls && inv_deg && cur && count && bound && ovf_ptr && lines &&
                 ovf && n_items >= 0 && vthr >= kLineSlots,
             "lg_spread_tile_rows_f64: bad arguments");
  LG_REQUIRE(tile >= 1 && tile <= 8192 && item_begin >= 0,
             "lg_spread_tile_rows_f64: tile %d not in [1, 8192]", tile);
  if (n_items == 0) return LG_OK;
  const size_t need = lg_spread_tile_rows_ws_bytes(n_items);
  if (!ws || ws_bytes < need) {
    set_error("lg_spread_tile_rows_f64: workspace %zu < %zu bytes", ws_bytes, need);
    return LG_ERR_WORKSPACE;
  }
  hipStream_t s = (hipStream_t)stream;
  int64_t *n_hub = (int64_t *)ws;
  int64_t *hub_rows = n_hub + 1;
  if (hipMemsetAsync(n_hub, 0, sizeof(int64_t), s) != hipSuccess) {
    set_error("lg_spread_tile_rows_f64: hipMemsetAsync failed");
    return LG_ERR_HIP;
  }
  k_tile_rows<<<dim3((unsigned)((n_items + 3) / 4)), dim3(256), 0, s>>>(
      item_rowptr, item_users, user_items, user_cls, n_items, cur, count, item_begin, bound, vthr,
      ovf_ptr, (uint32_t *)lines, (uint32_t *)ovf, row_len);
  launch_hub_list(bound, n_items, vthr, n_hub, hub_rows, s);
  k_tile_rows_hub<<<dim3(1024), dim3(256), (size_t)tile * sizeof(double), s>>>(
      hub_rows, n_hub, item_rowptr, item_users, user_items, inv_deg, cur, count, item_begin, tile,
      ovf_ptr, (uint32_t *)lines, (uint32_t *)ovf, row_len);
  return launch_status("lg_spread_tile_rows_f64");
}

extern "C" int lg_spread_tile_resource_f64(const int64_t *user_rowptr,
                                           const int32_t *user_items, const double *ra_edge,
                                           int64_t n_users, const void *lines, const void *ovf,
                                           int32_t null_row,
                                           const double *rbeta, const double *inv_cls,
                                           int32_t item_begin, int32_t tile, int32_t width,
                                           double *F, int64_t ldf, lg_stream_t stream) {
  LG_REQUIRE(user_rowptr && user_items && ra_edge && lines && ovf && rbeta && inv_cls && F &&
                 n_users >= 0 && ldf >= tile,
             "lg_spread_tile_resource_f64: bad arguments");
  LG_REQUIRE(tile >= 1 && tile <= 8192 && width >= 1 && width <= tile,
             "lg_spread_tile_resource_f64: tile %d / width %d", tile, width);
  LG_REQUIRE(null_row >= 0 && null_row < (1 << 25) - 1,
             "tile walk: %d items exceed the 32-bit line offsets", null_row);
  if (n_users == 0) return LG_OK;
  WalkArgs a{};
  a.user_rowptr = user_rowptr;
  a.user_items = user_items;
  a.ra_edge = ra_edge;
  a.n_users = n_users;
  a.lines = (const uint4 *)lines;
  a.ovf = (const uint4 *)ovf;
  a.null_row = null_row;
  a.item_begin = item_begin;
  a.tile = tile;
  a.width = width;
  a.rbeta = rbeta;
  a.g_inv = inv_cls;
  a.F = F;
  a.ldf = ldf;
  const int st = launch_walk<MODE_F, 0, 1>(a, (hipStream_t)stream);
  if (st != LG_OK) return st;
  return launch_status("lg_spread_tile_resource_f64");
}

extern "C" int lg_tile_topk_f64(const double *F, int64_t ldf, int64_t n_rows,
                                int32_t item_begin, int32_t n_cols, const float *eu,
                                const float *ei, int32_t dim, const int64_t *ex_rowptr,
                                const int32_t *ex_col, int32_t excl_mode, int32_t k,
                                int32_t first, double *io_val, int64_t *io_idx,
                                lg_stream_t stream) {
  LG_REQUIRE(F && io_val && io_idx && n_rows >= 0 && n_cols >= 1 && ldf >= n_cols &&
                 item_begin >= 0 && (int64_t)item_begin + n_cols < 0x7fffffff,
             "lg_tile_topk_f64: bad arguments");
  LG_REQUIRE(k >= 1 && k <= 128, "lg_tile_topk_f64: k=%d not in [1,128]", k);
  LG_REQUIRE(!eu == !ei, "lg_tile_topk_f64: eu/ei must both be set or both NULL");
  LG_REQUIRE(!eu || dim == 32 || dim == 64 || dim == 128,
             "lg_tile_topk_f64: dim %d not in {32,64,128}", dim);
  LG_REQUIRE(excl_mode == LG_EXCL_DROP || excl_mode == LG_EXCL_NONE,
             "lg_tile_topk_f64: bad excl_mode %d", excl_mode);
  LG_REQUIRE(!ex_rowptr == !ex_col, "lg_tile_topk_f64: ex_rowptr/ex_col must both be set");
  LG_REQUIRE(!(eu && excl_mode == LG_EXCL_NONE && ex_rowptr),
             "lg_tile_topk_f64: a G factor with exclusions requires LG_EXCL_DROP");
  if (n_rows == 0) return LG_OK;
  hipStream_t s = (hipStream_t)stream;
  const int M = k <= 32 ? 1 : (k <= 64 ? 2 : 4);
  const int drop = excl_mode == LG_EXCL_DROP;
  switch (eu ? dim : 0) {
    case 0: launch_tile_topk<0>(M, F, ldf, n_rows, item_begin, n_cols, eu, ei, ex_rowptr, ex_col, drop, k, first, io_val, io_idx, s); break;
    case 32: launch_tile_topk<32>(M, F, ldf, n_rows, item_begin, n_cols, eu, ei, ex_rowptr, ex_col, drop, k, first, io_val, io_idx, s); break;
    case 64: launch_tile_topk<64>(M, F, ldf, n_rows, item_begin, n_cols, eu, ei, ex_rowptr, ex_col, drop, k, first, io_val, io_idx, s); break;
    default: launch_tile_topk<128>(M, F, ldf, n_rows, item_begin, n_cols, eu, ei, ex_rowptr, ex_col, drop, k, first, io_val, io_idx, s); break;
  }
  return launch_status("lg_tile_topk_f64");
}
