// K3s, the fused walk: k_tile_walk over the W tiles that spread_build.hip writes, in the
// line format of tile_lines.h (the algorithm is described there). This file holds the walk
// and nothing else -- profiles/pmc_traffic.json keys the walk's traffic record on this
// file's sha256, so an edit here means "the walk changed". spread_ref.hip includes it for
// the F-writing instantiation (MODE_F), which only the test-reference library launches.
#include <stdio.h>
#include <stdlib.h>

#include "score_stream.h"
#include "tile_lines.h"

namespace lg {

// ------------------------------------------------------------ the tile walk kernel
// One launch per tile. Persistent waves (NW per workgroup, one workgroup per CU; each wave
// takes users u, u + G, u + 2G, ... with G = all waves). A wave's work is a stream of
// BATCHES of at most 64 of a user's rows (every user has at least one, possibly empty):
// lane (g, h) = (lane / 8, lane % 8) loads unit h of row 8q + g for q < 8, so one load
// instruction moves 8 whole lines. The stream is software-pipelined: while batch t is
// decoded, the lines and ra of batch t+1 and the item ids of batch t+2 are in flight (and
// the row pointers of the user after that). Each path is added with one LDS atomic
// (ds_add_f64); rows whose header says "slow" (V rows, far degree classes) take a general
// decode, overflow runs are collected in LDS and loaded together after the batch.
//
// MODE_F:    F[u][j - item_begin] = rb_j * acc[j] (lg_spread_tile_resource_f64).
// MODE_TOPK: the tile's columns of (G *) F merge into the running per-user top-K lists
//            (lg_spread_tile_resource_topk_f64); F never leaves LDS. A column's score can
//            only beat the list's K-th value tau if acc * rb_max (* gb) > tau, rb_max = the
//            tile's largest rb and gb = the (user, 64-column chunk) upper bound of the fp32
//            score chain from lg_score_chunk_bound (bf16 MFMA + a rigorous rounding margin):
//            only those columns get rb_j and (with G) the exact chain score. Ids grow along
//            the walk, so "beats" is v > tau (a tie loses to the older, smaller id).
// MODE_RANK: where given targets stand among all columns (lg_spread_tile_resource_rank_f64),
//            in two phases. Value phase: v of the user's targets inside the tile -- MODE_TOPK's
//            value of that column, bit for bit -- goes to val[position in tgt_col]. Count phase:
//            the tile's columns become their values in place in acc (excluded and screened-out
//            columns -inf), then every target's count of columns before it under (value desc,
//            item asc) is added to cnt[position], kRankPass targets per pass over acc, per-lane
//            counters reduced once per pass. With G a column gets the exact chain score only if
//            its bound (MODE_TOPK's two tests, with >= : an equal value with a smaller id is
//            before the target) reaches tau = the user's worst ranking target value, which never
//            moves; a column below it is before no target.
constexpr int MODE_F = 0, MODE_TOPK = 1, MODE_RANK = 2;
constexpr int kRankPass = LG_SPREAD_RANK_ROW_MAX;  // targets per counting pass over acc
constexpr int kWalkQ = 8;       // line loads per lane per batch: 8 rows each, 64 rows
constexpr int kBatchRows = 8 * kWalkQ;
// per-wave scratch list: the batch's overflow rows during the decode, the exact-score queue
// (column, f) during the scan -- a drain round can queue one candidate per lane, so it holds
// at least 64 entries whatever the batch size
constexpr int kOvfList = kBatchRows > 64 ? kBatchRows : 64;
constexpr int kDecodePhase = 4;  // lines whose class reads precede their adds
// q dwords per lane loaded with the user's state (256 columns each: a whole 2048-column
// tile); the columns of wider tiles past them are screened by their chunk bound alone (q =
// 255), so the scan issues no memory loads
constexpr int kQPre = 8;
static_assert(kWalkQ % kDecodePhase == 0, "decode phase must divide the batch's line loads");

struct WalkArgs {
  const int64_t *user_rowptr;
  const int32_t *user_items;
  const double *ra_edge;      // ra of user_items[p], aligned with user_items
  int64_t n_users;
  const uint4 *lines;         // n_items + 1 lines (the last all zero)
  const uint4 *ovf;
  int32_t null_row;           // = n_items
  int32_t item_begin, tile, width;
  const double *rbeta;  // all items: 1 / beta
  const double *g_inv;  // fl(1/k) by class number (index 0 unused)
  // MODE_F
  double *F;
  int64_t ldf;
  // MODE_TOPK
  const float *eu, *ei;       // rows' user embeddings / all item embeddings (or NULL)
  const float *gb;            // [n_users][nch] score bounds (with eu)
  int32_t nch;
  const uint8_t *qb;          // [n_users][qstride] per-column 8-bit bounds (or NULL)
  int32_t qstride;
  const int64_t *ex_rowptr;   // exclusions (dropped), with a per-row cursor
  const int32_t *ex_col;
  int64_t *ex_cur;
  int k, first;
  double *io_val;
  int64_t *io_idx;
  // MODE_RANK (with the G and exclusion fields above)
  const int64_t *tgt_rowptr;  // the rows' targets, any order, any ids
  const int32_t *tgt_col;
  int phase;                  // 0: values, 1: counts
  double *val;                // aligned with tgt_col: written by phase 0, read by phase 1
  int64_t *cnt;               // aligned with tgt_col: phase 1 adds the tile's counts
};

// accumulator columns per wave: the tile rounded up to whole 512-column scan steps
__host__ __device__ constexpr int acc_cols(int tile) { return (tile + 511) / 512 * 512; }

// per wave: acc[acc_cols(tile)] and the overflow list (decode; the exact-score queue during
// the scan); the running list itself lives in registers
template <int MODE, int D, int M>
__host__ __device__ constexpr size_t walk_wave_bytes(int tile) {
  return ((size_t)acc_cols(tile) * 8 + (size_t)kOvfList * 12 + 15) & ~(size_t)15;
}
__host__ __device__ constexpr size_t walk_shared_bytes(int tile) {
  // class table + the block's rb maxima + rb of the tile's columns + its 64-column chunks'
  // rb maxima
  return (size_t)kInvTab * 8 + 16 * 8 + (size_t)((tile + 1) & ~1) * 8 + 64 * 8;
}


// The fast decode's two LDS addresses of a P slot s (class << 16 | column, column < 8192),
// one VALU op each: fl(1/k) of the class at byte s >> 13 (s_inv at LDS address 0; bits
// 13-15 of the column are 0), and the column's acc entry at acc_base + 8 (s & 0xFFFF).
typedef __attribute__((address_space(3))) double lds_f64;
__device__ __forceinline__ double slot_inv_fast(uint32_t s) {
  return *(const lds_f64 *)(uintptr_t)(s >> 13);
}
// Branch-free form: an empty slot (s == 0, value 0) adds its 0.0 to the lane's own dummy
// word instead (no exec-mask branch per slot; the dummies are lane-distinct: no conflicts).
__device__ __forceinline__ void slot_add_nobranch(uint32_t acc_base, uint32_t dummy, uint32_t s,
                                                  double v) {
  uint32_t addr;
  asm("v_mad_u32_u16 %0, %1, 8, %2" : "=v"(addr) : "v"(s), "v"(acc_base));
  addr = s ? addr : dummy;
  __hip_atomic_fetch_add((lds_f64 *)(uintptr_t)addr, v, __ATOMIC_RELAXED,
                         __HIP_MEMORY_SCOPE_WORKGROUP);
}

// fl(1/k) of a P slot's degree class (general decode: classes >= kInvTab from memory)
__device__ __forceinline__ double slot_inv(uint32_t s, const double *s_inv,
                                           const double *__restrict__ g_inv) {
  const uint32_t c = s >> 16;
  const bool far = c >= (uint32_t)kInvTab;
  const double inv = s_inv[far ? 0u : c];
  if (__builtin_expect(__ballot(far) != 0, 0)) {  // (a separate load: not a flat select)
    const double g = __builtin_nontemporal_load(g_inv + (far ? c : 0u));
    return far ? g : inv;
  }
  return inv;
}

// General decode of one 16-byte unit: a V entry (x has bit 31) or 4 P slots (zero words:
// padding). head: unit 0 of a line, whose word x is the row header (y, z, w are slots of a
// P row and zero in a V row).
__device__ __forceinline__ void add_unit(double *acc, uint4 w, bool head, double ra,
                                         const double *s_inv, const double *__restrict__ g_inv) {
  const bool isv = !head && (w.x & kEntV);
  const uint32_t sx = head ? 0u : w.x;
  // P slot words only (a V entry's y / z are its value: never decoded as classes)
  const uint32_t py = isv ? 0u : w.y, pz = isv ? 0u : w.z, pw = isv ? 0u : w.w;
  const double i0 = slot_inv(isv ? 0u : sx, s_inv, g_inv);
  const double v0 = (isv ? __hiloint2double((int)w.z, (int)w.y) : i0) * ra;
  const double v1 = slot_inv(py, s_inv, g_inv) * ra;
  const double v2 = slot_inv(pz, s_inv, g_inv) * ra;
  const double v3 = slot_inv(pw, s_inv, g_inv) * ra;
  if (sx) lds_add(acc, sx & 0xFFFFu, v0);
  if (py) lds_add(acc, py & 0xFFFFu, v1);
  if (pz) lds_add(acc, pz & 0xFFFFu, v2);
  if (pw) lds_add(acc, pw & 0xFFFFu, v3);
}

// A unit of a V row's overflow run: one entry (or a zero padding unit), ra * general_W into
// its column (add_unit's V case without its four class reads of P slots)
__device__ __forceinline__ void add_unit_v(double *acc, uint4 w, double ra) {
  if (w.x & kEntV) lds_add(acc, w.x & 0xFFFFu, __hiloint2double((int)w.z, (int)w.y) * ra);
}
// data unit q of a dense V row's run: columns 2q and 2q + 1 (zero values skipped)
__device__ __forceinline__ void add_unit_d(double *acc, uint4 w, int q, double ra) {
  const double a = __hiloint2double((int)w.y, (int)w.x), b = __hiloint2double((int)w.w, (int)w.z);
  if (a != 0.0) lds_add(acc, (uint32_t)(2 * q), a * ra);
  if (b != 0.0) lds_add(acc, (uint32_t)(2 * q + 1), b * ra);
}

// Fast decode (P rows whose classes are all < kInvTab): s_inv sits at LDS address 0.
__device__ __forceinline__ void add_slot_fast(double *acc, uint32_t s, double ra,
                                              const double *s_inv) {
  const double inv = s_inv[s >> 16];
  if (s) lds_add(acc, s & 0xFFFFu, inv * ra);
}

// The exact fp32 scores of 16 columns against one user row: column m = lane % 16 as A row m
// (ir: its item row + (lane / 16) D / 4), the user row as every B column (ur likewise). The
// per-element sums are the fp32 chain acc = fmaf(u[g*D/4+s], i[g*D/4+s], acc) (s outer, g
// inner) of lg_score_topk_f32; column mm's sum: lane 16 (mm / 4), element mm % 4.
template <int D>
__device__ __forceinline__ f32x4 chain_mfma16(const float *ir, const float *ur) {
  constexpr int Qd = D / 4;              // MFMA steps
  constexpr int H = Qd < 16 ? Qd : 16;   // steps per load round (<= 16 VGPRs each)
  f32x4 sc4 = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int h0 = 0; h0 < Qd; h0 += H) {
    float av[H], bv[H];
    load_piece<H>(ir + h0, av);
    load_piece<H>(ur + h0, bv);
#pragma unroll
    for (int s = 0; s < H; ++s)
      sc4 = __builtin_amdgcn_mfma_f32_16x16x4f32(av[s], bv[s], sc4, 0, 0, 0);
  }
  return sc4;
}

// A batch of the wave's stream: rows [r0, r1) of user u (whose rows end at e); xc / xh =
// the user's exclusion cursor and row end (prefetched with its row pointers). 32-bit fields
// (the host requires users, interactions and exclusions < 2^31): the stream state then fits
// the SGPRs without spilling into VGPR lanes.
struct Batch {
  int32_t u, r0, r1, e;
  bool first;
  int32_t xc, xh;
};

// The top-K state of a batch's user, loaded with the batch's lines (every batch loads it:
// the loads are unconditional, so the compiler's vmcnt bookkeeping never waits for a
// younger load than the one it needs): the running list (lane, 64 + lane), the chunk score
// bound, the per-column 8-bit bounds of the first kQPre * 256 columns and the next 64
// excluded items.
struct UState {
  int lid0, lid1;
  double lv0, lv1;
  float gb;
  uint32_t q[kQPre];
  int32_t xw;
};

// SEED: the first tile's instance (lists start empty): the finish scores the columns with the
// largest bounds first (below); a separate instance so the other tiles' code is untouched
template <int MODE, int D, int M, bool SEED = false>
__global__ __launch_bounds__(512) void k_tile_walk(WalkArgs a) {
  constexpr int Q = kWalkQ;
  extern __shared__ double lds[];
  const int nw = blockDim.x / 64;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / 64);
  const int lane = lane_id();
  const int gh = lane & 7;     // unit of the line this lane loads
  const int grow = lane >> 3;  // row of the 8-row load group
  const uint32_t hmask = gh == 0 ? 0u : 0xFFFFFFFFu;  // word x of unit 0 is the header
  const int tile = a.tile;
  double *s_inv = lds;  // at LDS address 0 (the fast decode indexes it with class * 8)
  double *s_red = s_inv + kInvTab;
  double *s_rb = s_red + 16;  // rb of the tile's columns (0 past the width)
  // per 64-column chunk: the largest rb (G screen, tile <= 4096); the waves' areas after it
  // (16-byte aligned: the tile's rb padded to an even count)
  double *s_rbc = s_rb + ((tile + 1) & ~1);
  char *mine = reinterpret_cast<char *>(s_rbc + 64) +
               (size_t)wave * walk_wave_bytes<MODE, D, M>(tile);
  double *acc = reinterpret_cast<double *>(mine);
  const uint32_t acc_base = (uint32_t)(uintptr_t)(lds_f64 *)acc;
  // the lane's dummy word for empty slots: its entry of the overflow list (rewritten before
  // every use; adding 0.0 leaves it unchanged meanwhile)
  const uint32_t dummy_addr = acc_base + 8u * (uint32_t)(acc_cols(tile) + lane);
  double *ovl_ra = acc + acc_cols(tile);  // overflow list (decode)
  uint32_t *ovl_ent = reinterpret_cast<uint32_t *>(ovl_ra + kOvfList);

  for (int c = threadIdx.x; c < kInvTab; c += blockDim.x) s_inv[c] = a.g_inv[c];
  double rmax = 0.0;  // the tile's largest rb (top-K prefilter)
  for (int j = threadIdx.x; j < tile; j += blockDim.x) {
    const double rb = j < a.width ? a.rbeta[a.item_begin + j] : 0.0;
    s_rb[j] = rb;
    rmax = fmax(rmax, rb);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) rmax = fmax(rmax, __shfl_xor(rmax, o));
  if (lane == 0) s_red[wave] = rmax;
  for (int j = lane; j < acc_cols(tile); j += 64) acc[j] = 0.0;
  __syncthreads();
  if (MODE != MODE_F && D > 0) {
    for (int c = wave; 64 * c < tile && c < 64; c += nw) {
      double m = s_rb[64 * c + lane < tile ? 64 * c + lane : 0];
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) m = fmax(m, __shfl_xor(m, o));
      if (lane == 0) s_rbc[c] = m;
    }
    __syncthreads();
  }
  rmax = 0.0;
  for (int w = 0; w < nw; ++w) rmax = fmax(rmax, s_red[w]);
  // acc * rb_j > tau  implies  acc * rb_max * (1 + 2^-50) > tau (rounding of both products)
  const double rscale = rmax * (1.0 + 0x1p-50);

  const int64_t G = (int64_t)gridDim.x * nw;
  const int64_t n_users = a.n_users;
  const int64_t u_first = (int64_t)blockIdx.x * nw + wave;
  if (u_first >= n_users) return;

  // row pointers (and exclusion cursor) of the next new user of the stream, prefetched one
  // user ahead. Lane-varying loads (lane 0 / 1: the row's start / end, resp. exclusion cursor /
  // row end) keep the values in VGPRs until the user starts: a wave-uniform load is read into
  // SGPRs right away, and hipcc then waits for it where it is issued -- vmcnt(0), draining
  // every batch line in flight at each new user. Reissued unconditionally at every step
  // (clamped past the last user; the same address until a user starts): a load issued only
  // when a user starts leaves a register copy at the join, which hipcc also guards with
  // vmcnt(0).
  const bool has_ex = MODE != MODE_F && a.ex_rowptr != nullptr;
  int32_t uq = (int32_t)u_first;
  int32_t pr = 0, px = 0;  // lanes 0, 1: the prefetched (start, end) / (cursor, end)
  // (positions < 2^31: the low dword of each int64 entry, one 4-byte load -- a whole int64
  // load's unused high half would pin a register whose reuse hipcc guards with a vmcnt wait)
  auto pre_load = [&]() __attribute__((always_inline)) {
    const int64_t uu = uq < n_users ? uq : n_users - 1;
    pr = reinterpret_cast<const int32_t *>(a.user_rowptr)[2 * (uu + (lane & 1))];
    if (has_ex) {  // (uniform)
      const int64_t *p = (lane & 1) ? a.ex_rowptr + uu + 1 : a.ex_cur + uu;
      px = *reinterpret_cast<const int32_t *>(p);
    }
  };
  pre_load();
  auto new_user = [&]() __attribute__((always_inline)) {
    const int32_t bq = __builtin_amdgcn_readlane(pr, 0), eq = __builtin_amdgcn_readlane(pr, 1);
    const int32_t xcq = has_ex ? __builtin_amdgcn_readlane(px, 0) : 0;
    const int32_t xhq = has_ex ? __builtin_amdgcn_readlane(px, 1) : 0;
    Batch y{uq, bq, bq + kBatchRows < eq ? bq + kBatchRows : eq, eq, true, xcq, xhq};
    uq += (int32_t)G;
    return y;
  };
  const Batch kEnd{(int32_t)n_users, 0, 0, 0, false, 0, 0};  // past the end of the stream
  auto next_batch = [&](const Batch &x) __attribute__((always_inline)) {
    if (x.u >= n_users) return kEnd;
    if (x.r1 < x.e) {
      Batch y{x.u, x.r1, x.r1 + kBatchRows < x.e ? x.r1 + kBatchRows : x.e, x.e, false, x.xc,
              x.xh};
      return y;
    }
    if (x.u + G >= n_users) return kEnd;
    return new_user();
  };
  // item ids of a batch's rows (lanes of one 8-lane group: one row)
  // Buffer loads with 32-bit offsets: a batch's item ids and ra through a descriptor based
  // at its first row (lane offsets are per-lane constants + immediates; rows past the batch
  // are out of range and read 0), the lines through one descriptor for the tile.
  const __amdgpu_buffer_rsrc_t r_lines = __builtin_amdgcn_make_buffer_rsrc(
      (void *)a.lines, 0, (int)((uint32_t)(a.null_row + 1) * 128u), 0x00020000);
  auto load_ids = [&](const Batch &x, int32_t (&it)[Q]) __attribute__((always_inline)) {
    {  // (unconditional: an empty batch reads 0 through a 0-byte descriptor)
      const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
          (void *)(a.user_items + x.r0), 0, (int)((x.r1 - x.r0) * 4), 0x00020000);
#pragma unroll
      for (int q = 0; q < Q; ++q)
        it[q] = (int32_t)__builtin_amdgcn_raw_buffer_load_b32(rs, (uint32_t)(grow * 4 + 32 * q),
                                                              0, 0);
    }
  };
  // lines and ra of a batch (rows past r1 read the zero line, and ra 0)
  auto load_rows = [&](const Batch &x, const int32_t (&it)[Q], uint4 (&w)[Q], double (&ra)[Q])
      __attribute__((always_inline)) {
    // (every load group is issued even past a short last batch: skipping them with a
    // uniform branch measured 40 % slower -- the branches cost the loads their overlap)
    const int nr = (int)(x.r1 - x.r0);
    const __amdgpu_buffer_rsrc_t rr = __builtin_amdgcn_make_buffer_rsrc(
        (void *)(a.ra_edge + x.r0), 0, nr * 8, 0x00020000);
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      const bool in = 8 * q + grow < nr;
      const uint32_t row = in ? (uint32_t)it[q] : (uint32_t)a.null_row;
      const auto v = __builtin_amdgcn_raw_buffer_load_b128(r_lines, row * 128u + 16u * gh, 0, 0);
      w[q] = uint4{v[0], v[1], v[2], v[3]};
      const auto d = __builtin_amdgcn_raw_buffer_load_b64(rr, (uint32_t)(grow * 8 + 64 * q), 0, 0);
      ra[q] = __builtin_bit_cast(double, d);
    }
  };

  // ---- top-K state of a batch's user (MODE_TOPK), loaded with the batch's lines: every load
  // is issued (clamped user, 0-byte descriptors for absent operands), the consumers apply the
  // masks at the finish
  constexpr bool kTwo = M > 2;  // k > 64: the list spans two registers per lane
  const bool has_qb = MODE != MODE_F && D > 0 && a.qb != nullptr;
  auto load_state = [&](const Batch &x, UState &st) __attribute__((always_inline)) {
    if constexpr (MODE == MODE_TOPK) {
      const int k = a.k;
      const int64_t us = x.u < n_users ? x.u : n_users - 1;
      // ids < 2^31 (and -1): the low dword of the int64 entry
      const int *idx32 = reinterpret_cast<const int *>(a.io_idx);
      const int e0 = lane < k ? lane : k - 1;
      st.lid0 = idx32[2 * (us * k + e0)];
      st.lv0 = a.io_val[us * k + e0];
      if constexpr (kTwo) {
        const int e1 = 64 + lane < k ? 64 + lane : k - 1;
        st.lid1 = idx32[2 * (us * k + e1)];
        st.lv1 = a.io_val[us * k + e1];
      }
      if constexpr (D > 0) {
        st.gb = a.gb[us * a.nch + (lane < a.nch ? lane : 0)];
        const __amdgpu_buffer_rsrc_t rq = __builtin_amdgcn_make_buffer_rsrc(
            has_qb ? (void *)(a.qb + us * a.qstride) : (void *)a.lines, 0,
            has_qb ? a.qstride : 0, 0x00020000);
        // (the whole offset in voffset + the immediate, both range-checked against qstride:
        // a tile narrower than kQPre * 256 columns reads 0 past its row instead of the next
        // user's -- or, for the last user, past the allocation)
#pragma unroll
        for (int kk = 0; kk < kQPre; ++kk)
          st.q[kk] = __builtin_amdgcn_raw_buffer_load_b32(rq, (uint32_t)(4 * lane + 256 * kk), 0, 0);
      }
      const int32_t nx = x.xh - x.xc;
      const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc(
          has_ex ? (void *)(a.ex_col + x.xc) : (void *)a.lines, 0,
          has_ex ? (int)(4 * (nx < 64 ? nx : 64)) : 0, 0x00020000);
      st.xw = (int32_t)__builtin_amdgcn_raw_buffer_load_b32(rx, (uint32_t)(4 * lane), 0, 0);
    }
  };

  // ---- decode one batch into acc
  auto decode = [&](const Batch &x, uint4 (&w)[Q], const double (&ra)[Q])
      __attribute__((always_inline)) {
#ifdef LG_WALK_PROBE  // measurement builds only (wrong lists): 2 = no decode (lines loaded only)
    if (LG_WALK_PROBE == 2) {
      uint32_t h = 0;
#pragma unroll
      for (int q = 0; q < Q; ++q) h ^= w[q].x ^ w[q].y ^ w[q].z ^ w[q].w ^ (uint32_t)ra[q];
      if (h == 0x12345678u && lane == 64) acc[0] = 1.0;  // (keeps the loads; never true)
      return;
    }
#endif
    uint32_t hdr = 0;
#pragma unroll
    for (int q = 0; q < Q; ++q) hdr |= w[q].x & ~hmask;  // the group heads' headers
    const bool slow = __ballot(hdr & kHdrSlow) != 0;
    const bool ovf = __ballot(hdr & kHdrOvf) != 0;
    if (!slow) {
      // The LDS serves a wave's operations in order, so a class-table read issued after an
      // atomic returns only once the atomic is done: the reads of H lines' slots go out
      // first, then their adds (one wait per phase, not one per slot).
      // (line groups wholly past a short batch's rows hold the zero line: their reads and
      // adds are skipped with a wave-uniform branch; their loads were issued regardless)
      constexpr int H = kDecodePhase;
      const int nr = (int)(x.r1 - x.r0);
#pragma unroll
      for (int q0 = 0; q0 < Q; q0 += H) {
        if (8 * q0 >= nr) break;
        double inv[H][4];
#pragma unroll
        for (int q = 0; q < H; ++q) {
          if (8 * (q0 + q) >= nr) break;
          inv[q][0] = slot_inv_fast(w[q0 + q].x & hmask);
          inv[q][1] = slot_inv_fast(w[q0 + q].y);
          inv[q][2] = slot_inv_fast(w[q0 + q].z);
          inv[q][3] = slot_inv_fast(w[q0 + q].w);
        }
#pragma unroll
        for (int q = 0; q < H; ++q) {
          if (8 * (q0 + q) >= nr) break;
          const uint32_t sv[4] = {w[q0 + q].x & hmask, w[q0 + q].y, w[q0 + q].z, w[q0 + q].w};
#pragma unroll
          for (int t = 0; t < 4; ++t)
            slot_add_nobranch(acc_base, dummy_addr, sv[t], inv[q][t] * ra[q0 + q]);
        }
      }
    } else {
#pragma unroll
      for (int q = 0; q < Q; ++q) add_unit(acc, w[q], gh == 0, ra[q], s_inv, a.g_inv);
    }
    if (ovf) {  // overflow runs: collected, then up to 4 rows' first 64 units in flight
      int nov = 0;
#pragma unroll
      for (int q = 0; q < Q; ++q) {
        const bool o = gh == 0 && (w[q].x & kHdrOvf);
        const uint64_t bal = __ballot(o);
        if (o) {
          const int p = nov + __popcll(bal & lanemask_lt());
          ovl_ent[p] = w[q].x & (kHdrPtr | kHdrV);  // (the run's first unit; a V row's bit)
          ovl_ra[p] = ra[q];
        }
        nov += __popcll(bal);
      }
      wave_sync();
      for (int t0 = 0; t0 < nov; t0 += 4) {
        uint4 y4[4];
        uint32_t ou4[4];
        double r4[4];
        bool v4[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const bool in = t0 + j < nov;
          const uint32_t e = ovl_ent[in ? t0 + j : t0];
          v4[j] = (e & kHdrV) != 0;
          ou4[j] = e & kHdrPtr;
          r4[j] = ovl_ra[in ? t0 + j : t0];
          y4[j] = a.ovf[(int64_t)ou4[j] + lane];
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if (t0 + j >= nov) continue;
          const uint32_t n0 = (uint32_t)__shfl((int)y4[j].x, 0);
          const bool dn = (n0 & kRunDense) != 0;  // (a dense V row: unit q -> columns 2q, 2q+1)
          const uint32_t n = n0 & ~kRunDense;
          if (lane == 0 || (uint32_t)lane > n) y4[j] = uint4{0u, 0u, 0u, 0u};
          if (dn) add_unit_d(acc, y4[j], lane - 1, r4[j]);
          else if (v4[j]) add_unit_v(acc, y4[j], r4[j]);
          else add_unit(acc, y4[j], false, r4[j], s_inv, a.g_inv);
          // runs longer than 63 units (hub items' V rows: up to a whole tile of entries): 4
          // chunks of 64 units in flight per round instead of one load -> add at a time
          for (uint32_t c = 64; c <= n; c += 256) {
            uint4 z[4];
#pragma unroll
            for (int p = 0; p < 4; ++p) {
              const uint32_t cc = c + 64 * p + lane;
              z[p] = cc <= n ? a.ovf[(int64_t)ou4[j] + cc] : uint4{0u, 0u, 0u, 0u};
            }
#pragma unroll
            for (int p = 0; p < 4; ++p) {
              if (c + 64 * p > n) break;  // (uniform)
              if (dn) add_unit_d(acc, z[p], (int)(c + 64 * p) + lane - 1, r4[j]);
              else if (v4[j]) add_unit_v(acc, z[p], r4[j]);
              else add_unit(acc, z[p], false, r4[j], s_inv, a.g_inv);
            }
          }
        }
      }
      wave_sync();
    }
  };

  // excluded items of this tile (the next run of the user's sorted exclusion row, from the
  // user's cursor; xw0 = its first 64 entries, one per lane): acc = -inf, the cursor moves on
  auto mark_excluded = [&](const Batch &x, int32_t xw0) __attribute__((always_inline)) {
    int64_t xpos = x.xc;
    const int64_t xhi = x.xh;
    int32_t xw = has_ex && xpos + lane < xhi ? xw0 : 0x7fffffff;
    const int32_t lim = a.item_begin + a.width;
    if (has_ex) {
      for (;;) {
        const bool in = xw < lim;
        if (in && xw >= a.item_begin) acc[xw - a.item_begin] = neg_inf<double>();
        const int nin = __popcll(__ballot(in));
        xpos += nin;
        if (nin < 64) break;
        xw = xpos + lane < xhi ? a.ex_col[xpos + lane] : 0x7fffffff;  // > 64 in one tile
      }
      if (lane == 0) a.ex_cur[x.u] = xpos;
    }
  };

  // ---- the user's tile of F: written out (MODE_F), merged into its top-K list (MODE_TOPK)
  // or ranked against (MODE_RANK)
  auto finish_user = [&](const Batch &x, UState &st) __attribute__((always_inline)) {
    const int64_t u = x.u;
    wave_sync();
#ifdef LG_WALK_PROBE  // measurement builds only (wrong lists): 1 = no scan (acc zeroed only)
    if (LG_WALK_PROBE == 1) {
      for (int j = 2 * lane; j < acc_cols(tile); j += 128)
        *reinterpret_cast<double2 *>(acc + j) = double2{0.0, 0.0};
      wave_sync();
      return;
    }
#endif
    if constexpr (MODE == MODE_F) {
      double *row = a.F + u * a.ldf;
      for (int j = lane; j < tile; j += 64) {
        __builtin_nontemporal_store(acc[j] * s_rb[j], row + j);
        acc[j] = 0.0;
      }
    } else if constexpr (MODE == MODE_RANK) {
      // the user's targets: positions [tb, te) of tgt_col; val and cnt are aligned with it
      const int64_t tb = a.tgt_rowptr[u], te = a.tgt_rowptr[u + 1];
      const int wend = (a.width + 511) & ~511;  // acc is used in whole 512-column steps
      auto zero_acc = [&]() __attribute__((always_inline)) {
        for (int j = 2 * lane; j < wend; j += 128)
          *reinterpret_cast<double2 *>(acc + j) = double2{0.0, 0.0};
        wave_sync();
      };
      if (a.phase == 0) {
        // ---- values: 16 targets per round, target m of the round in the lanes with
        // lane % 16 = m (the MFMA batch's A rows); MODE_TOPK's v = (double)score * (acc * rb)
        const int m = lane & 15;
        for (int64_t p0 = tb; p0 < te; p0 += 16) {
          const int64_t p = p0 + m;
          const int64_t c = (p < te ? (int64_t)a.tgt_col[p] : -1) - a.item_begin;
          const bool in = p < te && c >= 0 && c < a.width;
          if (!__ballot(in)) continue;  // (uniform)
          const int cc = in ? (int)c : 0;
          const double f = acc[cc] * s_rb[cc];
          double v = f;
          if constexpr (D > 0) {
            const int g = lane >> 4;
            const f32x4 sc4 = chain_mfma16<D>(a.ei + (int64_t)(a.item_begin + cc) * D + g * (D / 4),
                                              a.eu + u * D + g * (D / 4));
            const int src = 16 * (m >> 2);  // target m's sum: lane 16 (m / 4), element m % 4
            const float e0 = __shfl(sc4[0], src), e1 = __shfl(sc4[1], src);
            const float e2 = __shfl(sc4[2], src), e3 = __shfl(sc4[3], src);
            const float sc = (m & 3) == 0 ? e0 : (m & 3) == 1 ? e1 : (m & 3) == 2 ? e2 : e3;
            v = (double)sc * f;
          }
          if (in && lane < 16) a.val[p] = v;
        }
        zero_acc();
        return;
      }
      // ---- counts
      mark_excluded(x, x.xc + lane < x.xh ? a.ex_col[x.xc + lane] : 0x7fffffff);
      wave_sync();
      // tau: the worst ranking target value (a target ranks iff its value is > -inf)
      double tau = __builtin_huge_val();
      uint64_t live = 0;
      for (int64_t p0 = tb; p0 < te; p0 += 64) {
        const double v = p0 + lane < te ? a.val[p0 + lane] : neg_inf<double>();
        const bool r = v > neg_inf<double>();
        live |= __ballot(r);
        tau = r && v < tau ? v : tau;
      }
      if (!live) {  // nothing to count (no target, or none that ranks)
        zero_acc();
        return;
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const double t2 = __shfl_xor(tau, o);
        tau = t2 < tau ? t2 : tau;
      }
      // step 1: acc[j] becomes column j's value, -inf for excluded columns, columns past the
      // width and (G) columns whose bound is below tau
      if constexpr (D == 0) {
        for (int j = 2 * lane; j < wend; j += 128) {
          double2 y = *reinterpret_cast<const double2 *>(acc + j);
          y.x = j < a.width ? y.x * s_rb[j < a.width ? j : 0] : neg_inf<double>();
          y.y = j + 1 < a.width ? y.y * s_rb[j + 1 < a.width ? j + 1 : 0] : neg_inf<double>();
          *reinterpret_cast<double2 *>(acc + j) = y;
        }
      } else {
        int ncand = 0;
        double *cq_f = ovl_ra;     // queued f (the decode's overflow list, free here)
        uint32_t *cq_j = ovl_ent;  // queued column
        // the queued columns' exact values into acc (MODE_TOPK's flush, stored not inserted)
        auto score_queue = [&]() __attribute__((always_inline)) {
          wave_sync();
          const int m = lane & 15, g = lane >> 4;
          for (int b0 = 0; b0 < ncand; b0 += 16) {
            const int nb = ncand - b0 < 16 ? ncand - b0 : 16;
            const int ci = b0 + (m < nb ? m : 0);
            const f32x4 sc4 = chain_mfma16<D>(
                a.ei + (int64_t)(a.item_begin + (int)cq_j[ci]) * D + g * (D / 4),
                a.eu + u * D + g * (D / 4));
            if (m == 0) {  // candidates 4 g .. 4 g + 3: this lane's four sums
#pragma unroll
              for (int e = 0; e < 4; ++e) {
                const int mm = 4 * g + e;
                const float sc = e == 0 ? sc4[0] : e == 1 ? sc4[1] : e == 2 ? sc4[2] : sc4[3];
                if (mm < nb) acc[cq_j[b0 + mm]] = (double)sc * cq_f[b0 + mm];
              }
            }
          }
          ncand = 0;
          wave_sync();
        };
        // MODE_TOPK's screen scales, per 64-column chunk c in lane c
        const double gp = (double)fmaxf(a.gb[u * a.nch + (lane < a.nch ? lane : 0)], 0.f);
        const double sc_v = s_rbc[lane < a.nch ? lane : 0] * (1.0 + 0x1p-50) * gp * (1.0 / 255.0);
        const double bq_v = gp * (1.0 / 255.0) * (1.0 + 0x1p-50);
        const __amdgpu_buffer_rsrc_t rq = __builtin_amdgcn_make_buffer_rsrc(
            has_qb ? (void *)(a.qb + u * a.qstride) : (void *)a.lines, 0,
            has_qb ? a.qstride : 0, 0x00020000);
        const double2 ninf2{neg_inf<double>(), neg_inf<double>()};
        for (int c0 = 0; c0 < a.width; c0 += 512) {
          // the 8-bit bounds of the lane's columns (without qb: 255, the chunk bound alone)
          uint32_t qa = 0xFFFFFFFFu, qb2 = 0xFFFFFFFFu;
          if (has_qb) {  // (uniform; range-checked against qstride)
            qa = __builtin_amdgcn_raw_buffer_load_b32(rq, (uint32_t)(4 * lane + c0), 0, 0);
            qb2 = __builtin_amdgcn_raw_buffer_load_b32(rq, (uint32_t)(4 * lane + c0 + 256), 0, 0);
          }
          double sv[8];
#pragma unroll
          for (int hh = 0; hh < 2; ++hh)
#pragma unroll
            for (int pp = 0; pp < 2; ++pp) {
              const int j = c0 + 256 * hh + 4 * lane + 2 * pp;
              const double2 y = *reinterpret_cast<const double2 *>(acc + j);
              *reinterpret_cast<double2 *>(acc + j) = ninf2;
              sv[4 * hh + 2 * pp] = y.x;
              sv[4 * hh + 2 * pp + 1] = y.y;
            }
          if (c0 + 512 > a.width) {
#pragma unroll
            for (int t = 0; t < 8; ++t) {
              const int j = c0 + 256 * (t >> 2) + 4 * lane + (t & 3);
              if (j >= a.width) sv[t] = neg_inf<double>();
            }
          }
          const double sc0 = __shfl(sc_v, ((c0 + 4 * lane) >> 6) & 63);
          const double sc1 = __shfl(sc_v, ((c0 + 256 + 4 * lane) >> 6) & 63);
          uint32_t mask = 0;
#pragma unroll
          for (int t = 0; t < 8; ++t) {  // (excluded: b = -inf or NaN, never taken)
            const uint32_t qq = t < 4 ? qa : qb2;
            const double qv = (double)((qq >> (8 * (t & 3))) & 0xFFu);
            const double b = sv[t] * qv * (t < 4 ? sc0 : sc1);
            mask |= b >= tau ? 1u << t : 0u;
          }
          while (__ballot(mask != 0)) {
            const bool has = mask != 0;
            const int t = has ? __ffs(mask) - 1 : 0;
            mask &= mask - 1;
            double s = sv[0];
#pragma unroll
            for (int y = 1; y < 8; ++y) s = t == y ? sv[y] : s;
            const int j = c0 + 256 * (t >> 2) + 4 * lane + (t & 3);
            const double f = has ? s * s_rb[has ? j : 0] : -1.0;
            const uint32_t qq = t < 4 ? qa : qb2;
            const double bq = (double)((qq >> (8 * (t & 3))) & 0xFFu) *
                              __shfl(bq_v, (j >> 6) & 63);
            const bool cand = has && bq * f >= tau;
            const uint64_t bal = __ballot(cand);
            if (bal) {
              const int nb = __popcll(bal);
              if (ncand + nb > kOvfList) score_queue();  // (nb <= 64 <= kOvfList)
              if (cand) {
                const int p = ncand + __popcll(bal & lanemask_lt());
                cq_f[p] = f;
                cq_j[p] = (uint32_t)j;
              }
              ncand += nb;
              if (ncand >= 16) score_queue();
            }
          }
        }
        if (ncand) score_queue();
      }
      wave_sync();
      // step 2: kRankPass targets per pass over acc, per-lane counters reduced once per pass;
      // a target that does not rank compares as NaN (before nothing, after nothing)
      for (int64_t p0 = tb; p0 < te; p0 += kRankPass) {
        const int np = (int)(te - p0 < kRankPass ? te - p0 : kRankPass);
        double tvl = __builtin_nan("");
        int til = 0;
        if (lane < np) {
          const double v = a.val[p0 + lane];
          tvl = v > neg_inf<double>() ? v : tvl;
          til = a.tgt_col[p0 + lane];
        }
        if (!__ballot(tvl == tvl)) continue;  // (uniform)
        int64_t mine = 0;
        if (np == 1) {  // leave-one-out: one compare per column
          const double tv = __shfl(tvl, 0);
          const int ti = __shfl(til, 0);
          int c = 0;
          for (int j = 2 * lane; j < wend; j += 128) {
            const double2 y = *reinterpret_cast<const double2 *>(acc + j);
            c += before(y.x, a.item_begin + j, tv, ti) ? 1 : 0;
            c += before(y.y, a.item_begin + j + 1, tv, ti) ? 1 : 0;
          }
#pragma unroll
          for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
          mine = c;
        } else {
          double tv[kRankPass];
          int ti[kRankPass], c[kRankPass];
#pragma unroll
          for (int i = 0; i < kRankPass; ++i) {
            tv[i] = __shfl(tvl, i);
            ti[i] = __shfl(til, i);
            c[i] = 0;
          }
          for (int j = 2 * lane; j < wend; j += 128) {
            const double2 y = *reinterpret_cast<const double2 *>(acc + j);
#pragma unroll
            for (int i = 0; i < kRankPass; ++i) {
              c[i] += before(y.x, a.item_begin + j, tv[i], ti[i]) ? 1 : 0;
              c[i] += before(y.y, a.item_begin + j + 1, tv[i], ti[i]) ? 1 : 0;
            }
          }
#pragma unroll
          for (int i = 0; i < kRankPass; ++i) {
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) c[i] += __shfl_xor(c[i], o);
            mine = lane == i ? c[i] : mine;
          }
        }
        // one wave owns the user in every launch of the walk: a plain load-add-store
        if (lane < np && tvl == tvl) a.cnt[p0 + lane] += mine;
      }
      zero_acc();
    } else {
      const int k = a.k;
      // the running list in registers: entry lane (L0, I0) and 64 + lane (L1, I1), sorted by
      // (value desc, id asc); empty entries (-inf, kPadId); a first tile starts empty
      const bool ok0 = !a.first && lane < k && st.lid0 >= 0;
      double L0 = ok0 ? st.lv0 : neg_inf<double>();
      int I0 = ok0 ? st.lid0 : kPadId;
      double L1 = neg_inf<double>();
      int I1 = kPadId;
      if constexpr (kTwo) {
        const bool ok1 = !a.first && 64 + lane < k && st.lid1 >= 0;
        L1 = ok1 ? st.lv1 : neg_inf<double>();
        I1 = ok1 ? st.lid1 : kPadId;
      }
      const float gbv = st.gb;
      uint32_t (&qr)[kQPre] = st.q;
      if (!has_qb) {
#pragma unroll
        for (int kk = 0; kk < kQPre; ++kk) qr[kk] = 0xFFFFFFFFu;
      }
      auto kth = [&](double &tv, int &ti) __attribute__((always_inline)) {
        if (!kTwo || k <= 64) {
          tv = __shfl(L0, k - 1);
          ti = __shfl(I0, k - 1);
        } else {
          tv = __shfl(L1, k - 65);
          ti = __shfl(I1, k - 65);
        }
      };
      double tau;
      int tau_id;
      kth(tau, tau_id);
      bool dirty = a.first != 0;
      // insert (v, id) (wave-uniform) if it beats the k-th entry: its rank is the number of
      // entries before it; the entries from that rank on move one place down
      auto insert1 = [&](double v, int id) __attribute__((always_inline)) {
        if (!before(v, id, tau, tau_id)) return;
        dirty = true;
        int pos = __popcll(__ballot(before(L0, I0, v, id)));
        if constexpr (kTwo) pos += __popcll(__ballot(before(L1, I1, v, id)));
        const double up0 = __shfl_up(L0, 1);
        const int iu0 = __shfl_up(I0, 1);
        if constexpr (kTwo) {
          const double up1 = __shfl_up(L1, 1);
          const int iu1 = __shfl_up(I1, 1);
          const double c0 = __shfl(L0, 63);
          const int ic0 = __shfl(I0, 63);
          const int p1 = 64 + lane;
          const double n1 = p1 > pos ? (lane == 0 ? c0 : up1) : (p1 == pos ? v : L1);
          const int m1 = p1 > pos ? (lane == 0 ? ic0 : iu1) : (p1 == pos ? id : I1);
          L1 = p1 < k ? n1 : neg_inf<double>();
          I1 = p1 < k ? m1 : kPadId;
        }
        L0 = lane > pos ? up0 : (lane == pos ? v : L0);
        I0 = lane > pos ? iu0 : (lane == pos ? id : I0);
        if (lane >= k) { L0 = neg_inf<double>(); I0 = kPadId; }
        kth(tau, tau_id);
      };
      mark_excluded(x, st.xw);
      wave_sync();
      // The scan: lane l reads columns c0 + 2l, c0 + 2l + 1 (ds_read_b128), 4 reads in flight
      // (512 columns). A column can enter only if acc > thr, thr = tau / (rb_max (1 + 2^-50)
      // [* max(gb, 0)]) (>= -0.5: excluded columns hold -1; every rounding of
      // fl(gb fl(acc rb_j)) > tau is covered by the 2^-50 margin); those get rb_j and (with G)
      // the exact score. The list order (value desc, id asc) is total, so the order in which
      // candidates are inserted does not matter.
      // Exact scores in batches (D > 0): the columns that pass the bound test are queued in
      // LDS (column, f) and scored 16 at a time by v_mfma_f32_16x16x4_f32 -- candidate m as
      // A row m (its item row), the user row as every B column -- whose per-element sums are
      // the fp32 chain acc = fmaf(u[g*D/4+s], i[g*D/4+s], acc) (s outer, g inner) of
      // lg_score_topk_f32. One load round trip per 16 candidates instead of a dependent
      // per-lane chain of item-row loads; the queue is flushed when it holds 16, when the list
      // is not full yet (tau = -inf: every column passes), and at the end of the scan.
      int ncand = 0;
      double *cq_f = ovl_ra;     // queued f (the decode's overflow list, free during the scan)
      uint32_t *cq_j = ovl_ent;  // queued column
      auto flush = [&]() __attribute__((always_inline)) {
#ifdef LG_WALK_PROBE  // 3 = no exact scores: candidates inserted with their f as the score
        if (LG_WALK_PROBE == 3) {
          wave_sync();
          for (int mm = 0; mm < ncand; ++mm) insert1(cq_f[mm], a.item_begin + (int)cq_j[mm]);
          ncand = 0;
          wave_sync();
          return;
        }
#endif
        if constexpr (D > 0) {
          constexpr int Qd = D / 4;
          wave_sync();
          const int m = lane & 15, g = lane >> 4;
          for (int b0 = 0; b0 < ncand; b0 += 16) {
            const int nb = ncand - b0 < 16 ? ncand - b0 : 16;
            const int ci = b0 + (m < nb ? m : 0);
            const float *ir = a.ei + (int64_t)(a.item_begin + (int)cq_j[ci]) * D + g * Qd;
            const float *ur = a.eu + u * D + g * Qd;
            const f32x4 sc4 = chain_mfma16<D>(ir, ur);
            // candidate mm's sum: lane 16 (mm / 4), element mm % 4
            for (int mm = 0; mm < nb; ++mm) {
              const float e = (mm & 3) == 0 ? sc4[0] : (mm & 3) == 1 ? sc4[1]
                            : (mm & 3) == 2 ? sc4[2] : sc4[3];
              const float sc = __shfl(e, 16 * (mm >> 2));
              insert1((double)sc * cq_f[b0 + mm], a.item_begin + (int)cq_j[b0 + mm]);
            }
          }
          ncand = 0;
          wave_sync();
        }
      };
      // The scan, 512 columns per iteration: lane l takes columns c0 + 4l .. + 3 and
      // c0 + 256 + 4l .. + 3 (ds_read_b128 x 4). A column can enter only if
      //   no G:  acc > thr = tau / (rb_max (1 + 2^-50))            (excluded: acc = -inf)
      //   G:     acc * q * (rbmax_c (1 + 2^-50) max(gb, 0) / 255) > tau   (c = the chunk)
      // (gb * q / 255 >= the exact score, q = the column's 8-bit bound, 255 without qb; the
      // 2^-50 margin covers every rounding of fl(G fl(acc rb_j)) > tau). The lanes' passing
      // columns form a bit mask that one loop drains (one candidate per lane per round): rb_j,
      // then (G) the column bound times f and the exact chain score, then the insertion. The
      // list order (value desc, id asc) is total, so the insertion order does not matter.
      double thr_s = tau / rscale;
      double sc_v = 0.0, bq_v = 0.0;  // per 64-column chunk c in lane c (D > 0)
      if constexpr (D > 0) {
        // the pre-screen scale of chunk c: its own largest rb (not the tile's), so a column
        // passes only if acc * q * rbmax_c (1 + 2^-50) gb / 255 > tau
        const double gp = (double)fmaxf(gbv, 0.f);
        sc_v = s_rbc[lane < a.nch ? lane : 0] * (1.0 + 0x1p-50) * gp * (1.0 / 255.0);
        bq_v = gp * (1.0 / 255.0) * (1.0 + 0x1p-50);
      }
      // Seeding (the first tile's instance; G, k <= 64, a list that is not full): with tau = -inf
      // every column would pass and be scored exactly until the list fills and tau climbs from
      // whatever the first columns scored. Instead the columns whose pre-screen bound
      // b = acc q sc is at least t_hi = the k-th largest of the lanes' maximum bounds (so at
      // least k columns) are scored first (pass A), tau starts at the k-th best of them, and
      // the scan below skips exactly those columns (the same b, computed the same way). The
      // candidate set and the list order are unchanged, so the list is the same.
      bool seeded = false;
      double t_hi = 0.0;
      if constexpr (SEED && D > 0 && !kTwo) {  // (kTwo: k > 64, two list registers per lane)
        if (tau == neg_inf<double>()) {
          // step s8's columns c0 = 512 s8 + ...: the 8 accumulator values of the lane (read
          // only; the scan below zeroes them) and their bounds b, computed as the scan does
          auto read8 = [&](int c0, double (&sv)[8]) __attribute__((always_inline)) {
#pragma unroll
            for (int hh = 0; hh < 2; ++hh)
#pragma unroll
              for (int pp = 0; pp < 2; ++pp) {
                const int j = c0 + 256 * hh + 4 * lane + 2 * pp;
                const double2 x = *reinterpret_cast<const double2 *>(acc + j);
                sv[4 * hh + 2 * pp] = x.x;
                sv[4 * hh + 2 * pp + 1] = x.y;
              }
            if (c0 + 512 > a.width) {
#pragma unroll
              for (int t = 0; t < 8; ++t) {
                const int j = c0 + 256 * (t >> 2) + 4 * lane + (t & 3);
                if (j >= a.width) sv[t] = neg_inf<double>();
              }
            }
          };
          auto qsel = [&](int i) __attribute__((always_inline)) {  // qr[i] for a uniform i
            uint32_t v = 0xFFFFFFFFu;  // (columns past 256 kQPre: the chunk bound alone)
#pragma unroll
            for (int x = 0; x < kQPre; ++x) v = i == x ? qr[x] : v;
            return v;
          };
          auto bound = [&](int c0, int t, double svt, uint32_t qa, uint32_t qb2)
              __attribute__((always_inline)) {
            const double sc = __shfl(sc_v, ((c0 + 256 * (t >> 2) + 4 * lane) >> 6) & 63);
            const uint32_t qq = t < 4 ? qa : qb2;
            const double qv = (double)((qq >> (8 * (t & 3))) & 0xFFu);
            return svt * qv * sc;
          };
          double lmax = neg_inf<double>();
#pragma unroll 1
          for (int c0 = 0; c0 < a.width; c0 += 512) {
            double sv[8];
            read8(c0, sv);
            const uint32_t qa = qsel(c0 >> 8), qb2 = qsel((c0 >> 8) + 1);
#pragma unroll
            for (int t = 0; t < 8; ++t) {
              const double bt = bound(c0, t, sv[t], qa, qb2);
              lmax = bt > lmax ? bt : lmax;  // (NaN: skipped)
            }
          }
          // the k-th largest lane maximum: bitonic sort of the 64 values, descending
          double v = lmax;
#pragma unroll
          for (int sz = 2; sz <= 64; sz <<= 1)
#pragma unroll
            for (int st2 = sz >> 1; st2 > 0; st2 >>= 1) {
              const double o = __shfl_xor(v, st2);
              const bool keep_max = ((lane & sz) == 0) == ((lane & st2) == 0);
              v = keep_max ? (o > v ? o : v) : (o < v ? o : v);
            }
          t_hi = __shfl(v, k - 1);
          seeded = true;
          // pass A: score every column with b >= t_hi (16 at a time), insert
#pragma unroll 1
          for (int c0 = 0; c0 < a.width; c0 += 512) {
            double sv[8];
            read8(c0, sv);
            const uint32_t qa = qsel(c0 >> 8), qb2 = qsel((c0 >> 8) + 1);
            uint32_t mask = 0;
#pragma unroll
            for (int t = 0; t < 8; ++t) {  // (excluded columns: b = -inf or NaN, never taken)
              const double bt = bound(c0, t, sv[t], qa, qb2);
              mask |= bt >= t_hi && bt > neg_inf<double>() ? 1u << t : 0u;
            }
            while (__ballot(mask != 0)) {
              const bool has = mask != 0;
              const int t = has ? __ffs(mask) - 1 : 0;
              mask &= mask - 1;
              double sx = sv[0];
#pragma unroll
              for (int x = 1; x < 8; ++x) sx = t == x ? sv[x] : sx;
              const int j = c0 + 256 * (t >> 2) + 4 * lane + (t & 3);
              const double f = has ? sx * s_rb[has ? j : 0] : -1.0;
              const uint64_t bal = __ballot(has);
              const int nb = __popcll(bal);
              if (ncand + nb > kOvfList) flush();
              if (has) {
                const int p = ncand + __popcll(bal & lanemask_lt());
                cq_f[p] = f;
                cq_j[p] = (uint32_t)j;
              }
              ncand += nb;
              if (ncand >= 16) flush();
            }
          }
          if (ncand) flush();
        }
      }
      const double2 zero2{0.0, 0.0};
      for (int c0 = 0; c0 < a.width; c0 += 512) {
        const uint32_t qa = qr[0], qb2 = qr[1];
#pragma unroll
        for (int k = 0; k + 2 < kQPre; ++k) qr[k] = qr[k + 2];
        qr[kQPre - 2] = 0xFFFFFFFFu;  // (columns past 256 kQPre: the chunk bound alone)
        qr[kQPre - 1] = 0xFFFFFFFFu;
        double sv[8];
#pragma unroll
        for (int hh = 0; hh < 2; ++hh)
#pragma unroll
          for (int pp = 0; pp < 2; ++pp) {
            const int j = c0 + 256 * hh + 4 * lane + 2 * pp;
            // (acc holds whole 512-column steps: no bounds branch, the 4 reads go out together)
            const double2 x = *reinterpret_cast<const double2 *>(acc + j);
            *reinterpret_cast<double2 *>(acc + j) = zero2;
            sv[4 * hh + 2 * pp] = x.x;
            sv[4 * hh + 2 * pp + 1] = x.y;
          }
        if (c0 + 512 > a.width) {  // the last step of a partial tile: columns past the width
#pragma unroll
          for (int t = 0; t < 8; ++t) {
            const int j = c0 + 256 * (t >> 2) + 4 * lane + (t & 3);
            if (j >= a.width) sv[t] = neg_inf<double>();
          }
        }
        double sc0 = 0.0, sc1 = 0.0;
        if constexpr (D > 0) {
          sc0 = __shfl(sc_v, ((c0 + 4 * lane) >> 6) & 63);
          sc1 = __shfl(sc_v, ((c0 + 256 + 4 * lane) >> 6) & 63);
        }
        uint32_t mask = 0;
#pragma unroll
        for (int t = 0; t < 8; ++t) {
          bool pre;
          if constexpr (D > 0) {
            const uint32_t qq = t < 4 ? qa : qb2;
            const double qv = (double)((qq >> (8 * (t & 3))) & 0xFFu);
            const double b = sv[t] * qv * (t < 4 ? sc0 : sc1);
            // (seeded: pass A scored the columns with b >= t_hi, b > -inf)
            pre = b > tau && !(seeded && b >= t_hi && b > neg_inf<double>());
          } else {
            pre = sv[t] > thr_s;
          }
          mask |= pre ? 1u << t : 0u;
        }
        while (__ballot(mask != 0)) {
          const bool has = mask != 0;
          const int t = has ? __ffs(mask) - 1 : 0;
          mask &= mask - 1;
          double s = sv[0];
#pragma unroll
          for (int x = 1; x < 8; ++x) s = t == x ? sv[x] : s;
          const int j = c0 + 256 * (t >> 2) + 4 * lane + (t & 3);
          const double f = has ? s * s_rb[has ? j : 0] : -1.0;
          if constexpr (D > 0) {
            const uint32_t qq = t < 4 ? qa : qb2;
            const double bq = (double)((qq >> (8 * (t & 3))) & 0xFFu) *
                              __shfl(bq_v, (j >> 6) & 63);
            // (>=: tau moves while this step's columns are drained -- its mask was taken at
            // the step's start -- so a column of the step that ties the new k-th value may
            // still have the smaller id; insert1 decides by (value, id). Columns of later
            // steps and tiles have larger ids: their strict mask test stands.)
            const bool cand = has && bq * f >= tau;
            const uint64_t bal = __ballot(cand);
            if (bal) {
              const int nb = __popcll(bal);
              if (ncand + nb > kOvfList) flush();  // (nb <= 64 <= kOvfList)
              if (cand) {
                const int p = ncand + __popcll(bal & lanemask_lt());
                cq_f[p] = f;
                cq_j[p] = (uint32_t)j;
              }
              ncand += nb;
              if (ncand >= 16 || tau == neg_inf<double>()) flush();
            }
          } else {
            uint64_t bal = __ballot(has && before(f, a.item_begin + j, tau, tau_id));
            while (bal) {
              const int l = __ffsll((long long)bal) - 1;
              bal &= bal - 1;
              insert1(__shfl(f, l), a.item_begin + __shfl(j, l));
            }
            thr_s = tau / rscale;
          }
        }
      }
      if (ncand) flush();
      if (dirty) {
        if (lane < k) {
          a.io_val[u * k + lane] = I0 != kPadId ? L0 : neg_inf<double>();
          a.io_idx[u * k + lane] = I0 != kPadId ? I0 : -1;
        }
        if (kTwo && 64 + lane < k) {
          a.io_val[u * k + 64 + lane] = I1 != kPadId ? L1 : neg_inf<double>();
          a.io_idx[u * k + 64 + lane] = I1 != kPadId ? I1 : -1;
        }
      }
      wave_sync();
    }
  };

  // ---- the pipeline: c (decoded now; lines in wc), d (lines in flight in wd), n2 (ids in
  // flight in it2). Two register sets (lines, ra, user state) alternate between c and d. Every
  // step issues the same loads (empty batches read the zero line / 0 bytes), so the wait
  // before a decode counts the two younger batches' loads instead of draining them.
  int32_t it2[Q];
  uint4 w0[Q], w1[Q];
  double ra0[Q], ra1[Q];
  UState s0, s1;
  Batch c = new_user();
  pre_load();
  load_ids(c, it2);
  load_rows(c, it2, w0, ra0);
  load_state(c, s0);
  Batch d = next_batch(c);
  pre_load();
  load_ids(d, it2);
  load_rows(d, it2, w1, ra1);
  load_state(d, s1);
  Batch n2 = next_batch(d);
  pre_load();
  load_ids(n2, it2);
  auto step = [&](uint4 (&wc)[Q], double (&rc)[Q], UState &sc) __attribute__((always_inline)) {
    // c's user state (loaded two steps ago) is taken here, where the wait for it counts the
    // younger batches' loads; at the finish, behind the exclusion loop's load, the compiler
    // would drain every load in flight
    if constexpr (MODE == MODE_TOPK) {
      asm volatile("" : "+v"(sc.lid0), "+v"(sc.lv0), "+v"(sc.xw));
      if constexpr (kTwo) asm volatile("" : "+v"(sc.lid1), "+v"(sc.lv1));
      if constexpr (D > 0) {
        asm volatile("" : "+v"(sc.gb));
#pragma unroll
        for (int kk = 0; kk < kQPre; ++kk) asm volatile("" : "+v"(sc.q[kk]));
      }
    }
    decode(c, wc, rc);
    if (c.r1 >= c.e) finish_user(c, sc);
    // batch t+2 into the freed registers (issued before the scan instead: 1.5 % slower)
    load_rows(n2, it2, wc, rc);
    load_state(n2, sc);
    const Batch n3 = next_batch(n2);
    pre_load();
    load_ids(n3, it2);
    c = d;
    d = n2;
    n2 = n3;
    return c.u < n_users;
  };
  for (;;) {
    if (!step(w0, ra0, s0)) break;
    if (!step(w1, ra1, s1)) break;
  }
}

}  // namespace lg

using namespace lg;

// waves per workgroup: as many as the LDS holds next to the shared tables (<= 8), one
// workgroup per CU, persistent
template <int MODE, int D, int M>
static int launch_walk(const WalkArgs &a, hipStream_t s) {
  const size_t per = walk_wave_bytes<MODE, D, M>(a.tile);
  const size_t shared = walk_shared_bytes(a.tile);
  const size_t budget = 160 * 1024;
  int nw = (int)((budget - shared) / per);
  if (nw > 8) nw = 8;
  if (nw < 1) {
    set_error("tile walk: tile %d needs %zu bytes of LDS per wave", a.tile, per + shared);
    return LG_ERR_ARG;
  }
  const int64_t want = (a.n_users + nw - 1) / nw;
  const int cus = device_cus();
  const int64_t cap = cus > 0 ? cus : 256;
  const unsigned blocks = (unsigned)(want < cap ? want : cap);
  const size_t lds = shared + (size_t)nw * per;
  bool seeded = false;
  if constexpr (MODE == MODE_TOPK && D > 0 && M <= 2) {  // (the seeded finish: k <= 64 with G)
    if (a.first) {
      k_tile_walk<MODE, D, M, true><<<dim3(blocks), dim3(64 * nw), lds, s>>>(a);
      seeded = true;
    }
  }
  if (!seeded) k_tile_walk<MODE, D, M><<<dim3(blocks), dim3(64 * nw), lds, s>>>(a);
  return LG_OK;
}

extern "C" size_t lg_spread_tile_resource_topk_lds_bytes(int32_t tile, int32_t k, int32_t dim) {
  // one wave's share plus the workgroup's tables (the launch fits as many waves as it can)
  const int M = k <= 64 ? 2 : 4;
  const size_t per = M == 2 ? (dim > 64 ? walk_wave_bytes<MODE_TOPK, 128, 2>(tile)
                                        : walk_wave_bytes<MODE_TOPK, 64, 2>(tile))
                            : walk_wave_bytes<MODE_TOPK, 128, 4>(tile);
  return per + walk_shared_bytes(tile);
}

template <int D>
static int launch_fused(int M, const WalkArgs &a, hipStream_t s) {
  return M == 2 ? launch_walk<MODE_TOPK, D, 2>(a, s) : launch_walk<MODE_TOPK, D, 4>(a, s);
}

extern "C" int lg_spread_tile_resource_topk_f64(
    const int64_t *user_rowptr, const int32_t *user_items, const double *ra_edge,
    int64_t n_users, const void *lines, const void *ovf, int32_t null_row, const double *rbeta,
    const double *inv_cls, int32_t item_begin, int32_t tile, int32_t width, const float *eu,
    const float *ei, int32_t dim, const float *gb, int32_t n_chunks, const uint8_t *qb,
    int32_t qstride, const int64_t *ex_rowptr,
    const int32_t *ex_col, int64_t *ex_cur, int32_t k, int32_t first, double *io_val,
    int64_t *io_idx, int64_t n_positions, int64_t n_ex_positions, lg_stream_t stream) {
  LG_REQUIRE(user_rowptr && user_items && ra_edge && lines && ovf && rbeta && inv_cls &&
                 io_val && io_idx && n_users >= 0 && n_users < 0x7fffffff && item_begin >= 0,
             "lg_spread_tile_resource_topk_f64: bad arguments");
  // (the walk's stream positions are 32-bit)
  LG_REQUIRE(n_positions >= 0 && n_positions < 0x7fffffff && n_ex_positions >= 0 &&
                 n_ex_positions < 0x7fffffff,
             "lg_spread_tile_resource_topk_f64: %lld interactions / %lld exclusions exceed the "
             "walk's 32-bit positions", (long long)n_positions, (long long)n_ex_positions);
  LG_REQUIRE(tile >= 1 && tile <= 8192 && width >= 1 && width <= tile &&
                 (int64_t)item_begin + width < 0x7fffffff,
             "lg_spread_tile_resource_topk_f64: tile %d / width %d", tile, width);
  LG_REQUIRE(k >= 1 && k <= 128, "lg_spread_tile_resource_topk_f64: k=%d not in [1,128]", k);
  LG_REQUIRE(!eu == !ei && !eu == !gb,
             "lg_spread_tile_resource_topk_f64: eu, ei and gb go together");
  LG_REQUIRE(!eu || dim == 32 || dim == 64 || dim == 128,
             "lg_spread_tile_resource_topk_f64: dim %d not in {32,64,128}", dim);
  LG_REQUIRE(!eu || n_chunks == (width + 63) / 64,
             "lg_spread_tile_resource_topk_f64: n_chunks %d != ceil(width / 64)", n_chunks);
  LG_REQUIRE(!qb || (eu && qstride >= (width + 255) / 256 * 256),
             "lg_spread_tile_resource_topk_f64: qb needs eu and qstride >= width rounded to 256");
  LG_REQUIRE(!eu || n_chunks <= 64,
             "lg_spread_tile_resource_topk_f64: a G factor needs width <= 4096 (one chunk "
             "bound per lane), got %d", width);
  LG_REQUIRE(!ex_rowptr == !ex_col && !ex_rowptr == !ex_cur,
             "lg_spread_tile_resource_topk_f64: ex_rowptr/ex_col/ex_cur go together");
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
  a.eu = eu;
  a.ei = ei;
  a.gb = gb;
  a.nch = n_chunks;
  a.qb = qb;
  a.qstride = qstride;
  a.ex_rowptr = ex_rowptr;
  a.ex_col = ex_col;
  a.ex_cur = ex_cur;
  a.k = k;
  a.first = first;
  a.io_val = io_val;
  a.io_idx = io_idx;
  hipStream_t s = (hipStream_t)stream;
  const int M = k <= 64 ? 2 : 4;
  int st;
  switch (eu ? dim : 0) {
    case 0: st = launch_fused<0>(M, a, s); break;
    case 32: st = launch_fused<32>(M, a, s); break;
    case 64: st = launch_fused<64>(M, a, s); break;
    default: st = launch_fused<128>(M, a, s); break;
  }
  if (st != LG_OK) return st;
  return launch_status("lg_spread_tile_resource_topk_f64");
}

extern "C" int lg_spread_tile_resource_rank_f64(
    const int64_t *user_rowptr, const int32_t *user_items, const double *ra_edge,
    int64_t n_users, const void *lines, const void *ovf, int32_t null_row, const double *rbeta,
    const double *inv_cls, int32_t item_begin, int32_t tile, int32_t width, const float *eu,
    const float *ei, int32_t dim, const float *gb, int32_t n_chunks, const uint8_t *qb,
    int32_t qstride, const int64_t *ex_rowptr, const int32_t *ex_col, int64_t *ex_cur,
    const int64_t *tgt_rowptr, const int32_t *tgt_col, int32_t phase, double *val, int64_t *cnt,
    int64_t n_positions, int64_t n_ex_positions, lg_stream_t stream) {
  const char *who = "lg_spread_tile_resource_rank_f64";
  LG_REQUIRE(user_rowptr && user_items && ra_edge && lines && ovf && rbeta && inv_cls &&
                 tgt_rowptr && tgt_col && val && n_users >= 0 && n_users < 0x7fffffff &&
                 item_begin >= 0,
             "%s: bad arguments", who);
  LG_REQUIRE(phase == LG_SPREAD_RANK_VALUES || phase == LG_SPREAD_RANK_COUNTS,
             "%s: phase %d is neither LG_SPREAD_RANK_VALUES nor LG_SPREAD_RANK_COUNTS", who,
             phase);
  LG_REQUIRE(phase == LG_SPREAD_RANK_VALUES || cnt, "%s: the count phase needs cnt", who);
  // (the walk's stream positions are 32-bit)
  LG_REQUIRE(n_positions >= 0 && n_positions < 0x7fffffff && n_ex_positions >= 0 &&
                 n_ex_positions < 0x7fffffff,
             "%s: %lld interactions / %lld exclusions exceed the walk's 32-bit positions", who,
             (long long)n_positions, (long long)n_ex_positions);
  LG_REQUIRE(tile >= 1 && tile <= 8192 && width >= 1 && width <= tile &&
                 (int64_t)item_begin + width < 0x7fffffff,
             "%s: tile %d / width %d", who, tile, width);
  LG_REQUIRE(!eu == !ei, "%s: eu and ei go together", who);
  // (the value phase screens nothing: gb is read by the count phase only)
  LG_REQUIRE(eu ? (phase == LG_SPREAD_RANK_VALUES || gb) : !gb,
             "%s: gb goes with eu and ei (the count phase needs it)", who);
  LG_REQUIRE(!eu || dim == 32 || dim == 64 || dim == 128, "%s: dim %d not in {32,64,128}", who,
             dim);
  LG_REQUIRE(!gb || n_chunks == (width + 63) / 64, "%s: n_chunks %d != ceil(width / 64)", who,
             n_chunks);
  LG_REQUIRE(!qb || (gb && qstride >= (width + 255) / 256 * 256),
             "%s: qb needs gb and qstride >= width rounded to 256", who);
  LG_REQUIRE(!eu || width <= 4096,
             "%s: a G factor needs width <= 4096 (one chunk bound per lane), got %d", who, width);
  LG_REQUIRE(!ex_rowptr == !ex_col && !ex_rowptr == !ex_cur,
             "%s: ex_rowptr/ex_col/ex_cur go together", who);
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
  a.eu = eu;
  a.ei = ei;
  a.gb = gb;
  a.nch = n_chunks;
  a.qb = qb;
  a.qstride = qstride;
  // (exclusions drop columns from the counts; the values are those of the columns themselves)
  const bool counts = phase == LG_SPREAD_RANK_COUNTS;
  a.ex_rowptr = counts ? ex_rowptr : nullptr;
  a.ex_col = counts ? ex_col : nullptr;
  a.ex_cur = counts ? ex_cur : nullptr;
  a.tgt_rowptr = tgt_rowptr;
  a.tgt_col = tgt_col;
  a.phase = counts ? 1 : 0;
  a.val = val;
  a.cnt = cnt;
  hipStream_t s = (hipStream_t)stream;
  int st;
  switch (eu ? dim : 0) {
    case 0: st = launch_walk<MODE_RANK, 0, 2>(a, s); break;
    case 32: st = launch_walk<MODE_RANK, 32, 2>(a, s); break;
    case 64: st = launch_walk<MODE_RANK, 64, 2>(a, s); break;
    default: st = launch_walk<MODE_RANK, 128, 2>(a, s); break;
  }
  if (st != LG_OK) return st;
  return launch_status(who);
}
