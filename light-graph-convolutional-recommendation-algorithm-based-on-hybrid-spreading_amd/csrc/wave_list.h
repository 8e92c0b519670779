// A wave-owned candidate list of {double, int} entries in LDS, for the selection kernels of
// rows_topk.hip. Two policies behind one interface:
//
//   RegList<M>  CAP = 64 M (M = 2, 4; k <= CAP / 2). New entries go behind the n already
//               there; a compaction sorts all of them in registers (wave_compact<double, M>).
//   LdsList<H>  CAP = 2 H (H = 256, 512, 1024; k <= H). Two halves of H entries: A, always
//               sorted, and B, the entries admitted since the last compaction. A compaction
//               sorts B alone, takes the better of A[H - 1 - j] and B[j] into A (which leaves
//               the H best of both there, as a bitonic sequence) and runs the log2(H) merge
//               stages over A: about 0.45 of sorting A and B together. Two waves' lists merge
//               the same way without any sort. Sorting works on 256-entry chunks: a chunk is
//               loaded into registers (4 entries per lane), every bitonic stage of stride
//               < 256 runs there (register swaps and wave shuffles, wave_bitonic_stages of
//               common.h), and only the strides >= 256 are compare-exchanges through LDS.
//
// A list is the counters only; every member that touches the entries takes the wave's
// (ks, ids)[CAP] -- a list that kept the two pointers made hipcc form the wave's base address
// once, up front, and schedule all of k_rows_topk differently (k = 128 without G measured
// 0.46 % slower than with the pointers passed per call, which compiles to the code of the
// kernels written without a list type). Use, by one wave:
//   List L; if constexpr (List::kPadded) L.init(ks, ids);   (RegList has nothing to pad, and
//                                                  naming its (ks, ids) this early is the
//                                                  same base address formed up front)
//   pos = L.slot(rank); write (ks, ids)[pos]; L.add(n)   up to 64 entries per step
//   if (L.full()) { wave_sync(); L.compact(ks, ids, keep, tau, tau_id); }   room for another 64
//   wave_sync(); n = L.compact(ks, ids, keep, tau, tau_id)   the best `keep` sorted at [0, n)
//   n = L.append(ks, ids, pks, pids, n1, keep, tau, tau_id)  after a compact: a partner's
//                                                  sorted n1 <= keep entries merged in
// compact and append follow wave_compact's contract (common.h): they return the new count
// and set (tau, tau_id) to the last kept entry when the list holds `keep`, else {-inf, kPadId}.
// The order is (value desc, id asc) throughout.
#pragma once

#include "common.h"

namespace lg {

template <int M>
struct RegList {
  static constexpr int CAP = 64 * M;
  static_assert(CAP >= 128, "a merge holds two lists of k <= CAP / 2");
  static constexpr bool kPadded = false;  // nothing to set up: there is no init
  int n = 0;  // entries, the sorted ones first

  __device__ __forceinline__ int slot(int rank) const { return n + rank; }
  __device__ __forceinline__ void add(int c) { n += c; }
  __device__ __forceinline__ bool full() const { return n > CAP - 64; }
  __device__ __forceinline__ int compact(double *ks, int *ids, int keep, double &tau,
                                         int &tau_id) {
    return n = wave_compact<double, M>(ks, ids, n, keep, tau, tau_id);
  }
  __device__ __forceinline__ int append(double *ks, int *ids, const double *pks,
                                        const int *pids, int n1, int keep, double &tau,
                                        int &tau_id) {
    for (int e = lane_id(); e < n1; e += 64) {  // (n + n1 <= 2 keep <= CAP)
      ks[n + e] = pks[e];
      ids[n + e] = pids[e];
    }
    wave_sync();
    n += n1;
    return compact(ks, ids, keep, tau, tau_id);
  }
};

constexpr int kChunk = 256;  // entries a wave sorts in registers: 4 per lane
constexpr int kChunkM = kChunk / 64;

__device__ __forceinline__ void chunk_load(const double *ks, const int *ids, int base,
                                           double (&k)[kChunkM], int (&id)[kChunkM]) {
  const int lane = lane_id();
#pragma unroll
  for (int j = 0; j < kChunkM; ++j) {
    k[j] = ks[base + j * 64 + lane];
    id[j] = ids[base + j * 64 + lane];
  }
}

__device__ __forceinline__ void chunk_store(double *ks, int *ids, int base,
                                            const double (&k)[kChunkM],
                                            const int (&id)[kChunkM]) {
  const int lane = lane_id();
#pragma unroll
  for (int j = 0; j < kChunkM; ++j) {
    ks[base + j * 64 + lane] = k[j];
    ids[base + j * 64 + lane] = id[j];
  }
}

// The bitonic stages (size; stride = size / 2 .. 1) over the entries [0, P) of a wave-owned LDS
// list (P a multiple of kChunk): the strides >= kChunk as compare-exchanges through LDS (P / 2
// disjoint pairs per stage, two per lane per trip with their reads issued together; p < half
// is wave-uniform: half % 128 == 0 whenever such a stride exists), the rest chunk by chunk in
// registers. The caller has synchronised the wave's LDS writes.
__device__ __forceinline__ void lds_size_stages(double *ks, int *ids, int P, int size) {
  const int lane = lane_id();
  const int half = P >> 1;
  for (int stride = size >> 1; stride >= kChunk; stride >>= 1) {
    for (int p0 = lane; p0 < half; p0 += 128) {
      double a[2], b[2];
      int ia[2], ib[2], lo[2];
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const int p = p0 + 64 * q;
        lo[q] = ((p & ~(stride - 1)) << 1) | (p & (stride - 1));
        a[q] = ks[lo[q]];
        ia[q] = ids[lo[q]];
        b[q] = ks[lo[q] + stride];
        ib[q] = ids[lo[q] + stride];
      }
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const bool desc = (lo[q] & size) == 0;
        const bool swap = before(a[q], ia[q], b[q], ib[q]) != desc;
        if (swap) {
          ks[lo[q]] = b[q];
          ids[lo[q]] = ib[q];
          ks[lo[q] + stride] = a[q];
          ids[lo[q] + stride] = ia[q];
        }
      }
    }
    wave_sync();
  }
  double k[kChunkM];
  int id[kChunkM];
  for (int base = 0; base < P; base += kChunk) {
    chunk_load(ks, ids, base, k, id);
    wave_bitonic_stages<double, kChunkM, kChunk / 2>(k, id, base, size);
    chunk_store(ks, ids, base, k, id);
  }
  wave_sync();
}

// Bitonic sort of the P entries (ks, ids)[0, P) of a wave-owned LDS list (P a power of two,
// a multiple of kChunk) into the output order: entry 0 is the best by (value desc, id asc).
// The callers pad with {-inf, kPadId}, which sorts last.
__device__ __forceinline__ void lds_chunk_sort(double *ks, int *ids, int P) {
  double k[kChunkM];
  int id[kChunkM];
  // every chunk sorted on its own: the stages of size <= kChunk
  for (int base = 0; base < P; base += kChunk) {
    chunk_load(ks, ids, base, k, id);
    wave_bitonic_stages<double, kChunkM, 1>(k, id, base, 2);
    wave_bitonic_stages<double, kChunkM, 2>(k, id, base, 4);
    wave_bitonic_stages<double, kChunkM, 4>(k, id, base, 8);
    wave_bitonic_stages<double, kChunkM, 8>(k, id, base, 16);
    wave_bitonic_stages<double, kChunkM, 16>(k, id, base, 32);
    wave_bitonic_stages<double, kChunkM, 32>(k, id, base, 64);
    wave_bitonic_stages<double, kChunkM, 64>(k, id, base, 128);
    wave_bitonic_stages<double, kChunkM, 128>(k, id, base, 256);
    chunk_store(ks, ids, base, k, id);
  }
  wave_sync();
  for (int size = 2 * kChunk; size <= P; size <<= 1) lds_size_stages(ks, ids, P, size);
}

// A = [0, H), always sorted best-first with {-inf, kPadId} behind its cnt entries, and
// B = [H, H + m), the m <= H entries admitted since the last compaction (or a partner
// wave's sorted list).
template <int H>
struct LdsList {
  static constexpr int CAP = 2 * H;
  static_assert(H >= kChunk && (H & (H - 1)) == 0, "the list and its new entries: k <= H each");
  static constexpr bool kPadded = true;  // init pads A before the first entry
  int cnt = 0, m = 0;  // entries of the sorted list, new entries behind it

  __device__ __forceinline__ void init(double *ks, int *ids) {
    for (int e = lane_id(); e < H; e += 64) {
      ks[e] = neg_inf<double>();
      ids[e] = kPadId;
    }
    wave_sync();
  }
  __device__ __forceinline__ int slot(int rank) const { return H + m + rank; }  // (< CAP)
  __device__ __forceinline__ void add(int c) { m += c; }
  __device__ __forceinline__ bool full() const { return m > H - 64; }

  // Merge B into A and keep A's best `keep` <= H as the list: B is sorted (unless it already
  // is) over the next power of two >= m, then one flip stage -- A[H - 1 - j] takes the better
  // of itself and B[j]; of two best-first sequences that leaves the H best of both in A, as a
  // bitonic sequence -- and the log2(H) stages of a bitonic merge of A alone. About 0.45 of a
  // full sort of A and B at m = H, less for a short B, no sort at all for a sorted one.
  // The caller has synchronised B's writes.
  __device__ __forceinline__ int merge_b(double *ks, int *ids, bool sorted, int keep,
                                         double &tau, int &tau_id) {
    const int lane = lane_id();
    if (m == 0) return cnt;  // (wave-uniform; tau stands)
    double *kb = ks + H;
    int *ib = ids + H;
    if (!sorted) {
      int P = kChunk;
      while (P < m) P <<= 1;
      for (int e = m + lane; e < P; e += 64) {
        kb[e] = neg_inf<double>();
        ib[e] = kPadId;
      }
      wave_sync();
      lds_chunk_sort(kb, ib, P);
    }
    for (int j = lane; j < m; j += 64) {  // (B's entries past m are padding: no exchange)
      const int i = H - 1 - j;
      const double vb = kb[j];
      const int xb = ib[j];
      if (before(vb, xb, ks[i], ids[i])) {
        ks[i] = vb;
        ids[i] = xb;
      }
    }
    wave_sync();
    lds_size_stages(ks, ids, H, H);
    cnt = cnt + m < keep ? cnt + m : keep;
    m = 0;
    if (cnt == keep && keep > 0) { tau = ks[keep - 1]; tau_id = ids[keep - 1]; }
    else { tau = neg_inf<double>(); tau_id = kPadId; }
    wave_sync();
    return cnt;
  }
  __device__ __forceinline__ int compact(double *ks, int *ids, int keep, double &tau,
                                         int &tau_id) {
    return merge_b(ks, ids, false, keep, tau, tau_id);
  }
  __device__ __forceinline__ int append(double *ks, int *ids, const double *pks,
                                        const int *pids, int n1, int keep, double &tau,
                                        int &tau_id) {
    for (int e = lane_id(); e < n1; e += 64) {  // (n1 <= keep <= H)
      ks[H + e] = pks[e];
      ids[H + e] = pids[e];
    }
    wave_sync();
    m = n1;
    return merge_b(ks, ids, true, keep, tau, tau_id);
  }
};

}  // namespace lg
