/*
 * lgcnhs.h — C ABI of the MI355X (gfx950) hot path for LGCNHS
 * (Light Graph Convolutional Recommendation based on Hybrid Spreading).
 *
 * Every entry point replaces one piece of arithmetic that the reference runs inside
 * third-party kernels (PyG 2.6.1, torch 1.13.1, numpy 1.24.3/MKL). The reference has no
 * FFI of its own (it is pure Python), so the "binding" a maintainer adds is the ctypes
 * stub shown in INTEGRATION.md; the reference call site each function replaces is cited
 * on the function.
 *
 * Conventions (all functions):
 *   - Plain device pointers, sizes and a stream. No allocation, no free, no host sync:
 *     the caller owns every buffer; work is enqueued on `stream` (a hipStream_t, NULL =
 *     the default stream). Safe to capture into a hipGraph.
 *   - Return LG_OK (0) or an LG_ERR_* code; lg_last_error() gives a thread-local message.
 *     Nothing is thrown across the ABI.
 *   - Graph rows are CSR: int64 rowptr[n_rows+1] (absolute offsets), int32 column ids,
 *     columns ascending inside a row (the order of the reference's coalesced COO,
 *     utils/graph.py:32-33). Node ids cover users then items (items offset by U).
 *   - Embeddings are row-major fp32 [n, dim]; spreading matrices are row-major fp64.
 *   - Top-K output is sorted by (value desc, index asc); unused slots hold index -1.
 */
#ifndef LGCNHS_H
#define LGCNHS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void *lg_stream_t; /* hipStream_t */

enum lg_status {
  LG_OK = 0,
  LG_ERR_ARG = 1,         /* bad size / null pointer / unsupported dim or k */
  LG_ERR_HIP = 2,         /* a HIP runtime call failed (launch error) */
  LG_ERR_WORKSPACE = 3,   /* workspace smaller than the *_ws_bytes() answer */
};

/* ABI version of this header (bumped on any signature change). */
#define LG_ABI_VERSION 17
int lg_abi_version(void);
/* Message of the last failing call on this thread ("" if none). */
const char *lg_last_error(void);

/* ------------------------------------------------------------------------------------
 * Graph format and normalisation
 * ------------------------------------------------------------------------------------ */

/* rowptr[r] = lower_bound(keys, r) for r in [0, n_rows]; `keys` = the row id of each of
 * `nnz` entries, sorted ascending. Replaces the dense (U+I)^2 -> to_sparse_coo() round trip
 * of utils/graph.py:22-35 (convertEdgeIndexToAdjMatrix) as the way the graph reaches the
 * propagation kernel. */
int lg_csr_rowptr_from_sorted(const int64_t *keys, int64_t nnz, int64_t n_rows,
                              int64_t *rowptr, lg_stream_t stream);

/* dis[n] = deg(n)^-1/2 with deg(n) = rowptr[n+1]-rowptr[n] (in-degree as a target),
 * inf -> 0. PyG 2.6.1 gcn_norm(add_self_loops=False), called at
 * model/LightGCN/model.py:53 and model/LightGCNOpti/model.py:65. */
int lg_gcn_norm_f32(const int64_t *rowptr, int64_t n_nodes, float *dis,
                    lg_stream_t stream);

/* w[e] = dis[src[e]] * dis[row_offset + r] for every entry e of row r: the edge weights
 * gcn_norm returns (model/LightGCN/model.py:53, second tuple element). Only needed by
 * callers that ask for the weights; the propagation kernel recomputes them on the fly. */
int lg_gcn_edge_weight_f32(const int64_t *rowptr, const int32_t *src, const float *dis,
                           int64_t n_rows, int64_t row_offset, float *w,
                           lg_stream_t stream);

/* ------------------------------------------------------------------------------------
 * LightGCN propagation: one layer of  e^{l+1} = D^-1/2 A D^-1/2 e^l  over a row range,
 * with the layer mean of model/LightGCN/model.py:66-69 fused into the epilogue.
 * Replaces PyG propagate (index_select + message + scatter_add,
 * model/LightGCN/model.py:61-63,76-84) and torch.stack/mean (:66-69).
 *
 * For r in [0, n_rows), node g = row_offset + r:
 *   v[g] = sum_{e in row r, s = src[e]} w_e * x[s]      (w_e = w[e], or dis[s]*dis[g]
 *                                                          when w is NULL; same value)
 *   y[g] = v[g]                                   if y != NULL
 *   acc_mode FIRST: acc[g] = x0[g] + v[g]
 *            MID  : acc[g] = acc[g] + v[g]
 *            LAST : out[g] = (acc[g] + v[g]) / denom
 *            ONLY : out[g] = (x0[g] + v[g]) / denom            (a 1-layer model)
 *            NONE : nothing
 * x, y, x0, acc, out are [*, dim] arrays indexed by node id g (row-sharded callers pass
 * full-size arrays and their own row range). dim in {32, 64, 128, 256}. w (optional) is
 * the per-entry gcn_norm weight of lg_gcn_edge_weight_f32, indexed like src; passing it
 * streams 4 B/edge instead of gathering dis[s]. y must not alias x.
 * Rows with more than long_threshold entries (<= 0: none) are skipped; the caller runs
 * them through lg_spmm_long_rows_f32 (power-law hubs).
 * ------------------------------------------------------------------------------------ */
enum lg_acc_mode {
  LG_ACC_NONE = 0,
  LG_ACC_FIRST = 1,
  LG_ACC_MID = 2,
  LG_ACC_LAST = 3,
  LG_ACC_ONLY = 4,
};
int lg_spmm_layer_f32(const int64_t *rowptr, const int32_t *src, const float *dis,
                      const float *w, const float *x, float *y, const float *x0, float *acc,
                      float *out, int64_t n_rows, int64_t row_offset, int32_t dim,
                      int32_t acc_mode, float denom, int64_t long_threshold,
                      lg_stream_t stream);

/* lg_spmm_layer_f32 for a sparse input x (the backward pass of the same call sites,
 * reference model/LightGCN/train.py:150 `loss.backward()` through model.py:62): live[n]
 * (uint8, one per source node) == 0 promises that row n of x is all zero, and its gather is
 * skipped (its contribution is added as 0). Same sums as lg_spmm_layer_f32 when the
 * promise holds. Long rows (above long_threshold) are left to lg_spmm_long_rows_f32. */
int lg_spmm_layer_live_f32(const int64_t *rowptr, const int32_t *src, const float *dis,
                           const float *w, const float *x, float *y, const float *x0,
                           float *acc, float *out, int64_t n_rows, int64_t row_offset,
                           int32_t dim, int32_t acc_mode, float denom, int64_t long_threshold,
                           const uint8_t *live, lg_stream_t stream);

/* The long rows skipped above, cut into segments [seg_beg[s], seg_end[s]) of src/w
 * (seg_node[s] = node id of the segment's row): one wave per segment writes a partial sum
 * into partial[n_seg, dim] (caller-owned workspace), then long row j (node long_node[j],
 * segments seg_ptr[j] .. seg_ptr[j+1]) adds its partials in order and runs the same
 * y / acc_mode epilogue as lg_spmm_layer_f32. Deterministic (no atomics). */
int lg_spmm_long_rows_f32(const int64_t *seg_beg, const int64_t *seg_end,
                          const int32_t *seg_node, int64_t n_seg, const int32_t *long_node,
                          const int64_t *seg_ptr, int64_t n_long, const int32_t *src,
                          const float *dis, const float *w, const float *x, float *y,
                          const float *x0, float *acc, float *out, int32_t dim,
                          int32_t acc_mode, float denom, float *partial, lg_stream_t stream);

/* Output-restricted layers (the forward of one BPR training step, reference
 * model/LightGCN/train.py:30 `model.forward` + :31-45 indexing the mini-batch's rows: the loss
 * reads layer L only at the batch's rows, layer L-1 only there and at their neighbours, ...):
 * lg_spmm_layer_f32 / lg_spmm_long_rows_f32 computing only the rows r whose row_mask[r]
 * (uint8, per node id) is non-zero; every other row of y / acc / out is left untouched. Each
 * computed row is bitwise the unrestricted call's. lg_mark_neighbors_u8 sets out_mask[r] = 1
 * for every row r of in_mask and every source of its entries (the rows the layer below must
 * produce for it); out_mask is not cleared first and must not alias in_mask. */
int lg_spmm_layer_rows_f32(const int64_t *rowptr, const int32_t *src, const float *dis,
                           const float *w, const float *x, float *y, const float *x0,
                           float *acc, float *out, int64_t n_rows, int64_t row_offset,
                           int32_t dim, int32_t acc_mode, float denom, int64_t long_threshold,
                           const uint8_t *row_mask, lg_stream_t stream);
int lg_spmm_long_rows_masked_f32(const int64_t *seg_beg, const int64_t *seg_end,
                                 const int32_t *seg_node, int64_t n_seg,
                                 const int32_t *long_node, const int64_t *seg_ptr,
                                 int64_t n_long, const int32_t *src, const float *dis,
                                 const float *w, const float *x, float *y, const float *x0,
                                 float *acc, float *out, int32_t dim, int32_t acc_mode,
                                 float denom, float *partial, const uint8_t *row_mask,
                                 lg_stream_t stream);
int lg_mark_neighbors_u8(const int64_t *rowptr, const int32_t *src, int64_t n_rows,
                         const uint8_t *in_mask, uint8_t *out_mask, lg_stream_t stream);

/* fp16 layer storage (opt-in, inference): the same propagation call sites
 * (model/LightGCN/model.py:61-69, model/LightGCNOpti/model.py:74) with the per-layer
 * embeddings e^l held as IEEE binary16 between layers, so a layer gathers 2*dim bytes per
 * edge instead of 4*dim. Only the gather operand is 16-bit:
 *   xh^0 = f16(e0)                       lg_rows_f32_to_f16: round to nearest even,
 *                                        subnormals kept, |v| > 65504 -> +-inf, NaN -> NaN
 *   v[g] = sum_e w_e * f32(xh[s_e])      the products, additions and order of
 *                                        lg_spmm_layer_f32 run on the widened input f32(xh):
 *                                        v is that call's result bit for bit (ordinary rows
 *                                        and, through lg_spmm_long_rows_f16, hub rows)
 *   yh[g] = f16(v[g])                    if yh != NULL: the next layer's operand
 *   acc_mode epilogue                    as lg_spmm_layer_f32, in fp32 on the unrounded v;
 *                                        x0 (the fp32 e0), acc and out stay fp32
 * xh, yh are [*, dim] binary16 arrays indexed by node id (8-byte aligned rows: dim in
 * {32, 64, 128, 256}); yh must not alias xh. Every other argument, the argument checks and
 * the long_threshold contract are lg_spmm_layer_f32's / lg_spmm_long_rows_f32's (the
 * `partial` workspace stays fp32 [n_seg, dim]; segments are added in order). No allocation,
 * no host sync. lg_rows_f32_to_f16 converts n_rows * dim contiguous values (xh must not
 * alias x). */
int lg_rows_f32_to_f16(const float *x, int64_t n_rows, int32_t dim, void *xh,
                       lg_stream_t stream);
int lg_spmm_layer_f16(const int64_t *rowptr, const int32_t *src, const float *dis,
                      const float *w, const void *xh, void *yh, const float *x0, float *acc,
                      float *out, int64_t n_rows, int64_t row_offset, int32_t dim,
                      int32_t acc_mode, float denom, int64_t long_threshold,
                      lg_stream_t stream);
int lg_spmm_long_rows_f16(const int64_t *seg_beg, const int64_t *seg_end,
                          const int32_t *seg_node, int64_t n_seg, const int32_t *long_node,
                          const int64_t *seg_ptr, int64_t n_long, const int32_t *src,
                          const float *dis, const float *w, const void *xh, void *yh,
                          const float *x0, float *acc, float *out, int32_t dim,
                          int32_t acc_mode, float denom, float *partial, lg_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Full-catalog scoring with exclusion mask and top-K.
 * Replaces  score = e0_u @ e0_i^T ; score[train|val positives] = -1024 ; topk(score, k)
 * of model/LightGCN/recommend.py:83-114 (same code: LightGCNOpti/recommend.py:83-114,
 * LightGCN/evaluation.py:31-51). The U x I score matrix is never materialised.
 *
 * score(u, i) is the fp32 fused-multiply-add chain, in this element order,
 *   acc = 0; for s in [0, dim/4): for g in [0, 4): acc = fmaf(eu[u][g*dim/4+s], ei[i][g*dim/4+s], acc)
 * (what v_mfma_f32_16x16x4_f32 computes), replaced by mask_value when i is in the user's
 * exclusion row ex_col[ex_rowptr[u] .. ex_rowptr[u+1]) (sorted ascending).
 * eu = [n_users, dim] (a sharded caller passes its own user block and the matching
 * ex_rowptr slice), ei = [n_items, dim]. k in [1, 128]; dim in {32, 64, 128}.
 * n_splits >= 1 splits the item range over that many workgroup sets (for small user
 * counts); the workspace holds the partial lists.
 * ------------------------------------------------------------------------------------ */
size_t lg_score_topk_ws_bytes(int64_t n_users, int64_t n_items, int32_t dim, int32_t k,
                              int32_t n_splits);
int lg_score_topk_f32(const float *eu, const float *ei, int64_t n_users, int64_t n_items,
                      int32_t dim, const int64_t *ex_rowptr, const int32_t *ex_col,
                      float mask_value, int32_t k, int32_t n_splits, float *out_val,
                      int64_t *out_idx, void *ws, size_t ws_bytes, lg_stream_t stream);

/* lg_score_topk_f32 (csrc/topk_plain.hip) with a bf16 MFMA screen (csrc/topk.hip K2r): the
 * same outputs bit for bit (values, ids, order). eu_bf16 / ei_bf16: lg_bound_prep_f32's bf16 copies of eu / ei
 * (16-byte aligned). umarg[u] (fp32, per user) must bound |bf16 MFMA product - fp32 chain|
 * over every item, with slack for the fp32 roundings of the screen's own compares:
 *   umarg[u] >= (||du|| I + (||eu[u]|| + ||du||) DI + (2.01 dim 2^-24 + 2^-22) ||eu[u]|| I)
 * with du = eu[u] - bf16(eu[u]), I = max_i ||ei[i]||, DI = max_i ||ei[i] - bf16(ei[i])||
 * (lgcnhs.ops.screen_margins, from lg_bound_prep_f32's norm_up / err_up; the round-3 form
 * 0.0081 ||eu[u]|| I is larger and also valid). Any input is memory-safe and gives
 * lg_score_topk_f32's lists: a umarg[u] that is NaN, negative or +inf (non-finite
 * embeddings), and any NaN bf16 product, is no bound -- those items enter the user's list
 * and get the exact chain (NaN chain scores never rank, as in lg_score_topk_f32). One pass keeps per user the items whose bound can still reach the k-th
 * largest lower bound, and ranks those by the exact chain at the end (every k <= 128).
 * Workspace: lg_score_topk_screened_ws_bytes (the per-split partial lists as
 * lg_score_topk_f32's, plus for k > 32 the per-user list slabs of 128 / 256 8-byte entries per
 * split that the main pass keeps its lists in); splits as lg_score_topk_f32. On catalogs of
 * >= 1024 k items a
 * screen-only seed pass over the first 1/16 of the items runs first and leaves each user's
 * starting threshold in out_val[u * k + k - 1] (overwritten by the result); the outputs do
 * not depend on it. */
size_t lg_score_topk_screened_ws_bytes(int64_t n_users, int64_t n_items, int32_t dim,
                                       int32_t k, int32_t n_splits);
int lg_score_topk_screened_f32(const float *eu, const float *ei, const void *eu_bf16,
                               const void *ei_bf16, const float *umarg, int64_t n_users,
                               int64_t n_items, int32_t dim, const int64_t *ex_rowptr,
                               const int32_t *ex_col, float mask_value, int32_t k,
                               int32_t n_splits, float *out_val, int64_t *out_idx, void *ws,
                               size_t ws_bytes, lg_stream_t stream);

/* lg_score_topk_f32 for every k in [1, 1024] (csrc/topk_wide.hip K2w): the torch.topk(score, k)
 * of model/LightGCN/recommend.py:83-114 (same code: LightGCNOpti/recommend.py:83-114,
 * LightGCN/evaluation.py:31-51) at any RECOMMEND["k"] up to 1024. The contract is
 * lg_score_topk_f32's: the same score chain, mask, order (score desc, item asc), padding
 * (-inf / -1 when fewer than k items rank; NaN and -inf scores never rank), dim in
 * {32, 64, 128} and n_splits in [1, 4096]; for k <= 128 the outputs equal
 * lg_score_topk_f32's bit for bit. Each (split, user) keeps its candidate list in a slab of
 * 512 / 1024 / 2048 8-byte entries (k <= 256 / 512 / 1024) of the workspace, so the workspace
 * is always needed: lg_score_topk_wide_ws_bytes = splits x n_users x slab bytes (0 for
 * arguments the call refuses), 8-byte aligned. A caller short of memory passes user blocks
 * (eu rows and the matching ex_rowptr slice, as lgcnhs.ops.score_topk does).
 * LG_ERR_WORKSPACE when ws is NULL or short; LG_ERR_ARG on a null pointer, bad dim, k or
 * n_splits, a half-set exclusion pair or a misaligned ws, before any launch. n_users = 0
 * returns LG_OK. Never allocates, never syncs. */
size_t lg_score_topk_wide_ws_bytes(int64_t n_users, int64_t n_items, int32_t dim, int32_t k,
                                   int32_t n_splits);
int lg_score_topk_wide_f32(const float *eu, const float *ei, int64_t n_users, int64_t n_items,
                           int32_t dim, const int64_t *ex_rowptr, const int32_t *ex_col,
                           float mask_value, int32_t k, int32_t n_splits, float *out_val,
                           int64_t *out_idx, void *ws, size_t ws_bytes, lg_stream_t stream);

/* lg_score_topk_f32 for a short list of users (csrc/topk_batch.hip K2b): the request form of
 * model/LightGCN/recommend.py:83-114 -- the top-k of n_batch <= 64 rows user_ids[b] of the
 * full user table, without gathering embedding or exclusion rows. Row b of the outputs equals
 * lg_score_topk_f32's row user_ids[b] bit for bit (score chain, mask, strict admission, order,
 * padding). user_ids (device, int64) may repeat and need not be sorted; NULL means
 * 0 .. n_batch-1. ex_rowptr / ex_col are the FULL table's exclusion CSR (n_table_users + 1
 * row pointers), indexed by user id. An id outside [0, n_table_users) reads no table row of
 * its own (the index is clamped) and its output row is padding. k in [1, 128], dim in
 * {32, 64, 128}, n_items < 2^31 - 1. The items are divided over every wave of a grid that
 * fills the device; the workspace holds one partial list per (workgroup, user):
 * lg_score_topk_batch_ws_bytes, which does not depend on the device (0 for arguments the call
 * refuses). */
size_t lg_score_topk_batch_ws_bytes(int64_t n_batch, int64_t n_items, int32_t dim, int32_t k);
/* model/LightGCN/recommend.py:83-114 for the users of one request (above). LG_ERR_ARG on a
 * null pointer, n_batch outside [1, 64], bad dim or k, a half-set exclusion pair;
 * LG_ERR_WORKSPACE when ws is NULL or short; all before any launch. Never allocates, never
 * syncs. */
int lg_score_topk_batch_f32(const float *eu, const float *ei, const int64_t *user_ids,
                            int64_t n_batch, int64_t n_table_users, int64_t n_items, int32_t dim,
                            const int64_t *ex_rowptr, const int32_t *ex_col, float mask_value,
                            int32_t k, float *out_val, int64_t *out_idx, void *ws,
                            size_t ws_bytes, lg_stream_t stream);

/* lg_score_topk_batch_f32 restricted to a candidate item set (csrc/topk_items.hip K2i): the
 * request form of model/LightGCN/recommend.py:83-114 with a catalog filter. item_ids (device,
 * int32) holds n_cand strictly ascending ids in [0, n_items). Row b of the outputs is the
 * first k of {(v(user_ids[b], i), i) : i in item_ids} under (value desc, item id asc), v the
 * fp32 chain score of lg_score_topk_f32 or mask_value where i is in the user's exclusion row;
 * NaN and -inf never rank; shorter rows are padded with {-inf, -1}; the ids returned are real
 * item ids. That is lg_score_topk_f32(eu, ei[item_ids], ...) with the exclusion columns
 * renumbered to positions in item_ids and the ids mapped back, bit for bit, and with
 * item_ids = 0 .. n_items-1 lg_score_topk_f32's rows themselves -- without gathering a row:
 * only the candidates' rows of ei are read. user_ids, ex_rowptr / ex_col (the FULL table's
 * exclusion CSR, indexed by user id) and out-of-range user ids as in lg_score_topk_batch_f32.
 * n_batch in [1, 16], k in [1, 128], dim in {32, 64, 128}, 1 <= n_cand <= n_items < 2^31 - 1.
 * Memory-safe on any list: an id outside [0, n_items) reads row 0 and never enters a list; a
 * list that is not ascending gives unspecified lists. The candidate positions are divided over
 * every wave of a grid that fills the device; the workspace holds one partial list per
 * (workgroup, user): lg_score_topk_batch_items_ws_bytes = min(512, ceil(n_cand / 16)) x
 * n_batch x k x 8, device-independent (0 for arguments the call refuses). */
size_t lg_score_topk_batch_items_ws_bytes(int64_t n_batch, int64_t n_cand, int32_t dim,
                                          int32_t k);
/* model/LightGCN/recommend.py:83-114 for the users of one request over a candidate item set
 * (above). LG_ERR_ARG on a null pointer, n_batch outside [1, 16], bad dim, k, n_items or
 * n_cand, a half-set exclusion pair; LG_ERR_WORKSPACE when ws is NULL or short; all before any
 * launch. Never allocates, never syncs. */
int lg_score_topk_batch_items_f32(const float *eu, const float *ei, const int64_t *user_ids,
                                  int64_t n_batch, int64_t n_table_users, int64_t n_items,
                                  const int32_t *item_ids, int64_t n_cand, int32_t dim,
                                  const int64_t *ex_rowptr, const int32_t *ex_col,
                                  float mask_value, int32_t k, float *out_val, int64_t *out_idx,
                                  void *ws, size_t ws_bytes, lg_stream_t stream);

/* Top-k where every row has its own candidate list (csrc/topk_cand.hip K2c): the request form
 * of model/LightGCN/recommend.py:83-114 behind a per-user retrieval stage, and the ranking of a
 * held-out positive among sampled negatives. The candidates are a CSR: cand_rowptr (device,
 * int64, n_rows + 1), cand_col (device, int32), ids strictly ascending inside a row and in
 * [0, n_items). Row r is scored for user user_ids[r] (device, int64; NULL: user r). Output row
 * r is the first k of {(v(u_r, i), i) : i in candidate row r} under (value desc, item id asc),
 * v the fp32 chain score of lg_score_topk_f32 or mask_value where i is in u_r's row of
 * ex_rowptr / ex_col (the FULL table's exclusion CSR, indexed by user id); NaN and -inf never
 * rank; shorter rows are padded with {-inf, -1}; the ids returned are real item ids. That is
 * lg_score_topk_f32(eu[u_r], ei[cand_r], ...) with the exclusion columns renumbered and the ids
 * mapped back, bit for bit, without gathering a row. max_len is the caller's bound on the row
 * length: a row's candidates at positions >= max_len are ignored (defined, not an error). Each
 * row is scored in n_seg in [1, 4096] segments of split_len(max_len, n_seg) positions (one wave
 * per segment); the result does not depend on n_seg. n_seg > 1 keeps one partial list per
 * (segment, row) in the workspace: lg_score_topk_cand_ws_bytes = n_seg x n_rows x k x 8 (0 for
 * n_seg == 1 and for arguments the call refuses). k in [1, 128], dim in {32, 64, 128},
 * n_items < 2^31 - 1, max_len in [1, 2^31). Memory-safe on any list: a candidate id outside
 * [0, n_items) reads row 0 and never ranks, a user id outside [0, n_table_users) gives an
 * all-padding row, a row that is not ascending gives unspecified lists. */
size_t lg_score_topk_cand_ws_bytes(int64_t n_rows, int32_t dim, int32_t k, int32_t n_seg);
/* model/LightGCN/recommend.py:83-114 per row over the row's own candidates (above). LG_ERR_ARG
 * on a null pointer, n_rows < 1 or n_rows x n_seg / 4 past the grid limit, bad n_items,
 * max_len, dim, k or n_seg, a half-set exclusion pair; LG_ERR_WORKSPACE when the segments in
 * use need a workspace and ws is NULL or short; all before any launch. Never allocates, never
 * syncs. */
int lg_score_topk_cand_f32(const float *eu, const float *ei, const int64_t *user_ids,
                           int64_t n_rows, int64_t n_table_users, int64_t n_items,
                           const int64_t *cand_rowptr, const int32_t *cand_col, int64_t max_len,
                           int32_t dim, const int64_t *ex_rowptr, const int32_t *ex_col,
                           float mask_value, int32_t k, int32_t n_seg, float *out_val,
                           int64_t *out_idx, void *ws, size_t ws_bytes, lg_stream_t stream);
/* The scores of given (user, item) pairs -- the score[u, i] of model/LightGCN/recommend.py:83-114
 * read at the candidates only (csrc/topk_cand.hip): lg_score_topk_cand_f32's inputs, gather and
 * chain with no lists. out (device, fp32, one per entry of cand_col) gets at every position p
 * the chain score of (u_r, cand_col[p]), r the row of p, or mask_value where the item is in
 * u_r's exclusion row; -inf at positions >= max_len within their row, for an id outside
 * [0, n_items) and in the rows of a user id outside the table. Rows need not be ascending.
 * Refusals as above (no k, n_seg or workspace). Never allocates, never syncs. */
int lg_score_cand_f32(const float *eu, const float *ei, const int64_t *user_ids, int64_t n_rows,
                      int64_t n_table_users, int64_t n_items, const int64_t *cand_rowptr,
                      const int32_t *cand_col, int64_t max_len, int32_t dim,
                      const int64_t *ex_rowptr, const int32_t *ex_col, float mask_value,
                      float *out, lg_stream_t stream);

/* The rank of given (user, item) pairs over the FULL catalog (csrc/rank.hip K2k): what an
 * evaluation on held-out items asks (MRR, AUC, mean rank, recall / NDCG at any cut-off) and no
 * list of k answers past position k. With v(u, j) = mask_value where j is in u's row of
 * ex_rowptr / ex_col (the FULL table's exclusion CSR, indexed by user id), else the fp32 chain
 * score of lg_score_topk_f32, and better(a, ja, b, jb) = a > b || (a == b && ja < jb):
 *     rank(u, i) = #{ j in [0, n_items), j != i : better(v(u, j), j, v(u, i), i) }   (0 = first)
 * Excluded items rank at mask_value, an excluded target has v = mask_value, NaN follows the
 * formula literally (never better; nothing is better than a NaN target). For finite scores and
 * k <= 1024: rank < k iff the top-k list of u holds i at position rank. Rows follow
 * lg_score_topk_cand_f32's conventions: row r belongs to user user_ids[r] (device, int64; NULL:
 * user r), its targets are tgt_col[tgt_rowptr[r] .. tgt_rowptr[r + 1]) (device, int64 / int32),
 * in any order. out_rank (device, int64) and out_score (device, fp32) have one entry per entry of
 * tgt_col; out_score gets v(u, i). max_targets in [1, LG_RANK_ROW_MAX] is the caller's bound on a
 * row's length: positions >= max_targets of a row get {-1, -inf} (defined, not an error; a longer
 * list is several rows with the same user id). A target id outside [0, n_items) gets {-1, -inf},
 * a user id outside [0, n_table_users) {-1, -inf} for its whole row; memory-safe on any input.
 * The items are counted in n_splits in [1, 4096] ranges of split_len(n_items, n_splits) items;
 * integer counts: the result does not depend on n_splits. The workspace holds a threshold and an
 * id per target slot and one int32 count per (split, slot): lg_score_rank_ws_bytes(n_rows,
 * n_targets, dim, n_splits) = n_targets x (8 + 4 n_splits) with n_targets = n_rows x max_targets,
 * the slots of the call (0 for arguments the call refuses). dim in {32, 64, 128}, n_items <
 * 2^31 - 1. */
#define LG_RANK_ROW_MAX 4
size_t lg_score_rank_ws_bytes(int64_t n_rows, int64_t n_targets, int32_t dim, int32_t n_splits);
/* LG_ERR_ARG on a null pointer (user_ids and the exclusion pair may be NULL), n_rows < 1 or
 * n_rows x n_splits past the grid limit, bad n_table_users, n_items, max_targets, dim or
 * n_splits, a half-set exclusion pair; LG_ERR_WORKSPACE when ws is NULL or short; all before any
 * launch. Never allocates, never syncs. */
int lg_score_rank_f32(const float *eu, const float *ei, const int64_t *user_ids, int64_t n_rows,
                      int64_t n_table_users, int64_t n_items, const int64_t *tgt_rowptr,
                      const int32_t *tgt_col, int32_t max_targets, int32_t dim,
                      const int64_t *ex_rowptr, const int32_t *ex_col, float mask_value,
                      int32_t n_splits, int64_t *out_rank, float *out_score, void *ws,
                      size_t ws_bytes, lg_stream_t stream);

/* Dense masked score matrix G[u][i] (same score definition and mask as above), written
 * with leading dimension ldg. Replaces getAllocateMat's matmul + masks
 * (model/SpreadLightGCN/model.py:74-104, model/SpreadLightGCNOpti/model.py:139-169). */
int lg_score_dense_f32(const float *eu, const float *ei, int64_t n_users, int64_t n_items,
                       int32_t dim, const int64_t *ex_rowptr, const int32_t *ex_col,
                       float mask_value, float *G, int64_t ldg, lg_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Hybrid spreading (model/SpreadMethod/model.py), fp64, from the interaction matrix A
 * held sparse: user rows (user_rowptr/user_items) and item rows (item_rowptr/item_users).
 * ------------------------------------------------------------------------------------ */

/* gW[i][j] = sum_{v in users(i), ascending} [j in items(v)] * (1 / k_v), k_v = |items(v)|.
 * = np.dot(A.T / k_u, A) of getSpreadingGeneralMat (model/SpreadMethod/model.py:14-27).
 * gW is [n_items, n_items], fully written (zeros included). */
int lg_spread_general_f64(const int64_t *item_rowptr, const int32_t *item_users,
                          const int64_t *user_rowptr, const int32_t *user_items,
                          int64_t n_users, int64_t n_items, double *gW,
                          lg_stream_t stream);

/* W = lg_hybrid_weight_f64(lg_spread_general_f64(...), k_item, lambda, either transpose)
 * bit for bit, without general_W in memory (general_W is exactly symmetric): getSpreading-
 * GeneralMat + HybridS (model/SpreadMethod/model.py:14-27, 63-85) for one lambda. W is
 * [n_items, n_items], fully written; ws: lg_spread_hybrid_ws_bytes(n_items, n_users) bytes. */
size_t lg_spread_hybrid_ws_bytes(int64_t n_items, int64_t n_users);
int lg_spread_hybrid_f64(const int64_t *item_rowptr, const int32_t *item_users,
                         const int64_t *user_rowptr, const int32_t *user_items,
                         const double *k_item, int64_t n_users, int64_t n_items, double lambda,
                         double *W, void *ws, size_t ws_bytes, lg_stream_t stream);

/* W[i][j] = gWsrc[i][j] / den, den = k_i^(1-lambda) * k_j^lambda, den == 0 -> 1, with
 * gWsrc = gW (transpose_gw = 0) or gW^T (transpose_gw = 1). HybridS,
 * model/SpreadMethod/model.py:63-85 (the .T variants: SpreadMethod/recommend.py:91,101). */
int lg_hybrid_weight_f64(const double *gW, const double *k_item, int64_t n_items,
                         double lambda, int32_t transpose_gw, double *W,
                         lg_stream_t stream);

/* F[u][j] = sum_{i in items(u), ascending} W[i][j] : getResource's np.dot(A, W)
 * (model/SpreadMethod/model.py:88-99) for user rows [0, n_users). */
int lg_spread_resource_f64(const int64_t *user_rowptr, const int32_t *user_items,
                           const double *W, int64_t n_users, int64_t n_items, double *F,
                           int64_t ldf, lg_stream_t stream);

/* Per-row top-K over dense fp64 rows F[r][0..n_cols) (leading dim ldf), optionally
 * multiplied by the fp32 score G[r][j] (eu/ei non-NULL; same chain as lg_score_topk_f32,
 * promoted to fp64 before the product, as numpy's G * F does:
 * model/SpreadLightGCN/model.py:151). Exclusion rows ex_* (may be NULL):
 *   excl_mode DROP: excluded columns are removed (argsort + filter of
 *                   model/SpreadMethod/recommend.py:39-47);
 *   excl_mode NONE: nothing is removed (the unfiltered ProbS/movielens branch,
 *                   model/SpreadMethod/recommend.py:49-50).
 * With a G factor the exclusions must be DROP (G's -1024 mask is then never observable).
 * k in [1, 128] (lg_rows_topk_wide_f64 below takes k up to 1024). Rows with fewer than k
 * survivors are padded with index -1. */
enum lg_excl_mode { LG_EXCL_DROP = 0, LG_EXCL_NONE = 1 };
int lg_rows_topk_f64(const double *F, int64_t ldf, int64_t n_rows, int64_t n_cols,
                     const float *eu, const float *ei, int32_t dim,
                     const int64_t *ex_rowptr, const int32_t *ex_col, int32_t excl_mode,
                     int32_t k, double *out_val, int64_t *out_idx, lg_stream_t stream);

/* lg_rows_topk_f64 for k in [1, 1024]: the reference's argsort + filter + [:k] takes any
 * RECOMMEND["k"] (model/SpreadMethod/recommend.py:31-50, model/SpreadLightGCN/recommend.py;
 * G * F: model/SpreadLightGCN/model.py:151). Same arguments, values, admission (v > the
 * K-th value: NaN and -inf never rank), order (value desc, column asc), exclusion modes and
 * {-inf, -1} padding; the candidate lists live in LDS (512 / 1024 / 2048 entries for
 * k <= 256 / 512 / 1024), no workspace. At k <= 128 its lists are lg_rows_topk_f64's bit for
 * bit. */
int lg_rows_topk_wide_f64(const double *F, int64_t ldf, int64_t n_rows, int64_t n_cols,
                          const float *eu, const float *ei, int32_t dim,
                          const int64_t *ex_rowptr, const int32_t *ex_col, int32_t excl_mode,
                          int32_t k, double *out_val, int64_t *out_idx, lg_stream_t stream);

/* lg_spread_resource_f64 + lg_rows_topk_(wide_)f64 over a candidate item set, fused: row r of
 * the output is the first k (in [1, 1024]) of {(v(r, j), j) : j in item_ids[0..n_cand), j not
 * dropped by r's exclusions} under (value desc, item id asc), v(r, j) = (G[r][j] *) F[r][j],
 * F[r][j] = sum_{i in user_items of row r, ascending} W[i][j] over the full n_items x n_items
 * W (a candidate set restricts the ranked columns, never the spreading), G as above
 * (eu [n_rows, dim], ei [n_items, dim]: the full item table). item_ids: strictly ascending
 * ids in [0, n_items), n_cand in [0, n_items] (0: every row is padding). Exclusion columns are
 * item ids; modes, admission (NaN and -inf never rank) and the {-inf, -1} padding as
 * lg_rows_topk_f64; out_idx holds item ids. Bit for bit lg_rows_topk_(wide_)f64 on the
 * columns item_ids of lg_spread_resource_f64's F with ei[item_ids], the exclusions renumbered
 * and the ids mapped back; no F, no gather, no workspace. Memory-safe on any list: an id
 * outside [0, n_items) never ranks, a list that is not ascending gives unspecified lists. */
int lg_spread_rows_topk_items_f64(const int64_t *user_rowptr, const int32_t *user_items,
                                  const double *W, int64_t n_rows, int64_t n_items,
                                  const int32_t *item_ids, int64_t n_cand,
                                  const float *eu, const float *ei, int32_t dim,
                                  const int64_t *ex_rowptr, const int32_t *ex_col,
                                  int32_t excl_mode, int32_t k, double *out_val,
                                  int64_t *out_idx, lg_stream_t stream);

/* The rank of given (row, column) targets over dense fp64 rows (csrc/rows_rank.hip K4k): where
 * a user's held-out items stand among ALL items in the order of the spreading / LGCNHS
 * recommendation (argsort + filter of model/SpreadMethod/recommend.py:31-50; G * F:
 * model/SpreadLightGCN/model.py:151), at any depth. F, ldf, n_cols, eu (one row per row of F),
 * ei, dim, the exclusion CSR (aligned with F's n_f_rows rows) and excl_mode as
 * lg_rows_topk_f64; v(r, j) = F[r][j] or (double)G[r][j] * F[r][j], that entry's values bit
 * for bit. A column j RANKS for row r iff v(r, j) > -inf (NaN and -inf never rank) and, under
 * LG_EXCL_DROP, j is not in r's exclusion row. Kernel row q in [0, n_krows) names F row
 * krow_f[q] (device, int64) and the targets t_col[t_rowptr[q] .. t_rowptr[q + 1]) (device,
 * int64 [n_krows + 1] / int32): any order, duplicates allowed, at most LG_ROWS_RANK_ROW_MAX of
 * them -- the caller's contract (a longer target list is several kernel rows with the same F
 * row); the kernel clamps a longer row to the maximum and never writes out of bounds. out_rank
 * (device, int64) and out_val (device, fp64) are aligned with t_col: for a target i of row r
 *     out_val  = v(r, i)
 *     out_rank = #{ ranked j != i : v(r, j) > v(r, i) || (v(r, j) == v(r, i) && j < i) }
 *                if i ranks, else -1                                            (0 = first)
 * so for any k <= 1024: rank < k iff lg_rows_topk_(wide_)f64's row holds i at position rank,
 * with a bit-equal value. A target named twice gets the same rank twice. A target id outside
 * [0, n_cols) gets {-1, -inf}, as does every target of a kernel row whose F row is outside
 * [0, n_f_rows); an entry of t_col that belongs to no kernel row keeps what the caller put
 * there. No workspace, no global atomics (16.5 KiB of LDS per row), integer counts: the result
 * does not depend on how a row's columns are split over waves. LG_ERR_ARG, before any launch,
 * on a null pointer (eu / ei and the exclusion pair may be NULL, each pair together), bad
 * sizes, dim not in {32, 64, 128}, a bad excl_mode, a G factor with exclusions but
 * LG_EXCL_NONE. n_krows = 0: LG_OK, nothing runs. */
#define LG_ROWS_RANK_ROW_MAX 1024
int lg_rows_rank_f64(const double *F, int64_t ldf, int64_t n_f_rows, int64_t n_cols,
                     const float *eu, const float *ei, int32_t dim,
                     const int64_t *ex_rowptr, const int32_t *ex_col, int32_t excl_mode,
                     int64_t n_krows, const int64_t *krow_f, const int64_t *t_rowptr,
                     const int32_t *t_col, int64_t *out_rank, double *out_val,
                     lg_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Factored spreading over item tiles: the path for catalogs whose I x I general_W / W do
 * not fit (SURVEY.md §8 a9 "K3s"; C5 = 1M x 1M would need 8 TB per matrix). The values of
 * lg_spread_general_f64 -> lg_hybrid_weight_f64 -> lg_spread_resource_f64
 * (-> lg_rows_topk_f64), i.e. the reference's getSpreadingGeneralMat / HybridS /
 * getResource / recommendForAllUser (model/SpreadMethod/model.py:14-99,
 * model/SpreadMethod/recommend.py:31-50, model/SpreadLightGCN/model.py:151), without ever
 * holding an I x I or U x I matrix, as
 *   F[u][j] = rb_j * sum over the paths u -> i -> v -> j of fl(1/k_v) * ra_i
 * (ra = 1/alpha, rb = 1/beta; each term within a few ulp of the reference's W entry, the
 * summation order the walk's own, fixed). Tiles [j0, j0 + tile) of item columns are built
 * a group of <= 16 at a time: lg_spread_group_cursor -> lg_spread_group_bound ->
 * lg_spread_group_units -> (inclusive scan of the units) -> lg_spread_group_rows_f64; each
 * tile is then walked by lg_spread_tile_resource_topk_f64 (running top-K lists), with
 * lg_score_chunk_bound's score bounds when there is a G factor. The orchestration
 * (lgcnhs.ops.spread_topk_tiled) is host code; see DESIGN.md §5 K3s. The per-tile build
 * passes, the F-writing walk and the two-kernel top-K merge that these replace are kept,
 * as bitwise references for the tests, in include/lgcnhs_ref.h (lib/liblgcnhs_ref.so only).
 * ------------------------------------------------------------------------------------ */

/* ra[i] = 1 / alpha[i], rb[i] = 1 / beta[i] (a zero factor -> 1: the reference's den == 0
 * rule, model/SpreadMethod/model.py:81-82; such rows / columns hold no paths). */
int lg_hybrid_recip_f64(const double *k_item, int64_t n_items, double lambda, double *ra,
                        double *rb, lg_stream_t stream);

/* inv[v] = fl(1 / (rowptr[v+1] - rowptr[v])): the (A.T / k_u) factor of
 * model/SpreadMethod/model.py:21-25, as lg_spread_general_f64 computes it. */
int lg_inv_degree_f64(const int64_t *rowptr, int64_t n_rows, double *inv,
                      lg_stream_t stream);

/* Spreading for item baskets that are not rows of A (csrc/spread_rows.hip K3r): the F row of
 * getSpreadingGeneralMat / HybridS / getResource (model/SpreadMethod/model.py:14-27, 63-85,
 * 88-99) for any 0/1 row B over the items -- a new visitor's cart, a session, one item --
 * regrouped so that no I x I matrix and no tile is built:
 *     T[v] = inv_ku[v] * sum_{i in items(v), i in B} ra[i]      lg_spread_rows_weight_f64
 *     F[j] = rb[j]     * sum_{v in users(j)}         T[v]       lg_spread_rows_resource_f64
 * (ra, rb: lg_hybrid_recip_f64; inv_ku: lg_inv_degree_f64), one sweep of A by user and one of
 * A by item for a block of at most LG_SPREAD_ROWS_BLOCK baskets. The baskets of the block are a
 * CSR (basket_rowptr int64 [n_baskets + 1], offsets into basket_items int32; an id outside
 * [0, n_items) is skipped, an item named twice counts once).
 *
 * The order of every sum is a function of the one list it runs over: the terms of a basket are
 * added one at a time in ascending position of the list, from +0.0; a list longer than
 * LG_SPREAD_ROWS_SEG positions is cut at multiples of it, each segment summed so, and the
 * segments' sums added in segment order. It does not depend on the grid, the device, the
 * block's other baskets, the basket's place in the block or timing; there is no floating-point
 * atomic. Users whose T row is zero are skipped by test (their mark word is 0), which changes
 * no bit. The lists longer than LG_SPREAD_ROWS_SEG are named by the caller, once per A:
 * long_ids (device, int32 [n_long], ascending list ids) and long_ptr (device, int64
 * [n_long + 1], the exclusive prefix sum of ceil(len / LG_SPREAD_ROWS_SEG)), n_long_units =
 * long_ptr[n_long]; both NULL with n_long = 0. A long user missing from the table counts as a
 * zero T row (its mark word is cleared), a long item missing from it gets no F column written;
 * no table makes a kernel read or write outside the arrays.
 *
 * T is [n_users, n_baskets] fp64 (leading dimension n_baskets) and user_marks one 64-bit word
 * per user, bit b set iff T[v, b] != 0: only those entries of T are written by pass 1 and read
 * by pass 2 (T needs no clearing), every word of user_marks is written. F is [n_baskets, ldf]:
 * columns [0, n_items) of every row are written, zeros included. ws: device scratch of
 * lg_spread_rows_weight_ws_bytes(n_items, n_long_units) / lg_spread_rows_resource_ws_bytes(
 * n_long_units) bytes (the per-item basket words and the segments' partial sums). LG_ERR_ARG,
 * before any launch, on a null pointer, n_baskets outside [1, LG_SPREAD_ROWS_BLOCK], negative
 * or >= 2^31-1 sizes, ldf < n_items, a bad long-list table size, and on a NULL or short
 * workspace (the message names ws_bytes). */
#define LG_SPREAD_ROWS_BLOCK 64
#define LG_SPREAD_ROWS_SEG 4096
size_t lg_spread_rows_weight_ws_bytes(int64_t n_items, int64_t n_long_units);
int lg_spread_rows_weight_f64(const int64_t *user_rowptr, const int32_t *user_items,
                              int64_t n_users, int64_t n_items, const double *ra,
                              const double *inv_ku, const int64_t *basket_rowptr,
                              const int32_t *basket_items, int32_t n_baskets,
                              const int32_t *long_ids, const int64_t *long_ptr, int64_t n_long,
                              int64_t n_long_units, double *T, uint64_t *user_marks, void *ws,
                              size_t ws_bytes, lg_stream_t stream);
size_t lg_spread_rows_resource_ws_bytes(int64_t n_long_units);
int lg_spread_rows_resource_f64(const int64_t *item_rowptr, const int32_t *item_users,
                                int64_t n_items, int64_t n_users, const double *T,
                                const uint64_t *user_marks, const double *rb,
                                int32_t n_baskets, const int32_t *long_ids,
                                const int64_t *long_ptr, int64_t n_long, int64_t n_long_units,
                                double *F, int64_t ldf, void *ws, size_t ws_bytes,
                                lg_stream_t stream);

/* Line format of a tile (lgcnhs_ref.h lg_spread_tile_rows_f64 builds one tile at a time):
 * row i of general_W restricted to the tile as one 128-byte line at lines + 128 i (32
 * uint32 words) plus, for rows that do not fit, a run of 16-byte units in ovf. Word 0 =
 * header: bit 31 V format, bit 30 overflow, bit 29 "slow" (V rows, P rows with a class
 * >= 512), bits 0-28 the run's first unit (whose .x = the number of data units after it).
 *   P rows (bound[i] <= vthr): one word per (user v, item j) pair behind the row, users
 *     ascending then items ascending: bits 0-15 j - item_begin, bits 16-30 user_cls[v] (a
 *     1-based class of v's degree: inv_cls[user_cls[v]] = fl(1/k_v)); 0 = padding.
 *   V rows (hub items, bound[i] > vthr): one 16-byte entry per distinct column, ascending:
 *     {0x80000000 | (j - item_begin), fp64 general_W[i][j] (lo, hi), 0}.
 * Lambda-independent (a sweep reuses the tile); line n_items (the walk's padding row) is
 * zeroed by the caller.
 *
 * Group build: n_tiles (<= 16; <= 8 for tiles wider than 4096) consecutive tiles at once, each
 * (item row, user) pair visited once per group instead of once per tile. Tile t of the group
 * is [group_begin + t tile, min(group_begin + (t + 1) tile, stop)).
 * lg_spread_group_cursor: counts[v][0..15] (16 uint16 per user, 16-byte aligned, unused
 *   tiles 0) = user v's items in each tile, end[v] = the position after the group's last
 *   (cur[v] = the first position with item >= group_begin; cur and end must not alias;
 *   positions < 2^32), rec[v] (16 bytes per user, 16-byte aligned) = the user's record for
 *   the rows pass: its class (user_cls) and up to 6 of its group items in place, else cur.
 * lg_spread_group_bound: bound[t][i] ([n_tiles][n_items] int64) = the (user, tile item)
 *   pairs behind row i of W in tile t (its paths).
 * lg_spread_group_units: units[t][i] ([n_tiles][n_items] int64) = the overflow units of
 *   row i in tile t (1 + ceil((bound - 31) / 4) for P rows with bound > 31, 1 + (min(bound,
 *   width_t) - 7) for V rows with more than 7 entries, else 0); the caller's inclusive scan
 *   of the flat array (units_incl) places every run: tile t's runs start at unit
 *   units_incl[t n_items - 1] (0 for t = 0), each row's run at its exclusive prefix.
 * lg_spread_group_rows_f64: the lines and runs of every tile t of the group, tile t's
 *   lines at lines + t (n_items + 1) 128 bytes (each tile's line n_items zeroed by the
 *   caller), its runs in ovf as units_incl places them (header pointers relative to the
 *   tile's first unit: each tile's lines and runs are the per-tile build's, bit for bit);
 *   ovf holds units_incl[n_tiles n_items - 1] + 64 units; row_len as [n_tiles][n_items];
 *   vthr in [31, 65535]; cur / counts / rec from lg_spread_group_cursor; ws:
 *   lg_spread_group_rows_ws_bytes(n_items, n_tiles) bytes. */
int lg_spread_group_cursor(const int64_t *user_rowptr, const int32_t *user_items,
                           const uint16_t *user_cls, int64_t n_users, int32_t group_begin,
                           int32_t tile, int32_t n_tiles, int32_t stop, const int64_t *cur,
                           int64_t *end, uint16_t *counts, void *rec, lg_stream_t stream);
int lg_spread_group_bound(const int64_t *item_rowptr, const int32_t *item_users,
                          int64_t n_items, const uint16_t *counts, int32_t n_tiles,
                          int64_t *bound, lg_stream_t stream);
int lg_spread_group_units(const int64_t *bound, int64_t n_items, int32_t group_begin,
                          int32_t tile, int32_t n_tiles, int32_t stop, int64_t vthr,
                          int64_t *units, lg_stream_t stream);
size_t lg_spread_group_rows_ws_bytes(int64_t n_items, int32_t n_tiles);
int lg_spread_group_rows_f64(const int64_t *item_rowptr, const int32_t *item_users,
                             const int32_t *user_items, const double *inv_deg,
                             int64_t n_items, const int64_t *cur, const uint16_t *counts,
                             const void *rec, int32_t group_begin, int32_t tile,
                             int32_t n_tiles, int32_t stop, const int64_t *bound, int64_t vthr,
                             const int64_t *units_incl, void *lines, void *ovf,
                             int32_t *row_len, void *ws, size_t ws_bytes, lg_stream_t stream);

/* cur[v] = first position of user v's item row (ascending) with item >= item_begin: the
 * cursor state for a tile walk that starts at item_begin (an item-range shard of a
 * multi-GPU run) instead of 0. */
int lg_spread_tile_seek(const int64_t *user_rowptr, const int32_t *user_items,
                        int64_t n_users, int32_t item_begin, int64_t *cur, lg_stream_t stream);

/* Merge n_lists sorted top-K lists per row, in_val/in_idx laid out [n_lists][n_rows][k]
 * (value desc, index asc; index -1 = empty), into out_val/out_idx [n_rows][k] in the same
 * order: the per-item-range lists of lg_spread_tile_resource_topk_f64 (disjoint item ranges,
 * the multi-GPU shards) give the lists
 * a single walk over all items would. k in [1, 128] (lg_topk_lists_merge_wide_f64 takes k up
 * to 1024). */
int lg_topk_lists_merge_f64(const double *in_val, const int64_t *in_idx, int32_t n_lists,
                            int64_t n_rows, int32_t k, double *out_val, int64_t *out_idx,
                            lg_stream_t stream);

/* lg_topk_lists_merge_f64 for k in [1, 1024] (same layout, order and padding; the list in
 * LDS): merges the item-range shards' lists of a spreading run whose RECOMMEND["k"] exceeds
 * 128 (the [:k] of model/SpreadMethod/recommend.py:31-50 over the union of the ranges). */
int lg_topk_lists_merge_wide_f64(const double *in_val, const int64_t *in_idx, int32_t n_lists,
                                 int64_t n_rows, int32_t k, double *out_val,
                                 int64_t *out_idx, lg_stream_t stream);

/* The tile walk: each user's F columns [item_begin, item_begin + width) are accumulated in
 * LDS (the values of the F-writing reference walk, lgcnhs_ref.h, bit for bit) and merged
 * straight into the running top-K lists
 * io_val/io_idx [n_users][k] (first != 0: start empty); F is never written to memory. G
 * factor: eu = the rows' user embeddings, ei = all item embeddings, gb =
 * lg_score_chunk_bound's [n_users][n_chunks] bounds for this tile (n_chunks =
 * ceil(width / 64) <= 64) and optionally qb/qstride, its per-column 8-bit bounds: only
 * columns whose bound (gb * q / 255 with qb) times F can beat the K-th value get the exact
 * score chain.
 * Exclusions (dropped): ex_rowptr/ex_col as in lg_rows_topk_f64 plus a per-row cursor
 * ex_cur[n_users] positioned at the walk's first item by lg_spread_tile_seek(ex_rowptr,
 * ex_col, ...) and advanced here. Walked over tiles in ascending order, the lists equal
 * lg_rows_topk_f64 over the F rows the walk sums. k in [1, 128] (larger k: the host peels
 * passes of 128, lgcnhs.ops.spread_topk_tiled); dim in
 * {32, 64, 128}. The walk keeps its stream positions in 32 bits: n_users, the interactions
 * and the exclusions must each be < 2^31; n_positions / n_ex_positions are upper bounds of
 * user_rowptr[n_users] / ex_rowptr[n_users] (the lengths of user_items / ex_col, 0 without
 * exclusions), checked here -- the library does not read device memory on the host.
 * lg_spread_tile_resource_topk_lds_bytes: LDS of one wave plus the
 * workgroup's tables (the launch fits as many waves per CU as the LDS holds). */
size_t lg_spread_tile_resource_topk_lds_bytes(int32_t tile, int32_t k, int32_t dim);
int lg_spread_tile_resource_topk_f64(const int64_t *user_rowptr, const int32_t *user_items,
                                     const double *ra_edge, int64_t n_users,
                                     const void *lines, const void *ovf, int32_t null_row,
                                     const double *rbeta,
                                     const double *inv_cls, int32_t item_begin, int32_t tile,
                                     int32_t width, const float *eu, const float *ei,
                                     int32_t dim, const float *gb, int32_t n_chunks,
                                     const uint8_t *qb, int32_t qstride,
                                     const int64_t *ex_rowptr, const int32_t *ex_col,
                                     int64_t *ex_cur, int32_t k, int32_t first,
                                     double *io_val, int64_t *io_idx, int64_t n_positions,
                                     int64_t n_ex_positions, lg_stream_t stream);

/* The tile walk with a counting finish: where the rows' targets (tgt_rowptr int64 [n_users + 1]
 * / tgt_col int32: any order, duplicates allowed, any ids) stand among ALL columns of the F the
 * walk sums, lg_rows_rank_f64's definitions, without ever holding a row. val and cnt are aligned
 * with tgt_col. Two phases, each a launch per tile with lg_spread_tile_resource_topk_f64's tile,
 * user-side and G arguments:
 *   LG_SPREAD_RANK_VALUES  every target inside [item_begin, item_begin + width) gets
 *       val[p] = v, the value lg_spread_tile_resource_topk_f64 would insert for that column,
 *       bit for bit (F, or the fp32 chain score promoted to fp64 times F). gb / qb and the
 *       exclusion arguments are not read (may be NULL). Only the tiles that hold a target need a
 *       launch, and only the rows with a target there; entries of val whose target lies in no
 *       tile keep the caller's value (-inf: does not rank).
 *   LG_SPREAD_RANK_COUNTS  over ALL tiles in ascending order, after the values: cnt[p] += the
 *       number of columns j of the tile, not dropped by the row's exclusions (ex_* and the
 *       cursor ex_cur as in lg_spread_tile_resource_topk_f64), whose (value, item) is before
 *       (val[p], tgt_col[p]) under (value desc, item asc). Targets whose val is NaN or -inf are
 *       skipped. With G only columns whose bound (gb, qb) reaches the row's worst ranking val
 *       get the exact score: a column below it is before no target. cnt starts at 0; after the
 *       last tile it is the rank of every target that ranks (the caller drops the targets its
 *       exclusions name). A row is owned by one wave per launch and the launches of a walk are
 *       serialized on the stream: plain adds, no workspace, independent of the grid.
 * Any number of targets per row: the counting runs LG_SPREAD_RANK_ROW_MAX targets per pass over
 * the row's tile in LDS. Never allocates; sizes and limits as lg_spread_tile_resource_topk_f64. */
#define LG_SPREAD_RANK_ROW_MAX 8
#define LG_SPREAD_RANK_VALUES 0
#define LG_SPREAD_RANK_COUNTS 1
int lg_spread_tile_resource_rank_f64(const int64_t *user_rowptr, const int32_t *user_items,
                                     const double *ra_edge, int64_t n_users,
                                     const void *lines, const void *ovf, int32_t null_row,
                                     const double *rbeta,
                                     const double *inv_cls, int32_t item_begin, int32_t tile,
                                     int32_t width, const float *eu, const float *ei,
                                     int32_t dim, const float *gb, int32_t n_chunks,
                                     const uint8_t *qb, int32_t qstride,
                                     const int64_t *ex_rowptr, const int32_t *ex_col,
                                     int64_t *ex_cur, const int64_t *tgt_rowptr,
                                     const int32_t *tgt_col, int32_t phase, double *val,
                                     int64_t *cnt, int64_t n_positions, int64_t n_ex_positions,
                                     lg_stream_t stream);

/* x_bf16[r] = bf16(x[r]) (round to nearest even), norm_up[r] = ||x[r]||_2 rounded up to
 * fp32: the operands of lg_score_chunk_bound (csrc/gbound.hip). err_up (optional, may be
 * NULL): err_up[r] = ||x[r] - x_bf16[r]||_2 rounded up, the rounding-error norms the
 * screened top-K's margin umarg is built from (lgcnhs.ops.screen_margins). */
int lg_bound_prep_f32(const float *x, int64_t n_rows, int32_t dim, void *x_bf16,
                      float *norm_up, float *err_up, lg_stream_t stream);

/* Widest item tile lg_score_chunk_bound accepts (64 chunks of 64 columns). */
#define LG_BOUND_MAX_WIDTH 4096

/* gb[u][c] (fp32, [n_users][ceil(width / 64)]) >= the fp32 score chain e0_u . e0_j of every
 * column j of chunk c = [item_begin + 64c, item_begin + 64c + 64) of the tile: the bf16 MFMA
 * product's chunk maximum plus a rigorous rounding margin (csrc/gbound.hip). u/i from
 * lg_bound_prep_f32 of the users' rows and of all items. dim in {32, 64, 128}. qb (optional,
 * [n_users][qstride] bytes, qstride >= width rounded up to 256): per column j,
 * q = ceil(255 (G_bf16 + margin) / gb) in [0, 255], so gb * q / 255 >= the chain score too
 * (csrc/gbound.hip). width <= LG_BOUND_MAX_WIDTH (LG_ERR_ARG otherwise). */
int lg_score_chunk_bound(const void *u_bf16, const float *u_norm, int64_t n_users,
                         const void *i_bf16, const float *i_norm, int32_t dim,
                         int32_t item_begin, int32_t width, float *gb, uint8_t *qb,
                         int32_t qstride, lg_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Recommendation-list metrics (reference metrics/accurate.py and
 * metrics/diversity.py). recs is a [n_rows][k] int64 list matrix (recommendDictToTensor,
 * utils/trans.py:82-92); entries < 0 are padding and match nothing.
 * ------------------------------------------------------------------------------------ */

/* hit[q * k + p] = 1 if recs[eval_rows[q]][p] is in test row q (pos_rowptr/pos_col: one
 * sorted row per evaluated user, in eval_rows order), else 0: the `item in items` labels of
 * calPrecisionAndRecall / calNDCG (metrics/accurate.py:24-31, :69-76). */
int lg_rec_hits(const int64_t *recs, int64_t n_rows, int32_t k, const int64_t *eval_rows,
                int64_t n_eval, const int64_t *pos_rowptr, const int32_t *pos_col,
                uint8_t *hit, lg_stream_t stream);

/* *total = sum over ordered pairs of rows u != v of |set(recs[u]) & set(recs[v])|, computed
 * exactly as sum_i c_i (c_i - 1) over the per-item list counts c_i (written to counts[n_items],
 * items >= n_items ignored): calHammingDistance (metrics/diversity.py:15-63) is
 * 1 - total / (k n_rows (n_rows - 1)). */
int lg_rec_pair_overlap(const int64_t *recs, int64_t n_rows, int32_t k, int64_t n_items,
                        int32_t *counts, uint64_t *total, lg_stream_t stream);

/* part[r * k + p] = sum over q > p with recs[r][q] != recs[r][p], both items of nonzero
 * item_degree, of co(a, b) / sqrt(deg_a * deg_b), co = |users(a) & users(b)| over the item
 * columns item_rowptr/item_users (sorted) of the binary interaction matrix:
 * calInternalSimilarity (metrics/diversity.py:66-115) is 2 * sum(part) / (n_rows k (k-1)). */
int lg_rec_intra_similarity_f64(const int64_t *recs, int64_t n_rows, int32_t k,
                                const int64_t *item_rowptr, const int32_t *item_users,
                                const int64_t *item_degree, int64_t n_items, double *part,
                                lg_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* LGCNHS_H */
