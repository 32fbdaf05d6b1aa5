/* hgnn — MI355X (gfx950) hetero message-passing hot path, C ABI.
 *
 * Drop-in boundary for the per-relation SAGE aggregation the reference reaches through PyG
 * (SAGEConv((-1,-1), h) at train_gnn.py:158-160, called at train_gnn.py:177-198,
 * inference.py:143-166, test_gnn.py:141-166).  The reference has no FFI of its own (it is
 * pure Python over torch_geometric), so each entry point below names the PyG/ATen
 * step it replaces; INTEGRATION.md shows the ctypes binding a maintainer adds.
 *
 * Conventions
 *   - every pointer is DEVICE memory owned by the caller (PyTorch's caching allocator in the
 *     shipped host code); the library allocates nothing persistent, scratch comes in `ws`;
 *   - all work is stream-ordered on `stream` (a hipStream_t passed as void*); no host syncs,
 *     no hipMalloc/hipFree inside, so every call can be captured into a hipGraph;
 *   - row-major fp32 feature tables ([rows, d] contiguous); int32 CSR; int64 COO inputs;
 *   - return 0 (HGNN_OK) or an HGNN_E_* code; hgnn_last_error_string() (thread-local) says why.
 */
#ifndef HGNN_H_
#define HGNN_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HGNN_OK 0
#define HGNN_E_ARG 1001         /* bad shape / null pointer / size out of range */
#define HGNN_E_HIP 1002         /* a HIP runtime error (launch failure) */
#define HGNN_E_WS 1003          /* workspace too small */
#define HGNN_E_UNSUPPORTED 1004 /* shape outside what the kernels implement */

#define HGNN_MEAN 1        /* multiply each row sum by 1/deg (deg 0 -> 0) */
#define HGNN_ACCUMULATE 2  /* out += result instead of out = result */

#define HGNN_MAX_SEG 6     /* input segments of one fused linear */

typedef void* hgnn_stream_t; /* hipStream_t */

int hgnn_version(void);
const char* hgnn_last_error_string(void);

/* ---- K5: COO -> CSR, stable (each row keeps the COO edge order) -------------------------------
 * Replaces PyG's implicit scatter over unsorted COO (train_gnn.py:28,55 keep edges chronological;
 * train_gnn.py:128-133 masks out-of-range ids, train_gnn.py:142 flips for rev_engages).
 * Groups edges by key (dst for the forward CSR, src for the backward CSC):
 *   rowptr[n_keys+1], col[e] = other[perm[e]], perm[e] = original edge id.
 * Edges whose key is outside [0,n_keys) or whose other is outside [0,n_other) are dropped (sorted
 * to the end, excluded from rowptr); their count is written to *d_invalid (device int32).
 * E < 2^31.  Workspace: hgnn_coo_to_csr_ws_bytes(E, n_keys). */
size_t hgnn_coo_to_csr_ws_bytes(int64_t E, int64_t n_keys);
int hgnn_coo_to_csr(const int64_t* key, const int64_t* other, int64_t E, int64_t n_keys,
                    int64_t n_other, int32_t* rowptr, int32_t* col, int32_t* perm,
                    int32_t* d_invalid, void* ws, size_t ws_bytes, hgnn_stream_t stream);

/* Stable sort of int32 keys in [0,n_keys) carrying one or two int32 payloads (b may be NULL):
 * rowptr[n_keys+1] over the sorted keys, payloads in key order.  Out-of-range keys are dropped
 * and counted in *d_invalid.  d_invalid == NULL declares the keys already validated (the fused
 * loss validates its negatives in hgnn_edge_score_fwd): no extra pass over the keys then, and an
 * out-of-range key is still never dereferenced, only misplaced.  `keys` is never written.
 * Used per step to group the sampled negatives by post. */
size_t hgnn_sort_pairs_ws_bytes(int64_t E, int64_t n_keys);
int hgnn_sort_pairs_i32(const int32_t* keys, const int32_t* a, const int32_t* b, int64_t E,
                        int64_t n_keys, int32_t* rowptr, int32_t* a_sorted, int32_t* b_sorted,
                        int32_t* d_invalid, void* ws, size_t ws_bytes, hgnn_stream_t stream);

/* As hgnn_sort_pairs_i32 for int64 keys (e.g. torch.randint negatives as drawn): out-of-range
 * keys always go to the dropped sentinel and are counted in *d_invalid (required). */
int hgnn_sort_pairs_i64(const int64_t* keys, const int32_t* a, const int32_t* b, int64_t E,
                        int64_t n_keys, int32_t* rowptr, int32_t* a_sorted, int32_t* b_sorted,
                        int32_t* d_invalid, void* ws, size_t ws_bytes, hgnn_stream_t stream);

/* Transpose of a CSR (rowptr[n_rows+1] / col[E], columns in [0, n_cols) — not re-validated)
 * into its CSC: t_rowptr[n_cols+1], t_col[E] = the row of each entry, t_perm[E] = its CSR
 * position, stable (rows ascending within a column); t_w (nullable) = 1/deg(row) per entry, the
 * weight of the mean's backward.  One call instead of COO -> sort for the backward of a relation
 * whose edges come grouped by destination (sampled blocks).  ws: hgnn_sort_pairs_ws_bytes(E, n_cols). */
int hgnn_csr_transpose(const int32_t* rowptr, const int32_t* col, int64_t n_rows, int64_t E,
                       int64_t n_cols, int32_t* t_rowptr, int32_t* t_col, int32_t* t_perm,
                       float* t_w, void* ws, size_t ws_bytes, hgnn_stream_t stream);

/* hgnn_csr_transpose for n_rel (<= 8) CSRs in one sort (the relations of one sampled block):
 * relation r's CSR rowptr[r][n_rows[r]+1] / col[r][E[r]] with columns in [0, n_cols[r]); outputs
 * per relation exactly as hgnn_csr_transpose's.  ws: hgnn_csr_transpose_multi_ws_bytes(sum of E,
 * sum of n_cols). */
size_t hgnn_csr_transpose_multi_ws_bytes(int64_t E_total, int64_t n_cols_total);
int hgnn_csr_transpose_multi(int32_t n_rel, const int32_t* const* rowptr,
                             const int32_t* const* col, const int64_t* n_rows, const int64_t* E,
                             const int64_t* n_cols, int32_t* const* t_rowptr,
                             int32_t* const* t_col, int32_t* const* t_perm, float* const* t_w,
                             void* ws, size_t ws_bytes, hgnn_stream_t stream);

/* The loss's negatives drawn and grouped in one call: exactly hgnn_uniform_i32(d_seed, E, n_keys,
 * neg_out) followed by hgnn_sort_pairs_i32(neg_out, a, NULL, E, n_keys, rowptr, a_sorted, NULL,
 * NULL, ...), with the draws computed inside the sort's first pass instead of being written and
 * read back (neg_out, E int32 in position order, may be NULL).  Replaces the reference's
 * torch.randint negatives (train_gnn.py:272) plus the grouping the fused dP gather needs.
 * Workspace: hgnn_sort_pairs_ws_bytes(E, n_keys). */
int hgnn_draw_sort_negatives(const uint64_t* d_seed, const int32_t* a, int64_t E, int64_t n_keys,
                             int32_t* neg_out, int32_t* rowptr, int32_t* a_sorted, void* ws,
                             size_t ws_bytes, hgnn_stream_t stream);

/* ---- degree-skew plan ----------------------------------------------------------------------
 * Rows with more than `chunk` edges are split into ceil(deg/chunk) chunks, each summed by its own
 * wave into a partial slot, then reduced in chunk order (deterministic).  Two phases so the host
 * can size the plan: count writes {n_heavy, n_chunks} to d_counts2 (device int32[2]). */
size_t hgnn_plan_ws_bytes(int64_t n_rows);
int hgnn_plan_count(const int32_t* rowptr, int64_t n_rows, int32_t chunk, int32_t* d_counts2,
                    void* ws, size_t ws_bytes, hgnn_stream_t stream);
int hgnn_plan_fill(const int32_t* rowptr, int64_t n_rows, int32_t chunk, int32_t* heavy_rows,
                   int32_t* heavy_first, void* ws, size_t ws_bytes, hgnn_stream_t stream);
/* inv_deg[i] = 1/(rowptr[i+1]-rowptr[i]) or 0 for an empty row. */
int hgnn_inv_degree(const int32_t* rowptr, int64_t n_rows, float* inv_deg, hgnn_stream_t stream);

/* ---- hot-row flags -------------------------------------------------------------------------
 * col_hot[k] = col[k] | 0x80000000 when source row col[k] is among the n_hot most referenced of
 * the n_src rows, else col[k]: same order and length as col, read by the gathers below in its
 * place.  A row's reference count is deg_rowptr[i+1] - deg_rowptr[i] (the rowptr of the opposite
 * grouping, n_src + 1 entries); equal counts go to the lower id, so the set is deterministic.
 * *d_hot_edges (device int64, zeroed by the call) receives the number of edges whose row is
 * flagged; the caller keeps hot_edges / n_edges (the hot rows' share) with col_hot.  The flag
 * takes bit 31, so n_src above 2^31 is refused (HGNN_E_ARG).  Static per graph: built once. */
size_t hgnn_hot_cols_ws_bytes(int64_t n_src);
int hgnn_hot_cols(const int32_t* deg_rowptr, int64_t n_src, const int32_t* col, int64_t n_edges,
                  int64_t n_hot, int32_t* col_hot, int64_t* d_hot_edges, void* ws,
                  size_t ws_bytes, hgnn_stream_t stream);
/* The rule by which a gather with a col_hot takes the two-policy loads (1) or its old path (0):
 * a hot row is read with the default cache policy, every other row with nt loads, which keep it
 * out of L2 and the Infinity Cache, so the caches hold the Zipf head instead of a tail of rows
 * referenced once or twice.  On when the gathered table has at least 256 MiB (it outgrows the
 * Infinity Cache), a col_hot is given and the hot rows' share of the edges is at least 0.5
 * (cfg4's K1 / K2 over the 1M-row post table gain 6.5 - 7 % with 32768 - 131072 hot rows, 48 -
 * 65 % of the edges; with 8192 rows, 35 %, nothing; with 4096, 29 %, they lose 5 %).
 * Environment: HGNN_HOT_ROWS=0 off, HGNN_HOT_ROWS=force on for any table that comes with a
 * col_hot (tests).  No GPU needed.  The loss's scoring pass has no such path: measured, it lost
 * at every number of hot rows. */
int32_t hgnn_hot_rows_policy(int64_t table_bytes, int32_t has_col_hot, float hot_share);
/* The nt rule of a gather launch, as its launcher applies it.  `score` != 0 (the dP score
 * gathers): the rows of a source table of n_x * d * elem_bytes >= 1 GiB are read with nt loads
 * (elem_bytes: 4 for fp32 and zero-packed rows, which count by their unpacked size, 2 for bf16)
 * and the output rows are then stored nt too.  `score` == 0 (K1 / K2, every job of
 * hgnn_gather_reduce_multi): no nt loads; the fp32 output rows are stored nt where
 * n_rows * d * 4 >= 1 GiB.  Sets *nt_load and *nt_store to 0 / 1.  No GPU needed. */
int32_t hgnn_gather_nt_policy(int64_t n_x, int32_t d, int32_t elem_bytes, int32_t score,
                              int64_t n_rows, int32_t* nt_load, int32_t* nt_store);

/* ---- K1/K2: segmented gather-reduce over a CSR ----------------------------------------------
 *   out[i,:] (+)= s_i * sum_{p in [rowptr[i],rowptr[i+1])} w_p * x[col[p],:]
 * with w_p = (edge_w ? edge_w[p] : 1) * (col_w ? col_w[col[p]] : 1), s_i = 1/deg_i under
 * HGNN_MEAN (0 for deg 0), else 1.  Heavy rows follow the plan (slab: n_chunks*d floats).
 * Any d >= 1 (float4 path when d % 4 == 0). */
int hgnn_gather_reduce(const float* x, int64_t n_x, int32_t d, const int32_t* rowptr,
                       const int32_t* col, int64_t n_rows, const float* edge_w,
                       const float* col_w, int32_t flags, const int32_t* heavy_rows,
                       const int32_t* heavy_first, int64_t n_heavy, int64_t n_chunks,
                       int32_t chunk, float* slab, float* out, hgnn_stream_t stream);
/* hgnn_gather_reduce with a col_hot of the same grouping (hgnn_hot_cols, nullable) and its hot
 * share: where hgnn_hot_rows_policy(n_x * d * 4, col_hot != NULL, hot_share) says so, a separate
 * instantiation of the kernel reads col_hot and loads cold rows nt; otherwise exactly
 * hgnn_gather_reduce.  The edge order is the same, so the sums are bitwise the same either way.
 * acc_limit > 0 (with HGNN_ACCUMULATE): only rows below it accumulate, as in
 * hgnn_gather_reduce_multi (here heavy rows included). */
int hgnn_gather_reduce_hot(const float* x, int64_t n_x, int32_t d, const int32_t* rowptr,
                           const int32_t* col, int64_t n_rows, const float* edge_w,
                           const float* col_w, int32_t flags, const int32_t* heavy_rows,
                           const int32_t* heavy_first, int64_t n_heavy, int64_t n_chunks,
                           int32_t chunk, float* slab, float* out, int64_t acc_limit,
                           const int32_t* col_hot, float hot_share, hgnn_stream_t stream);

/* K1 forward: aggr = mean_{(j->i)} x_src[j]  — PyG propagate(aggr='mean') inside SAGEConv:
 * x_src.index_select(0, src) + scatter(..., dst, reduce='mean'), train_gnn.py:177-198. */
/* n_jobs (<= 8) gathers of one row width in one launch, as hgnn_gather_reduce each (job j: x[j]
 * of n_x[j] rows, rowptr[j] / col[j] over n_rows[j] rows, edge_w[j] nullable, the shared flags)
 * into DISTINCT outputs out[j]; rows are never split (no heavy-row plan: short rows, e.g. sampled
 * blocks), d % 4 == 0 and d <= 512.  With HGNN_ACCUMULATE, acc_limit[j] > 0 (acc_limit nullable)
 * limits the accumulation to rows below it and writes the other rows fresh (a K2 into a gradient
 * whose prefix holds the root term: no zero-fill of the rest).  The per-relation K1s of a sampled
 * layer (and each round of its K2s) as one graph node.  Results exactly those of the single calls
 * (on a zeroed remainder). */
int hgnn_gather_reduce_multi(int32_t n_jobs, const float* const* x, const int64_t* n_x, int32_t d,
                             const int32_t* const* rowptr, const int32_t* const* col,
                             const int64_t* n_rows, const float* const* edge_w, int32_t flags,
                             const int64_t* acc_limit, float* const* out, hgnn_stream_t stream);

/* hgnn_gather_reduce with a per-row output scale: out[i,:] (+)= row_w[i] * sum_p w_p x[col[p],:]
 * (row_w replaces HGNN_MEAN's 1/segment length; not both).  With row_w = 1/deg of the whole
 * relation this is one pass of a mean split over source blocks: the passes over the blocks' CSRs
 * (HGNN_ACCUMULATE from the second on) sum to the relation's mean, each pass reading only its
 * block of the source table. */
int hgnn_gather_reduce_scaled(const float* x, int64_t n_x, int32_t d, const int32_t* rowptr,
                              const int32_t* col, int64_t n_rows, const float* edge_w,
                              const float* col_w, const float* row_w, int32_t flags,
                              const int32_t* heavy_rows, const int32_t* heavy_first,
                              int64_t n_heavy, int64_t n_chunks, int32_t chunk, float* slab,
                              float* out, hgnn_stream_t stream);
int hgnn_gather_mean_fwd(const float* x_src, int64_t n_src, int32_t d, const int32_t* rowptr,
                         const int32_t* col, int64_t n_dst, const int32_t* heavy_rows,
                         const int32_t* heavy_first, int64_t n_heavy, int64_t n_chunks,
                         int32_t chunk, float* slab, float* aggr, hgnn_stream_t stream);

/* K2 backward: grad_x_src[j] (+)= sum_{(j->i)} grad_aggr[i] * inv_deg[i], walking the transposed
 * CSR (grouped by source; t_col holds destinations) — autograd of the mean scatter. */
int hgnn_scatter_mean_bwd(const float* grad_aggr, int64_t n_dst, const float* inv_deg,
                          const int32_t* t_rowptr, const int32_t* t_col, int64_t n_src,
                          int32_t d, const int32_t* heavy_rows, const int32_t* heavy_first,
                          int64_t n_heavy, int64_t n_chunks, int32_t chunk, float* slab,
                          float* grad_x_src, int32_t accumulate, hgnn_stream_t stream);

/* ---- K3/K4: fused multi-segment linear (fp32 MFMA) -------------------------------------------
 * Replaces SAGEConv's lin_l/lin_r addmm plus WeightedRGCN's weighted sum + ReLU
 * (train_gnn.py:187-198):
 *   out[n, h] = act( sum_s xs[s][n, ks[s]] @ w[:, off_s:off_s+ks[s]]^T + bias )
 * w is [h, sum(ks)] row-major (torch Linear layout), act = ReLU when relu != 0.
 * `out` should not alias an input segment: at h = 128 and sum(ks) = 384 / 512 the split kernels
 * run as two column blocks that pass partial rows through `out`, and a call whose `out` overlaps
 * an xs[s] (or `add`) range is routed to the general f32-input kernels instead. */
int hgnn_linear_fwd(int32_t n_seg, const float* const* xs, const int32_t* ks, int64_t n_rows,
                    const float* w, int32_t h, const float* bias, int32_t relu, float* out,
                    hgnn_stream_t stream);

/* hgnn_linear_fwd with an additive input: out = act( sum_s xs[s] @ w_s^T + bias + add ), add is
 * [n_rows, h] (nullable).  The destination update of a relation whose lin_l was applied to the
 * SOURCE table before the mean gather (mean is linear: lin_l(mean x_j) = mean(lin_l x_j) - 
 * ops.py "pre-projected relations"): add = the gathered projected rows. */
int hgnn_linear_fwd_add(int32_t n_seg, const float* const* xs, const int32_t* ks, int64_t n_rows,
                        const float* w, int32_t h, const float* bias, const float* add,
                        int32_t relu, float* out, hgnn_stream_t stream);

/* The relation-weighted fused weight of one destination update (WeightedRGCN's
 * relu(w_direct * conv_a + w_social * conv_b), train_gnn.py:187-198, folded into one K3):
 *   w_out = [s_1 wl_1 | ... | s_R wl_R | sum_r s_r wr_r]   ([h, sum_r k_r + k_root], row-major)
 *   b_out = sum_r s_r bl_r                                 (nullable; needs some bl_r)
 * wl[r]: [h, k_r]; wr[r]: [h, k_root] or NULL (no lin_r; k_root = 0 when every wr is NULL);
 * bl[r]: [h] or NULL.  n_rel <= HGNN_MAX_SEG - 1.  Bitwise the torch expression (products and sums
 * rounded separately, in relation order).  Replaces the per-step cat/mul/add chain. */
int hgnn_fuse_weights(int32_t n_rel, const float* const* wl, const int32_t* k,
                      const float* const* wr, int32_t k_root, const float* const* bl,
                      const float* scale, int32_t h, float* w_out, float* b_out,
                      hgnn_stream_t stream);
/* Its adjoint: dwl[r] = s_r dw[:, block r], dwr[r] = s_r dw[:, root block], dbl[r] = s_r db
 * (every output array and entry nullable). */
int hgnn_split_weight_grads(int32_t n_rel, const float* dw, const float* db, const int32_t* k,
                            int32_t k_root, const float* scale, int32_t h, float* const* dwl,
                            float* const* dwr, float* const* dbl, hgnn_stream_t stream);

/* Both for n_groups (<= 4) destination updates of one layer in one launch: group g's relations
 * are the flattened entries [base_g, base_g + n_rel[g]) of wl / k / wr / bl / scale (and of
 * dwl / dwr / dbl), base_g = n_rel[0] + ... + n_rel[g - 1]; w_out[g] / b_out[g] (b_out or its
 * entries nullable) and dw[g] / db[g] per group, h shared.  Results exactly those of the
 * single-update calls. */
int hgnn_fuse_weights_multi(int32_t n_groups, const int32_t* n_rel, const float* const* wl,
                            const int32_t* k, const float* const* wr, const int32_t* k_root,
                            const float* const* bl, const float* scale, int32_t h,
                            float* const* w_out, float* const* b_out, hgnn_stream_t stream);
int hgnn_split_weight_grads_multi(int32_t n_groups, const int32_t* n_rel, const float* const* dw,
                                  const float* const* db, const int32_t* k, const int32_t* k_root,
                                  const float* scale, int32_t h, float* const* dwl,
                                  float* const* dwr, float* const* dbl, hgnn_stream_t stream);

/* hgnn_linear_fwd_add that also writes the ReLU mask of `out` as bits (relu != 0, h % 32 == 0):
 * bit c % 32 of mask[row * (h / 32) + c / 32] = out[row][c] > 0, 16-B aligned.  The backward
 * (hgnn_linear_bwd_mask) reads h/8 bytes per row instead of out's 4h: autograd's saved ReLU
 * output is only ever used for that mask (train_gnn.py:198's activation). */
int hgnn_linear_fwd_mask(int32_t n_seg, const float* const* xs, const int32_t* ks,
                         int64_t n_rows, const float* w, int32_t h, const float* bias,
                         const float* add, int32_t relu, float* out, uint32_t* mask,
                         hgnn_stream_t stream);

/* Backward of hgnn_linear_fwd.  dz = dout * (out > 0) when out != NULL (ReLU), else dout.
 *   dxs[s] = dz @ w[:, seg s]           (skipped for NULL entries)
 *   dw     = dz^T @ [xs...]             (NULL: skipped; same for db = colsum(dz))
 * Deterministic (per-block partials reduced in block order).  Workspace:
 * hgnn_linear_bwd_ws_bytes(n_rows, sum(ks), h). */
size_t hgnn_linear_bwd_ws_bytes(int64_t n_rows, int32_t k_total, int32_t h);
/* hgnn_linear_bwd that also writes the masked dz ([n_rows, h], dz_out) — the gradient a
 * pre-projected relation's K2 scatters (ops.py) — from the pass that masks it anyway. */
int hgnn_linear_bwd_dz(int32_t n_seg, const float* const* xs, const int32_t* ks, int64_t n_rows,
                       const float* w, int32_t h, const float* dout, const float* out,
                       float* const* dxs, float* dw, float* db, float* dz_out, void* ws,
                       size_t ws_bytes, hgnn_stream_t stream);
/* hgnn_linear_bwd_dz with the ReLU mask also given as the bits of hgnn_linear_fwd_mask: the
 * persistent backward kernels read the bits, the others `out` (both required). */
int hgnn_linear_bwd_mask(int32_t n_seg, const float* const* xs, const int32_t* ks,
                         int64_t n_rows, const float* w, int32_t h, const float* dout,
                         const float* out, const uint32_t* mask, float* const* dxs, float* dw,
                         float* db, float* dz_out, void* ws, size_t ws_bytes,
                         hgnn_stream_t stream);
/* hgnn_linear_bwd_mask where bit s of dx_accumulate adds segment s's input gradient into what
 * dxs[s] already holds instead of storing it: a node table whose gradient has several producers
 * (layer 1's post output at layer 2: the post update's root term and the pre-projected
 * relation's projection) gets the second one in the same pass, not through a separate add —
 * autograd's gradient accumulation of train_gnn.py:283's backward. */
int hgnn_linear_bwd_ex(int32_t n_seg, const float* const* xs, const int32_t* ks,
                       int64_t n_rows, const float* w, int32_t h, const float* dout,
                       const float* out, const uint32_t* mask, float* const* dxs,
                       uint32_t dx_accumulate, float* dw, float* db, float* dz_out, void* ws,
                       size_t ws_bytes, hgnn_stream_t stream);
/* Several K3 calls at once — job j is hgnn_linear_fwd_mask(n_seg[j], the next n_seg[j] entries
 * of xs / ks, n_rows[j], w[j], h, bias[j], NULL, relu[j], out[j], mask[j]) — in one launch per
 * column block where two jobs both take the K = 384 / 512 split path with the same K (a sampled
 * layer's two destination types: ops._HeteroLayer), job by job otherwise.  bias / relu / mask
 * may be NULL (none for every job).  A pair only runs side by side when neither job writes what
 * the other reads (byte ranges checked; else job by job).  Replaces the per-destination-type
 * lin_l / lin_r calls of HeteroConv (reference train_gnn.py:147-200), like hgnn_linear_fwd. */
int hgnn_linear_fwd_multi(int32_t n_jobs, const int32_t* n_seg, const float* const* xs,
                          const int32_t* ks, const int64_t* n_rows, const float* const* w,
                          int32_t h, const float* const* bias, const int32_t* relu,
                          float* const* out, uint32_t* const* mask, hgnn_stream_t stream);
/* Backward of hgnn_linear_fwd_multi: job j is hgnn_linear_bwd_ex(n_seg[j], xs / ks / dxs from
 * the job's entries, n_rows[j], w[j], h, dout[j], out[j], mask[j], dx_accumulate[j], dw[j], db[j],
 * NULL, its workspace).  ws: hgnn_linear_bwd_multi_ws_bytes (the jobs' hgnn_linear_bwd_ws_bytes
 * one after the other).  out / mask / dx_accumulate / dw / db may be NULL (none for every job). */
size_t hgnn_linear_bwd_multi_ws_bytes(int32_t n_jobs, const int64_t* n_rows,
                                      const int32_t* k_total, int32_t h);
int hgnn_linear_bwd_multi(int32_t n_jobs, const int32_t* n_seg, const float* const* xs,
                          const int32_t* ks, const int64_t* n_rows, const float* const* w,
                          int32_t h, const float* const* dout, const float* const* out,
                          const uint32_t* const* mask, float* const* dxs,
                          const uint32_t* dx_accumulate, float* const* dw, float* const* db,
                          void* ws, size_t ws_bytes, hgnn_stream_t stream);
/* Adam (torch.optim.Adam, the reference's optimizer: train_gnn.py:207) over n_tensors fp32
 * parameters in one launch (per 32 tensors): p, m, v updated in place from g.  step: one device
 * float, the steps done so far — the launch uses step + 1 and writes it back once every block has
 * read it (capturable: no host value); done: one device uint32, zero between launches (the
 * launch leaves it zero).  One update per (step, done) pair in flight. */
int hgnn_adam_multi(int32_t n_tensors, float* const* params, const float* const* grads,
                    float* const* exp_avg, float* const* exp_avg_sq, const int64_t* numel,
                    float* step, uint32_t* done, double lr, double beta1, double beta2, double eps,
                    double weight_decay, hgnn_stream_t stream);
/* A 64-bit checksum of the bit patterns of n_elems fp32 words (one streaming pass):
 *   *d_out = sum_i bits(x[i]) * (0x9E3779B97F4A7C15 + 2 i)  (mod 2^64)
 * Integer sums only, so the value does not depend on the order of the blocks; any single flipped
 * bit and any exchange of two unequal words change it.  d_out: one device uint64 (8-byte aligned;
 * zeroed by the call on the same stream).  A caller that keeps a result computed from a static
 * table (e.g. hgnn_gather_mean_fwd of the model's inputs, run once) can keep this value beside it
 * and compare it later to detect a table rewritten in place. */
int hgnn_table_fingerprint(const float* x, int64_t n_elems, uint64_t* d_out,
                           hgnn_stream_t stream);
int hgnn_linear_bwd(int32_t n_seg, const float* const* xs, const int32_t* ks, int64_t n_rows,
                    const float* w, int32_t h, const float* dout, const float* out,
                    float* const* dxs, float* dw, float* db, void* ws, size_t ws_bytes,
                    hgnn_stream_t stream);

/* dP of the fused loss with each edge's weight recomputed from its score (no weight arrays):
 *   out[r,:] (+)= sum_{p in row r} w(<x[col[p]],:>, rowvec[r,:]>) * x[col[p],:]
 *   mode 1 (positive edges): w(s) = c*inv_e*(sigmoid(s) - 1), c = *cscale
 *   mode 2 (negative edges): w(s) = inv_e*sigmoid(s)
 * i.e. dL/dP[r] of hgnn_edge_score_fwd's loss (train_gnn.py:276-281) for x = U, rowvec = P.
 * Heavy rows / slab as hgnn_gather_reduce. */
int hgnn_score_gather(const float* x, int64_t n_x, const float* rowvec, int32_t d,
                      const int32_t* rowptr, const int32_t* col, int64_t n_rows, int32_t mode,
                      const float* cscale, float inv_e, const int32_t* heavy_rows,
                      const int32_t* heavy_first, int64_t n_heavy, int64_t n_chunks,
                      int32_t chunk, float* slab, float* out, int32_t accumulate,
                      hgnn_stream_t stream);

/* Both dP gathers of the fused loss in one pass (replaces a mode-1 hgnn_score_gather over the
 * positives followed by an accumulating mode-2 one over the negatives):
 *   out[r,:] = sum_{p in rowptr/col row r} w_1(s) x[col[p],:]  +  sum_{p in rowptr_n/col_n row r}
 *              w_2(s) x[col_n[p],:]
 * with w_1, w_2 as hgnn_score_gather's modes 1 and 2.  The heavy-row plan applies to the positive
 * list only (the uniform negatives have no heavy rows); every row is written (no accumulate). */
int hgnn_score_gather2(const float* x, int64_t n_x, const float* rowvec, int32_t d,
                       const int32_t* rowptr, const int32_t* col, const int32_t* rowptr_n,
                       const int32_t* col_n, int64_t n_rows, const float* cscale, float inv_e,
                       const int32_t* heavy_rows, const int32_t* heavy_first, int64_t n_heavy,
                       int64_t n_chunks, int32_t chunk, float* slab, float* out,
                       hgnn_stream_t stream);

/* ---- edge scoring + weighted BCE (train_gnn.py:259-281), fused with its gradient --------------
 * Positive edges grouped by user (rowptr_u/col_u = post ids); neg_u_order[k] = the negative post
 * drawn for position k; to_post_pos[k] = that edge's position in the post-grouped CSR.
 *   loss = c * mean softplus(-<U[u],P[p]>) + mean softplus(<U[u],P[n]>),  c = *cscale
 *          (= mean(pos_weights): BCEWithLogitsLoss() reduces to a scalar first)
 * Writes dU (dL/dU for a unit upstream gradient, row-owned, no atomics).  Optional (may be NULL):
 * per position (neg_key, neg_user) — the validated negative and its user, for sorting by post;
 * hpos[post-grouped
 * pos] (weight of U[u] in dP[p], needs to_post_pos) and neg_w (weight in dP[n]) — not needed when
 * dP is formed by hgnn_score_gather, which recomputes both;
 * part needs hgnn_edge_score_parts(n_users) floats (16-B aligned); *err counts out-of-range negatives
 * (err nullable: not counted — a caller whose negatives are valid by construction). */
int64_t hgnn_edge_score_parts(int64_t n_users);
/* The two size rules of the scoring pass, as its launcher applies them (no GPU needed).
 * hgnn_score_nt_policy: 1 where the post table, n_posts * d elements of 2 (bf16 != 0) or 4 bytes,
 * has at least 256 MiB: the negatives' rows are then read with nt loads and the dU rows stored nt
 * (the NT instantiations of every hgnn_edge_score_fwd* entry).  hgnn_loss_one_pass: 1 where the
 * block partials (one per 4 users) are summed by one block, at most 65536 of them, i.e. up to
 * 262144 users; 0 where two reduction kernels run. */
int32_t hgnn_score_nt_policy(int64_t n_posts, int32_t d, int32_t bf16);
int32_t hgnn_loss_one_pass(int64_t n_users);
int hgnn_edge_score_fwd(const float* U, const float* P, int32_t d, int64_t n_users,
                        int64_t n_posts, const int32_t* rowptr_u, const int32_t* col_u,
                        const int64_t* neg_u_order, const int32_t* to_post_pos, int64_t n_edges,
                        const float* cscale, float* dU, float* hpos, int32_t* neg_key,
                        int32_t* neg_user, float* neg_w, float* part, float* loss, int32_t* err,
                        hgnn_stream_t stream);

/* K3 at H = 128 and K = 128 / 256 runs on bf16 MFMA as an fp32-exact three-piece split (each
 * fp32 operand = three bf16 pieces, six piece products per fp32 product, f32 accumulation:
 * fp32-class error; each operand element split once per block), and K = 384 / 512
 * (every segment a multiple of 16 columns) as two column blocks on the same kernels, unless
 * HGNN_K3_X6=0.  on = 1 / 0 selects the split or the f32-input MFMA kernels for the calls that
 * follow (process-wide, not thread-safe against calls in flight); on < 0 only queries.  Returns
 * the previous setting. */
int hgnn_set_k3_split(int32_t on);

/* Single-input forms, one PyG Linear at a time (SURVEY §8b names; same kernels as above):
 *   hgnn_linear_fwd_f32:   out[n,h] = x[n,k] @ w[h,k]^T (+ bias[h] when non-NULL)
 *   hgnn_linear_dgrad_f32: dx[n,k]  = dy[n,h] @ w
 *   hgnn_linear_wgrad_f32: dw[h,k]  = dy^T @ x, db[h] = colsum(dy) (db may be NULL);
 *                          ws: hgnn_linear_bwd_ws_bytes(n, k, h) */
int hgnn_linear_fwd_f32(const float* x, int64_t n_rows, int32_t k, const float* w, int32_t h,
                        const float* bias, float* out, hgnn_stream_t stream);
int hgnn_linear_dgrad_f32(const float* dy, int64_t n_rows, int32_t h, const float* w, int32_t k,
                          float* dx, hgnn_stream_t stream);
int hgnn_linear_wgrad_f32(const float* x, const float* dy, int64_t n_rows, int32_t k, int32_t h,
                          float* dw, float* db, void* ws, size_t ws_bytes, hgnn_stream_t stream);

/* ---- K4 standalone: WeightedRGCN's weighted relation sum + ReLU (train_gnn.py:187-198) -------
 *   out[e] = act( sum_r weights[r] * ins[r][e] ),  e < n elements, n_in <= HGNN_MAX_SEG
 * (weights: HOST array; ins: HOST array of device pointers).  The model path folds this into K3;
 * these are for callers that combine per-relation SAGEConv outputs themselves.
 * Backward: dins[r][e] = weights[r] * dout[e] * (relu ? out[e] > 0 : 1)  (NULL dins[r] skipped). */
int hgnn_hetero_epilogue(int32_t n_in, const float* const* ins, const float* weights, int64_t n,
                         int32_t relu, float* out, hgnn_stream_t stream);
int hgnn_hetero_epilogue_bwd(int32_t n_in, const float* weights, int64_t n, int32_t relu,
                             const float* out, const float* dout, float* const* dins,
                             hgnn_stream_t stream);

/* hgnn_edge_score_fwd with int32 negatives (as hgnn_uniform_i32 draws them) and without the
 * optional per-position outputs (the dP side is formed by hgnn_score_gather). */
int hgnn_edge_score_fwd_i32(const float* U, const float* P, int32_t d, int64_t n_users,
                            int64_t n_posts, const int32_t* rowptr_u, const int32_t* col_u,
                            const int32_t* neg_u_order, int64_t n_edges, const float* cscale,
                            float* dU, float* part, float* loss, int32_t* err,
                            hgnn_stream_t stream);
/* hgnn_edge_score_fwd_i32 with the negatives drawn in the kernel: the negative of position k is
 * the draw hgnn_uniform_i32(d_seed, n_edges, n_posts) would write at k (train_gnn.py:272's
 * torch.randint, one per positive edge), so no position-order array is written or read (the
 * fused loss passes neg_out = NULL to hgnn_draw_sort_negatives and this the same seed). */
int hgnn_edge_score_fwd_draw(const float* U, const float* P, int32_t d, int64_t n_users,
                             int64_t n_posts, const int32_t* rowptr_u, const int32_t* col_u,
                             const uint64_t* d_seed, int64_t n_edges, const float* cscale,
                             float* dU, float* part, float* loss, int32_t* err,
                             hgnn_stream_t stream);
/* n uniform int32 draws in [0, hi) (the negatives of train_gnn.py:272), counter-based from the
 * 64-bit seed at d_seed (device memory: a torch Generator draws it without a host sync). */
int hgnn_uniform_i32(const uint64_t* d_seed, int64_t n, int32_t hi, int32_t* out,
                     hgnn_stream_t stream);
/* x[0:n] *= *d_scale in place, a no-op when *d_scale == 1 (read on the device).  The fused
 * loss's autograd backward: its dU/dP are formed in the forward and scaled by the incoming
 * gradient (1 for loss.backward()).  x 16-byte aligned. */
int hgnn_scale_unless_one(float* x, int64_t n, const float* d_scale, hgnn_stream_t stream);

/* ---- bf16 row storage (opt-in: HGNN_ROW_DTYPE=bf16 in the Python layer) ------------------------
 * The forward gathers and the link loss read one row per edge from a table that is a layer
 * output.  In this mode they read a bf16 copy of it (half the bytes) and widen each element to
 * fp32 where it is summed; accumulators, outputs, gradients and everything else stay fp32.  A
 * result equals what the fp32 entry point gives on the table R(T) = float(bf16(T)), up to fp32
 * summation order (the lane mapping differs).  bf16 tables cross the boundary as uint16_t,
 * 16-byte aligned, row-major [n, d] with d % 8 == 0.  No atomics; bitwise reproducible. */

/* out[i] = bf16(x[i]), round to nearest even (bitwise torch's float -> bfloat16 for every
 * non-NaN value; NaN -> 0x7fc0).  A streaming pass with 16-B accesses and a tail for
 * n_elems % 8; n_elems = 0 is fine.  x and out 16-byte aligned. */
int hgnn_rows_to_bf16(const float* x, int64_t n_elems, uint16_t* out, hgnn_stream_t stream);

/* ReLU's backward fused into the cast (opt-in bf16 gradient rows, HGNN_GRAD_ROW_DTYPE=bf16 in the
 * Python layer): dz[r][c] = bf16(out[r][c] > 0 ? dout[r][c] : +0), rounded as hgnn_rows_to_bf16
 * does — bitwise that cast of the dz_out hgnn_linear_bwd_dz writes, in 6 bytes per element
 * (+ 16 B of mask per row) instead of 10.  Exactly one of out_act (the forward's [n_rows, h]
 * output) and mask (the bits hgnn_linear_fwd_mask wrote: 4 words per row at every h, column j at
 * bit 4 (j / 16) + j % 4 of word (j / 4) % 4) is the predicate; both or neither: HGNN_E_ARG.
 * h % 8 == 0; with mask also h % 16 == 0 and h <= 128 (else HGNN_E_UNSUPPORTED, the message
 * names h).  Every pointer 16-byte aligned; n_rows = 0 is fine with null pointers. */
int hgnn_relu_grad_to_bf16(const float* dout, const float* out_act, const uint32_t* mask,
                           int64_t n_rows, int32_t h, uint16_t* dz, hgnn_stream_t stream);

/* hgnn_gather_reduce_hot and hgnn_gather_reduce_scaled in one, over a bf16 source table x:
 * edge_w / col_w / row_w (row_w replaces HGNN_MEAN, not both), HGNN_MEAN / HGNN_ACCUMULATE,
 * acc_limit, the heavy-row plan with its fp32 slab, col_hot / hot_share (all nullable as there).
 * out is fp32.  The cache policies take the table's real size, n_x * d * 2 bytes.  d % 8 == 0
 * and d <= 1024, else HGNN_E_UNSUPPORTED (the message names d). */
int hgnn_gather_reduce_bf16(const uint16_t* x, int64_t n_x, int32_t d, const int32_t* rowptr,
                            const int32_t* col, int64_t n_rows, const float* edge_w,
                            const float* col_w, const float* row_w, int32_t flags,
                            const int32_t* heavy_rows, const int32_t* heavy_first,
                            int64_t n_heavy, int64_t n_chunks, int32_t chunk, float* slab,
                            float* out, int64_t acc_limit, const int32_t* col_hot,
                            float hot_share, hgnn_stream_t stream);

/* hgnn_score_gather2 with x (U) and rowvec (P) both bf16; fp32 out.  Same d rule. */
int hgnn_score_gather2_bf16(const uint16_t* x, int64_t n_x, const uint16_t* rowvec, int32_t d,
                            const int32_t* rowptr, const int32_t* col, const int32_t* rowptr_n,
                            const int32_t* col_n, int64_t n_rows, const float* cscale,
                            float inv_e, const int32_t* heavy_rows, const int32_t* heavy_first,
                            int64_t n_heavy, int64_t n_chunks, int32_t chunk, float* slab,
                            float* out, hgnn_stream_t stream);

/* The scoring pass (hgnn_edge_score_fwd) with bf16 U and P: the score <U[u], P[p]> is the same
 * number here and in hgnn_score_gather2_bf16.  The negatives come in exactly one of the three
 * forms of the fp32 entries: neg_i64 (hgnn_edge_score_fwd), neg_i32 (.._i32) or d_seed (.._draw:
 * the draws hgnn_uniform_i32 makes); the other two NULL.  fp32 dU, part, loss and err as there;
 * the optional per-position outputs (hpos, neg_key, neg_w) are not produced.  d % 8 == 0 and
 * d <= 512, else HGNN_E_UNSUPPORTED. */
int hgnn_edge_score_fwd_bf16(const uint16_t* U, const uint16_t* P, int32_t d, int64_t n_users,
                             int64_t n_posts, const int32_t* rowptr_u, const int32_t* col_u,
                             const int64_t* neg_i64, const int32_t* neg_i32,
                             const uint64_t* d_seed, int64_t n_edges, const float* cscale,
                             float* dU, float* part, float* loss, int32_t* err,
                             hgnn_stream_t stream);

/* ---- zero-packed fp32 rows (HGNN_ZPACK=auto|0|1 in the Python layer; csrc/zpack.h) ------------
 * A table whose rows are mostly zero bit patterns (a ReLU output), stored as mask + non-zero
 * values for a gather that reads one row per edge.  d = 64 or 128 only.  Row r sits in a slot of
 * hgnn_zpack_slot_bytes(d) bytes (d = 128: 640, d = 64: 384; 0 for any other d) at byte r * slot:
 * bytes [0, 16) the mask (bit c set iff the bit pattern of x[r][c] is non-zero, so -0.0,
 * denormals and NaN are stored and the format is lossless), bytes [16, 16 + 4 nnz) the stored
 * values in column order; the rest of the slot is never written. */
int64_t hgnn_zpack_slot_bytes(int32_t d);

/* Whether a table of table_bytes (unpacked) and width d should be read packed: HGNN_ZPACK=0
 * never, =1 whenever d is 64 or 128, auto (the default): d is 64 or 128, the table is at least
 * 1 GiB and relu_out says it is a fused-ReLU output. */
int32_t hgnn_zpack_policy(int64_t table_bytes, int32_t d, int32_t relu_out);

/* The streaming pack pass: x [n_rows, d] fp32 (16-byte aligned) -> out, n_rows *
 * hgnn_zpack_slot_bytes(d) bytes, 128-byte aligned.  hist, if not NULL, is a device array of 6
 * counters the pass ADDS into: hist[l] counts the rows whose mask + values take l 128-B lines
 * (1 .. 5).  Other d: HGNN_E_UNSUPPORTED. */
int hgnn_zpack_rows(const float* x, int64_t n_rows, int32_t d, void* out, int64_t* hist,
                    hgnn_stream_t stream);

/* hgnn_score_gather2 with the source table x given zero-packed (xz from hgnn_zpack_rows, n_x
 * slots).  rowvec (P) stays unpacked.  Same lanes, same order of every sum: out is bitwise what
 * hgnn_score_gather2 writes for the unpacked table.  The cache policy goes by the unpacked size
 * n_x * d * 4, as there.  d = 64 or 128, else HGNN_E_UNSUPPORTED. */
int hgnn_score_gather2_zp(const void* xz, int64_t n_x, const float* rowvec, int32_t d,
                          const int32_t* rowptr, const int32_t* col, const int32_t* rowptr_n,
                          const int32_t* col_n, int64_t n_rows, const float* cscale, float inv_e,
                          const int32_t* heavy_rows, const int32_t* heavy_first, int64_t n_heavy,
                          int64_t n_chunks, int32_t chunk, float* slab, float* out,
                          hgnn_stream_t stream);

/* ---- per-edge positive weights in the fused loss (opt-in: weighting="edge" in the Python layer) --
 *   loss = mean_e( w_e * softplus(-<U[u_e],P[p_e]>) ) + mean_e softplus(<U[u_e],P[n_e]>)
 * i.e. (pos_weights * BCEWithLogits(pos_scores, 1, reduction='none')).mean() + neg_loss: every
 * positive edge's loss term and gradient carry that edge's own weight, where the entries above
 * carry the one scalar c the reference's arithmetic collapses them to.  The gradient weight of
 * positive edge e in dU and dP is c * w_e / E * (sigmoid(s_e) - 1) with c = *cscale, which stays a
 * global factor (1 for the plain per-edge loss); the negatives are unchanged.  edge_w is an fp32
 * device array over the positions of the grouping it sits beside (it follows that col array).
 * Same lanes, same order of every sum, no atomics: with every weight one power of two, a result is
 * bitwise the unweighted entry's with cscale scaled by it.  A null edge_w with rows to process is
 * HGNN_E_ARG, before any launch. */

/* The scoring pass with per-edge weights: edge_w[k] belongs to position k of rowptr_u / col_u (the
 * user-grouped order).  The negatives in exactly one of the three forms (the other two NULL), dU,
 * part, loss and err as hgnn_edge_score_fwd_bf16 has them; the optional per-position outputs are
 * not produced.  fp32 rows: the widths of hgnn_edge_score_fwd (d <= 512). */
int hgnn_edge_score_fwd_w(const float* U, const float* P, int32_t d, int64_t n_users,
                          int64_t n_posts, const int32_t* rowptr_u, const int32_t* col_u,
                          const float* edge_w, const int64_t* neg_i64, const int32_t* neg_i32,
                          const uint64_t* d_seed, int64_t n_edges, const float* cscale, float* dU,
                          float* part, float* loss, int32_t* err, hgnn_stream_t stream);
/* ... with bf16 U and P (hgnn_edge_score_fwd_bf16's rule: d % 8 == 0 and d <= 512, else
 * HGNN_E_UNSUPPORTED). */
int hgnn_edge_score_fwd_w_bf16(const uint16_t* U, const uint16_t* P, int32_t d, int64_t n_users,
                               int64_t n_posts, const int32_t* rowptr_u, const int32_t* col_u,
                               const float* edge_w, const int64_t* neg_i64,
                               const int32_t* neg_i32, const uint64_t* d_seed, int64_t n_edges,
                               const float* cscale, float* dU, float* part, float* loss,
                               int32_t* err, hgnn_stream_t stream);

/* hgnn_score_gather2 with per-edge weights on the first list: edge_w[p] belongs to position p of
 * rowptr / col (the post-grouped order; a heavy row's chunks read it at their absolute positions),
 *   w_1(s) = c * inv_e * edge_w[p] * (sigmoid(s) - 1);
 * the second list (the negatives, w_2) carries none and does not read edge_w.  The _zp and _bf16
 * forms are hgnn_score_gather2_zp's and hgnn_score_gather2_bf16's, with their d rules; the _zp
 * result is bitwise hgnn_score_gather2_w's on the unpacked table. */
int hgnn_score_gather2_w(const float* x, int64_t n_x, const float* rowvec, int32_t d,
                         const int32_t* rowptr, const int32_t* col, const float* edge_w,
                         const int32_t* rowptr_n, const int32_t* col_n, int64_t n_rows,
                         const float* cscale, float inv_e, const int32_t* heavy_rows,
                         const int32_t* heavy_first, int64_t n_heavy, int64_t n_chunks,
                         int32_t chunk, float* slab, float* out, hgnn_stream_t stream);
int hgnn_score_gather2_w_zp(const void* xz, int64_t n_x, const float* rowvec, int32_t d,
                            const int32_t* rowptr, const int32_t* col, const float* edge_w,
                            const int32_t* rowptr_n, const int32_t* col_n, int64_t n_rows,
                            const float* cscale, float inv_e, const int32_t* heavy_rows,
                            const int32_t* heavy_first, int64_t n_heavy, int64_t n_chunks,
                            int32_t chunk, float* slab, float* out, hgnn_stream_t stream);
int hgnn_score_gather2_w_bf16(const uint16_t* x, int64_t n_x, const uint16_t* rowvec, int32_t d,
                              const int32_t* rowptr, const int32_t* col, const float* edge_w,
                              const int32_t* rowptr_n, const int32_t* col_n, int64_t n_rows,
                              const float* cscale, float inv_e, const int32_t* heavy_rows,
                              const int32_t* heavy_first, int64_t n_heavy, int64_t n_chunks,
                              int32_t chunk, float* slab, float* out, hgnn_stream_t stream);

/* ---- popularity-weighted negatives (opt-in) ---------------------------------------------------
 * The table of a discrete distribution over the posts and the draws from it.
 *   q[n_posts]        int64 weights, each in [0, 2^32), their sum T in [1, 2^63)
 *   cdf[n_posts + 1]  the exclusive cumulative sums, cdf[n_posts] = T (hgnn_weighted_cdf_build;
 *                     integers, so exact and independent of the summation order)
 *   draw c            x = splitmix64(*d_seed + c * golden), the word hgnn_uniform_i32 forms before
 *                     its shift; r = (x * T) >> 64, the high half of the 64 x 64-bit product; the
 *                     draw is the unique post j with cdf[j] <= r < cdf[j + 1].
 * A post of weight 0 is never drawn.  The search runs between two entries of a guide table
 * (hgnn_weighted_guide_build): guide[b], b in [0, n_guide], is the post holding b << shift (the last
 * post where that is T or more); the caller chooses shift and n_guide with
 * (T - 1) >> shift < n_guide.  The caller reads T = cdf[n_posts] once per distribution.
 * Workspace of the cdf: hgnn_weighted_cdf_ws_bytes(n_posts). */
size_t hgnn_weighted_cdf_ws_bytes(int64_t n_posts);
int hgnn_weighted_cdf_build(const int64_t* q, int64_t n_posts, int64_t* cdf, void* ws,
                            size_t ws_bytes, hgnn_stream_t stream);
int hgnn_weighted_guide_build(const int64_t* cdf, int64_t n_posts, int64_t T, int32_t shift,
                              int32_t n_guide, int32_t* guide, hgnn_stream_t stream);
/* out[c] = draw c for c in [0, n); the seed is read from device memory (no host sync). */
int hgnn_weighted_i32(const uint64_t* d_seed, int64_t n, const int64_t* cdf, int64_t n_posts,
                      int64_t T, const int32_t* guide, int32_t shift, int32_t n_guide,
                      int32_t* out, hgnn_stream_t stream);
/* Draws that avoid the posts a user has seen.  Draw i = p * n_neg + j belongs to user-grouped
 * position p, whose user is user_of_pos[p]; attempt t = 0 .. tries - 1 is draw i + t * n above, so
 * attempt 0 is hgnn_weighted_i32's.  The first attempt not in the user's seen list (seen_rowptr
 * [n_users + 1] / seen_col, ascending per user) is kept; if all are seen the last is kept and
 * *d_kept_seen (device int64, nullable, never zeroed here) is incremented.  cdf == NULL: the
 * uniform distribution, attempt t being hgnn_uniform_i32's draw at that counter (guide, T unused). */
int hgnn_weighted_avoid_i32(const uint64_t* d_seed, int64_t n, int32_t n_neg, const int64_t* cdf,
                            int64_t n_posts, int64_t T, const int32_t* guide, int32_t shift,
                            int32_t n_guide, const int32_t* user_of_pos, int64_t n_users,
                            const int32_t* seen_rowptr, const int32_t* seen_col, int32_t tries,
                            int32_t* out, int64_t* d_kept_seen, hgnn_stream_t stream);

/* The degree-skew plan made on the device with nothing read back: hgnn_plan_fill into arrays
 * sized by a bound (heavy_rows[max_heavy], heavy_first[max_heavy + 1]) and the two counts
 * {n_heavy, n_chunks} left in d_counts2 (device int32[2]).  For lists of n_pairs entries in all,
 * max_heavy = n_pairs / chunk bounds the heavy rows and 2 * max_heavy the chunks.
 * Workspace: hgnn_plan_ws_bytes(n_rows). */
int hgnn_plan_device(const int32_t* rowptr, int64_t n_rows, int32_t chunk, int64_t max_heavy,
                     int32_t* heavy_rows, int32_t* heavy_first, int32_t* d_counts2, void* ws,
                     size_t ws_bytes, hgnn_stream_t stream);

/* hgnn_score_gather2 for negatives whose lists are skewed (drawn by popularity): the negatives'
 * lists longer than `chunk` are summed chunk by chunk into neg_slab (2 * neg_max_heavy rows of d
 * floats), one wave per chunk, by the plan hgnn_plan_device made from rowptr_n with the same
 * chunk; a fix-up in fixed order then adds the positives' partial sums and the negatives' to the
 * row, so two runs are bitwise equal.  The grid is sized by neg_max_heavy; waves beyond the
 * device-side counts return at once.  rows: the format of x and rowvec (HGNN_ROWS_*; zero-packed:
 * x packed, rowvec fp32); edge_w: the positives' per-edge weights or NULL. */
#define HGNN_ROWS_F32 0
#define HGNN_ROWS_BF16 1
#define HGNN_ROWS_ZP 2
int hgnn_score_gather2_planned(int32_t rows, const void* x, int64_t n_x, const void* rowvec,
                               int32_t d, const int32_t* rowptr, const int32_t* col,
                               const float* edge_w, const int32_t* rowptr_n, const int32_t* col_n,
                               int64_t n_rows, const float* cscale, float inv_e,
                               const int32_t* heavy_rows, const int32_t* heavy_first,
                               int64_t n_heavy, int64_t n_chunks, int32_t chunk, float* slab,
                               const int32_t* neg_heavy_rows, const int32_t* neg_heavy_first,
                               const int32_t* d_neg_counts2, int64_t neg_max_heavy,
                               float* neg_slab, float* out, hgnn_stream_t stream);

/* ---- n_neg negatives per positive edge in the scoring pass (opt-in: neg_p of shape [E, k]) -----
 *   loss = <positive term> + 1/(E n_neg) sum_e sum_j softplus(<U[u_e],P[n_e,j]>)
 * The negatives are row-major [E, n_neg] in the user-grouped order: negative j of position p of
 * rowptr_u / col_u is element p * n_neg + j, in exactly one of the three forms (the other two
 * NULL); drawn ones are uniform_draw(*d_seed, p * n_neg + j, n_posts), which is what
 * hgnn_draw_sort_negatives and hgnn_uniform_i32 give for n = E * n_neg.
 * Scaling convention: the kernel keeps the two factors of the entries above, c * inv_e on a
 * positive edge and inv_e on a negative, so the caller passes
 *   n_edges = (positive edges of the whole loss) * n_neg     and     *cscale = c * n_neg,
 * which makes them c / E and 1 / (E n_neg); hgnn_score_gather2* takes the same pair
 * (inv_e = 1 / n_edges) for dP, its second list holding all E * n_neg negatives.  The positions
 * times n_neg must stay below 2^31 - 1 (the limit of the negatives sort; the caller's check).
 * edge_w: per-edge positive weights as hgnn_edge_score_fwd_w has them, or NULL for the collapsed
 * weighting.  One wave per user reads P[p_e] once and each P[n_e,j] once and writes dU[u] once, no
 * atomics; two runs are bitwise equal.  An out-of-range negative is counted into err and
 * contributes nothing.  The per-position outputs of hgnn_edge_score_fwd are not produced.
 * n_neg < 1, more or fewer than one negative form, and n_posts out of range with a seed are
 * HGNN_E_ARG; fp32 d > 512 is HGNN_E_UNSUPPORTED; all before any launch.  With n_neg = 1 the
 * results are those of hgnn_edge_score_fwd_w (or, edge_w NULL, hgnn_edge_score_fwd*). */
int hgnn_edge_score_fwd_k(const float* U, const float* P, int32_t d, int64_t n_users,
                          int64_t n_posts, const int32_t* rowptr_u, const int32_t* col_u,
                          const float* edge_w, const int64_t* neg_i64, const int32_t* neg_i32,
                          const uint64_t* d_seed, int32_t n_neg, int64_t n_edges,
                          const float* cscale, float* dU, float* part, float* loss, int32_t* err,
                          hgnn_stream_t stream);
/* ... with bf16 U and P (d % 8 == 0 and d <= 512, else HGNN_E_UNSUPPORTED). */
int hgnn_edge_score_fwd_k_bf16(const uint16_t* U, const uint16_t* P, int32_t d, int64_t n_users,
                               int64_t n_posts, const int32_t* rowptr_u, const int32_t* col_u,
                               const float* edge_w, const int64_t* neg_i64,
                               const int32_t* neg_i32, const uint64_t* d_seed, int32_t n_neg,
                               int64_t n_edges, const float* cscale, float* dU, float* part,
                               float* loss, int32_t* err, hgnn_stream_t stream);

/* ---- logQ correction of the link loss's scores (opt-in: logq= of the loss entry points) --------
 * A per-post table b (fp32 [n_posts], a constant: no gradient into it) moves the logit of every
 * scored pair, positive and negative alike:
 *   z(u, p) = <U[u], P[p]> - b[p]
 *   loss = <scales as below> sum softplus(-z_pos) + sum softplus(z_neg)
 *   dU[u] = sum h P[.],  dP[p] = sum h U[.],  h = scale * (sigmoid(z_pos) - 1)  or  scale * sigmoid(z_neg)
 * With b[p] = log(k Q(p)) for negatives drawn k per edge from Q this is the logQ correction of
 * sampled softmax / NCE.  The dot products, the rows read, the sums and their order are those of
 * the entries these stand beside; only the scalar fed to the sigmoid and the softplus moves.  As
 * in every entry of the loss the positives' coefficient sigmoid(z) - 1 is formed as -sigmoid(-z)
 * from the same exponential (b = log(1/T) puts z near +22, where the difference is exactly 0 in
 * fp32) and the softplus with a corrected log1p (csrc/bce_terms.h), so b = 0 gives their results,
 * and two runs are bitwise equal.  With bf16 rows b stays fp32.
 *
 * hgnn_edge_score_fwd_k_lq: hgnn_edge_score_fwd_k (any n_neg >= 1, edge_w nullable) with
 * post_bias = b.  Scaling convention: hgnn_edge_score_fwd_k's, n_edges = E * n_neg and
 * *cscale = c * n_neg.  Written: dU, part, loss and err; the per-position outputs of
 * hgnn_edge_score_fwd are not produced.  An out-of-range negative is counted into err, reads
 * post_bias[0] as it reads post 0, and contributes nothing.  post_bias == NULL is HGNN_E_ARG, the
 * rest as for hgnn_edge_score_fwd_k; all before any launch. */
int hgnn_edge_score_fwd_k_lq(const float* U, const float* P, int32_t d, int64_t n_users,
                             int64_t n_posts, const int32_t* rowptr_u, const int32_t* col_u,
                             const float* edge_w, const int64_t* neg_i64, const int32_t* neg_i32,
                             const uint64_t* d_seed, int32_t n_neg, int64_t n_edges,
                             const float* cscale, const float* post_bias, float* dU, float* part,
                             float* loss, int32_t* err, hgnn_stream_t stream);
/* ... with bf16 U and P (d % 8 == 0 and d <= 512, else HGNN_E_UNSUPPORTED); post_bias fp32. */
int hgnn_edge_score_fwd_k_lq_bf16(const uint16_t* U, const uint16_t* P, int32_t d,
                                  int64_t n_users, int64_t n_posts, const int32_t* rowptr_u,
                                  const int32_t* col_u, const float* edge_w,
                                  const int64_t* neg_i64, const int32_t* neg_i32,
                                  const uint64_t* d_seed, int32_t n_neg, int64_t n_edges,
                                  const float* cscale, const float* post_bias, float* dU,
                                  float* part, float* loss, int32_t* err, hgnn_stream_t stream);
/* hgnn_score_gather2 / _w / _zp / _bf16 with the offset: the post is the output row, so the wave
 * of an item (a row, or a chunk of a heavy row) reads row_bias[row] once, beside rowvec[row], and
 * subtracts it from every score of both lists before the sigmoid.  rows: the format of x and
 * rowvec (HGNN_ROWS_*, hgnn_score_gather2_planned's); edge_w: the positives' per-edge weights or
 * NULL; cscale and inv_e as hgnn_score_gather2 takes them.  Written: out (every row once) and the
 * slab; the slab and the fix-up hold sums and read no offset.  rows out of range and
 * row_bias == NULL are HGNN_E_ARG, a width the format does not take HGNN_E_UNSUPPORTED, then
 * hgnn_score_gather2's rules; all before any launch. */
int hgnn_score_gather2_lq(int32_t rows, const void* x, int64_t n_x, const void* rowvec, int32_t d,
                          const int32_t* rowptr, const int32_t* col, const float* edge_w,
                          const int32_t* rowptr_n, const int32_t* col_n, int64_t n_rows,
                          const float* cscale, float inv_e, const float* row_bias,
                          const int32_t* heavy_rows, const int32_t* heavy_first, int64_t n_heavy,
                          int64_t n_chunks, int32_t chunk, float* slab, float* out,
                          hgnn_stream_t stream);
/* hgnn_score_gather2_planned with the offset (its arguments, row_bias after inv_e): whole rows,
 * chunks of a row heavy in its positives and chunks of a row heavy in its negatives all subtract
 * row_bias[row]; the two slabs and the two fix-ups are unchanged.  rows out of range and
 * row_bias == NULL are HGNN_E_ARG, then hgnn_score_gather2_planned's rules; all before any
 * launch. */
int hgnn_score_gather2_planned_lq(int32_t rows, const void* x, int64_t n_x, const void* rowvec,
                                  int32_t d, const int32_t* rowptr, const int32_t* col,
                                  const float* edge_w, const int32_t* rowptr_n,
                                  const int32_t* col_n, int64_t n_rows, const float* cscale,
                                  float inv_e, const float* row_bias, const int32_t* heavy_rows,
                                  const int32_t* heavy_first, int64_t n_heavy, int64_t n_chunks,
                                  int32_t chunk, float* slab, const int32_t* neg_heavy_rows,
                                  const int32_t* neg_heavy_first, const int32_t* d_neg_counts2,
                                  int64_t neg_max_heavy, float* neg_slab, float* out,
                                  hgnn_stream_t stream);

/* ---- neighbour sampling for mini-batches (BASELINE cfg5; no reference counterpart) -----------
 * For each destination dst_ids[i] (rows of a destination-grouped CSR rowptr/col over n_rows):
 * keep all in-neighbours if deg <= fanout (or fanout < 0), else `fanout` distinct neighbour
 * positions drawn uniformly (Floyd's algorithm, counter-based hash of (seed, dst id, draw)).
 * out_rowptr[n_dst+1] is written first; with out_col == NULL only the counts are produced (read
 * out_rowptr[n_dst] to size out_col).  fanout in 1..64 or < 0.  ws: hgnn_sample_ws_bytes(n_dst). */
size_t hgnn_sample_ws_bytes(int64_t n_dst);
int hgnn_sample_neighbors(const int32_t* rowptr, const int32_t* col, int64_t n_rows,
                          const int32_t* dst_ids, int64_t n_dst, int32_t fanout, uint64_t seed,
                          int32_t* out_rowptr, int32_t* out_col, void* ws, size_t ws_bytes,
                          hgnn_stream_t stream);
/* The fill phase alone, for an out_rowptr an earlier count-only hgnn_sample_neighbors call made
 * (same rowptr, dst_ids, fanout): one launch.  Destination ids outside [0, n_rows) have no
 * neighbours in either phase (never dereferenced). */
int hgnn_sample_fill(const int32_t* rowptr, const int32_t* col, int64_t n_rows,
                     const int32_t* dst_ids, int64_t n_dst, int32_t fanout, uint64_t seed,
                     const int32_t* out_rowptr, int32_t* out_col, hgnn_stream_t stream);
/* One hop of the sampler over every relation into the frontier (at most 8), one launch per phase
 * (hgnn_sample_neighbors / hgnn_sample_fill per relation, batched; the samples are identical).
 * Count: out_rowptrs[r][n_dst[r]+1] zero-based per relation, d_totals[r] (device int32) = its
 * size; ws: hgnn_sample_hop_ws_bytes(sum of n_dst).  Fill: relation r's sample into out_cols[r]
 * (d_totals[r] entries).  Host arrays of n_rel entries; one fanout and seed for the hop. */
size_t hgnn_sample_hop_ws_bytes(int64_t n_total_dst);
int hgnn_sample_hop_count(int32_t n_rel, const int32_t* const* rowptrs, const int64_t* n_rows,
                          const int32_t* const* dst_ids, const int64_t* n_dst, int32_t fanout,
                          int32_t* const* out_rowptrs, int32_t* d_totals, void* ws,
                          size_t ws_bytes, hgnn_stream_t stream);
int hgnn_sample_hop_fill(int32_t n_rel, const int32_t* const* rowptrs, const int32_t* const* cols,
                         const int64_t* n_rows, const int32_t* const* dst_ids,
                         const int64_t* n_dst, int32_t fanout, uint64_t seed,
                         const int32_t* const* out_rowptrs, int32_t* const* out_cols,
                         hgnn_stream_t stream);

/* Next layer's node set of one type: nodes_out = [prefix (order kept), then every item id not in
 * prefix, once, in order of first appearance in items]; local_out[k] = position of items[k] in
 * nodes_out; *d_count = total.  Prefix ids distinct; ids are non-negative int32.  nodes_out holds
 * n_prefix + n_items entries.  O(n_prefix + n_items) work (a hash set over this call's ids),
 * deterministic.  ws: hgnn_relabel_ws_bytes(n_prefix, n_items). */
size_t hgnn_relabel_ws_bytes(int64_t n_prefix, int64_t n_items);
int hgnn_relabel(const int32_t* prefix, int64_t n_prefix, const int32_t* items, int64_t n_items,
                 int32_t* local_out, int32_t* nodes_out, int32_t* d_count, void* ws,
                 size_t ws_bytes, hgnn_stream_t stream);
/* hgnn_relabel that also checks the prefix (a mini-batch's seeds): d_count2[0] = the count,
 * d_count2[1] = flags, bit 0 a repeated prefix id, bit 1 a prefix id outside [0, id_limit)
 * (id_limit 0: a type with no nodes, every id flagged; id_limit < 0: no range check).
 * The outputs are unspecified when a flag is set; nothing is read out of bounds. */
int hgnn_relabel_checked(const int32_t* prefix, int64_t n_prefix, int64_t id_limit,
                         const int32_t* items, int64_t n_items, int32_t* local_out,
                         int32_t* nodes_out, int32_t* d_count2, void* ws, size_t ws_bytes,
                         hgnn_stream_t stream);
/* Every node type of a hop in one call (n_types <= 8): type t's prefix prefix[t][n_prefix[t]],
 * its items the consecutive range n_items[t] of `items` (types in order), its node set into
 * nodes_out[t] (n_prefix[t] + n_items[t] entries), the local ids of all items into local_out
 * (per type, as hgnn_relabel); ids < id_limit[t] (required when n_types > 1: the table is keyed
 * by id * n_types + t, so id_limit * n_types < 2^31).  d_count2: with check, (count, flags) per
 * type as hgnn_relabel_checked; without, the counts only.  The same nodes and local ids as one
 * hgnn_relabel per type.  ws: hgnn_relabel_multi_ws_bytes(sum of n_prefix, sum of n_items). */
size_t hgnn_relabel_multi_ws_bytes(int64_t n_prefix_total, int64_t n_items_total);
int hgnn_relabel_multi(int32_t n_types, const int32_t* const* prefix, const int64_t* n_prefix,
                       const int64_t* id_limit, const int32_t* items, const int64_t* n_items,
                       int32_t* local_out, int32_t* const* nodes_out, int32_t* d_count2,
                       int32_t check, void* ws, size_t ws_bytes, hgnn_stream_t stream);

/* Static-capacity copies of sampled blocks (a captured mini-batch step replays one HIP graph over
 * fixed buffers).  Item i (n_items <= 16): the CSR rowptr[i] (n_dst[i] + 1) / col[i] (e[i]) into
 * rowptr_out[i] (d_cap[i] + 1) / col_out[i] (e_cap[i]); the e_cap - e padding entries get sources
 * dummy[i] + (k mod spread[i]) (spread optional, >= 1: padded source rows taken in turn, so the
 * transposed grouping has no long row) and are spread over the padded rows n_dst .. d_cap - 1
 * (d_cap > n_dst required when
 * e_cap > e), so the copy is a valid CSR of d_cap rows whose first n_dst rows are the input's.
 * map[i] (optional): real entries become map[i][col] (a block's local ids -> global ids).
 * d_cap[i] < 0: col only (a node-id list padded with dummy[i]).  Replaces nothing in the
 * reference (which trains full-batch); it feeds forward_blocks' static form (minibatch.py). */
int hgnn_pad_csr_multi(int32_t n_items, const int32_t* const* rowptr, const int32_t* const* col,
                       const int32_t* const* map, const int64_t* n_dst, const int64_t* e,
                       int32_t* const* rowptr_out, int32_t* const* col_out, const int64_t* d_cap,
                       const int64_t* e_cap, const int32_t* dummy, const int32_t* spread,
                       hgnn_stream_t stream);

/* The outermost block's destination rows of a static step (minibatch.StaticBlocks.prepare),
 * gathered with the staged batch in one launch: item i (n_items <= 8) writes
 * out[i][r][0..d) = src[i][ids[i][r]][0..d) for r < n_rows[i]; d % 4 == 0, 16-byte aligned rows,
 * ids in range (not validated).  Replaces the per-type x.index_select of the captured step. */
int hgnn_gather_rows_multi(int32_t n_items, const float* const* src, const int32_t* const* ids,
                           const int64_t* n_rows, int64_t d, float* const* out,
                           hgnn_stream_t stream);

/* A link mini-batch's loss structures in one call (minibatch.LinkLoss.prepare; the reference's
 * loss, train_gnn.py:259-281, over a batch's positive pairs and their negatives): the E pairs
 * (pu[i], pp[i]) with negative pn[i] — local ids, users < n_users, posts < n_posts, not
 * validated — grouped by user, stable: rowptr_u[n_users+1], col_p / neg / uop[E] (post, negative,
 * user per position); the same pairs by post (hgnn_csr_transpose of rowptr_u / col_p: p_rowptr
 * [n_posts+1], p_users / p_perm[E]); the negatives by post (hgnn_sort_pairs_i32(neg, uop):
 * n_rowptr[n_posts+1], n_users_sorted[E]) — the dP gather's order.  Exactly the three calls it
 * replaces.  ws: hgnn_link_group_ws_bytes(E). */
size_t hgnn_link_group_ws_bytes(int64_t E);
int hgnn_link_group(const int32_t* pu, const int32_t* pp, const int32_t* pn, int64_t E,
                    int64_t n_users, int64_t n_posts, int32_t* rowptr_u, int32_t* col_p,
                    int32_t* neg, int32_t* uop, int32_t* p_rowptr, int32_t* p_users,
                    int32_t* p_perm, int32_t* n_rowptr, int32_t* n_users_sorted, void* ws,
                    size_t ws_bytes, hgnn_stream_t stream);

/* hgnn_link_group for n_neg >= 1 negatives per pair (pn[E * n_neg], row-major: row i the negatives
 * of batch pair i) and two optional inputs (opt-in; minibatch.LinkLoss with num_neg / weighting=
 * "edge" / logq).  The stable sort by user carries the batch position as its payload, and one
 * kernel fills from it:
 *   rowptr_u, col_p, uop, p_rowptr, p_users, p_perm   as hgnn_link_group
 *   neg[E * n_neg]          row p = the negatives of user-grouped position p
 *                           (hgnn_edge_score_fwd_k's layout)
 *   n_rowptr[n_posts + 1] / n_users_sorted[E * n_neg]
 *                           all E * n_neg (negative post, user) pairs grouped by post, stable
 *   w != NULL (fp32 [E], batch order): w_user[E] = the weights by user-grouped position, w_post[E]
 *                           = by post-grouped position, w_post[i] = w_user[p_perm[i]] (exact copies)
 *   logq != NULL (fp32, the global table) with seeds_p[n_seeds] (the batch's local -> global post
 *   ids): logq_local[n_posts], logq_local[j] = logq[seeds_p[j]] for j < the seeds' count — n_seeds,
 *   or min(n_seeds, *d_n_seeds) when d_n_seeds (device int32, hgnn_link_seeds*'s d_counts + 1) is
 *   given: the count then never leaves the device — and 0 for the rows after it (padded tables),
 *   which no pair refers to.  logq and seeds_p are both given or both NULL.
 * Nothing is read back; every launch is sized by E, n_neg, n_users, n_posts.  With n_neg = 1 and
 * no optional input the nine common outputs equal hgnn_link_group's bit for bit.
 * ws: hgnn_link_group_k_ws_bytes(E, n_neg). */
size_t hgnn_link_group_k_ws_bytes(int64_t E, int32_t n_neg);
int hgnn_link_group_k(const int32_t* pu, const int32_t* pp, const int32_t* pn, const float* w,
                      const float* logq, const int32_t* seeds_p, int64_t n_seeds,
                      const int32_t* d_n_seeds, int64_t E, int32_t n_neg, int64_t n_users,
                      int64_t n_posts, int32_t* rowptr_u, int32_t* col_p, int32_t* neg,
                      int32_t* uop, int32_t* p_rowptr, int32_t* p_users, int32_t* p_perm,
                      int32_t* n_rowptr, int32_t* n_users_sorted, float* w_user, float* w_post,
                      float* logq_local, void* ws, size_t ws_bytes, hgnn_stream_t stream);

/* ---- sync-free static sampling (minibatch.StaticSampler; csrc/sampler_static.hip) ------------
 * The eager sampler's results (hgnn_sample_hop_count / _fill, hgnn_relabel_multi) followed by
 * hgnn_pad_csr_multi, written straight into static-capacity buffers with every count kept on
 * the device, so a batch is queued without a host read-back.  Not in the reference (it trains
 * full-batch, train_gnn.py:254); it feeds the captured cfg5 step.
 *
 * hgnn_link_seeds: a link batch (minibatch.link_batch): the B <= 2048 positives edge_ids into the
 * (src, dst) rows of the positive relation and their negatives neg[B] (int64 ids < 2^31 - 1);
 * seeds_u[B] / seeds_p[2B] = the distinct users / posts (positives' posts and negatives)
 * ascending, d_counts[2] = their numbers, pu / pp / pn[B] = each pair's local ids (ranks). */
int hgnn_link_seeds(const int64_t* src, const int64_t* dst, const int64_t* edge_ids,
                    const int64_t* neg, int64_t B, int32_t* seeds_u, int32_t* seeds_p,
                    int32_t* pu, int32_t* pp, int32_t* pn, int32_t* d_counts,
                    hgnn_stream_t stream);
/* hgnn_link_seeds for n_neg >= 1 negatives per positive (opt-in; minibatch.LinkSampler with
 * num_neg >= 2 or weighted draws): the negatives row-major [B, n_neg] as int64 (neg_i64,
 * torch.randint's) or int32 (neg_i32, hgnn_weighted*_i32's) — exactly one of the two non-NULL.
 * Block 1 ranks B * (1 + n_neg) post keys, the positives' posts first, then the negatives in
 * row-major order: seeds_p[B * (1 + n_neg)] ascending and distinct, pp[B], pn[B * n_neg] the local
 * ids in the same layout, d_counts[2].  Nothing past the counts is written.  Capacity:
 * B * (1 + n_neg) <= 16384 keys (128 KiB of LDS in one workgroup; B = 1024 with n_neg <= 15,
 * B = 2048 with n_neg <= 7), else HGNN_E_ARG before any launch.  With n_neg = 1 the outputs equal
 * hgnn_link_seeds's. */
int hgnn_link_seeds_k(const int64_t* src, const int64_t* dst, const int64_t* edge_ids,
                      const int64_t* neg_i64, const int32_t* neg_i32, int64_t B, int32_t n_neg,
                      int32_t* seeds_u, int32_t* seeds_p, int32_t* pu, int32_t* pp, int32_t* pn,
                      int32_t* d_counts, hgnn_stream_t stream);

/* One hop of n_rel (<= 8) relations, fanout 1..64: relation r samples the first *d_n_dst[r] ids
 * of dst_ids[r] (global CSR rowptrs[r] / cols[r] over n_rows[r] destinations; the count lives on
 * the device, caps[r] bounds it and leaves >= 1 padded row) exactly as hgnn_sample_hop_fill with
 * `seed`: out_rowptrs[r][caps[r] + 1] = the real rows then padded rows spread as
 * hgnn_pad_csr_multi does, fill_outs[r] = the sampled global source ids in CSR order,
 * tail_outs[r][E .. ecaps[r]) = padding entries dummy[r] + (k mod spread[r]), d_E[r] = E.
 * ws: hgnn_sample_hop_ws_bytes(sum of caps). */
int hgnn_sample_hop_static(int32_t n_rel, const int32_t* const* rowptrs,
                           const int32_t* const* cols, const int64_t* n_rows,
                           const int32_t* const* dst_ids, const int32_t* const* d_n_dst,
                           const int64_t* caps, const int64_t* ecaps, int32_t fanout,
                           uint64_t seed, int32_t* const* out_rowptrs, int32_t* const* fill_outs,
                           int32_t* const* tail_outs, const int32_t* dummy,
                           const int32_t* spread, int32_t* d_E, void* ws, size_t ws_bytes,
                           hgnn_stream_t stream);

/* hgnn_relabel_multi over capacity layouts: type ty's prefix = the first *d_n_prefix[ty] ids of
 * prefix[ty]; the items are n_irel (<= 8) relations' runs, relation q in slots item_caps[q] long
 * (consecutive, grouped by source type irel_type[q] ascending), its first d_E[q] valid.  Writes
 * nodes_out[ty] (zeroed past the count up to nodes_caps[ty]), each valid item's local id into
 * local_out[q], d_count[ty] = the node counts.  ws: hgnn_relabel_static_ws_bytes(sum of
 * prefix_caps, sum of item_caps). */
size_t hgnn_relabel_static_ws_bytes(int64_t prefix_cap_total, int64_t item_cap_total);
int hgnn_relabel_static(int32_t n_types, const int32_t* const* prefix,
                        const int32_t* const* d_n_prefix, const int64_t* prefix_caps,
                        int32_t* const* nodes_out, const int64_t* nodes_caps, int32_t n_irel,
                        const int32_t* items, const int64_t* item_caps, const int32_t* irel_type,
                        const int32_t* d_E, int32_t* const* local_out, int32_t* d_count,
                        void* ws, size_t ws_bytes, hgnn_stream_t stream);

/* ---- ranking metrics of the evaluation (train_gnn.py:289-367), batched ----------------------
 * scores [n_rows][ld]: one row per test user over the n_cand sorted test candidates (a GEMM of
 * user and candidate embeddings, computed by the caller).  Per row:
 *   top-k, k = min(K, n_cand), ordered by (score desc, candidate index asc)  -> topk_idx (opt.)
 *   recall[r] = |top-k ∩ true(r)| / true_count[r]   (true_count counts duplicate test edges)
 *   ndcg[r]   = sklearn ndcg_score(binary relevance, scores, k=K), tie-averaged (ignore_ties=False)
 * true_rowptr/true_cand: each row's sorted unique relevant candidate indices.  K <= 63.
 * Scores are assumed finite. */
int hgnn_topk_metrics(const float* scores, int64_t n_rows, int64_t n_cand, int64_t ld,
                      const int32_t* true_rowptr, const int32_t* true_cand,
                      const int32_t* true_count, int32_t K, int32_t* topk_idx, double* recall,
                      double* ndcg, hgnn_stream_t stream);

/* ---- edge construction from raw ids -------------------------------------------
 * Replaces the host loops that map entity ids to node indices row by row:
 * build_edge_index_safe (train_gnn.py:40-73), build_test_edges (test_gnn.py:34-55) and the
 * Series.map(dict) + dropna of build_graph.py:383-402.
 *
 * An id map is a dict {key: value} as an open-addressing table of 16-B slots in device memory.
 * Keys are integers (key_ints[n]) or strings in the Arrow layout (key_offsets[n+1] int64 byte
 * offsets into key_bytes, UTF-8; key_bytes and q_bytes must be readable 16 bytes past their last
 * string, as Arrow's 64-B buffer padding guarantees); keys distinct.  capacity: hgnn_idmap_capacity(n_keys) (a power
 * of two >= 2 n_keys, >= 16); slots: 16·capacity bytes.  The key arrays (and vals) must stay alive
 * for lookups: the table stores key rows, and string matches are confirmed byte by byte. */
int64_t hgnn_idmap_capacity(int64_t n_keys);
int hgnn_idmap_build(const int64_t* key_ints, const int64_t* key_offsets, const uint8_t* key_bytes,
                     int64_t n_keys, void* slots, int64_t capacity, hgnn_stream_t stream);
/* dict.get for n_q queries: out[q] = vals[row of the key equal to query q], or -1 when absent or
 * q_valid[q] == 0 (q_valid may be NULL).  vals == NULL returns the key row.  Integer queries
 * (q_ints) need an integer-keyed map; string queries (q_offsets + q_bytes) a string-keyed one. */
int hgnn_idmap_lookup(const void* slots, int64_t capacity, const int64_t* key_ints,
                      const int64_t* key_offsets, const uint8_t* key_bytes, const int64_t* vals,
                      const int64_t* q_ints, const int64_t* q_offsets, const uint8_t* q_bytes,
                      const uint8_t* q_valid, int64_t n_q, int64_t* out, hgnn_stream_t stream);
/* Keep the rows i in [0,n) whose every column cols[c][i] >= 0 (c < n_cols <= 4), in order:
 * outs[o][k] = cols[out_col[o]][i] for the k-th kept row (n_outs <= 4; one column may feed several
 * outputs, e.g. the post column of both the engage and the author edge list).  *d_count (device)
 * = kept rows; with n_outs == 0 only the count is produced.  n < 2^31.
 * ws: hgnn_compact_rows_ws_bytes(n).  cols/outs/out_col are HOST arrays of device pointers. */
size_t hgnn_compact_rows_ws_bytes(int64_t n);
int hgnn_compact_rows(const int64_t* const* cols, int32_t n_cols, int64_t n,
                      int64_t* const* outs, const int32_t* out_col, int32_t n_outs,
                      int32_t* d_count, void* ws, size_t ws_bytes, hgnn_stream_t stream);

/* As hgnn_topk_metrics for a subset of rows: score row r belongs to row row_map[r] of the true
 * sets and of recall / ndcg (topk_idx stays indexed by r). */
int hgnn_topk_metrics_rows(const float* scores, int64_t n_rows, int64_t n_cand, int64_t ld,
                           const int32_t* row_map, const int32_t* true_rowptr,
                           const int32_t* true_cand, const int32_t* true_count, int32_t K,
                           int32_t* topk_idx, double* recall, double* ndcg, hgnn_stream_t stream);

/* Fused scoring + top-L (the evaluation's GEMM and torch.topk, train_gnn.py:330-340, and
 * inference.py:427-429): for each output row r (user U[rows ? rows[r] : r], d floats) the L best
 * of the n_cand candidates P[c] by <U, P[c]> (fp32 MFMA), score desc then index asc, written to
 * topv / topi [n_rows][L].  The [rows, n_cand] score matrix is never materialised.
 * d in {64, 128}; U and P row-major, 16-B aligned; 1 <= L <= min(64, n_cand). */
size_t hgnn_score_topk_lds_bytes(int32_t d, int32_t L);
int hgnn_score_topk(const float* U, const int32_t* rows, int64_t n_rows, const float* P,
                    int64_t n_cand, int32_t d, int32_t L, float* topv, int32_t* topi,
                    hgnn_stream_t stream);
/* hgnn_score_topk over bf16 tables (uint16_t bit patterns, as the bf16 row storage above): the
 * scores come from bf16 MFMA (16x16x32) with fp32 accumulation, so a list is what hgnn_score_topk
 * gives on the widened tables float(U), float(P), up to fp32 summation order.  topv / topi stay
 * fp32 / int32, so hgnn_topk_finish takes them as they are.  Same contract otherwise: d in
 * {64, 128}; U and P row-major, 16-B aligned; 1 <= L <= min(64, n_cand); score desc then index
 * asc; no sync, no allocation, graph-capturable; the same argument checks and error codes.  A
 * workgroup takes 128 users (8 waves x 16) and streams the candidates in chunks of 64 or, where
 * that lets one more workgroup live on the CU, 32; hgnn_score_topk_bf16_lds_bytes is the dynamic
 * LDS of the (d, L) launch: two chunk buffers and 128 L 8 B of lists, <= 160 KiB for every legal
 * L. */
size_t hgnn_score_topk_bf16_lds_bytes(int32_t d, int32_t L);
int hgnn_score_topk_bf16(const uint16_t* U, const int32_t* rows, int64_t n_rows,
                         const uint16_t* P, int64_t n_cand, int32_t d, int32_t L, float* topv,
                         int32_t* topi, hgnn_stream_t stream);
/* hgnn_score_topk / hgnn_score_topk_bf16 with per-row exclusion lists (serving: leave out the
 * posts a user has already engaged with): output row r never lists the candidates
 * excl_col[excl_rowptr[e] .. excl_rowptr[e + 1]), e = excl_rows ? excl_rows[r] : r.  excl_rows is
 * independent of rows: with both set to the same user ids, U and the lists are keyed alike.
 * Caller's contract, not checked (it would take a pass and a sync): each list strictly ascending,
 * its entries in [0, n_cand), excl_rowptr non-decreasing.  The kernel tests the exclusion where it
 * masks the candidates past n_cand, before the threshold test, so an excluded candidate never
 * reaches a list; each list is walked once, at most one chunk's entries per chunk.
 * A row with fewer than L candidates left ends with empty slots: topv = -inf, topi = -1.  Such
 * lists are not input for hgnn_topk_finish, which expects L real entries per row.
 * Everything else is hgnn_score_topk's contract: d in {64, 128}; U and P row-major, 16-B aligned;
 * 1 <= L <= min(64, n_cand); score desc then index asc; no sync, no allocation,
 * graph-capturable; the same argument checks and error codes, and HGNN_E_ARG for a null
 * excl_rowptr or excl_col.  The dynamic LDS is that of the plain kernels (the bf16 launch may
 * choose the other chunk size than hgnn_score_topk_bf16_lds_bytes reports: the excluding kernel
 * holds more registers, which changes where a 32-candidate chunk buys a resident workgroup). */
int hgnn_score_topk_excl(const float* U, const int32_t* rows, int64_t n_rows, const float* P,
                         int64_t n_cand, int32_t d, int32_t L, const int32_t* excl_rowptr,
                         const int32_t* excl_col, const int32_t* excl_rows, float* topv,
                         int32_t* topi, hgnn_stream_t stream);
int hgnn_score_topk_excl_bf16(const uint16_t* U, const int32_t* rows, int64_t n_rows,
                              const uint16_t* P, int64_t n_cand, int32_t d, int32_t L,
                              const int32_t* excl_rowptr, const int32_t* excl_col,
                              const int32_t* excl_rows, float* topv, int32_t* topi,
                              hgnn_stream_t stream);
/* Recall / NDCG (as hgnn_topk_metrics) from hgnn_score_topk or hgnn_score_topk_bf16 lists with
 * L = min(K, n_cand) + 1 (or min(K, n_cand) when n_cand <= K).  A row whose K-th value ties the
 * (K+1)-th needs the whole row for sklearn's tie groups: it gets tie_flag = 1 and no outputs;
 * redo those rows with materialised scores (hgnn_topk_metrics_rows). */
int hgnn_topk_finish(const float* topv, const int32_t* topi, int64_t n_rows, int32_t L,
                     int64_t n_cand, int32_t K, const int32_t* true_rowptr,
                     const int32_t* true_cand, const int32_t* true_count, double* recall,
                     double* ndcg, int32_t* tie_flag, hgnn_stream_t stream);

/* ---- Hard (model-scored) negatives: the n_neg top-scored of n_cand candidates per edge ---------
 * hgnn_hard_negatives: for every positive edge, in the user-grouped order of rowptr_u / col_u
 * (the arrays hgnn_edge_score_fwd_k takes), score its n_cand = M candidate posts against the
 * edge's user and write the n_neg = k best as int32 out[E, k].  One wave per user, U[u] in
 * registers, the M post rows streamed per edge as the scoring pass streams them; nothing but ids
 * is written, and no gradient is involved.
 *
 * Candidates: cand32, int32 row-major [E, M] (candidate j of position p is element p * M + j), or
 * cand_seed, a device seed: candidate p * M + j is uniform_draw(*seed, p * M + j, n_posts),
 * exactly what hgnn_uniform_i32 writes for that seed.  Exactly one of the two is non-null.
 *
 * Per position p (user u, positive post c+ = col_u[p], candidates c_0 .. c_{M-1}):
 *   scores    s_j = the kernel's fp32 dot product <U[u], P[c_j]> (bf16 rows widened to fp32);
 *             a NaN score counts as -inf.
 *   eligible  column j with 0 <= c_j < n_posts, c_j != c+, and c_j not already picked for p.
 *             An out-of-range id is counted once in err and its row is never loaded (the load is
 *             clamped to row 0).
 *   picks     pick r = 0 .. k-1 is the eligible, not yet taken column of the greatest score, the
 *             lowest column on equal scores; out[p, r] is its post id.  So a row of out is in
 *             descending score order and holds distinct posts.
 *   short     with no eligible column left, the pick is the lowest untaken in-range column,
 *             whatever it holds; with none of those, c+.  Each such pick adds 1 to *short_count.
 *             Every value written is therefore a valid post id.
 * The result is deterministic; the two counters are the only atomics.  err (int32, nullable) is
 * zeroed by the entry, as the loss entries do; short_count (int64, nullable) is only incremented.
 *
 * Limits: 1 <= n_neg <= n_cand <= 64, 1 <= n_posts < 2^31 - 1.  Widths as hgnn_edge_score_fwd:
 * fp32 rows d <= 512, bf16 rows d % 8 == 0 and d <= 512, else HGNN_E_UNSUPPORTED.  Bad sizes, a
 * null U, P, rowptr_u, col_u or out, and both or neither candidate source are HGNN_E_ARG.  All
 * before any launch.  Rows are indexed as (int64_t)id * d. */
int hgnn_hard_negatives(const float* U, const float* P, int32_t d, int64_t n_users,
                        int64_t n_posts, const int32_t* rowptr_u, const int32_t* col_u,
                        const int32_t* cand32, const uint64_t* cand_seed, int32_t n_cand,
                        int32_t n_neg, int32_t* out, int64_t* short_count, int32_t* err,
                        hgnn_stream_t stream);
/* ... with bf16 U and P. */
int hgnn_hard_negatives_bf16(const uint16_t* U, const uint16_t* P, int32_t d, int64_t n_users,
                             int64_t n_posts, const int32_t* rowptr_u, const int32_t* col_u,
                             const int32_t* cand32, const uint64_t* cand_seed, int32_t n_cand,
                             int32_t n_neg, int32_t* out, int64_t* short_count, int32_t* err,
                             hgnn_stream_t stream);
/* The positions of a user a wave takes per chunk at n_cand candidates (0: n_cand out of range):
 * min(64, hgnn_hard_neg_lds_words() / (n_cand | 1)), the kernel parking a chunk's scores and ids
 * in two per-wave LDS arrays of hgnn_hard_neg_lds_words() words at an odd per-position stride. */
int32_t hgnn_hard_neg_chunk(int32_t n_cand);
int32_t hgnn_hard_neg_lds_words(void);

/* ---- sampled-softmax (InfoNCE) link loss (opt-in: edge_softmax_loss) -----------------------------
 * One (1 + k)-way classification per positive edge e = (u, p_0) with negatives p_1 .. p_k:
 *   z_j = <U[u], P[p_j]> / temperature - b[p_j]          (b = post_bias, NULL: 0)
 *   loss = sum_e g_e (logsumexp_j z_j - z_0),    g_e = *cscale / n_edges * (edge_w ? edge_w[e] : 1)
 * with pi_j = exp(z_j - lse_e) the coefficients of the gradient are
 *   positive  -g_e (sum_{j >= 1} pi_j) / temperature   (= g_e (pi_0 - 1) / temperature, formed
 *                                                        without the cancellation)
 *   negative j g_e pi_j / temperature
 * and dU[u] = sum coefficient x P row, dP[p] = sum coefficient x U row.  A coefficient depends on
 * all 1 + k logits of its edge, so it is produced once, by the scoring pass, and carried to the dP
 * gather (hgnn_coef_gather2_planned) instead of being recomputed there.
 *
 * hgnn_edge_softmax_fwd: one wave per user (U[u] in registers) walks each of its edges' 1 + k post
 * rows once with an online softmax (running maximum, rescaled sums: nothing is exponentiated
 * unshifted) and writes
 *   dU        [n_users, d] fp32, every row once, no atomics
 *   loss      the scalar above (deterministic reduction through part, hgnn_softmax_parts floats)
 *   coef_neg  [n_edges, n_neg] fp32 in the user-grouped order of the negatives (an out-of-range
 *             negative: 0)
 *   coef_pos  [n_edges] fp32; position p of rowptr_u / col_u writes coef_pos[slot_of[p]], or
 *             coef_pos[p] with slot_of == NULL (slot_of: int32 [n_edges], the position's index in
 *             the post-grouped order the dP gather reads)
 *   err       (nullable) zeroed, then the count of out-of-range negatives; such a negative takes no
 *             part in its edge's softmax (logit -inf), reads post 0 and post_bias of nothing.
 * rows: HGNN_ROWS_F32 or HGNN_ROWS_BF16, the format of U and P (post_bias, edge_w stay fp32).  The
 * negatives are row-major [n_edges, n_neg] in the user-grouped order, int64 or int32 (exactly one
 * non-null).  n_edges is the number of positive edges (no n_neg scaling convention here).
 * HGNN_E_ARG: rows out of range, d <= 0 or a negative size, n_neg outside 1 .. 63, temperature
 * not finite or <= 0, n_edges * n_neg >= 2^31 - 1, a null pointer, both or neither form of the
 * negatives.  HGNN_E_UNSUPPORTED: fp32 d > 512, bf16 d % 8 != 0 or d > 512.  All before any
 * launch.  Two runs are bitwise equal. */
int hgnn_edge_softmax_fwd(int32_t rows, const void* U, const void* P, int32_t d, int64_t n_users,
                          int64_t n_posts, const int32_t* rowptr_u, const int32_t* col_u,
                          const float* edge_w, const int64_t* neg_i64, const int32_t* neg_i32,
                          int32_t n_neg, int64_t n_edges, const float* cscale,
                          const float* post_bias, float temperature, const int32_t* slot_of,
                          float* dU, float* coef_pos, float* coef_neg, float* part, float* loss,
                          int32_t* err, hgnn_stream_t stream);
/* The positions of a user a wave takes per chunk at n_neg negatives (0: n_neg out of range):
 * min(64, 640 / ((n_neg + 1) | 1)), the kernel parking a chunk's ids and logits in per-wave LDS at
 * [position][column] with an odd stride, as hgnn_hard_negatives does. */
int32_t hgnn_softmax_chunk(int32_t n_neg);
/* floats of hgnn_edge_softmax_fwd's `part` scratch for n_users users */
int64_t hgnn_softmax_parts(int64_t n_users);

/* dP of the softmax loss: out[r] = sum_{p in [rowptr[r], rowptr[r+1])} coef_pos[p] x[col[p]]
 *                                + sum_{q in [rowptr_n[r], rowptr_n[r+1])} coef_neg[q] x[col_n[q]]
 * hgnn_score_gather2_planned's two lists per output row, its chunk / slab / fix-up plan for both
 * (the positives' static plan; the negatives' made by hgnn_plan_device from rowptr_n with the same
 * chunk, neg_slab holding 2 * neg_max_heavy rows of d floats) and its three formats of x (rows:
 * HGNN_ROWS_*), with each pair's weight read at its position in its list instead of recomputed:
 * coef_neg is the scoring pass's coef_neg carried through the negatives' sort as its second
 * payload.  No rowvec, no cscale, no offsets: it reads no P rows.  Written: out (every row once),
 * the two slabs.  Sums run in the lists' stable order; two runs are bitwise equal.
 * HGNN_E_ARG: rows out of range, d <= 0 or another bad size, a null rowptr / rowptr_n / out, a
 * plan without its arrays.  HGNN_E_UNSUPPORTED: a width the format does not take (bf16: d % 8 == 0
 * and d <= 1024; zero-packed: 64 or 128; fp32: d <= 1024).  All before any launch. */
int hgnn_coef_gather2_planned(int32_t rows, const void* x, int64_t n_x, int32_t d,
                              const int32_t* rowptr, const int32_t* col, const float* coef_pos,
                              const int32_t* rowptr_n, const int32_t* col_n,
                              const float* coef_neg, int64_t n_rows, const int32_t* heavy_rows,
                              const int32_t* heavy_first, int64_t n_heavy, int64_t n_chunks,
                              int32_t chunk, float* slab, const int32_t* neg_heavy_rows,
                              const int32_t* neg_heavy_first, const int32_t* d_neg_counts2,
                              int64_t neg_max_heavy, float* neg_slab, float* out,
                              hgnn_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* HGNN_H_ */
