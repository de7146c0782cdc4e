/* clipx.h — C ABI of libclipx_hip.so: the MI355X (gfx950) kernels behind the CLIP
 * train-step hot path of lezhang7/colxlip.
 *
 * The reference is pure Python over PyTorch ATen ops; it has no FFI of its own
 * (SURVEY.md §8b).  Each entry point below replaces the ATen call(s) the reference
 * issues at the cited file:line (paths relative to reference src/colxlip/).  All
 * pointers are DEVICE pointers borrowed for the duration of one enqueue; nothing is
 * retained or freed.  `stream` is a hipStream_t (0 = default stream).  Every function
 * only enqueues work (no sync, no allocation) and returns 0, or a negative code with
 * a message readable through clipx_last_error() (thread-local).
 *
 * dtype: activation / GEMM-operand element type of the call.
 *   CLIPX_F32  — parity mode, every operand fp32 (exact-f32 MFMA).
 *   CLIPX_BF16 — performance mode, bf16 operands, fp32 accumulation and statistics.
 * Biases, LayerNorm gains/biases, statistics, gradients of parameters and the loss
 * path are always fp32.
 */
#ifndef CLIPX_H
#define CLIPX_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { CLIPX_F32 = 0, CLIPX_BF16 = 1 };
enum { CLIPX_ACT_NONE = 0, CLIPX_ACT_GELU = 1, CLIPX_ACT_QUICKGELU = 2 };

const char* clipx_last_error(void);
int clipx_version(void);

/* ---- linear layers: nn.Linear / F.linear / `@ proj` --------------------------------
 * fwd   transformer.py:236-238 (mlp), nn.MultiheadAttention in/out proj :228,253-255,
 *       `pooled @ self.proj` :831, `pooled @ self.text_projection` :1096,
 *       conv1 as a patch GEMM :549-555,702.
 *   y[M,N] = act(x[M,K] . w[N,K]^T + bias[N]) (+ residual[M,N]);  if u_out != NULL the
 *   pre-activation is stored there too (needed by the GELU backward).
 *   y_dtype may be CLIPX_F32 to get fp32 output from bf16 operands.                  */
int clipx_linear_fwd(int dtype, int M, int N, int K, const void* x, const void* w,
                     const float* bias, int act, void* u_out, const void* residual,
                     void* y, int y_dtype, void* stream);
/* dgrad (autograd of the above): dx[M,K] = dy[M,N] . w[N,K]; bf16 mode reads the
 * K-major copy wt[K,N] instead (w may be NULL).  If act != NONE: dx *= act'(u[M,K]).
 * dy_dtype: CLIPX_F32 allowed only in f32 mode.                                        */
int clipx_linear_dgrad(int dtype, int M, int N, int K, const void* dy, const void* w,
                       const void* wt, int act, const void* u, void* dx, void* stream);
/* wgrad: dw[N,K] (fp32) = beta*dw + dy[M,N]^T . x[M,K]; when db != NULL also the bias
 * gradient db[N] = beta_b*db + sum_m dy[m,n] from the same pass over dy.  ws: scratch
 * (256-B aligned) for split-M partial slabs and bias partials; ws_bytes may be 0 when
 * db == NULL (no split).                                                                */
int clipx_linear_wgrad(int dtype, int M, int N, int K, const void* dy, const void* x,
                       float* dw, float beta, float* db, float beta_b,
                       void* ws, size_t ws_bytes, void* stream);
/* Up to four wgrads that reduce over the SAME M rows in one call -- the four linear layers of a residual block
 * (reference transformer.py:213-268: in_proj, out_proj, c_fc, c_proj; their weight gradients are what autograd's
 * MultiheadAttention / Linear backward produce one by one).  bf16: ONE grid for all of them (fewer row splits, a fraction of the
 * fp32 slab traffic, see csrc/gemm_bf16_tn.hip); where the grouped kernel does not apply, and in f32, the problems run one by
 * one -- same results contract as clipx_linear_wgrad.  Host arrays of `nprob` entries; db[i] may be NULL.  `ws` must hold
 * clipx_linear_wgrad_group_ws_bytes(...) bytes, 256-B aligned.                                                              */
size_t clipx_linear_wgrad_group_ws_bytes(int dtype, int M, int nprob, const int* N, const int* K);
int clipx_linear_wgrad_group(int dtype, int M, int nprob, const int* N, const int* K, const void* const* dy,
                             const void* const* x, float* const* dw, const float* beta, float* const* db,
                             const float* beta_b, void* ws, size_t ws_bytes, void* stream);
size_t clipx_linear_wgrad_ws_bytes(int dtype, int M, int N, int K);
/* column sums (bias gradients): out[N] = beta*out + sum_m a[m,n].                      */
int clipx_colsum(int dtype, int M, int N, const void* a, float* out, float beta,
                 void* ws, size_t ws_bytes, void* stream);
size_t clipx_colsum_ws_bytes(int M, int N);
/* backward of the MLP activation (nn.GELU / QuickGELU, transformer.py:237) fused with the c_fc bias gradient:
 * du[m,n] = dh[m,n] * act'(u[m,n]) (du may alias dh or u); colsum[n] = beta*colsum[n] + sum_m du[m,n].
 * ws as for clipx_colsum.                                                                  */
int clipx_act_bwd_colsum(int dtype, int M, int N, int act, const void* dh, const void* u, void* du,
                         float* colsum, float beta, void* ws, size_t ws_bytes, void* stream);

/* generic fp32 GEMM with element strides (loss path, loss.py:145-152 and its autograd):
 *   C[m,n] = alpha * sum_k A[m*a_rs + k*a_cs] * B[k*b_rs + n*b_cs] + beta * C[m,n]       */
int clipx_gemm_f32(int M, int N, int K, const float* A, long a_rs, long a_cs,
                   const float* B, long b_rs, long b_cs, float* C, long ldc,
                   float alpha, float beta, void* stream);

/* ---- LayerNorm: transformer.py:14-29 (eps 1e-5, fp32 statistics) --------------------
 * row r of the output reads input row (row_index ? row_index[r] : r).                   */
int clipx_layernorm_fwd(int dtype, int rows, int width, const void* x, const int* row_index,
                        const float* gamma, const float* beta, float eps, void* y,
                        float* mean, float* rstd, void* stream);
/* dx_out[row] = (dx_res ? dx_res[row] : 0) + LN'(dy); row mapping as in fwd (scatter).
 * partial sums of dgamma, dbeta and of dx_out columns go to ws; clipx_layernorm_bwd_finish
 * folds them: dgamma = beta_acc*dgamma + sum, same for dbeta, colsum (either may be NULL). */
int clipx_layernorm_bwd(int dtype, int rows, int width, const void* dy, const void* x,
                        const int* row_index, const float* gamma, const float* mean,
                        const float* rstd, const void* dx_res, void* dx_out,
                        float* ws, size_t ws_bytes, void* stream);
int clipx_layernorm_bwd_finish(int width, const float* ws, float* dgamma, float* dbeta,
                               float* colsum, float beta_acc, void* stream);
size_t clipx_layernorm_ws_bytes(int width);

/* ---- attention core of nn.MultiheadAttention (transformer.py:253-255): -------------
 * qkv[b*L, 3*heads*hd] packed q|k|v, out[b*L, heads*hd]; softmax(q k^T / sqrt(hd) + mask) v
 * with mask = -inf above the diagonal when causal (transformer.py:960-966).             */
int clipx_attention_fwd(int dtype, int batch, int L, int heads, int hd, int causal,
                        const void* qkv, void* out, void* stream);
int clipx_attention_bwd(int dtype, int batch, int L, int heads, int hd, int causal,
                        const void* qkv, const void* dout, void* dqkv, void* stream);
/* The same pair with the softmax statistic handed over, as flash attention does (the ATen call site is the same
 * scaled_dot_product_attention inside nn.MultiheadAttention, transformer.py:253-255; torch's flash backend saves `logsumexp`
 * for its backward in the same way): lse[batch*heads, L] fp32 = log2-domain log-sum-exp of the scaled scores of every query,
 * written by the forward; the backward takes it together with the forward's output and derives delta = rowsum(dout * out)
 * instead of making an extra sweep over the keys.  Available (clipx_attention_lse_supported == 1) for the shapes that run on the
 * online-softmax kernels: bf16, head dim 64 with 129 <= L <= 608 (ViT-B/16, ViT-L/14-336) or head dim 80 with L <= 288 (ViT-H/14).     */
int clipx_attention_lse_supported(int dtype, int L, int hd);
int clipx_attention_fwd_lse(int dtype, int batch, int L, int heads, int hd, int causal,
                            const void* qkv, void* out, float* lse, void* stream);
int clipx_attention_bwd_lse(int dtype, int batch, int L, int heads, int hd, int causal,
                            const void* qkv, const void* dout, const void* out, const float* lse, void* dqkv, void* stream);

/* packed rows (sequences of different lengths stored back to back, see clipx_text_layout): block i works on sequence
 * seq_ids[i] (i when seq_ids == NULL), rows cu_rows[s] .. cu_rows[s+1]-1 of qkv / out.  max_len >= every sequence of the
 * launch; it selects the kernel's tile count, so a caller launches once per length bucket.  bf16: head dim 64, max_len <= 128;
 * f32: head dim 32/64/80 with the sequence resident in LDS.  Same arithmetic as clipx_attention_fwd/bwd per sequence.     */
int clipx_attention_packed_fwd(int dtype, int nseq, int max_len, int heads, int hd, int causal, const int* seq_ids,
                               const int* cu_rows, const void* qkv, void* out, void* stream);
int clipx_attention_packed_bwd(int dtype, int nseq, int max_len, int heads, int hd, int causal, const int* seq_ids,
                               const int* cu_rows, const void* qkv, const void* dout, void* dqkv, void* stream);

/* Attention of ONE query row per sequence: the last residual block of a tower whose output is read at the pooled position only
 * (reference transformer.py:757-783 `_pool`, 839-855 text_global_pool; the block itself is transformer.py:253-255).  Replaces
 * clipx_attention_fwd + a gather of row idx[s] / a scatter + clipx_attention_bwd with O(L d) work per sequence and head.
 * Sequences: rows s*L .. s*L+L-1 of qkv (cu_rows == NULL) or cu_rows[s] .. cu_rows[s+1]-1; idx[s] = absolute row of the pooled
 * query; causal: keys up to and including that row.  out[nseq, heads*hd]; lse[nseq*heads] (log2 domain) goes to the backward;
 * dqkv: every row of the nseq sequences is written (zeros in the query part of all rows but idx[s]).  bf16, head dim 64 / 80,
 * max_len (>= every sequence) <= 640 / 320: clipx_attention_pooled_supported.                                                  */
int clipx_attention_pooled_supported(int dtype, int max_len, int hd);
int clipx_attention_pooled_fwd(int dtype, int nseq, int L, int max_len, int heads, int hd, int causal, const void* qkv,
                               const int* idx, const int* cu_rows, void* out, float* lse, void* stream);
int clipx_attention_pooled_bwd(int dtype, int nseq, int L, int max_len, int heads, int hd, int causal, const void* qkv,
                               const void* dout, const float* lse, const int* idx, const int* cu_rows, void* dqkv, void* stream);
/* The same when the caller ran the block's in_proj as two GEMMs (nn.MultiheadAttention's packed in_proj_weight rows [0, d) = q,
 * [d, 3d) = k | v: torch/nn/functional.py `_in_projection_packed`): q [nseq, heads*hd] = the query of each sequence's pooled row
 * (row s), kv [rows, 2*heads*hd] = k | v of every row; backward: dq [nseq, heads*hd], dkv [rows, 2*heads*hd].                     */
int clipx_attention_pooled_fwd_split(int dtype, int nseq, int L, int max_len, int heads, int hd, int causal, const void* q,
                                     const void* kv, const int* idx, const int* cu_rows, void* out, float* lse, void* stream);
int clipx_attention_pooled_bwd_split(int dtype, int nseq, int L, int max_len, int heads, int hd, int causal, const void* q,
                                     const void* kv, const void* dout, const float* lse, const int* idx, const int* cu_rows,
                                     void* dq, void* dkv, void* stream);

/* ---- embeddings ----------------------------------------------------------------------
 * patchify: image[b,3,H,W] (img_dtype) -> patches[b*G*G, Kp] (dtype), inner order (c,py,px),
 * columns >= 3*P*P zero-filled (Kp >= 3*P*P; conv1 as GEMM, transformer.py:702-704).     */
int clipx_patchify(int img_dtype, int dtype, int batch, int H, int W, int P, int Kp,
                   const void* image, void* patches, void* stream);
/* ---- image input transform (factory.py:411-418 builds open_clip's image_transform_v2 for train and val: torchvision
 * RandomResizedCrop | Resize + CenterCrop, ToTensor, Normalize on PIL images; the datasets decode with PIL, data.py:732).
 * bytes: `nbytes` of uint8 HWC RGB images, stored back to back at any offsets.  meta: `batch` records of 48 bytes,
 *   { int64 offset; int32 h, w, top, left, bh, bw, vh, vw, oy, ox }: image i is bytes[offset, offset + 3*h*w), its source box
 *   rows top .. top+bh, columns left .. left+bw; (vh, vw) the virtual output size; (oy, ox) the origin of the H x W window of it
 *   (where the window reaches past the virtual output, out is left untouched).
 * out[i, c, y, x] (out_dtype, contiguous NCHW) = (level / 255 - mean[c]) / std[c], level = the pixel (oy + y, ox + x), channel c,
 *   of PIL's Image.resize((vw, vh), BICUBIC if bicubic else BILINEAR) of the boxed region: horizontal pass, round half up and
 *   clamp to [0, 255], vertical pass, round and clamp, in PIL's 22-bit fixed point (csrc/image_transform.hip).  Train: box = the random crop,
 *   (vh, vw) = (H, W), origin 0.  Val: box = the image, (vh, vw) = the resized size, window = the centre crop.
 * Per axis box / virtual size <= 16.  No byte outside an image's [offset, offset + 3*h*w) is read: the box is clamped to the
 *   image, and a record that breaks a limit leaves its image's output untouched (callers validate first: ops.image_geometry). */
int clipx_image_transform(int batch, const void* bytes, size_t nbytes, const void* meta, int H, int W, float mean0,
                          float mean1, float mean2, float std0, float std1, float std2, int bicubic, int out_dtype,
                          void* out, void* stream);
/* x0[b, 0] = cls + pos[0]; x0[b, 1+g] = tok[b*G2+g] + pos[1+g]  (transformer.py:707-709)  */
int clipx_vision_assemble(int dtype, int batch, int tokens, int width, const void* tok,
                          const float* cls, const float* pos, void* x0, void* stream);
/* backward: dtok[b*G2+g] = dx0[b,1+g]; dpos[l] = beta*dpos[l] + sum_b dx0[b,l];
 * dcls = beta*dcls + sum_b dx0[b,0].  ws: clipx_vision_assemble_bwd_ws_bytes() bytes (partial sums over batch parts,
 * added in a fixed order: the same result every run).                                  */
size_t clipx_vision_assemble_bwd_ws_bytes(int tokens, int width);
int clipx_vision_assemble_bwd(int dtype, int batch, int tokens, int width, const void* dx0,
                              void* dtok, float* dpos, float* dcls, float beta, float* ws, size_t ws_bytes, void* stream);
/* ---- patch dropout (PatchDropout, transformer.py:48-88, applied before ln_pre at :712): while training, each image keeps
 * `keep` = max(1, int(G2 * (1 - prob))) of its G2 patch tokens (:76-77); the tower runs on 1 + keep rows per image.
 * keep_idx: int32 [batch, keep] of patch positions in [0, G2), distinct within a row; no kernel assumes it sorted.
 * keep_index: the mask drawn on the device (replaces `torch.randn(batch, G2).topk(keep)`, :79-80): `keep` distinct positions
 * per sample, uniform without replacement, ascending, a function of (key, sample) only.  G2 <= 1024.                        */
int clipx_patch_keep_index(int batch, int G2, int keep, uint64_t key, int* keep_idx, void* stream);
/* patches[b*keep + j, Kp] = row b*G2 + keep_idx[b, j] of clipx_patchify (the same bits): the patch-embed GEMM input of the
 * kept patches only (conv1 as GEMM, transformer.py:702-704, followed by the gather x[batch_indices, patch_indices_keep] :82). */
int clipx_patchify_keep(int img_dtype, int dtype, int batch, int H, int W, int P, int Kp, int keep,
                        const int* keep_idx, const void* image, void* patches, void* stream);
/* x0[b, 0] = cls + pos[0]; x0[b, 1+j] = tok[b*keep+j] + pos[1 + keep_idx[b, j]]  (transformer.py:707-712 with :82-85): the
 * kept rows of clipx_vision_assemble, bit for bit.                                                                          */
int clipx_vision_assemble_keep(int dtype, int batch, int keep, int G2, int width, const void* tok,
                               const float* cls, const float* pos, const int* keep_idx, void* x0, void* stream);
/* backward: dtok[b*keep+j] = dx0[b, 1+j]; dpos[0] = beta*dpos[0] + sum_b dx0[b, 0], dcls likewise;
 * dpos[1+p] = beta*dpos[1+p] + sum over (b, j) with keep_idx[b, j] = p of dx0[b, 1+j] (beta*dpos exactly where no sample kept
 * p).  Partial sums over batch parts added in a fixed order: the same result every run.
 * ws: clipx_vision_assemble_keep_bwd_ws_bytes() bytes.                                                                       */
size_t clipx_vision_assemble_keep_bwd_ws_bytes(int G2, int width);
int clipx_vision_assemble_keep_bwd(int dtype, int batch, int keep, int G2, int width, const void* dx0, const int* keep_idx,
                                   void* dtok, float* dpos, float* dcls, float beta, float* ws, size_t ws_bytes, void* stream);
/* x0[b,l] = table[text[b,l]] + pos[l]   (transformer.py:980,988; text int64)             */
int clipx_text_embed(int dtype, int batch, int L, int width, int vocab, const int64_t* text,
                     const float* table, const float* pos, void* x0, void* stream);
/* dtable[text[b,l]] += dx0[b,l] (finite contributions below 16 in magnitude are summed in 64-bit fixed point, exact for
 * |v| >= 2^-40 at 176k rows, and rounded to fp32 once; others, NaN / inf included, are added in fp32; all-zero rows skipped);
 * dpos[l] = beta*dpos[l] + sum_b dx0[b,l].  dtable must already hold beta*dtable.  Both the same every run.
 * ws: clipx_text_embed_bwd_ws_bytes() bytes of scratch.                                  */
size_t clipx_text_embed_bwd_ws_bytes(int L, int width, int vocab);
int clipx_text_embed_bwd(int dtype, int batch, int L, int width, int vocab, const int64_t* text,
                         const void* dx0, float* dtable, float* dpos, float beta, void* ws, size_t ws_bytes, void* stream);
/* ---- row gather / scatter: only the pooled token of each sample leaves the last residual block (`x[:, 0]` transformer.py:695,
 * `x[arange, text.argmax(-1)]` :851), so the block's out_proj / MLP and their backward run on `batch` rows.
 * gather: dst[r] = src[row_index[r]];  scatter: dst (dst_rows x width) = 0 then dst[row_index[r]] = src[r], or with
 * accumulate != 0: dst[row_index[r]] += src[r] (dst untouched elsewhere; row_index entries are distinct).                */
int clipx_gather_rows(int dtype, int rows, int width, const void* src, const int* row_index, void* dst, void* stream);
int clipx_scatter_rows(int dtype, long dst_rows, int rows, int width, const void* src, const int* row_index, void* dst,
                       int accumulate, void* stream);

/* ---- packed text rows: the causal text tower only needs positions 0..EOT of each caption (transformer.py:839-855 pools
 * the EOT row, :960-966 masks everything behind a position): rows behind the EOT neither reach the loss nor receive a
 * gradient.  clipx_text_layout builds the packed layout on the device:
 *   header[8] : R live rows, Rp rows incl. filler sequences (Rp % row_align == 0), nseq = batch + fillers,
 *               #sequences of length <= 32 / <= 64 / longer, longest sequence, 0
 *   cu[nseq+1]: first row of each sequence; order[nseq]: sequence ids sorted (stably) by those three length classes
 *   row_tok[Rp], row_pos[Rp]: token id and position of every packed row (fillers: token 0)
 * Buffers must hold batch + 64 sequences and batch*L + row_align rows.  batch <= 8192.                                   */
int clipx_text_layout(int batch, int L, int vocab, int row_align, const int64_t* text, int* header, int* cu,
                      int* order, int* row_tok, int* row_pos, void* stream);
/* x0[r] = table[row_tok[r]] + pos[row_pos[r]]  (transformer.py:980,988 on the packed rows)                               */
int clipx_text_embed_packed(int dtype, int rows, int width, const int* row_tok, const int* row_pos,
                            const float* table, const float* pos, void* x0, void* stream);
/* dtable[row_tok[r]] += dx0[r] (summed like clipx_text_embed_bwd; zero rows skipped; dtable holds
 * beta*dtable already); dpos[t] = beta*dpos[t] + sum_{s: len_s > t} dx0[cu[s] + t].  Both the same every run.
 * ws: clipx_text_embed_packed_bwd_ws_bytes() bytes of scratch.                                                            */
size_t clipx_text_embed_packed_bwd_ws_bytes(int L, int width, int vocab);
int clipx_text_embed_packed_bwd(int dtype, int rows, int nseq, int L, int width, int vocab, const int* row_tok,
                                const int* cu, const void* dx0, float* dtable, float* dpos, float beta, void* ws,
                                size_t ws_bytes, void* stream);
/* idx[s] = cu[s+1] - 1: the EOT (pooled) row of caption s in the packed layout                                            */
int clipx_packed_eot_index(int batch, const int* cu, int* idx, void* stream);
/* idx[b] = b*L + argmax_l text[b,l] (first maximum; transformer.py:851)                  */
int clipx_eot_index(int batch, int L, const int64_t* text, int* idx, void* stream);
/* idx[b] = b*stride (CLS rows, transformer.py:695)                                       */
int clipx_stride_index(int batch, int stride, int* idx, void* stream);

/* ---- F.normalize(dim=-1, eps 1e-12) (model.py:552,606) -------------------------------- */
int clipx_l2norm_fwd(int rows, int width, const float* x, float* y, float* inv_norm, void* stream);
int clipx_l2norm_bwd(int rows, int width, const float* dy, const float* y, const float* inv_norm,
                     float* dx, void* stream);

/* ---- ClipLoss pieces (loss.py:119-130,175-180): symmetric softmax cross-entropy --------
 * ce_rows: lse[r] = logsumexp_j z[r,j]; loss_acc += weight * sum_r (lse[r] - z[r, r+label_off])
 * ce_cols: same over columns (labels: column c matches row c).                            */
int clipx_ce_rows(int rows, int cols, const float* z, long ldz, int label_off, float* lse,
                  float weight, float* loss_acc, void* stream);
int clipx_ce_cols(int rows, int cols, const float* z, long ldz, float* lse,
                  float weight, float* loss_acc, void* stream);
/* in place z -> dz = w_row*(exp(z - lse_row[r]) - [c == r+label_off])
 *                  + w_col*(exp(z - lse_col[c]) - [c == r+col_label_off])   (lse_col may be NULL; col_label_off != 0: the rows are
 *                    one rank's block of a taller matrix and lse_col its columns' log-sum-exps over ALL ranks' rows);
 * dscale_acc += sum(dz * z) / *scale_dev   (scale_dev: the device scalar logit_scale.exp()). */
int clipx_ce_grad(int rows, int cols, float* z, long ldz, int label_off, const float* lse_row,
                  float w_row, const float* lse_col, float w_col, int col_label_off, const float* scale_dev,
                  float* dscale_acc, void* stream);
/* ---- the same loss WITHOUT the logits matrix in memory (loss.py:145-152,175-180; tall-skinny exact-fp32 MFMA GEMM with
 * the softmax statistics in its epilogue).  z[p,q] = sum_e P[p,e]*Q[q,e], P = logit_scale * own features [np,E], Q the
 * other side's [nq,E].  fwd: lse_own[p] = logsumexp_q z[p,q]; loss_acc += w_own * sum_p (lse_own[p] - z[p, p+label_off]);
 * symmetric (np == nq, label_off == 0) also lse_oth[q] = logsumexp_p z[p,q], loss_acc += w_oth * sum_q (lse_oth[q] - z[q,q]).
 * ws: clipx_ce_fused_ws_bytes() bytes of scratch (per-tile partials: O(np*nq/64)).                                       */
size_t clipx_ce_fused_ws_bytes(int np, int nq, int symmetric);
int clipx_ce_fused_fwd(int np, int nq, int E, const float* P, const float* Q, int label_off, int symmetric,
                       float w_own, float w_oth, float* lse_own, float* lse_oth, float* loss_acc, void* ws,
                       size_t ws_bytes, void* stream);
/* bwd of one operand, logits recomputed tile by tile:  dP[p,:] = osc * sum_q dz(p,q) * Q[q,:],
 * ws: clipx_ce_fused_bwd_ws_bytes() bytes (partials of the blocks that split the q walk, summed in a fixed order),
 *   dz(p,q) = w_own*(exp(z - lse_own[p]) - [q == p+off_own]) + w_oth*(exp(z - lse_oth[q]) - [p == q+off_oth])
 * (a NULL lse pointer drops its term), osc = out_scale_mul * (*out_scale_dev if given) * (*gout_dev if given);
 * dscale_acc (optional) += sum dz*z / *scale_dev.  E in {16,32,64,128,256,512,640,768,1024}.                             */
size_t clipx_ce_fused_bwd_ws_bytes(int np, int nq, int E);
int clipx_ce_fused_bwd(int np, int nq, int E, const float* P, const float* Q, const float* lse_own, float w_own,
                       int off_own, const float* lse_oth, float w_oth, int off_oth, const float* out_scale_dev,
                       float out_scale_mul, const float* gout_dev, float* dP, float* dscale_acc,
                       const float* scale_dev, void* ws, size_t ws_bytes, void* stream);
/* ---- SigLipLoss (loss.py:498-521): sigmoid contrastive loss WITHOUT the logits matrix in memory (exact-fp32 MFMA tiles).
 *   z[i,j] = s*(A[i].B[j]) + beta, s = *scale_dev, beta = *bias_dev, A [r,E], B [c,E];
 *   y = +1 where j == i + pos_off, -1 elsewhere (pos_off < 0: negatives only, loss.py:489-493);
 *   loss = inv_r * sum softplus(-y z) (loss.py:508-516);  dz = -inv_r * y * sigmoid(-y z).
 * fused_fwd: out3 = [loss, sum dz*(A.B), sum dz] (d(scale), d(bias) at unit upstream gradient);
 *   dA = s * dz @ B (NULL: a loss-only walk, out3[1..2] = 0); accumulate != 0 adds to out3 and dA.  ws: clipx_sigmoid_fused_ws_bytes(r, c, E, dA != NULL) bytes.
 * fused_bwd: dB (+)= s * (*gout_dev if given) * dz^T @ A  (accumulate != 0 adds to dB).  ws: clipx_sigmoid_fused_bwd_ws_bytes().
 * Block and split partials are summed in a fixed order.  E in {16,32,64,128,256,512,640,768,1024}.                       */
size_t clipx_sigmoid_fused_ws_bytes(int r, int c, int E, int grad);
int clipx_sigmoid_fused_fwd(int r, int c, int E, const float* A, const float* B, const float* scale_dev,
                            const float* bias_dev, int pos_off, float inv_r, float* out3, float* dA, int accumulate,
                            void* ws, size_t ws_bytes, void* stream);
size_t clipx_sigmoid_fused_bwd_ws_bytes(int r, int c, int E);
int clipx_sigmoid_fused_bwd(int r, int c, int E, const float* A, const float* B, const float* scale_dev,
                            const float* bias_dev, int pos_off, float inv_r, const float* gout_dev, float* dB,
                            int accumulate, void* ws, size_t ws_bytes, void* stream);
/* the same on a materialised dot matrix z[rows, cols] = A @ B^T (any embed dim): in place z -> dz,
 * out3 = [loss, sum dz*z_in, sum dz].  ws: clipx_sigmoid_dense_ws_bytes() bytes.                                         */
size_t clipx_sigmoid_dense_ws_bytes(int rows, int cols);
int clipx_sigmoid_dense(int rows, int cols, float* z, long ldz, const float* scale_dev, const float* bias_dev,
                        int pos_off, float inv_r, float* out3, void* ws, size_t ws_bytes, void* stream);
/* ---- DistillClipLoss (loss.py:343-379): contrastive + distillation cross-entropy WITHOUT a logits matrix in memory
 * (exact-fp32 MFMA tiles).  Student s[p,q] = P[p].Q[q] (P = logit_scale * own features [np,Es], Q [nq,Es]); teacher
 * t[p,q] = TP[p].TQ[q] (TP = dist_logit_scale * own teacher features [np,Et], TQ [nq,Et]).
 * fused_fwd (loss.py:343-345,359-373): per row stats_own[3][np] = (lse_s, lse_t, X = sum_q softmax(t)*s);
 *   loss2[0] += w_own * sum_p (lse_s - s[p, p+label_off]),  loss2[1] += w_own * sum_p (lse_s - X);
 *   symmetric (np == nq, label_off == 0) also the same over columns into stats_oth[3][nq] with w_oth.
 *   ws: clipx_distill_fused_ws_bytes() bytes (per-tile partials: O(np*nq/64)).                                            */
size_t clipx_distill_fused_ws_bytes(int np, int nq, int symmetric);
int clipx_distill_fused_fwd(int np, int nq, int Es, int Et, const float* P, const float* Q, const float* TP, const float* TQ,
                            int label_off, int symmetric, float w_own, float w_oth, float* stats_own, float* stats_oth,
                            float* loss2, void* ws, size_t ws_bytes, void* stream);
/* fused_bwd (loss.py:343-379) of one student operand, both tiles recomputed:  dP[p,:] = osc * sum_q ds(p,q) * Q[q,:],
 *   ds = w_own*(g_c*(sigma_own - [q == p+off_own]) + g_d*(sigma_own - pi_own))
 *      + w_oth*(g_c*(sigma_oth - [p == q+off_oth]) + g_d*(sigma_oth - pi_oth)),
 *   sigma / pi: student / teacher softmax from the stats of fused_fwd (a NULL stats pointer drops its term);
 *   g_c = *gc_dev, g_d = *gd_dev (the upstream gradients of the two losses); osc = *out_scale_dev (NULL: 1);
 *   dscale_acc (optional) += sum ds*s / *scale_dev.  ws: clipx_distill_fused_bwd_ws_bytes() bytes.
 *   Es, Et in {16,32,64,128,256,512,640,768,1024}.                                                                          */
size_t clipx_distill_fused_bwd_ws_bytes(int np, int nq, int Es);
int clipx_distill_fused_bwd(int np, int nq, int Es, int Et, const float* P, const float* Q, const float* TP, const float* TQ,
                            const float* stats_own, float w_own, int off_own, const float* stats_oth, float w_oth,
                            int off_oth, const float* gc_dev, const float* gd_dev, const float* out_scale_dev, float* dP,
                            float* dscale_acc, const float* scale_dev, void* ws, size_t ws_bytes, void* stream);
/* the same on materialised logits s, t [rows, cols] (any embed dims; loss.py:343-379).  dense_fwd: stats and loss2 as
 *   fused_fwd (the rows always, the columns when symmetric).  dense_grad: in place s -> ds and (want_dt) t -> dt,
 *   dt = -sum_dir w * g_d * pi * (s - X);  dscales2 (optional) += [sum ds*s / *scale_dev, sum dt*t / *tscale_dev]
 *   (a NULL tscale_dev leaves dscales2[1]).  ws: clipx_distill_dense_ws_bytes() bytes.                                     */
size_t clipx_distill_dense_ws_bytes(int rows, int cols);
int clipx_distill_dense_fwd(int rows, int cols, const float* s, long lds, const float* t, long ldt, int label_off,
                            int symmetric, float w_row, float w_col, float* stats_row, float* stats_col, float* loss2,
                            void* ws, size_t ws_bytes, void* stream);
int clipx_distill_dense_grad(int rows, int cols, float* s, long lds, float* t, long ldt, int label_off,
                             const float* stats_row, float w_row, const float* stats_col, float w_col, const float* gc_dev,
                             const float* gd_dev, int want_dt, const float* scale_dev, const float* tscale_dev,
                             float* dscales2, void* ws, size_t ws_bytes, void* stream);
/* out[i] = x[i] * (*s_dev): `logit_scale * image_features` with the scale left on the device
 * (loss.py:145-152 multiplies the features first, then takes the matmul).                    */
int clipx_scale_by_dev(size_t n, const float* x, const float* s_dev, float* out, void* stream);

/* ---- parameter-side kernels -------------------------------------------------------------
 * cast fp32 master weights to bf16 operand copies: w16[n,k] and (optional) wt16[k,n].     */
int clipx_cast_weight(int N, int K, const float* w, void* w16, void* wt16, void* stream);
/* fp8 weights (BASELINE.json config 5; not in the reference, which picks operand precision at factory.py:290-313):
 * row_exp[n] = ceil(log2(max_k |w[n,k]| / 448)); w8[n,k] = OCP e4m3fn(w[n,k] * 2^-row_exp[n]) (optional);
 * w16[n,k] / wt16[k,n] (optional) = the dequantised values, exact in bf16 -- the operands the MFMA kernels read.        */
int clipx_quant_weight_e4m3(int N, int K, const float* w, int* row_exp, void* w8, void* w16, void* wt16, void* stream);
/* fp8 x fp8 forward linear on the CDNA4 fp8 MFMA (v_mfma_f32_16x16x128_f8f6f4, twice the bf16 rate):
 *   clipx_quant_rows_e4m3: x[M,K] (bf16) -> x8[M,K] e4m3 bytes + row_exp[M] (the weight rule, per activation row; K % 8 == 0, <= 8192)
 *   clipx_linear_fwd_fp8:  y[M,N] (bf16) = act(2^(x_exp[m] + w_exp[n]) * sum_k x8[m,k] w8[n,k] + bias) (+ residual), products
 *                          exact, sums fp32; u_out (optional) = the pre-activation; K % 128 == 0, N % 8 == 0.                  */
int clipx_quant_rows_e4m3(int M, int K, const void* x, int* row_exp, void* x8, void* stream);
/* LayerNorm forward (bf16, width % 256 == 0, <= 1280) that also emits the rows in that e4m3 form -- bit-identical to
 * clipx_quant_rows_e4m3 of its bf16 output, without the extra pass.                                                           */
int clipx_layernorm_fwd_q8(int rows, int width, const void* x, const float* gamma, const float* beta, float eps, void* y,
                           float* mean, float* rstd, void* y8, int* y_exp, void* stream);
int clipx_linear_fwd_fp8(int M, int N, int K, const void* x8, const int* x_exp, const void* w8, const int* w_exp,
                         const float* bias, int act, void* u_out, const void* residual, void* y, void* stream);
/* dgrad on the same kernel: dx[M,K] (bf16) = 2^(dy_exp[m] + wt_exp[k]) * sum_n dy8[m,n] wt8[k,n] (* act'(u[m,k]) when act != 0);
 * dy8 / wt8 = clipx_quant_rows_e4m3 of the gradient rows and of the [K,N] weight copy; N % 128 == 0, K % 8 == 0.            */
int clipx_linear_dgrad_fp8(int M, int N, int K, const void* dy8, const int* dy_exp, const void* wt8, const int* wt_exp,
                           int act, const void* u, void* dx, void* stream);
/* clipx_quant_weight_e4m3 (+ clipx_quant_rows_e4m3 of the [K,N] copy when wt8 is given) for MANY weights in three launches.
 * descs: device array of ntensors records { const float* w; uint8* w8; bf16* w16; bf16* wt16; uint8* wt8 (or null); int32* rexp;
 * int32* wtexp; int32 N; int32 K; uint32 b0_rows; uint32 b0_tiles; uint32 b0_trows; uint32 tiles_k } (80 bytes) with the running
 * block offsets of the three kernels: rows ceil(N/4), tiles ceil(N/32)*ceil(K/32), transposed rows ceil(K/4).                */
int clipx_quant_weight_multi(const void* descs, int ntensors, int blocks_rows, int blocks_tiles, int blocks_trows, void* stream);
/* the same for many weights in ONE launch.  descs: device array of ntensors records
 * { const float* w; bf16* w16; bf16* wt16; int32 N; int32 K; uint32 block0; uint32 tiles_k } (40 bytes), tiles_k =
 * ceil(K/32), block0 = running sum of ceil(N/32)*ceil(K/32) over the preceding records; total_blocks = that sum.     */
int clipx_cast_weight_multi(const void* descs, int ntensors, int total_blocks, void* stream);
/* fused AdamW over a flat fp32 arena (torch.optim.AdamW semantics, main.py:287-295):
 * p *= 1 - lr*wd; m,v update; p -= lr/bc1 * m / (sqrt(v)/sqrt(bc2) + eps); g *= gscale first. */
int clipx_adamw(size_t n, float* p, const float* g, float* m, float* v, float lr, float beta1,
                float beta2, float eps, float wd, float bc1, float bc2, float gscale, void* stream);
/* the same update for many tensors in ONE launch.  descs: device array of ntensors records
 * { float* p; const float* g; float* m; float* v; uint64 n; float wd; uint32 block0 } (48 bytes, natural
 * alignment), block0 = running sum of ceil(n/4096) over the preceding records; total_blocks = that sum. */
int clipx_adamw_multi(const void* descs, int ntensors, int total_blocks, float lr, float beta1,
                      float beta2, float eps, float bc1, float bc2, float gscale, void* stream);
/* out[0] += sum(x^2)  (clip_grad_norm_, train.py:201-203)                                  */
int clipx_sumsq(size_t n, const float* x, float* out, void* stream);
/* p = clamp(p, lo, hi) for a single float (logit_scale.clamp_, train.py:211-212)           */
int clipx_clamp1(float* p, float lo, float hi, void* stream);
int clipx_scale(size_t n, float* x, float s, void* stream);
/* flat casts for gradient buckets on the wire (DDP's reducer buckets, main.py:264-271: here the arena itself is the bucket
 * and a bf16 staging copy goes over xGMI): y[i] = (bf16)(x[i]*scale) / y[i] = (float)x[i]*scale.  x/y 16-B resp. 8-B aligned. */
int clipx_cast_f32_bf16(size_t n, const float* x, void* y, float scale, void* stream);
int clipx_cast_bf16_f32(size_t n, const void* x, float* y, float scale, void* stream);

/* ---- token-level MaxSim pieces of ColClipLoss (loss.py:20-46; "next" row) --------------------
 * The similarity tensor einsum('mnd,kqd->mknq') is produced chunk-wise by the GEMM entry points above as
 * S[(m,n), (k,q)]; these reduce it and build d(S) for the backward GEMMs.
 * maxsim_reduce: maxv[row,g] = max_qq S[row, g*q+qq], arg = first arg-max (loss.py:35).                         */
int clipx_maxsim_reduce(int dtype, long rows, int groups, int q, const void* S, float* maxv,
                        unsigned char* arg, void* stream);
/* masked_mean: out[m,g] = sum_n maxv[(m*n_tok+n),g] / (#{n: maxv != 0} + 1e-8)  (loss.py:37-44);
 * inv_count[m,g] = 1 / that denominator (kept for the backward).                                                */
int clipx_masked_mean(int ct, int n_tok, int groups, const float* maxv, float* out, float* inv_count,
                      void* stream);
/* maxsim_scatter (autograd of the two above): P[(m,n),(g,qq)] = dlogits[m,g]*inv_count[m,g] at qq == arg, else 0;
 * PT (optional) receives the transpose [(g,qq),(m,n)].                                                          */
int clipx_maxsim_scatter(int dtype, int ct, int n_tok, int groups, int q, const float* dlogits,
                         const float* inv_count, const unsigned char* arg, void* P, void* PT, void* stream);

/* ---- retrieval evaluation (train.py:457-508: per-row CPU argsort + search in the reference) ------------------
 * ranks[r] = min over the row's targets t of #{c : scores[r,c] > scores[r,t]} (0 = retrieved first).  Targets in
 * CSR form: tgt_idx[tgt_off[r] .. tgt_off[r+1]).  scores fp32 with row stride ld.                                  */
int clipx_retrieval_rank(int rows, int cols, const float* scores, long ld, const int* tgt_off,
                         const int* tgt_idx, int* ranks, void* stream);

/* ---- streaming top-k for late-interaction search (csrc/topk.hip; the reference ranks by sorting every row of the whole
 * score matrix on the CPU, train.py:457-508) ------------------------------------------------------------------------
 * One step of a running selection over a gallery that arrives tile by tile.  Tile: nq queries x nc candidates, fp32, element
 * (j, c) at scores[j * q_stride + c * c_stride], exactly one of the strides 1 (both orientations of the image-major tile of
 * clipx_maxsim_score_fold); candidate c is gallery position c_base + c.  best_val / best_idx [nq, k] (contiguous): afterwards a
 * query's list holds the first k, under the total order "larger value, then smaller position", of its old list together with
 * its candidates; values are copied bit for bit.  Empty slots are (-inf, -1) and sort last; -inf and NaN candidates are skipped.
 * Refused before any launch: k outside 1 .. 256, both strides different from 1, c_base < 0 or c_base + nc > 2^31 - 1.
 * nq == 0 or nc == 0 launches nothing.                                                                                   */
int clipx_topk_merge(int nq, int nc, int k, const float* scores, long q_stride, long c_stride, long c_base, float* best_val,
                     int* best_idx, void* stream);

/* ---- kernel selection (tests / experiments; not part of the reference's interface) ---------------------------
 * bf16 NT GEMM structure: 0 = eight-wave kernel only, 1 = one-wave-per-SIMD kernel with the deferred epilogue wherever
 * it applies (full 256x256 tiles, bf16 output), 2 = that kernel only for tiles of >= 14 k-steps (the default), -1 = follow
 * the CLIPX_NT5 environment variable again.                                                                        */
int clipx_select_nt_kernel(int which);
/* eight-wave PING-PONG NT kernel (csrc/gemm_bf16_nt8p.hip: the two waves of a SIMD alternate between a load segment and
 * an MFMA segment, half a k-step apart): 0 = never, 1 = wherever it applies (256x256 tiles, K % 64 == 0, bf16 output),
 * 2 = where the one-wave-per-SIMD kernel is not chosen, -1 = follow the CLIPX_NT_PP environment variable again.          */
int clipx_select_nt_pp(int which);
/* the same choice for the TN (wgrad) kernel: 0 = one-barrier kernel, 1 = ping-pong form where it applies (N, K multiples of
 * 256), -1 = follow CLIPX_TN_PP again.                                                                                  */
int clipx_select_tn_pp(int which);
/* The MLP's GELU with its derivative kept on EIGHT bits (bf16 kernels; csrc/gemm_epi.h G8_*; replaces nn.GELU after c_fc and its
 * autograd, reference transformer.py:235-239): fwd: y = GELU(x . w^T + bias) [M,N] bf16 and g8 [M,N] uint8 = round((GELU'(x . w^T +
 * bias) + 0.13) * 200); dgrad: dx [M,K] = (dy [M,N] . wt [K,N]^T) * (-0.13 + 0.005 * g8 [M,K]) (0 and 1 are on the grid).  What the bf16
 * pre-activation cost was its store and its read-back, not the polynomial (scripts/bench_epi.py).                              */
int clipx_linear_fwd_gelu8(int M, int N, int K, const void* x, const void* w, const float* bias, void* g8, void* y, void* stream);
int clipx_linear_dgrad_gelu8(int M, int N, int K, const void* dy, const void* wt, const void* g8, void* dx, void* stream);
/* ... and on the fp8 MFMA (precision fp8_mfma; operands as clipx_linear_fwd_fp8 / clipx_linear_dgrad_fp8)                  */
int clipx_linear_fwd_fp8_gelu8(int M, int N, int K, const void* x8, const int* x_exp, const void* w8, const int* w_exp,
                               const float* bias, void* g8, void* y, void* stream);
int clipx_linear_dgrad_fp8_gelu8(int M, int N, int K, const void* dy8, const int* dy_exp, const void* wt8, const int* wt_exp,
                                 const void* g8, void* dx, void* stream);

/* Fused MaxSim for bf16 token features with >= 16 tokens per image (csrc/colbert.hip, csrc/gemm_nt_maxsim.h; replaces the
 * einsum + max + masked mean of reference loss.py:20-46 without the similarity tensor in memory).
 * pack_text: cnt[m] = number of packed rows of sample m (its leading rows + ONE representative of the trailing rows that are
 *   bitwise equal to its last row), cu = exclusive scan (cu[nt] = packed rows in total).  pack_rows: packed [R, e] bf16,
 *   row_m[r] = sample, row_w[r] = how many original positions the row stands for.
 * gemm: S = packed . img^T reduced in the GEMM epilogue to per-(row, 64-column slot, segment) maxima: pmax / pidx are
 *   [2 * ceil(ni*q/64), ldp] (ldp >= R); for 16 <= q < 64 to per-(row, image, slot half) maxima, [2 * ni, ldp].
 *   finish: folds an image's partials in column order (first maximum wins) into maxvT / argT [ni, ld] at
 *   rows r0 .. r0+R.  mean: logits[m,k] = sum_r w_r maxvT[k,r] / (sum_r w_r [maxvT != 0] + 1e-8), inv_count = 1 / that denominator.
 * scatter_packed: P[r - r0, k*q + qq] = (qq == argT[k,r]) ? dlogits[m_r,k] * inv_count[m_r,k] : 0 (bf16) for rows r0 .. r0+R.
 * scale_rows: y[r,:] = w_r x[r,:].  expand: dtxt[m, n, :] = dpacked[cu[m] + min(n, cnt[m]-1), :].                        */
int clipx_maxsim_pack_text(int nt, int n_tok, int e, const void* txt, int* cnt, int* cu, void* stream);
int clipx_maxsim_pack_rows(int nt, int n_tok, int e, const void* txt, const int* cu, void* packed, int* row_m, float* row_w,
                           void* stream);
int clipx_maxsim_gemm(int R, int ni, int q, int e, const void* packed, const void* img, float* pmax, unsigned short* pidx,
                      int ld, void* stream);
/* gemm_fp8: the same partials (layout, tie rules) from e4m3 operands on the fp8 MFMA: packed8 [R, e] and img8 [ni * q, e] bytes
 *   with one power-of-two exponent per row (clipx_quant_rows_e4m3), S[r, c] = 2^(packed_exp[r] + img_exp[c]) * sum packed8 img8,
 *   the exponents applied BEFORE the maximum.  Needs e % 128 == 0, e >= 256, 16 <= q <= 65535, (ni * q) % 8 == 0 and 16-byte
 *   aligned operands; anything else is an error (ops.maxsim_scores_fp8 picks the route before it calls).                       */
int clipx_maxsim_gemm_fp8(int R, int ni, int q, int e, const void* packed8, const int* packed_exp, const void* img8,
                          const int* img_exp, float* pmax, unsigned short* pidx, int ld, void* stream);
int clipx_maxsim_finish(int R, int ldp, int r0, int ld, int ni, int q, const float* pmax, const unsigned short* pidx,
                        float* maxvT, unsigned short* argT, void* stream);
int clipx_maxsim_mean(int nt, int ni, int ld, const int* cu, const float* row_w, const float* maxvT, float* logits,
                      float* inv_count, void* stream);
/* score_fold (forward only: retrieval, get_logits without grad): the partials of one (image chunk, text chunk) straight to a
 * block of the dense image-major score matrix, scores[k, m] = scale * (alpha * G[k, m] + beta * tok[m, k]) for samples m < nm
 * (cu points at the chunk's first sample, packed rows cu[m] - rbase .. cu[m+1] - rbase of the partials, weights row_w[cu[m] ..])
 * and images k < ni, tok = the masked mean of maxsim_mean over the per-row maxima of maxsim_finish; G, scores point at the
 * block's first element.  G == NULL: no global term.  pmax == NULL: scale * G exactly (alpha = 1; the token term is skipped). */
int clipx_maxsim_score_fold(int nm, int ni, int q, int ldp, int rbase, const int* cu, const float* row_w, const float* pmax,
                            const float* G, long ld_g, float* scores, long ld_scores, float alpha, float beta, float scale,
                            void* stream);
int clipx_maxsim_scatter_packed(int R, int r0, int ld, int ni, int q, const int* row_m, const float* dlogits,
                                const float* inv_count, const unsigned short* argT, void* P, void* stream);
int clipx_maxsim_scale_rows(int R, int e, const float* row_w, const void* x, void* y, void* stream);
int clipx_maxsim_expand(int dtype, int nt, int n_tok, int e, const int* cu, const float* dpacked, void* dtxt, void* stream);

/* ---- gathered MaxSim for reranking (csrc/maxsim_pairs.hip; LateInteractionIndex.rerank) -----------------------------
 * out[i * ld_out + c] = scale * (alpha * Gp[i * ld_gp + c] + beta * MaxSim(pair)) for query i < nq and candidate slot c < C, the
 * pair being query i and gallery position p = cand[i * C + c]; p == -1 writes -inf and reads no token.  Gp == NULL: no global term.
 * gallery_is_image != 0: queries are texts [nq, n, e] bf16 with query_cnt [nq] (clipx_maxsim_pack_text's cnt), the gallery holds
 * images [.., q, e]; == 0: queries are images [nq, q, e], the gallery holds texts [.., n, e] with their cnt.  The gallery is
 * the index's chunked storage as it is: gal_tok is a DEVICE table of n_chunks base addresses of [chunk_items, q or n, e] bf16
 * tensors, gal_cnt (text gallery) one of [chunk_items] int32 tensors; position p is item p % chunk_items of chunk p / chunk_items.
 * MaxSim is the arithmetic of clipx_maxsim_score_fold on the first cnt rows of the text, row cnt - 1 weighted n - cnt + 1.
 * status: 4 bytes of device scratch.  Refused, with nothing scored and `out` untouched: q < 16, e % 64 != 0, e < 128, a query side
 * of more than 80 rows (image gallery: n, text gallery: q) or 128 KiB of staging (16-padded rows x (e + 8) x 2 bytes), C > 524280,
 * cand_stride != C, ld_out or ld_gp < C, n_items > n_chunks * chunk_items, and -- found by one read-only pass over cand and the
 * cnt it names, which costs a stream synchronisation -- a position outside [0, n_items) other than -1 or a cnt outside 1 .. n.
 * nq == 0 or C == 0 launches nothing.                                                                                          */
int clipx_maxsim_pairs(int gallery_is_image, int nq, int C, int q, int n, int e, const void* query, const int* query_cnt,
                       const void* gal_tok, const void* gal_cnt, int n_chunks, int chunk_items, long n_items, const int* cand,
                       long cand_stride, const float* Gp, long ld_gp, float* out, long ld_out, float alpha, float beta, float scale,
                       int* status, void* stream);

#ifdef __cplusplus
}
#endif
#endif
