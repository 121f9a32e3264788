/*
 * include/s2d_hip.h -- C ABI of libs2d_hip.so, the MI355X (gfx950) implementation of the S2D hot path.
 *
 * The reference (leonsick/s2d) exposes this path through Python/detectron2 registries and ONE native
 * FFI, the pybind module `MultiScaleDeformableAttention`
 * (model_training/mask2former/modeling/pixel_decoder/ops/src/vision.cpp:18-21,
 *  .../src/ms_deform_attn.h:25-66).  Every entry point below replaces the reference code cited next to it.
 *
 * Conventions: plain pointers to DEVICE memory and sizes, no framework types; the caller owns every
 * buffer; work is enqueued on `stream` and the call returns immediately; thread-safe per stream;
 * return 0 on success, a negative S2D_ERR_* code otherwise (never throws, never synchronises).
 * Layouts are stated per function.  "NHWC" = channels-last feature maps, which is also the reference's
 * [N, S, C] token layout once H*W is flattened.
 */
#ifndef S2D_HIP_H
#define S2D_HIP_H
#include <stdint.h>

#ifndef HIP_INCLUDE_HIP_HIP_RUNTIME_API_H
typedef struct ihipStream_t *hipStream_t;
#endif

#ifdef __cplusplus
extern "C" {
#endif

#define S2D_OK 0
#define S2D_ERR_ARG (-1)
#define S2D_ERR_LAUNCH (-2)

int s2d_abi_version(void);

/* Arithmetic of the dense contractions below (process-wide), all fp32 in / fp32 out:
 * 2 (default) = split-fp16 x3 on the f16 MFMA (x = h + l*2^-11; A.B^T ~= Ah.Bh^T + 2^-11 (Ah.Bl^T + Al.Bh^T), f32
 *     accumulation: ~5e-7 relative; operands must satisfy |x| < 65504);
 * 1 = split-bf16 x3 on the bf16 MFMA (~5e-6 relative, no range limit);
 * 0 = fp32-input MFMA (an exact f32 FMA chain, 1/16 of the 16-bit rate). */
int s2d_set_dense_mode(int mode);

/* ---- dense contractions (fp32-input MFMA) ------------------------------------------------------ */

/* C[b][M,N] = act((A[b][M,K] * B[b][N,K]^T) * scale[N] + bias[N] + res[b][M,N]); scale/bias/res may be NULL.
 * res_rows > 0: the residual is row-periodic, res[b][row % res_rows, :] (a per-position term shared by all frames, e.g.
 * pos . W^T of "(src + pos) . W^T", ms_deform_attn.py:107-108 via msdeformattn.py:68); res_cols > 0: only columns
 * < res_cols receive the residual (multiple of 4).
 * Replaces every nn.Linear / 1x1 Conv2d on the path (e.g. ms_deform_attn.py:98-104,124; msdeformattn.py:122-131;
 * video_mask2former_transformer_decoder.py:99-111,164-168,193-205) and the mask-logit einsum
 * "bqc,btchw->bqthw" (video_mask2former_transformer_decoder.py:455).  K, lda, ldb multiples of 4. */
int s2d_gemm_nt_f32(const float *A, const float *B, float *C, int M, int N, int K, long lda, long ldb, long ldc,
                    int batch, long strideA, long strideB, long strideC, const float *scale, const float *bias,
                    const float *res, long ldr, long strideR, int res_rows, int res_cols, int relu, const void *B_split,
                    hipStream_t stream);

/* The same contraction with nn.Dropout fused into the epilogue: C = act(dropout_p(A.B^T + bias) + res) -- the three dropout
 * sites of the pixel decoder's encoder layers in training mode (msdeformattn.py:101-125: dropout1 on the attention output,
 * dropout2 after the FFN activation (ReLU and a non-negative mask commute), dropout3 on the FFN output; each before its
 * residual add).  The mask is counter-based (ABI 10: 8 bits per element, one generator call per 16 elements): element (row, col)
 * of the [M,N] output is kept iff byte (col % 4) of word ((col % 16) / 4) of
 * Philox4x32-10(counter = (row0 + row, col / 16, site, 0), key = seed) is >= T = round(p * 256) (row0: the mask row of output
 * row 0, for a launch over a row range of a larger activation): P(drop) = T / 256, p quantised to 1 / 256; kept elements are
 * multiplied by 256 / (256 - T) = 1 / P(keep) (inverted dropout, unbiased for the realised keep probability); the backward
 * regenerates it (s2d_dropout_f32) instead of storing it.  Unbatched; N, ldc, ldr multiples of 8; dense mode 2 only
 * (S2D_ERR_ARG otherwise). */
int s2d_gemm_nt_dropout_f32(const float *A, const float *B, float *C, int M, int N, int K, long lda, long ldb, long ldc,
                            const float *bias, const float *res, long ldr, int relu, const void *B_split, float p,
                            uint64_t seed, unsigned site, unsigned row0, hipStream_t stream);

/* y[M,N] = x * mask / P(keep) with the mask of s2d_gemm_nt_dropout_f32 for the same (p, seed, site): the gradient of a
 * dropout site (and the mask itself, from x = 1).  N multiple of 8; y may alias x. */
int s2d_dropout_f32(const float *x, long M, int N, float p, uint64_t seed, unsigned site, unsigned row0, float *y, hipStream_t stream);

/* Static weights can be split into their fp16 hi/lo image once (dense mode 2) instead of in every launch that reads
 * them: out = s2d_split_weights_words(N,K) 32-bit words, laid out [N][ceil(K/32)][16 words hi | 16 words lo] (the LDS
 * row image of the kernels, zero padded past K).  Pass it as B_split / w_split together with the fp32 weights (the
 * other dense modes read those); NULL = split on the fly.  Results are bit-identical either way.  Unbatched B only. */
/* dgrad GEMM with the gate of the differentiated layer in its epilogue: C = gate[row][col] > 0 ? (A.B^T + res) * gate_scale : 0.
 * Replaces `grad_input = grad_output @ W` followed by the threshold_backward / dropout-scale pass autograd runs for
 * F.relu / nn.Dropout in the reference's FFNs (mask2former/modeling/pixel_decoder/msdeformattn.py:121-125,
 * mask2former_video/modeling/transformer_decoder/video_mask2former_transformer_decoder.py FFNLayer).  split-fp16 mode, N, ldc, ldr,
 * ldg multiples of 4; otherwise S2D_ERR_ARG. */
int s2d_gemm_nt_gate_f32(const float *A, const float *B, float *C, int M, int N, int K, long lda, long ldb, long ldc, const float *scale,
                         const float *res, long ldr, const float *gate, long ldg, float gate_scale, const void *B_split, hipStream_t stream);
/* ... and the convolution form (dgrad of a k x k convolution whose input came out of a ReLU; scale: the per-channel FrozenBatchNorm
 * factor of the layer that produced that input, detectron2 FrozenBatchNorm2d folded as in s2d_conv2d_nhwc_f32; gate [N,Ho,Wo,Cout]) */
int s2d_conv2d_nhwc_gate_f32(const float *x, const float *w, float *y, int N, int H, int W, int Cin, int Cout, int KH, int KW, int stride,
                             int pad, const float *scale, const float *gate, float gate_scale, const void *w_split, hipStream_t stream);
/* The GEMM with A pre-split as well: A_split is the s2d_split_weights_f16 image of A's M rows (an activation whose producer wrote it
 * in that layout, or a one-off conversion); B_split is required.  Same result bits as s2d_gemm_nt_f32 on the fp32 A.  Shapes the
 * wave-specialised kernel does not take (K < 224, K % 32, N % 4) return S2D_ERR_ARG. */
int s2d_gemm_nt_presplit_f32(const void *A_split, const float *B, float *C, int M, int N, int K, long ldb, long ldc, const float *bias,
                             const float *res, long ldr, int res_rows, int res_cols, int relu, const void *B_split, hipStream_t stream);
long s2d_split_weights_words(int N, int K);
/* launches of s2d_gemm_nt_f32 that the row-resident short-K kernel has taken so far in this process (S2D_GEMM_ROWS: 0 never,
 * 1 = default by a measured shape rule, 2 every launch the kernel accepts); the results do not depend on the setting */
long s2d_gemm_rows_launches(void);
int s2d_split_weights_f16(const float *W, int N, int K, long ldw, void *out, hipStream_t stream);

/* The encoder layer's feed-forward block in one launch (split-fp16 x3 arithmetic, dense mode 2's):
 *     xn = ln1_gamma ? LayerNorm(x; ln1_gamma, ln1_beta, eps) : x
 *     y  = LN2?( xn + dropout_p( W2 . dropout_p( relu( W1 . xn + b1 ) ) + b2 ) )      LN2 applied when ln2_gamma != NULL
 * i.e. `src = norm2(src + dropout3(linear2(dropout2(relu(linear1(src))))))` of MSDeformAttnTransformerEncoderLayer
 * (mask2former/modeling/pixel_decoder/msdeformattn.py:116-131), optionally with the layer's norm1 (:125) folded into the input side.
 * The F-wide hidden activation stays in registers.  x, y [M, C] fp32 (C = 256; F a multiple of 32, <= 2048); pack = the image
 * s2d_ffn_pack_f16 wrote from W1 [F, C] and W2 [C, F] (s2d_ffn_pack_words(C, F, Npost, pre) 32-bit words; -1 = unsupported sizes).
 * Dropout: p = 0 -> none; otherwise the counter-based masks of s2d_gemm_nt_dropout_f32 for (seed, site_hidden) on the [M, F] hidden
 * activation and (seed, site_out) on the [M, C] output, mask row of row 0 = row0 -- the same bits the two-launch form applies.
 * xn (optional, requires ln1_gamma): receives the normalised input.
 * Npost > 0 (a multiple of 32; requires both LayerNorms): the same launch also applies the NEXT encoder layer's merged projection to
 * every output row while it is still in registers -- post_out[row][n] = y[row] . Wpost[n]^T + post_pos[row % post_S][n] for
 * n < post_npos (a multiple of 32: the row-periodic `pos . W^T + b` term of the sampling offsets / attention logits, which carries
 * their bias -- post_bias is NOT read for these columns; post_ldpos its row stride) and y[row] . Wpost[n]^T + post_bias[n] for
 * post_npos <= n < Npost, row stride post_ld -- i.e. [sampling_offsets | attention_weights | value_proj] of
 * ops/modules/ms_deform_attn.py:98-104 applied to the layer output, which is the next layer's `src`.  Wpost [Npost, C] is packed behind
 * the FFN weights by s2d_ffn_pack_f16.
 * pre_bias != NULL (requires both LayerNorms and xn): the launch also takes over what precedes norm1 in the layer -- x is then the
 * deformable attention's sampled values [M, C] and the FFN's input row becomes
 *     x1 = pre_res + dropout_p( Wpre . x + pre_bias )        mask (seed, site_pre)
 * i.e. `src = src + dropout1(output_proj(samp))` (ms_deform_attn.py:124, msdeformattn.py:124-125) with pre_res the layer input [M, C];
 * Wpre [C, C] is packed behind Wpost (s2d_ffn_pack_f16's Wpre, s2d_ffn_pack_words' pre = 1).  xn receives norm1(x1) as before. */
long s2d_ffn_pack_words(int C, int F, int Npost, int pre);
int s2d_ffn_pack_f16(const float *W1, const float *W2, int C, int F, const float *Wpost, int Npost, const float *Wpre, void *out,
                     hipStream_t stream);
int s2d_ffn_fused_f32(const float *x, long M, int C, int F, const void *pack, const float *b1, const float *b2, const float *ln1_gamma,
                      const float *ln1_beta, const float *ln2_gamma, const float *ln2_beta, float eps, float p, uint64_t seed,
                      unsigned site_hidden, unsigned site_out, unsigned row0, float *xn, float *y, int Npost, const float *post_bias,
                      const float *post_pos, int post_S, int post_npos, long post_ldpos, float *post_out, long post_ld,
                      const float *pre_bias, const float *pre_res, unsigned site_pre, hipStream_t stream);

/* NHWC convolution as implicit GEMM: x [N,H,W,Cin] (Cin % 4 == 0), w [Cout][KH][KW][Cin],
 * y [N,Ho,Wo,Cout] = act(conv(x,w) * scale[Cout] + bias[Cout] + res).  Replaces detectron2 Conv2d+FrozenBN+ReLU
 * of the R50 trunk (build_resnet_backbone, call site kd_video_maskformer_model.py:132,135) and the FPN
 * 3x3 output conv (msdeformattn.py:264-281). */
int s2d_conv2d_nhwc_f32(const float *x, const float *w, float *y, int N, int H, int W, int Cin, int Cout, int KH,
                        int KW, int stride, int pad, const float *scale, const float *bias, const float *res,
                        int relu, const void *w_split, hipStream_t stream);

/* The two contractions with fp16 operands / f32 accumulate / f32 output -- autocast-LIKE (engine/train_loop.py:709 `with autocast():`,
 * SOLVER.AMP.ENABLED True in every shipped yaml; real autocast additionally rounds every output to fp16): operands rounded to fp16
 * (nearest-even), f32 accumulation by ONE fp16 MFMA per product, f32 out.  Opt-in, for the modules autocast runs in fp16 (the R50 trunk, the video decoder's linear layers, the
 * mask-logit einsum); the pixel decoder and the matcher force fp32 in the reference (msdeformattn.py:314, matcher.py:266-268) and
 * never take these.  Same arguments as s2d_gemm_nt_f32 / s2d_conv2d_nhwc_f32 without the pre-split image. */
int s2d_gemm_nt_amp_f32(const float *A, const float *B, float *C, int M, int N, int K, long lda, long ldb, long ldc, int batch,
                        long strideA, long strideB, long strideC, const float *scale, const float *bias, const float *res, long ldr,
                        long strideR, int res_rows, int res_cols, int relu, hipStream_t stream);
int s2d_conv2d_nhwc_amp_f32(const float *x, const float *w, float *y, int N, int H, int W, int Cin, int Cout, int KH, int KW, int stride,
                            int pad, const float *scale, const float *bias, const float *res, int relu, hipStream_t stream);

/* ---- multi-scale deformable attention (HBM/L2-bound gather, no MFMA) --------------------------------- */

/* Drop-in for MSDA.ms_deform_attn_forward (ops/src/ms_deform_attn.h:25-44, ops/src/vision.cpp:19; kernel
 * ops/src/cuda/ms_deform_im2col_cuda.cuh:242-304): value [N,S,M,D], sampling_loc [N,Lq,M,L,P,2] (x,y in
 * [0,1]), attn_w [N,Lq,M,L,P] -> out [N,Lq,M*D].  spatial shapes [L,2]=(H,W) and level starts [L] are HOST
 * int64 arrays (they are tiny and known on the host; the reference reads them from device memory).
 * No im2col_step chunking is needed. */
int s2d_msda_forward_f32(const float *value, const int64_t *shapes_host, const int64_t *level_start_host,
                         const float *loc, const float *attn_w, int N, int S, int M, int D, int L, int Lq, int P,
                         float *out, hipStream_t stream);

/* Drop-in for MSDA.ms_deform_attn_backward (ops/src/ms_deform_attn.h:46-66; kernels cuh:306-408, formulas
 * :119-163).  grad buffers are zero-initialised here, as the reference does (ms_deform_attn_cuda.cu:119-121). */
int s2d_msda_backward_f32(const float *value, const int64_t *shapes_host, const int64_t *level_start_host,
                          const float *loc, const float *attn_w, const float *grad_out, int N, int S, int M, int D,
                          int L, int Lq, int P, float *grad_value, float *grad_loc, float *grad_attn_w,
                          hipStream_t stream);

/* The same gradients without float atomics, bitwise reproducible (what the training step uses): the sampling graph is
 * inverted once per call -- samples keyed by their bilinear cell, histogram + prefix sum, stable radix sort -- and every
 * grad_value row is then written once by a gather over the four cells that touch its pixel; grad_loc / grad_attn are
 * query-owned.  workspace: s2d_msda_backward_workspace_bytes(...) bytes of device memory.  Lq, M, L, P as above; D == 32. */
long s2d_msda_backward_workspace_bytes(const int64_t *shapes_host, int N, int M, int L, int Lq, int P);
int s2d_msda_backward_sorted_f32(const float *value, const int64_t *shapes_host, const int64_t *level_start_host,
                                 const float *loc, const float *attn_w, const float *grad_out, int N, int S, int M, int D,
                                 int L, int Lq, int P, float *grad_value, float *grad_loc, float *grad_attn_w, void *workspace,
                                 long workspace_bytes, hipStream_t stream);
/* The same with row strides: value rows (n, s) are M * D floats at stride ldv, grad_value rows at stride ldg (column slices of
 * the merged projection output / of its gradient buffer: no contiguous copy of value, no concatenation of the gradients).
 * grad_loc == grad_attn_w == NULL: grad_value only (the caller takes the query-owned half from s2d_msda_fused_backward_query_f32). */
int s2d_msda_backward_sorted_strided_f32(const float *value, long ldv, const int64_t *shapes_host, const int64_t *level_start_host,
                                         const float *loc, const float *attn_w, const float *grad_out, int N, int S, int M, int D,
                                         int L, int Lq, int P, float *grad_value, long ldg, float *grad_loc, float *grad_attn_w,
                                         void *workspace, long workspace_bytes, hipStream_t stream);

/* The drop-in op with the reference's own argument kinds: spatial shapes [L,2] and level starts [L] as int64 DEVICE tensors,
 * read inside the kernels exactly as ms_deformable_im2col_gpu_kernel does (ops/src/cuda/ms_deform_attn_cuda.cu:60-75 passes
 * spatial_shapes.data<int64_t>() / level_start_index.data<int64_t>() straight to the kernels; the module builds both tensors
 * fresh on every forward, msdeformattn.py:82-83).  No host copy, no cache, no synchronisation: a one-thread kernel turns the two
 * tensors into the geometry record at the head of `workspace` and every kernel of the call reads it from there.
 * Shapes that fail the host form's argument checks (H, W <= 0; a level past S), or whose levels overlap (sum of H*W > S: the
 * reference would read the shared rows twice; the sorted backward's workspace is sized for disjoint levels), cannot be reported through the return code
 * without a sync: the call then produces zeros and sets the record's error flag, which s2d_msda_dev_status reads back.
 * workspace: s2d_msda_dev_forward_workspace_bytes() / s2d_msda_dev_backward_workspace_bytes(...) bytes of device memory, 16-B
 * aligned, private to the call until it has finished.  The backward is the atomic-free sorted form. */
long s2d_msda_dev_forward_workspace_bytes(void);
int s2d_msda_forward_dev_f32(const float *value, const int64_t *shapes_dev, const int64_t *level_start_dev, const float *loc,
                             const float *attn_w, int N, int S, int M, int D, int L, int Lq, int P, float *out, void *workspace,
                             hipStream_t stream);
long s2d_msda_dev_backward_workspace_bytes(int N, int S, int M, int L, int Lq, int P);
int s2d_msda_backward_dev_f32(const float *value, const int64_t *shapes_dev, const int64_t *level_start_dev, const float *loc,
                              const float *attn_w, const float *grad_out, int N, int S, int M, int D, int L, int Lq, int P,
                              float *grad_value, float *grad_loc, float *grad_attn_w, void *workspace, long workspace_bytes,
                              hipStream_t stream);
/* Failing loudly without a sync: `word` is an int in memory that both the GPU and the host can address (pinned host memory, e.g.
 * hipHostMalloc / torch's pin_memory; NULL: none), registered once for the process.  A *_dev call whose shapes are rejected stores 1
 * into it (system scope, never cleared by the library): the caller tests the word with a plain host read before / after its calls and
 * raises -- at the latest one call after the offending one has executed -- instead of training on zeros.  The drop-in module
 * (s2d_amd/compat/MultiScaleDeformableAttention.py) does exactly that. */
/* float64 instantiation of the drop-in op (the reference extension dispatches on floating types, ms_deform_attn_cuda.cu:69, :137; its
 * ops/test.py gradchecks in double): same argument kinds as the *_dev_f32 entries, no workspace.  Not a hot path -- one thread per
 * output channel, grad_value / grad_sampling_loc / grad_attn_weight accumulated with double atomics (as the reference's col2im kernels
 * do), so the gradients are reproducible to rounding, not bitwise.  A level that does not lie inside S contributes nothing. */
int s2d_msda_forward_dev_f64(const double *value, const int64_t *shapes_dev, const int64_t *level_start_dev, const double *loc,
                             const double *attn_w, int N, int S, int M, int D, int L, int Lq, int P, double *out, hipStream_t stream);
int s2d_msda_backward_dev_f64(const double *value, const int64_t *shapes_dev, const int64_t *level_start_dev, const double *loc,
                              const double *attn_w, const double *grad_out, int N, int S, int M, int D, int L, int Lq, int P,
                              double *grad_value, double *grad_loc, double *grad_attn_w, hipStream_t stream);

int s2d_msda_dev_error_word(int *word);
/* *err_host = the error flag of the *_dev call that used `workspace` (0 = shapes accepted).  Synchronises `stream`. */
int s2d_msda_dev_status(const void *workspace, int *err_host, hipStream_t stream);

/* Fused pixel-decoder form: also does softmax over L*P and loc = ref + off/(W_l,H_l)
 * (ops/modules/ms_deform_attn.py:101-109) with the query's own pixel centre as reference point
 * (msdeformattn.py:141-153).  offs_logits [N,S,ldoa]: per query M*L*P*2 raw offsets then M*L*P raw logits.
 * Requires D == 32, L*P == 12 (the shipped geometry, msdeformattn.py:232-239). */
int s2d_msda_fused_forward_f32(const float *value, int ldv, const int64_t *shapes_host, const float *offs_logits, int ldoa,
                               int N, int S, int M, int D, int L, int P, float *out, hipStream_t stream);

/* Backward of the fused form = prep (raw offsets / logits -> loc [N,S,M,L,P,2], softmaxed attn [N,S,M,L,P] with the
 * forward's reference points), s2d_msda_backward_f32 on those, chain (d_loc, d_attn -> d_offs_logits [N,S,ldd], the
 * gradient of the merged projection output: d_off = d_loc / (W_l, H_l), d_logit = a (d_a - sum a d_a)). */
int s2d_msda_fused_prep_f32(const float *offs_logits, int ldoa, const int64_t *shapes_host, int N, int S, int M, int L, int P,
                            float *loc, float *attn, hipStream_t stream);
int s2d_msda_fused_chain_f32(const float *attn, const float *grad_loc, const float *grad_attn, const int64_t *shapes_host, int N,
                             int S, int M, int L, int P, float *d_offs_logits, int ldd, hipStream_t stream);
/* The query-owned half of that backward in ONE launch for the S2D geometry (M = 8, D = 32, L = 3, P = 4; anything else: S2D_ERR_ARG):
 * d_offs_logits [N][S][ldd] straight from grad_out [N][S][M][32], the value rows (stride ldv) and the raw projection rows -- what
 * grad_loc / grad_attn of s2d_msda_backward_sorted*_f32 followed by s2d_msda_fused_chain_f32 give (reference: the grad_sampling_loc /
 * grad_attn_weight half of ms_deformable_col2im_gpu_kernel_*, ops/src/cuda/ms_deform_im2col_cuda.cuh:119-163, and autograd's chain
 * through ms_deform_attn.py:103-113), without those two tensors in memory.  16-B aligned value / offs_logits / grad_out rows. */
int s2d_msda_fused_backward_query_f32(const float *value, int ldv, const int64_t *shapes_host, const float *offs_logits, int ldoa,
                                      const float *grad_out, int N, int S, int M, int D, int L, int P, float *d_offs_logits, int ldd,
                                      hipStream_t stream);

/* ---- bandwidth-bound glue (HBM-bound, 16-B accesses) ----------------------------------------------- */

/* (x - mean)/std per frame + zero pad bottom/right to (Hp,Wp): kd_video_maskformer_model.py:263-269 and
 * detectron2 ImageList.from_tensors.  frames u8 [F,3,H0,W0] (the mapper's layout, dataset_mapper.py:306-404)
 * -> out f32 [F,Hp,Wp,4] (NHWC, 4th channel zero so the 7x7 stem runs as a Cin=4 implicit GEMM).
 * mean3/std3 are HOST arrays. */
int s2d_normalize_pad_nhwc4_f32(const uint8_t *frames, int F, int H0, int W0, int Hp, int Wp, const float *mean3_host,
                                const float *std3_host, float *out, hipStream_t stream);

/* 3x3/2 pad 1 max pool, NHWC (detectron2 BasicStem). y [N,(H+1)/2,(W+1)/2,C]. */
int s2d_maxpool3x3s2_nhwc_f32(const float *x, int N, int H, int W, int C, float *y, hipStream_t stream);
/* The same, also writing the arg-max tap (ky * 3 + kx, the first maximum in scan order) of every output element: argmax [N][Ho][Wo][C] bytes,
 * 4-byte aligned.  The training step keeps it for s2d_maxpool3x3s2_backward_idx_nhwc_f32. */
int s2d_maxpool3x3s2_nhwc_idx_f32(const float *x, int N, int H, int W, int C, float *y, unsigned char *argmax, hipStream_t stream);

/* y = GroupNorm_G(x)*gamma+beta [+ bilinear_resize(up [N,hu,wu,C] -> (H,W), align_corners=False)] [relu]; x NHWC.
 * nn.GroupNorm(32,256) at msdeformattn.py:213-226 and detectron2 get_norm("GN") at :261-281; the fused
 * upsample-add is msdeformattn.py:349.  stats_ws: s2d_groupnorm_workspace_doubles(N,H,W,G) doubles (statistics + the
 * per-block partials they are reduced from in a fixed order: no atomics, bitwise reproducible). */
long s2d_groupnorm_workspace_doubles(int N, int H, int W, int G);
int s2d_groupnorm_nhwc_f32(const float *x, int N, int H, int W, int C, int G, const float *gamma, const float *beta,
                           float eps, const float *up, int hu, int wu, int relu, double *stats_ws, float *y,
                           hipStream_t stream);

/* y = LayerNorm(x + res) over the last dim (res may be NULL): the post-norm residual blocks of
 * msdeformattn.py:116-131 and video_mask2former_transformer_decoder.py:41-51,99-111,164-168. */
int s2d_layernorm_f32(const float *x, const float *res, const float *gamma, const float *beta, long rows, int C,
                      float eps, float *y, hipStream_t stream);

/* y[i] = x[i] + b[i % bn] (n, bn multiples of 4): with_pos_embed / level-embed adds. */
int s2d_add_bcast_f32(const float *x, const float *b, long n, long bn, float *y, hipStream_t stream);

/* Sine position encoding written token-major [T*H*W, 2F] (+ add_c[2F] if not NULL).  T == 0: 2-D form
 * (mask2former/modeling/transformer_decoder/position_encoding.py:29-52); T > 0: 3-D form
 * (mask2former_video/modeling/transformer_decoder/position_encoding.py:29-57). */
int s2d_pe_sine_f32(int T, int H, int W, int num_pos_feats, const float *add_c, float *out, hipStream_t stream);

/* ---- masked cross-attention of the video decoder (fp32 MFMA QK^T / AV, streamed over keys) ----------- */

/* Attention-mask builder: bilinear-resize the pixel-major mask logits [B][T*hm*wm][ldq] to the level size
 * (hl,wl), threshold sigmoid<0.5 (== logit<0) and pack to bits [B][K=T*hl*wl][4] (bit q set = query q must NOT
 * attend key); unmasked [B][4] gets bit q set iff query q has at least one attendable key.
 * video_mask2former_transformer_decoder.py:460-465 (the x8 head repeat is implicit: heads share the bits).
 * compact != 0: mask_logits holds only the four bilinear source pixels of every key, [B][K][4][ldq] in the order
 * (y0,x0) (y0,x1) (y1,x0) (y1,x1) of the ATen align_corners=False source rule -- for a network whose intermediate mask
 * predictions feed nothing but the next layer's attention mask (the frozen teacher). */
int s2d_attn_mask_bits(const float *mask_logits, int ldq, int B, int Q, int T, int hm, int wm, int hl, int wl, int compact,
                       uint32_t *bits, uint32_t *unmasked, hipStream_t stream);

/* floats of workspace s2d_masked_attn_f32 needs */
long s2d_attn_workspace_floats(int B, int H, int K);

/* out[b][q][:] = concat_h softmax_k(q_h k_h^T / sqrt(32) + mask) v_h with q [B][Q][C], k/v [B][K] rows of C floats
 * at row strides ldk / ldv >= C (a column slice of a wider projection output; multiples of 4), already projected,
 * C = 32*H, Q <= 128.  bits/unmasked from s2d_attn_mask_bits (NULL = no mask: the self-attention
 * of :41-51); a query with no attendable key attends everywhere (the fix at :413).  lse (may be NULL) [B][H][128]
 * receives the base-2 log-sum-exp of the scaled scores, which the backward needs.  Replaces the core of
 * nn.MultiheadAttention at :99-111 without materialising the [B*8,Q,K] mask or the scores. */
int s2d_masked_attn_f32(const float *q, const float *k, const float *v, long ldk, long ldv, const uint32_t *bits,
                        const uint32_t *unmasked, int B, int Q, int K, int C, int H, float *workspace, float *out, float *lse,
                        hipStream_t stream);

/* Backward of s2d_masked_attn_f32.  lse [B][H][128]: the base-2 log-sum-exp the forward leaves when
 * its `lse` argument is non-NULL; out = the forward output; dout [B][Q][C].  dq [B][Q][C], dk / dv [B][K][C] (dense).
 * Probabilities are recomputed from lse; dQ partials over key ranges are added in a fixed order.  workspace:
 * s2d_attn_backward_workspace_floats(B, H, K) floats. */
long s2d_attn_backward_workspace_floats(int B, int H, int K);
int s2d_masked_attn_backward_f32(const float *q, const float *k, const float *v, long ldk, long ldv, const uint32_t *bits,
                                 const uint32_t *unmasked, const float *out, const float *lse, const float *dout, int B, int Q,
                                 int K, int C, int H, float *workspace, float *dq, float *dk, float *dv, hipStream_t stream);
/* The same with row strides on dk / dv (lddk, lddv >= C, multiples of 4, 16-B aligned bases): the gradients land in column slices of a wider
 * buffer -- the video decoder collects the key / value gradients of the three layers that share a memory level side by side for ONE
 * projection backward (video_mask2former_transformer_decoder.py:99-111 x 9 layers), without a copy per layer. */
int s2d_masked_attn_backward_strided_f32(const float *q, const float *k, const float *v, long ldk, long ldv, const uint32_t *bits,
                                         const uint32_t *unmasked, const float *out, const float *lse, const float *dout, int B, int Q,
                                         int K, int C, int H, float *workspace, float *dq, float *dk, long lddk, float *dv, long lddv,
                                         hipStream_t stream);

/* ---- VideoHungarianMatcher on the device -------------------------------------------------------------- */
/* A criterion pass handles NL prediction layers x B clips = NL*B independent "problems" (problem = layer*B +
 * clip) in one call.  Targets of the pass: tgt u8 [B][Nmax][T][H][W] -- binary masks, nonzero = set (the reference's
 * bool gt_masks, matcher.py:246; a clip with <= 32 targets is read through bit-interleaved words) -- with the per-clip count in DEVICE
 * memory (tgt_count[B]) so that distillation targets, whose number depends on teacher scores, need no host sync.
 * mask_logits are pixel-major [NL][B][T*hm*wm][ldq]; class_logits [NL][B][Q][2]. */

long s2d_matcher_workspace_floats(int NL, int B, int T, int P, int H, int W);

/* C[problem][Q][Nmax] (columns >= tgt_count[clip] are zero) = w_mask*cost_mask + w_class*cost_class +
 * w_dice*cost_dice at P shared random points per problem: matcher.py:236-287 (batch_sigmoid_ce_loss :38-62,
 * batch_dice_loss :15-30, point_sample).  coords [NL][B][P][2] injects the torch.rand(1,P,2) draws of :252
 * (parity mode); NULL = counter-based device RNG keyed by (seed, problem, point). */
int s2d_matcher_cost_f32(const float *mask_logits, const float *class_logits, const uint8_t *tgt, const int *tgt_count,
                         const float *coords, uint64_t seed, int NL, int B, int Q, int ldq, int T, int hm, int wm, int H,
                         int W, int Nmax, int P, float w_class, float w_mask, float w_dice, float *workspace, float *C,
                         hipStream_t stream);

/* Class-aware heads: s2d_matcher_cost_f32 on class_logits [NL][B][Q][C1] (C1 = C + 1 >= 2), class term -softmax_C1(l)[0]
 * (matcher.py:235-243: tgt_ids zeroed).  The workspace is s2d_matcher_c_workspace_floats floats (the cost pipeline's + the
 * [NL*B][Q] class column).  At C1 = 2 the cost matrix equals s2d_matcher_cost_f32's bit for bit. */
long s2d_matcher_c_workspace_floats(int NL, int B, int Q, int T, int P, int H, int W);
int s2d_matcher_cost_c_f32(const float *mask_logits, const float *class_logits, int C1, const uint8_t *tgt, const int *tgt_count,
                           const float *coords, uint64_t seed, int NL, int B, int Q, int ldq, int T, int hm, int wm, int H,
                           int W, int Nmax, int P, float w_class, float w_mask, float w_dice, float *workspace, float *C,
                           hipStream_t stream);

/* scipy.optimize.linear_sum_assignment (matcher.py:289) for nprob cost matrices C[problem][Q][Nmax] using the
 * first tgt_count[problem % B] columns.  idx_q/idx_t [nprob][min(Q,Nmax)] receive (query, target) pairs in scipy's
 * order (queries ascending), n_match[nprob] their number = min(Q, N).  Q <= 128, Nmax <= 128, Q*Nmax <= 12800. */
int s2d_lsap_f32(const float *C, const int *tgt_count, int nprob, int B, int Q, int Nmax, int *idx_q, int *idx_t,
                 int *n_match, hipStream_t stream);

/* ---- VideoSetCriterion on the device + distillation targets ------------------------------------------ */

/* prepare_distillation_targets (kd_video_maskformer_model.py:436-468, nms off): per clip keep the queries whose
 * teacher score softmax(logits)[q][0] is among the top `topk` and >= score_thr, in ascending query order, and
 * write masks = bilinear(teacher mask logits [B][T*hm*wm][ldq] -> (H,W), align_corners=False) > 0 as u8 planes
 * tgt [B][Nmax][T][H][W]; count[B], kept_q[B][Nmax], nonempty[B][Nmax][T] (DropLoss predicate) on the device. */
int s2d_kd_targets_u8(const float *t_class_logits, const float *t_mask_logits, float score_thr, int topk, int B, int Q,
                      int ldq, int T, int hm, int wm, int H, int W, int Nmax, uint8_t *tgt, int *count, int *kept_q,
                      int *nonempty, hipStream_t stream);

/* Class-aware s2d_kd_targets_u8 (kd_video_maskformer_model.py:436-468 with C = C1 - 1 >= 1 classes): top-`topk` over the
 * flattened softmax(l)[:, :-1] scores [Q*C] of each clip, kept when >= score_thr, emitted in ascending flat index q*C + c
 * (the order of the reference's topk(sorted=False) is undefined; at C = 1 this is s2d_kd_targets_u8's ascending query order).
 * label[b][n] = the pseudo target's class; a query may give several targets (one per label), each with its own plane.
 * workspace: s2d_kd_targets_c_workspace_bytes(B, Q, C1) bytes. */
long s2d_kd_targets_c_workspace_bytes(int B, int Q, int C1);
int s2d_kd_targets_c_u8(const float *t_class_logits, int C1, const float *t_mask_logits, float score_thr, int topk, int B, int Q,
                        int ldq, int T, int hm, int wm, int H, int W, int Nmax, void *workspace, uint8_t *tgt, int *count, int *kept_q,
                        int *label, int *nonempty, hipStream_t stream);

/* nonempty[b][n][t] = any(tgt[b][n][t]) for ground-truth targets (criterion.py:310-313). H*W % 16 == 0. */
int s2d_target_nonempty(const uint8_t *tgt, const int *count, int B, int Nmax, int T, int H, int W, int *nonempty,
                        hipStream_t stream);

/* H, W: the padded frame size of the targets (frames beyond 1.15 M pixels keep a bit-packed target plane per workgroup behind the
 * sample buffer: their plane does not fit LDS) */
long s2d_point_loss_workspace_bytes(int NL, int B, int Q, int Nmax, int T, int hm, int wm, int num_points,
                                    float oversample_ratio, float importance_ratio, int H, int W);

/* loss_masks for NL layers at once (criterion.py:292-356, point_features.py:63-116): losses[layer][0] = loss_mask,
 * [1] = loss_dice, both already divided by num_masks = max(sum_b tgt_count[b] / world_size, 1) (:404-409).
 * idx_q/idx_t/n_match from s2d_lsap_f32.  coords_over [NL][B*maxm*T][int(P*oversample)][2] and
 * coords_rand [NL][B*maxm*T][P - int(importance*P)][2] inject the two torch.rand draws of
 * point_features.py:90,112, indexed by the row's rank among the kept rows of its layer (parity mode);
 * NULL = device RNG.  drop_empty = temporal DropLoss ("masks-only" strategy, criterion.py:307-322). */
int s2d_point_loss_f32(const float *mask_logits, const uint8_t *tgt, const int *tgt_count, const int *nonempty,
                       const int *idx_q, const int *idx_t, const int *n_match, const float *coords_over,
                       const float *coords_rand, uint64_t seed, int NL, int B, int Q, int ldq, int T, int hm, int wm, int H,
                       int W, int Nmax, int num_points, float oversample_ratio, float importance_ratio, int drop_empty,
                       float world_size, void *workspace, float *losses, hipStream_t stream);

/* loss_labels (criterion.py:227-251) for one layer: class_logits [B][Q][2], idx_q [B][maxm], n_match [B]. */
int s2d_class_loss_f32(const float *class_logits, const int *idx_q, const int *n_match, int B, int Q, int maxm,
                       float eos_coef, float *loss_ce, hipStream_t stream);

/* s2d_class_loss_f32 on class_logits [B][Q][C1] (C1 >= 2): matched queries target class 0, the others class C1 - 1, weighted CE
 * with empty_weight (1, ..., 1, eos_coef) (criterion.py:227-251).  C1 = 2 gives s2d_class_loss_f32's bits. */
int s2d_class_loss_c_f32(const float *class_logits, int C1, const int *idx_q, const int *n_match, int B, int Q, int maxm,
                         float eos_coef, float *loss_ce, hipStream_t stream);

/* ---- eval-side step after the path: inference_video -------------------------------- */

/* kd_video_maskformer_model.py:532-538 (= video_maskformer_model.py:300-306): scores = softmax(class_logits
 * [Q][C+1])[:, :-1] flattened to [Q*C]; sorted top-K (descending; ties -> lower flat index); scores[K], query[K] =
 * flat // C, label[K] = flat % C on the device.  Q*C <= 16384, 1 <= K <= Q*C. */
int s2d_infer_select_f32(const float *class_logits, int Q, int C, int K, float *scores, int *query, int *label,
                         hipStream_t stream);

/* s2d_infer_select_f32 for any Q * C (no LDS bound; C = C1 - 1), same scores, sorted order and tie rule (equal scores: lower flat
 * index q*C + c first).  workspace: s2d_infer_select_c_workspace_bytes(Q, C1) bytes. */
long s2d_infer_select_c_workspace_bytes(int Q, int C1);
int s2d_infer_select_c_f32(const float *class_logits, int Q, int C1, int K, void *workspace, float *scores, int *query, int *label,
                           hipStream_t stream);

/* floats of workspace s2d_infer_masks_u8 needs (the K gathered low-resolution planes) */
long s2d_infer_workspace_floats(int K, int T, int hm, int wm);

/* 32-bit words of one bit-packed mask [T][oh][ow] (flat index i -> word i/32, bit i%32; tail bits zero) */
long s2d_mask_bit_words(int T, int oh, int ow);

/* masks[k] = bilinear( bilinear(mask_logits[query[k]] -> (Hp,Wp)) [:, :ih, :iw] -> (oh,ow) ) > 0, both resizes
 * align_corners=False, fp32, the expression tree of two F.interpolate calls (kd_video_maskformer_model.py:341-346,
 * :545-550).  mask_logits pixel-major [T*hm*wm][ldq]; masks u8 [K][T][oh][ow]; bits (may be NULL) [K][words] with
 * words = s2d_mask_bit_words(T,oh,ow).  Nothing of size [Q][T][Hp][Wp] is materialised. */
int s2d_infer_masks_u8(const float *mask_logits, int ldq, int T, int hm, int wm, int Hp, int Wp, int ih, int iw, int oh,
                       int ow, const int *query, int K, float *workspace, uint8_t *masks, uint32_t *bits,
                       hipStream_t stream);

/* Non-overlapping proposal index maps straight from the low-resolution logits (DAVIS unsupervised: one u8 label per pixel):
 * v_k = the two-stage bilinear value s2d_infer_masks_u8 thresholds, for proposal k's column query[k], formed by the same device
 * functions in the same float32 expression tree, so "proposal k holds the pixel" (v_k > 0; NaN and -0.0 hold nothing) is bit for
 * bit masks[k] of that call.  index u8 [T][oh][ow], every byte written: 0 = no proposal holds the pixel, k + 1 = proposal k.
 *   rule 0 ("rank")  1 + min{k : v_k > 0}: the best-ranked holder (query / score are in proposal order, best first, as
 *                    s2d_infer_select_f32 returns them); score may be NULL
 *   rule 1 ("prob")  among the holders, the k with the largest float32 score[k] / (1.f + expf(-v_k)); equal products: lower k
 * mask_logits pixel-major [T*hm*wm][ldq]; query int32 [K] (repeats allowed; an entry outside [0, ldq) is clamped into it),
 * score f32 [K], both on the device.  1 <= K <= 254 (255 is DAVIS' void label), ldq <= 128 and a multiple of 4, any oh / ow and
 * any alignment of index; offsets into index are 64-bit.  Nothing of size [K][T][oh][ow] exists at any point and no workspace
 * is needed: a workgroup stages the K selected columns of the logits under its 16 x 64 output tile in LDS, or, where K times
 * that window exceeds 40 KB, reads the logits directly.  Bad arguments return S2D_ERR_ARG and launch nothing. */
int s2d_infer_index_u8(const float *mask_logits, int ldq, int T, int hm, int wm, int Hp, int Wp, int ih, int iw,
                       int oh, int ow, const int *query, const float *score, int K, int rule,
                       uint8_t *index, hipStream_t stream);

/* bytes of LDS a workgroup of that call stages its window in (K * the largest window of any tile * 4); 0: the call takes the
 * direct path; -1: the sizes are refused */
long s2d_infer_index_lds_bytes(int ldq, int T, int hm, int wm, int Hp, int Wp, int ih, int iw, int oh, int ow, int K);

/* Stage-1 frame masks (s2d_amd/keymask/frame_masks.py; cutler/demo/predictor.py:237-355 overlay_masks_numpy), plane-free.  With
 * m_k,t = "proposal k holds the pixel", the bit s2d_infer_masks_u8 / s2d_infer_index_u8 form (same device functions, same float32
 * expression tree, v > 0; NaN and -0.0 hold nothing):
 *   areas int32 [K][T] (zeroed by the call) = set pixels of m_k,t at output size;
 *   order int32 [T][K] (may be NULL) = per frame the proposals in descending area, equal areas in proposal order: the stable sort
 *   s2d_mask_frame_areas_i32 documents, written by a follow-up launch of the same ranking kernel.
 * Same geometry, limits and refusals as s2d_infer_index_u8 (1 <= K <= 254, ldq <= 128 and a multiple of 4, query clamped); no
 * workspace, nothing of size [K][T][oh][ow].  Every proposal is evaluated at every pixel; a workgroup adds its tile's count once
 * per (k, t) with an integer atomic, so a second call gives the same bits.  Bad arguments: S2D_ERR_ARG, nothing launched. */
int s2d_infer_frame_areas_i32(const float *mask_logits, int ldq, int T, int hm, int wm, int Hp, int Wp, int ih, int iw,
                              int oh, int ow, const int *query, int K, int *areas, int *order, hipStream_t stream);

/* The paint pass: each frame starts black and the proposals are painted in order[t][0], order[t][1], ..., a later one over an
 * earlier one; so a pixel belongs to the holder with the LARGEST position in order[t] (with s2d_infer_frame_areas_i32's order: the
 * smallest area, among equal areas the higher k).  rgb u8 [T][oh][ow][3] = colors[k] (u8 [K][3]; by k, not by position) of that
 * owner or (0,0,0); index u8 [T][oh][ow] (may be NULL) = k + 1 of that owner or 0.  Every byte of both is written, at any alignment
 * (12 bytes of four pixels as three dwords where the address allows); 64-bit output offsets.  An order entry outside [0, K) is
 * clamped into it: a row that is no permutation gives unspecified colours and no out-of-range access.  Limits and refusals as
 * s2d_infer_index_u8. */
int s2d_infer_paint_u8(const float *mask_logits, int ldq, int T, int hm, int wm, int Hp, int Wp, int ih, int iw,
                       int oh, int ow, const int *query, int K, const int *order, const uint8_t *colors,
                       uint8_t *rgb, uint8_t *index, hipStream_t stream);

/* byte mask planes u8 [K][n] (0 / non-0) -> bit words [K][ceil(n/32)] in the layout above: feeds s2d_mask_pair_counts_u64 for
 * masks that exist as bytes -- the distillation pseudo targets under MODEL.MASK_FORMER.DISTILLATION_NMS
 * (kd_video_maskformer_model.py:484-520). */
int s2d_pack_mask_bits_u8(const uint8_t *masks, int K, long n, uint32_t *bits, hipStream_t stream);

/* inter[i][j] = sum(mask_i & mask_j) for all pairs of K bit-packed masks (diagonal = areas; sum(mask_i | mask_j) =
 * inter[i][i] + inter[j][j] - inter[i][j]): everything the greedy mask-NMS of :552-583 reads, in one launch instead
 * of two full-tensor reductions and a host sync per pair.  inter [K][K] (zeroed here).  This call, s2d_mask_plane_areas_u32,
 * s2d_mask_cross_counts_u64 and s2d_mask_frame_cross_counts_i32 are one set of kernels (csrc/mask_counts.hip). */
int s2d_mask_pair_counts_u64(const uint32_t *bits, int K, long words, unsigned long long *inter, hipStream_t stream);

/* ---- COCO run-length encoding of masks (wire format after inference_video / of the keymask annotations) ------- */

/* pycocotools rleEncode (third party, restated) of F binary masks u8 [F][H][W] (non-zero = set), column-major runs.
 * Pass 1: col_off [F][W] = exclusive count of run boundaries before column x (a boundary = pixel != its column-major
 * predecessor, the pixel before (0,0) counting as 0); nbound[F] = boundaries per mask (runs = nbound + 1); area[F] =
 * set pixels (mask_util.area); bbox [F][4] = x, y, w, h of the tight box, 0,0,0,0 if empty (mask_util.toBbox).
 * ytvis_eval.py:345-350, keymask_ident/annotations.py:100-106. */
int s2d_rle_count_u8(const uint8_t *masks, int F, int H, int W, int *col_off, int *nbound, int *area, int *bbox,
                     hipStream_t stream);

/* Pass 2: positions[frame_off[f] + i] = column-major index x*H + y of the i-th boundary of mask f (ascending);
 * frame_off[F] = exclusive prefix of nbound.  Run lengths are the differences (first run = positions[0], last =
 * H*W - positions[last]). */
int s2d_rle_positions_u8(const uint8_t *masks, int F, int H, int W, const int *col_off, const long *frame_off,
                         int *positions, hipStream_t stream);

/* maskApi.c rleToString on the device: the run lengths implied by `positions` (frame_off [F+1] = exclusive prefix of
 * nbound, ncounts = frame_off[F] + F runs in all) become the ASCII strings, concatenated in chars (capacity 7 * ncounts
 * bytes); str_off [F+1] = byte offset of every mask's string (str_off[F] = total).  hw = H*W.
 * workspace: s2d_rle_string_workspace_bytes(ncounts) bytes. */
long s2d_rle_string_workspace_bytes(long ncounts);
int s2d_rle_strings_u8(const int *positions, const long *frame_off, int F, long hw, long ncounts, void *workspace,
                       long workspace_bytes, uint8_t *chars, long *str_off, hipStream_t stream);

/* ---- YTVIS video-instance evaluation (s2d_amd/ytvis_eval.py; ytvoseval.py:176-222 computeIoU, ytvos.py:239-252 areas) -- */

/* pycocotools rleFrString (third party, restated) of F COCO RLE strings at once, one wave per string: string f is
 * chars[str_off[f] .. str_off[f+1]); its run ENDS (running sums of the counts, clamped to hw = H*W) go to
 * ends[str_off[f] + j], and nrun[f] = its number of runs.  Only frames with nrun[f] < 0 on entry are parsed: the others
 * already hold their ends (uncompressed RLE, prefixed on the host) or are absent (nrun = 0). */
int s2d_rle_parse_strings(const uint8_t *chars, const long *str_off, int F, long hw, int *ends, int *nrun, hipStream_t stream);

/* run ends (frame f: ends[run_off[f] .. + nrun[f]), column-major runs, the first one of zeros) -> bit planes
 * bits [F][ceil(H*W/32)] (row-major flat index i -> word i/32, bit i%32, tail bits zero: the s2d_pack_mask_bits_u8 layout
 * for planes of n = H*W).  A frame with nrun = 0 is an all-zero plane.  bits is zeroed by the call. */
int s2d_rle_decode_bits(const int *ends, const long *run_off, const int *nrun, int F, int H, int W, uint32_t *bits,
                        hipStream_t stream);

/* area[f] = popcount of plane f of bits [F][words_per_plane] (mask_util.area) */
int s2d_mask_plane_areas_u32(const uint32_t *bits, int F, long words_per_plane, unsigned *area, hipStream_t stream);

/* bbox [F][4] int = x, y, w, h of plane f of bits [F][words_per_plane] (words_per_plane = ceil(H*W/32), the layout above):
 * pycocotools rleToBbox (mask_util.toBbox) semantics, the tight box of the set pixels, 0,0,0,0 for an empty plane.  The
 * bboxes of the pseudo annotations written from a results.json (keymask_ident/convert_results_to_annotations.py:72). */
int s2d_mask_plane_bbox_u32(const uint32_t *bits, int F, int H, int W, long words_per_plane, int *bbox, hipStream_t stream);

/* inter[d][g] = sum over words of popcount(a[d] & b[g]) for D tracks a [D][words] against G tracks b [G][words] (a track =
 * its T frame planes back to back); inter [D][G] u64, zeroed by the call.  The D x G block of s2d_mask_pair_counts_u64. */
int s2d_mask_cross_counts_u64(const uint32_t *a, int D, const uint32_t *b, int G, long words, unsigned long long *inter,
                              hipStream_t stream);

/* Boundary band of F bit planes bits [F][ceil(H*W/32)] (the layout above; rows are not word-aligned unless W % 32 == 0), as
 * Boundary IoU defines it (Cheng et al., CVPR 2021; the published mask_to_boundary routine, restated): out = M & ~E, where
 * E is M eroded d times by a 3 x 3 square with everything outside the image counting as 0 -- one erosion by a
 * (2d+1) x (2d+1) square with a zero border, so every mask pixel within d of the image edge is boundary.  Valid for any
 * H, W >= 1 with H*W < 2^31 and any d >= 1 (2d+1 > min(H, W): E is empty and out = the mask); F times the tiles of a plane
 * (ceil(W/1024) word columns x about H/128 row bands at most) must stay below 2^31.  Input bits of a plane's last word at and
 * beyond H*W are ignored and written 0.  out [F][ceil(H*W/32)] may not alias bits; bitwise deterministic.
 * workspace: s2d_mask_boundary_workspace_words(F, H, W, d) words, 0 (workspace may be null) unless min(d, (min(H,W)+1)/2) > 64:
 * larger radii chain erosions of at most 64 through it.  The query returns -1 for arguments the call refuses. */
long s2d_mask_boundary_workspace_words(int F, int H, int W, int d);
int s2d_mask_boundary_bits_u32(const uint32_t *bits, int F, int H, int W, int d, uint32_t *workspace, long workspace_words,
                               uint32_t *out, hipStream_t stream);

/* The same band for a CHUNK of N images of different sizes in one launch (the COCO image evaluator: the planes of a chunk lie
 * in one flat buffer, and `out` is read by s2d_coco_mask_iou_ragged through the same img / tiles tables as `bits`).
 *
 * s2d_mask_boundary_ragged_plan is pure host code: it touches no device and runs on a machine without one.  spec is a HOST
 * int64 table [N][5] = {word0, F, H, W, d}: image n has F >= 0 planes of wpp = ceil(H*W/32) words, back to back from word
 * word0 of `bits`, and at the same offsets of `out` (COCO chunk layout: word0 = the image's dt_word, F = D + G).  It writes the
 * HOST int64 table plan [N][12], one row per image:
 *   0 word0   1 F   2 H   3 W      as given
 *   4 d       clamped to (min(H, W) + 1) / 2 (a window that does not fit leaves E empty: out = the mask)
 *   5 wpp     ceil(H*W / 32)
 *   6 S       row-aligned words per row, ceil(W / 32)
 *   7 TW      words per tile row: S cut evenly into ntx = ceil(S / 32) word tiles
 *   8 TR      rows per tile: H cut evenly into nty = ceil(H / (8192 / TW - 2d)) row bands
 *   9 ntx    10 nty
 *  11 wg0     the image's first workgroup: the exclusive prefix sum of F * ntx * nty
 * and *n_workgroups = the sum of F * ntx * nty, *lds_bytes = the largest 2 * TW * (TR + 2d) * 4 of any image that has planes
 * (0 if none has).  N == 0 and images with F == 0 are valid.  Returns S2D_ERR_ARG, with nothing written, for: H < 1, W < 1,
 * H*W >= 2^31, d < 1, F < 0; a clamped d above 64 (the ragged call is one pass: such an image goes through
 * s2d_mask_boundary_bits_u32, which chains passes); planes that leave [0, total_words); images whose word ranges overlap or
 * do not ascend; n_workgroups >= 2^31; lds_bytes > 65536.
 *
 * s2d_mask_boundary_ragged_u32 derives every plan row again from the first five columns of plan_host and refuses
 * (S2D_ERR_ARG, nothing launched, `out` untouched) a table that is not what the plan call writes; it also refuses a null
 * bits / out / plan_host / plan_dev and out == bits.  plan_dev is the caller's DEVICE copy of plan_host.  ONE kernel launch
 * for the whole chunk (none if no image has planes); when an image with planes has W % 32 != 0, one zero fill of
 * out[0 .. total_words) comes first.  Per plane the semantics are those of s2d_mask_boundary_bits_u32: padding bits are ignored
 * on input and written 0; bitwise deterministic.  Words of `out` that belong to no plane (gaps between images, the ranges of
 * images listed with F == 0 planes) are written 0 when the zero fill runs and are left alone otherwise: a caller that keeps
 * something there writes it after the call. */
int s2d_mask_boundary_ragged_plan(const long *spec, int N, long total_words, long *plan, long *n_workgroups, long *lds_bytes);
int s2d_mask_boundary_ragged_u32(const uint32_t *bits, long total_words, const long *plan_host, const long *plan_dev, int N,
                                 uint32_t *out, hipStream_t stream);

/* ---- DAVIS J&F evaluation (s2d_amd/davis_eval.py, csrc/davis_eval.hip; the davis2017 evaluation code restated, toolkit parity
 * unpinned).  All planes are in the flat layout above: [..][ceil(H*W/32)], pixel i -> word i/32, bit i%32, rows not word-aligned
 * unless W % 32 == 0; padding bits of a plane's last word are ignored on input and written 0. ------------------------------------ */

/* index u8 [T][H][W] (a DAVIS index PNG per frame) -> planes [K][T][wpf], plane k-1 = (index == k) for the labels 1..K, and
 * void_plane [T][wpf] = (index == 255).  Labels K+1..254 (and 0) set no bit.  0 <= K <= 254 (planes may be null for K = 0).  Every
 * output word is stored once: no zero fill is needed. */
int s2d_index_planes_u32(const uint8_t *index, int T, int H, int W, int K, uint32_t *planes, uint32_t *void_plane, hipStream_t stream);

/* seg2bmap without resize: out = (M != E) | (M != S) | (M != SE) for F planes, E / S / SE the east, south and south-east
 * neighbours with the image edge replicated (the last row compares only east, the last column only south, the bottom-right pixel
 * is 0).  out may not alias bits. */
int s2d_seg2bmap_bits_u32(const uint32_t *bits, int F, int H, int W, uint32_t *out, hipStream_t stream);

/* out = the F planes dilated by the disk {(dx, dy): dx^2 + dy^2 <= R^2}, pixels outside the image counting as 0; any H, W >= 1
 * with H*W < 2^31 (a disk larger than the image included), 1 <= R <= 64 in one pass; R > 64 returns S2D_ERR_ARG (disks do not
 * compose exactly on the lattice, so there is no chaining).  F times the tiles of a plane must stay below 2^31.  out may not alias
 * bits; bitwise deterministic. */
int s2d_disk_dilate_bits_u32(const uint32_t *bits, int F, int H, int W, int R, uint32_t *out, hipStream_t stream);

/* out [P][G][T] int32 = popcount(a[p][t] & b[g][t]) per frame, for a [P][T][words_per_frame] and b [G][T][words_per_frame]; zeroed
 * by the call.  T < 65536, words_per_frame < 2^26 (a plane of fewer than 2^31 pixels: every count fits).  The per-frame
 * companion of s2d_mask_cross_counts_u64, which sums whole tracks (the same kernel, csrc/mask_counts.hip). */
int s2d_mask_frame_cross_counts_i32(const uint32_t *a, int P, const uint32_t *b, int G, int T, long words_per_frame, int *out,
                                    hipStream_t stream);

/* ---- COCO image evaluation (s2d_amd/coco_eval.py, csrc/coco_eval.hip; COCOeval.computeIoU / evaluateImg and maskApi.c bbIou
 * restated, pycocotools parity unpinned).  Every call handles a CHUNK of N images of different sizes in one launch.
 *
 * Ragged layout.  The detections of the chunk are numbered flat, image after image (result order inside an image); so are the
 * ground truths (document order).  Per-detection arrays (area_d, dt_box [.][4], dt_area) and per-ground-truth arrays (area_g,
 * gt_box [.][4], gt_area, crowd, gt_ignore) are indexed by these flat numbers.  The pairs of an image are a row-major [D][G]
 * block; the blocks lie back to back in `inter` / `iou`.  img is a DEVICE int64 table [N][9], one row per image:
 *   0 dt_word  first word of the image's D detection planes in `bits` (planes back to back, `wpp` words each)
 *   1 gt_word  first word of its G ground-truth planes
 *   2 wpp      words per plane, ceil(H*W / 32): the plane layout of s2d_rle_decode_bits
 *   3 hw       H*W (< 2^31)
 *   4 D        5 G
 *   6 dt0      flat number of the image's first detection        7 gt0  of its first ground truth
 *   8 pair0    offset of its [D][G] block in `inter` / `iou`  (= sum of D*G of the images before it)
 * Columns 0-3 are read by the mask kernel only. ------------------------------------------------------------------------------- */

/* Mask IoU of every (detection, ground truth) pair of the chunk.  bits: all planes, placed as img says.  tiles: DEVICE int32
 * [n_tiles][3] = {image, ti, tj}: the 8 x 8 pair tile (detections 8*ti.., ground truths 8*tj..) one workgroup computes; the host
 * lists max(1, ceil(D/8)) * max(1, ceil(G/8)) tiles for every image with D + G > 0 (an image with only one kind still gets its
 * areas), each exactly once.  Outputs: inter[pair] = |d & g| (exact), area_d / area_g = pixels per plane, iou[pair] =
 * (double)i / (double)u with u = area_d + area_g - i, or u = area_d where crowd[g] != 0, and 0 where u == 0.  Bits of a plane's
 * last word at and beyond H*W are not counted.  Every output element is stored exactly once: no zero fill, no atomics, bitwise
 * deterministic. */
int s2d_coco_mask_iou_ragged(const uint32_t *bits, const long *img, int N, const int *tiles, int n_tiles, const uint8_t *crowd,
                             long long *inter, int *area_d, int *area_g, double *iou, hipStream_t stream);

/* Box IoU of every pair of the chunk, boxes [x, y, w, h] float64, in bbIou's operation order: w = min(x1+w1, x2+w2) - max(x1, x2),
 * h likewise; a pair with w <= 0 or h <= 0 is 0 (the clamp; no division); else i = w*h, u = crowd ? a_d : a_d + a_g - i with
 * a = w*h of each box, iou = i / u.  pair_off: DEVICE int64 [N+1] = pair0 of every image and the total n_pairs. */
int s2d_coco_box_iou_ragged(const double *dt_box, const double *gt_box, const uint8_t *crowd, const long *img, int N,
                            const long *pair_off, long n_pairs, double *iou, hipStream_t stream);

/* COCOeval.evaluateImg for n_groups groups x A area ranges x T thresholds in one launch.  A group is an image (or an image and a
 * category): groups is a DEVICE int64 table [n_groups][8] = {pair0, G_image (row stride of the image's IoU block), dt0, gt0,
 * dsel0, D, gsel0, G}; dsel[dsel0 .. +D) are the group's detections (flat numbers) in descending score order, already cut at
 * maxDets[-1]; gsel[gsel0 .. +G) its ground truths (flat numbers) in document order; dsel0 / gsel0 are the exclusive prefix sums
 * of D / G over the groups.  iou_thrs [T] and area_rng [A][2] are float64 DEVICE arrays, used as given.  Per problem (group, a):
 * the ground truths are stably sorted with the ignored ones last (ignored: gt_ignore != 0, or gt_area outside [lo, hi]); for each
 * threshold the detections are scanned in order, each over the sorted ground truths: a taken non-crowd one is skipped, the scan
 * stops at the first ignored one once a regular one is matched, iou < best is skipped (equal: the later wins; iou == t matches),
 * best starts at min(t, 1 - 1e-10).  An unmatched detection with dt_area outside the range is ignored.
 * Outputs (int32), with gb = A*gsel0 + a*G and db = A*dsel0 + a*D:
 *   gt_perm[gb + k]            position in gsel of the k-th sorted ground truth      gt_ignore_out[gb + k]  its ignore flag
 *   gt_match[T*gb + t*G + k]   position in dsel of the detection matched to it at threshold t, -1 if none
 *   dt_match[T*db + t*D + d]   sorted position k of the ground truth matched to detection d, -1 if none
 *   dt_ignore[T*db + t*D + d]  1 if the match is an ignored ground truth, or unmatched and out of range
 * Every element is stored; no inter-workgroup communication; all loop bounds are table entries. */
int s2d_coco_match(const double *iou, const long *groups, int n_groups, const int *dsel, const int *gsel, const double *dt_area,
                   const double *gt_area, const uint8_t *gt_ignore, const uint8_t *crowd, const double *iou_thrs, int T,
                   const double *area_rng, int A, int *dt_match, int *gt_match, int *dt_ignore, int *gt_ignore_out, int *gt_perm,
                   hipStream_t stream);

/* ---- Ragged RLE decode and the image self-training merge (s2d_amd/rle_ragged.py, s2d_amd/selftrain.py, csrc/rle_ragged.hip; the
 * reference's model_training/cutler/tools/get_self_training_ann.py).  The three calls above the keep rule are s2d_rle_parse_strings,
 * s2d_rle_decode_bits and s2d_mask_plane_bbox_u32 for a CHUNK of P planes of different sizes, one launch each; they share the device
 * bodies of those calls (csrc/rle_planes.h), so a plane comes out bit for bit as the fixed-size call writes it.
 *
 * Plane table.  plane is a DEVICE int64 table [P][4] = {word0, H, W, reserved 0}: plane p is H x W, row-major, in the
 * s2d_rle_decode_bits layout, ceil(H*W/32) words from word word0 of ONE flat buffer `bits` of total_words words.  With the planes of
 * an image back to back (its D planes, then its G planes) this is the COCO chunk layout above: s2d_coco_mask_iou_ragged reads the
 * buffer through its own img / tiles tables without a copy.  The caller checks the table (H, W >= 1, H*W < 2^31, word ranges inside
 * [0, total_words) and disjoint); a row that does not fit the buffer is skipped by the kernels (no read, no write; its box is 0,0,0,0).
 * All four calls only enqueue: no allocation, no synchronisation.  P == 0 (N == 0) is a no-op that returns S2D_OK; a negative count or
 * a null pointer returns S2D_ERR_ARG with nothing launched and nothing written. */

/* s2d_rle_parse_strings with the clamp hw = H*W of string f taken from plane[f]: one wave per string; strings with nrun[f] < 0 on entry
 * are parsed into ends[str_off[f] + j] and nrun[f] is set, the others (run ends already in place, or an absent plane with 0 runs) are
 * left alone.  str_off DEVICE int64 [P+1]. */
int s2d_rle_parse_ragged(const uint8_t *chars, const long *str_off, const long *plane, int P, int *ends, int *nrun, hipStream_t stream);

/* s2d_rle_decode_bits for the chunk.  run_off DEVICE int64 [P+1] (plane f owns the slots run_off[f] .. run_off[f+1]; nrun[f] beyond
 * them is cut).  tiles: DEVICE int32 [n_tiles][2] = {plane, column block of 256}; the host lists ceil(W/256) tiles for every plane,
 * each once (a plane without a tile stays all zero).  One launch with a 1-D grid over the tiles: a wave walks 64 columns of
 * its plane with that plane's H, W, word base and its own aligned = (W % 32 == 0) decision.  All total_words words of bits are zeroed
 * by the call, words of no plane included.  tiles may be null when n_tiles == 0. */
int s2d_rle_decode_ragged(const int *ends, const long *run_off, const int *nrun, const long *plane, int P, const int *tiles, int n_tiles,
                          uint32_t *bits, long total_words, hipStream_t stream);

/* s2d_mask_plane_bbox_u32 for the chunk: bbox [P][4] int = x, y, w, h of plane p (rleToBbox: the tight box), 0,0,0,0 for an empty
 * plane.  One workgroup per plane. */
int s2d_mask_plane_bbox_ragged_u32(const uint32_t *bits, const long *plane, int P, long total_words, int *bbox, hipStream_t stream);

/* The keep rule of the self-training merge on the outputs of s2d_coco_mask_iou_ragged (same img table), for a chunk whose D side is
 * the previous round's masks and whose G side is the kept predictions: keep[d] (int32, flat D numbering) = 1 iff EVERY g of the same
 * image has 2 * inter < area_d + area_g - inter (int64), so 1 for an image with G == 0.  This is the reference's
 * `iou_max < 0.5` on float32 inter / union, exactly, for images of fewer than 2^24 pixels; a pair with union == 0 (both masks empty)
 * fails the test, as the reference's NaN does.  inter / area_d / area_g / keep may be null when the chunk has no such element. */
int s2d_selftrain_keep_ragged(const long long *inter, const int *area_d, const int *area_g, const long *img, int N, int *keep,
                              hipStream_t stream);

/* s2d_mask_plane_areas_u32 for the chunk: area [P] = set bits of plane p (mask_util.area), the same device body; 0 for a row that
 * does not fit the buffer.  One workgroup per plane.  Arguments as s2d_mask_plane_bbox_ragged_u32's. */
int s2d_mask_plane_areas_ragged_u32(const uint32_t *bits, const long *plane, int P, long total_words, unsigned *area, hipStream_t stream);

/* The way back: bit planes of the chunk -> COCO RLE strings, the dual of the three calls above and the ragged form of
 * s2d_rle_count_u8 / s2d_rle_positions_u8 / s2d_rle_strings_u8, whose device bodies they run (csrc/rle_encode.h): the string of a
 * plane is byte for byte the string of the same byte mask.  They work on a SELECTION of planes, sel DEVICE int32 [S] (any order,
 * repeats allowed): only the planes a cleanup changed are encoded again.  col0 DEVICE int64 [S] = the widths W of the selection
 * before entry s, summed (the host knows them); col_off int32 [sum of W] is scratch between the first two calls.
 * s2d_rle_count_ragged_u32: nbound [S] = run boundaries of plane sel[s], area [S] its set pixels, bbox [S][4] = x, y, w, h (the tight
 * box, zeros for an empty plane).  s2d_rle_positions_ragged_u32: positions[frame_off[s] + j] = the column-major position of boundary
 * j; frame_off DEVICE int64 [S+1] = the exclusive scan of nbound.  s2d_rle_strings_ragged: as s2d_rle_strings_u8 with F = S and the
 * last run of entry s closed at its own H*W; ncounts = frame_off[S] + S; chars [7 * ncounts], str_off DEVICE int64 [S+1]; workspace
 * of s2d_rle_strings_ragged_workspace_bytes(ncounts) bytes.  Two read-backs per chunk: the boundary counts, then the strings.
 * An entry of sel that names no plane the buffer holds has no boundaries, area 0 and a zero box.  S == 0 is a no-op; a negative
 * count or a null pointer returns S2D_ERR_ARG with nothing launched. */
int s2d_rle_count_ragged_u32(const uint32_t *bits, const long *plane, int P, long total_words, const int *sel, int S,
                             const long *col0, int *col_off, int *nbound, int *area, int *bbox, hipStream_t stream);
int s2d_rle_positions_ragged_u32(const uint32_t *bits, const long *plane, int P, long total_words, const int *sel, int S,
                                 const long *col0, const int *col_off, const long *frame_off, int *positions, hipStream_t stream);
long s2d_rle_strings_ragged_workspace_bytes(long ncounts);
int s2d_rle_strings_ragged(const int *positions, const long *frame_off, const long *plane, int P, const int *sel, int S,
                           long ncounts, void *workspace, long workspace_bytes, uint8_t *chars, long *str_off, hipStream_t stream);

/* ---- Video self-training merge (s2d_amd/selftrain_video.py, csrc/selftrain_video.hip).  The rule is this project's own: the image
 * merge above carried to tubes (whole tracks); the reference has no video merge.  Both calls handle a CHUNK of N videos of different
 * sizes and lengths in one launch.
 *
 * Tube layout.  A track is its T frame planes back to back in the flat buffer of the ragged RLE decode (an absent frame is a plane
 * with 0 runs: all zero), so a track of an H x W video of T frames is T * wpp words.  The P side of a video (the previous round's
 * tracks) is its D tracks back to back, the Q side (the kept predictions) its G tracks.  P-side tracks of the chunk are numbered
 * flat, video after video; so are the Q-side tracks.  The pairs of a video are a row-major [D][G] block; the blocks lie back to
 * back in `inter` / `uni`.  videos is a DEVICE int64 table [N][11], one row per video:
 *    0 p_word  first word of the video's D P-side tracks in `bits`      1 q_word  first word of its G Q-side tracks
 *    2 wpp     words per plane, ceil(H*W / 32)                          3 hw      H*W (< 2^31)
 *    4 T       frames per track                                         5 D       6 G
 *    7 d0      flat number of the video's first P-side track            8 g0      of its first Q-side track
 *    9 pair0   offset of its [D][G] block in `inter` / `uni`           10 pres0   offset of its [D][T] block in `present`
 * present is a DEVICE uint8 array [n_present], n_present = sum of D*T: present[pres0 + d*T + t] != 0 where frame t is in the frame
 * set of P-side track d of the video (all ones when every frame counts).  A row that does not fit the buffers it names (negative
 * entries, wpp != ceil(hw/32), track words outside [0, total_words), present or pair block outside its array) is skipped by the
 * kernels: nothing is read or written for it. ------------------------------------------------------------------------------- */

/* Tube counts of every (P-side track d, Q-side track g) pair of the chunk, as unsigned 64-bit integers:
 *   inter[pair] = sum over the frames t of d's frame set of |d_t & g_t|
 *   uni[pair]   = sum over the same frames of |d_t| + |g_t| - |d_t & g_t|
 * A frame outside d's frame set adds nothing to either count of d's pairs.  Bits of a plane's last word at and beyond H*W are not
 * counted.  tiles: DEVICE int32 [n_tiles][3] = {video, ti, tj}: the 8 x 8 pair tile (P-side tracks 8*ti.., Q-side tracks 8*tj..); the
 * host lists ceil(D/8) * ceil(G/8) tiles for every video with D > 0 and G > 0, each exactly once.  max_track_words: the largest
 * T * wpp of the chunk (< 2^40); it only sizes the grid: the frame-words of a tile are split over workgroups whose partial sums are
 * added with integer atomics (a video whose T * wpp exceeds it is skipped).  accumulate == 0: inter and uni (n_pairs elements each)
 * are zeroed by the call; != 0: the call adds to what they hold, so a long video may be counted in slabs of frames, each slab its
 * own buffer, tables and call.  Exact integers, no float anywhere: the result does not depend on the order of the atomics and a
 * second call is bitwise equal.  The call only enqueues.  N == 0 or n_pairs == 0 is a no-op that returns S2D_OK; a negative count or
 * a null pointer returns S2D_ERR_ARG with nothing launched and nothing written (tiles may be null when n_tiles == 0). */
int s2d_tube_counts_ragged(const uint32_t *bits, long total_words, const long *videos, int N, const uint8_t *present, long n_present,
                           const int *tiles, int n_tiles, long max_track_words, unsigned long long *inter, unsigned long long *uni,
                           long n_pairs, int accumulate, hipStream_t stream);

/* The keep rule on the tube counts (same videos table; columns 5, 6, 7, 9 are read): keep[d] (int32 [n_keep], flat P-side numbering)
 * = 1 iff EVERY g of the same video has 2 * inter < uni (int64), so 1 for a video with G == 0.  A pair with uni == 0 (a track
 * with no frame in its frame set, or empty masks on both sides) fails the test, as in s2d_selftrain_keep_ragged.  inter / uni may
 * be null when n_pairs == 0, keep when n_keep == 0.  N == 0 is a no-op that returns S2D_OK; a negative count or another null
 * pointer returns S2D_ERR_ARG with nothing launched. */
int s2d_selftrain_keep_tube_ragged(const unsigned long long *inter, const unsigned long long *uni, long n_pairs, const long *videos, int N,
                                   int *keep, long n_keep, hipStream_t stream);

/* ---- test-time frame resize (s2d_amd/data/resize.py, data/test_loader.py): detectron2 ResizeTransform.apply_image =
 * PIL Image.resize(BILINEAR) on uint8 RGB frames, bit-exact ------------------------------------------------------------- */

/* LDS bytes of one s2d_resize_bilinear_u8 workgroup for a plan (rows_max input rows, span_q 16-byte chunks per staged row,
 * kh horizontal taps); a plan is launchable when this is <= 65536. */
long s2d_resize_lds_bytes(int rows_max, int span_q, int kh);

/* T frames src u8 [T][H0][W0][3] (HWC RGB) -> dst u8 [T][3][H1][W1] (CHW).  Per axis, PIL's coefficient table built on the host:
 * bounds int [out][2] = (first input index, tap count), coeffs int [out][k] = 22-bit fixed-point weights (k = kh / kv columns);
 * an axis of unchanged size takes the identity table (1 tap of weight 2^22).  Both tables are monotone (first index and first
 * index + count never decrease).  Horizontal pass first into a u8 intermediate, then vertical; every output is
 * clip8((2^21 + sum w * p) >> 22).  Launch plan: band_rows output rows per workgroup, rows_max >= input rows any band reaches,
 * span_q >= 16-byte chunks any 64-column tile's input span (from a 16-byte-aligned address) covers. */
int s2d_resize_bilinear_u8(const uint8_t *src, int T, int H0, int W0, const int *h_bounds, const int *h_coeffs, int kh,
                           const int *v_bounds, const int *v_coeffs, int kv, int H1, int W1, int band_rows, int rows_max,
                           int span_q, uint8_t *dst, hipStream_t stream);

/* ---- gradients of the dense layers: HBM-bound helpers around s2d_gemm_nt_f32 ----------- */

/* Weight-gradient contraction without transposed copies: C_slices[s][n][k] = sum over the rows m of slice s of
 * A[m][n] * B[m][k]  (A [rowsA][lda] = dY, B [rowsB][ldb] = X, both row-major; Mo = columns of A used, No = columns of B
 * used; slices of `chunk` rows (multiple of 32), ceil(rowsA / chunk) of them; rows m >= rowsB of B read as zero, so B may be
 * a view that starts some rows later, e.g. a convolution tap on the padded grid).  Same split-fp16 x3 arithmetic as
 * s2d_gemm_nt_f32 mode 2.  Slice s writes its [Mo][No] tile at C_slices + s * slice_stride (0 = Mo * No; larger: several
 * launches -- the taps of a convolution -- interleave their tiles so that one s2d_reduce_slices_f32 finishes them all).
 * Mo, No, lda, ldb multiples of 4; A, B 16-B aligned; each operand < 4 GiB.
 * colsum_slices (optional, [slices][Mo]): slice s also leaves the column sums of its rows of A -- the bias gradient of the same dY
 * (s2d_reduce_slices_f32 adds the slices) -- so dY is not read a second time for it. */
int s2d_gemm_tn_f32(const float *A, const float *B, float *C_slices, int Mo, int No, long rowsA, long rowsB, long lda, long ldb,
                    long chunk, long slice_stride, float *colsum_slices, hipStream_t stream);

/* Weight gradient of y = conv2d_nhwc(x [N][H][W][Cin], w [Cout][KH][KW][Cin], stride, pad), dy [N][Ho][Wo][Cout] (detectron2's Conv2d in the
 * R50 trunk and the pixel decoder, e.g. mask2former/modeling/pixel_decoder/msdeformattn.py:289-303; the reference leaves it to autograd's
 * convolution backward), on the TN kernel with the input pixel of every (output position, tap) addressed in place (pixels outside the image
 * read as zero): no padded copy of x, no copy of dy on the input grid.  ONE launch for all taps: slice s of the positions (chunk each, a
 * multiple of 32; S = ceil(N * Ho * Wo / chunk) <= 65535) leaves its partial gradients in part[s], laid out [Cout][KH][KW][Cin] like w;
 * s2d_reduce_slices_f32(part, S, Cout*KH*KW*Cin, Cout*KH*KW*Cin, beta, dw) finishes them in a fixed order.  Cin, Cout % 4 == 0, Ho, Wo > 1. */
int s2d_conv_wgrad_tn_f32(const float *dy, const float *x, int N, int H, int W, int Ci, int Ho, int Wo, int Co, int KH, int KW, int stride,
                          int pad, long chunk, float *part, hipStream_t stream);

/* out[c][r] = in[r][c]; in [R][ldi], out [C][ldo].  dW = dY^T . X runs as an NT GEMM on the transposed operands. */
int s2d_transpose_f32(const float *in, long R, long C, long ldi, float *out, long ldo, hipStream_t stream);

/* dst_t[i] += src_t[i] for a list of tensors in one launch (the "param.grad += g" glue of a training iteration): table [n][3] =
 * (src pointer, dst pointer, element count) as 64-bit words in DEVICE memory; block b adds elements [chunk_off[b], chunk_off[b] +
 * chunk) of tensor chunk_tensor[b].  No two entries may share a destination. */
int s2d_multi_add_f32(const long *table, const int *chunk_tensor, const long *chunk_off, int nchunks, int chunk, hipStream_t stream);

/* out[i] = beta * out[i] + sum_{s < S} part[s * stride + i], s ascending (fixed order: reproducible split-K) */
int s2d_reduce_slices_f32(const float *part, int S, long n, long stride, float beta, float *out, hipStream_t stream);
/* two such reductions with the same slice count in one launch (a weight gradient and its bias gradient): same bits as two calls */
int s2d_reduce_slices_pair_f32(const float *partA, long nA, long strideA, float betaA, float *outA, const float *partB, long nB, long strideB,
                               float betaB, float *outB, int S, hipStream_t stream);

/* part[s][c] = sum of in[r][c] over the rows of slice s (rows_per_slice rows each, ceil(R / rows_per_slice) slices):
 * bias gradients, finished by s2d_reduce_slices_f32 */
int s2d_colsum_slices_f32(const float *in, long R, long C, long ldi, long rows_per_slice, float *part, hipStream_t stream);

/* LayerNorm backward for y = LN(x + res) (res may be NULL) over the last dim C (C % 4 == 0, C <= 1024): dx [rows][C]
 * (= the gradient of x and of res), and per-workgroup partials part [blocks][2][C] (dgamma rows, then dbeta rows) with
 * blocks = s2d_layernorm_backward_blocks(rows); finish with s2d_reduce_slices_f32(part, blocks, 2*C, 2*C, ...). */
long s2d_layernorm_backward_blocks(long rows);
int s2d_layernorm_backward_f32(const float *x, const float *res, const float *dy, const float *gamma, long rows, int C,
                               float eps, float *dx, float *part, hipStream_t stream);

/* GroupNorm backward for y = GN_G(x) * gamma + beta, x / dy NHWC: dx, and per-block partials part_c
 * [s2d_groupnorm_backward_blocks(N,H,W)][2][C] (dgamma rows, dbeta rows), finished by s2d_reduce_slices_f32.  ws:
 * 2 * s2d_groupnorm_workspace_doubles(N,H,W,G) doubles.  The ReLU / upsample-add branches of the forward are separate
 * gradient steps (s2d_relu_scale_backward_f32, s2d_resize_bilinear_backward_nhwc_f32). */
long s2d_groupnorm_backward_blocks(int N, int H, int W);
int s2d_groupnorm_backward_f32(const float *x, const float *dy, const float *gamma, int N, int H, int W, int C, int G, float eps,
                               double *ws, float *dx, float *part_c, hipStream_t stream);

/* adjoint of bilinear_resize(up [N,hu,wu,C] -> (H,W), align_corners=False): dup [N,hu,wu,C] from dy [N,H,W,C] (gather
 * form, reproducible); the gradient of the upsample-add branch of s2d_groupnorm_nhwc_f32 (msdeformattn.py:349). */
int s2d_resize_bilinear_backward_nhwc_f32(const float *dy, int N, int H, int W, int C, int hu, int wu, float *dup,
                                          hipStream_t stream);

/* backward of s2d_maxpool3x3s2_nhwc_f32: dx [N,H,W,C] from x and dy [N,(H+1)/2,(W+1)/2,C]; ties go to the first maximum
 * in window scan order (torch's rule).  Gather form: reproducible. */
int s2d_maxpool3x3s2_backward_nhwc_f32(const float *x, const float *dy, int N, int H, int W, int C, float *dx,
                                       hipStream_t stream);
/* ... from the arg-max taps the forward stored (s2d_maxpool3x3s2_nhwc_idx_f32) instead of x: 4 bytes + (where the pixel is an arg-max) one dy row
 * per window, against 9 input rows per window for the recomputing form. */
int s2d_maxpool3x3s2_backward_idx_nhwc_f32(const unsigned char *argmax, const float *dy, int N, int H, int W, int C, float *dx,
                                           hipStream_t stream);

/* explicit im2col for convolutions with few input channels (the 7x7 stem): col [N*Ho*Wo][KH*KW*C] from x [N,H,W,C], zero
 * outside the image; the weight gradient is then one contraction dY^T . col (s2d_amd/backward.py:conv_weight_grad) */
int s2d_im2col_nhwc_f32(const float *x, int N, int H, int W, int C, int KH, int KW, int stride, int pad, float *col,
                        hipStream_t stream);

/* Depth-to-space step of a stride-2 3 x 3 convolution's input gradient (the R50 trunk's res3.0 / res4.0 / res5.0 conv2, STRIDE_IN_1X1 False):
 * the gradient is ONE stride-1 2 x 2 convolution of dY with 4 C output channels (a block of C per parity class (y & 1, x & 1) of the input
 * pixel; four ninths of the products of the zero-dilated form), G [N][Hg][Wg][4 C] with Hg = (H - 1) / 2 + 2, Wg = (W - 1) / 2 + 2, and
 * dx[n][y][x][c] = G[n][y / 2 + 1][x / 2 + 1][((y & 1) * 2 + (x & 1)) * C + c] * scale[c] (scale may be NULL), zeroed where gate [N][H][W][C]
 * (may be NULL) is <= 0.  C % 4 == 0. */
int s2d_pixel_shuffle2_gate_f32(const float *G, int N, int Hg, int Wg, int C, int H, int W, const float *scale, const float *gate, float *dx,
                                hipStream_t stream);

/* dz = dy * (y > 0) * scale[channel]: the gradient through y = relu(z * scale + bias), the conv / linear epilogue
 * (FrozenBN scale; scale NULL = 1; y NULL = no ReLU); dres (may be NULL) = dy * (y > 0), the gradient of a residual
 * added before the ReLU.  n elements, C innermost. */
int s2d_relu_scale_backward_f32(const float *dy, const float *y, const float *scale, long n, int C, float *dz, float *dres,
                                hipStream_t stream);

/* out = a + (y > 0 ? g : 0) over n elements (n % 4 == 0; out may alias a): a ResNet stage output's own gradient g joins the gradient a that the
 * next block returned already gated by that output's ReLU (y = the stage output), in one pass. */
int s2d_relu_gate_add_f32(const float *a, const float *g, const float *y, long n, float *out, hipStream_t stream);

/* ---- training-step callers after the loss: optimizer + EMA ------------------------------ */

/* Tensor table shared by the two entry points (all arrays on the device): ptrs [ntensors][5] = {param, grad or NULL,
 * exp_avg, exp_avg_sq, ema target or NULL} (float32 each, numel[i] elements); the work list (chunk_tensor[c],
 * chunk_off[c]) names a tensor and an element offset, `chunk` elements (multiple of 4) per entry, one workgroup each.
 *
 * GradScaler.unscale_ + clip_grad_norm_ over all parameters (train_net_video.py:188-203, engine/train_loop.py:709-726)
 * without touching the gradients and without a host sync: normbuf[0] = || grads * inv_scale ||_2, normbuf[1] =
 * min(1, max_norm / (norm + 1e-6)) (1 if max_norm <= 0), normbuf[2] = 1 if any gradient is inf/nan else 0.
 * partial: double[nchunks] scratch (fixed slots, fixed-order reduction: reproducible). */
int s2d_optim_grad_norm_f32(const void *const *ptrs, const long *numel, const int *chunk_tensor, const long *chunk_off,
                            int nchunks, int chunk, float inv_scale, float max_norm, double *partial, float *normbuf,
                            hipStream_t stream);

/* torch.optim.AdamW.step (train_net_video.py:205-213; single-tensor formula, fp32, its operation order) on
 * g * inv_scale * normbuf[1], fused with the EMA teacher update ema = ema_m * ema + (1 - ema_m) * param
 * (engine/train_loop.py:754-764; ema_m < 0: no EMA).  hyper [ntensors][2] = {lr, weight_decay} as double; lr is
 * multiplied by lr_factor (the scheduler's factor).  bias_correction1 = 1 - beta1^step, bias_correction2_sqrt =
 * sqrt(1 - beta2^step), formed by the caller in double as torch does.  normbuf NULL: no clipping, no inf check;
 * normbuf[2] != 0: parameters and moments are left untouched (GradScaler skips the step), the EMA still runs.
 * Tensors whose grad pointer is NULL get the EMA only.  The (unscaled, clipped) gradients are not written back. */
int s2d_optim_adamw_ema_f32(const void *const *ptrs, const long *numel, const double *hyper, const int *chunk_tensor,
                            const long *chunk_off, int nchunks, int chunk, double lr_factor, double beta1, double beta2,
                            double eps, double bias_correction1, double bias_correction2_sqrt, float inv_scale, double ema_m,
                            const float *normbuf, hipStream_t stream);

/* Backward of s2d_point_loss_f32: same arguments, the workspace the forward call left behind
 * (thresholds, tie state, stored point samples, per-row sums), plus the loss weights.  grad_rows
 * [NL*B*min(Q,Nmax)*T][hm*wm] = d(w_mask * loss_mask + w_dice * loss_dice, all layers) / d(logit map of row
 * ((layer*B + b)*maxm + slot)*T + t); rows of unmatched slots and dropped frames are zero.  The selected points are
 * exactly the forward's (same threshold, same tie rule); their gradients are scattered through the bilinear taps into an
 * LDS tile (one map part at a time) and written out once.  bit_scratch: unused (may be NULL) -- the forward leaves every target
 * plane of the pass bit-packed in the workspace.  Only for passes whose active rows all took the stored-sample path. */
int s2d_point_loss_backward_f32(const float *mask_logits, const uint8_t *tgt, const int *tgt_count, const int *nonempty,
                                const int *idx_q, const int *idx_t, const int *n_match, const float *coords_over,
                                const float *coords_rand, uint64_t seed, int NL, int B, int Q, int ldq, int T, int hm, int wm,
                                int H, int W, int Nmax, int num_points, float oversample_ratio, float importance_ratio,
                                int drop_empty, float world_size, void *workspace, float w_mask, float w_dice, float *grad_rows,
                                unsigned int *bit_scratch, hipStream_t stream);

/* Test hook for the RNG (timing) mode of s2d_point_loss_f32: the oversampled points of rows [0, nrows) for `seed` on an
 * (hm, wm) logit map, uv [nrows][n_over][2], and every row's strata bounds [nrows][9], from the same device functions the loss
 * kernels use.  The generator is this library's own (the reference draws torch.rand, point_features.py:89-93; parity tests inject
 * those draws): i.i.d. uniform points generated per map part -- an exact multinomial split over the parts' v bands, then uniform
 * inside each band -- which is the law of i.i.d. uniform points.  scratch_list: nrows + 1 ints.  row0 must be 0. */
int s2d_point_loss_rng_points(uint64_t seed, int hm, int wm, int row0, int nrows, int n_over, float *uv, int *bounds, int *scratch_list,
                              hipStream_t stream);

/* d(w_ce * loss_labels)/d(class_logits) for one layer (same arguments as s2d_class_loss_f32) -> [B][Q][2] */
int s2d_class_loss_backward_f32(const float *class_logits, const int *idx_q, const int *n_match, int B, int Q, int maxm,
                                float eos_coef, float w_ce, float *d_class_logits, hipStream_t stream);

/* d(w_ce * loss_labels)/d(class_logits) for class_logits [B][Q][C1] (same arguments as s2d_class_loss_c_f32) -> [B][Q][C1] */
int s2d_class_loss_backward_c_f32(const float *class_logits, int C1, const int *idx_q, const int *n_match, int B, int Q, int maxm,
                                  float eos_coef, float w_ce, float *d_class_logits, hipStream_t stream);

/* ---- keymask discovery (paths relative to /root/reference/keymask_ident) ------------------------------- */

/* pred_tracks_to_binary_masks(return_mask=False), cotracker_matching.py:453-503: tracks [T][Np][2] (x,y px) ->
 * masks u8 [T][H][W] (zeroed here); torch.round (half-to-even), keep 0<=x<W, 0<=y<H.  A point with a NaN or infinite coordinate is
 * dropped, as torch.round(x).long() (INT64_MIN) makes the reference drop it.  H and W < 2^24, else S2D_ERR_ARG. */
int s2d_tracks_to_masks_u8(const float *tracks, int T, int Np, int H, int W, uint8_t *masks, hipStream_t stream);

/* extract_mask_matches inner loops (:665-719) for ALL frames and object ids at once: counts[t][id] =
 * #(point pixels of frame t whose nearest-resized (:687-689) id-map value == id), total[t] = #point pixels.
 * compute_point_mask_intersection (:640-662) is then counts[t][oid] / total[t] (0.0 if total == 0), formed on the
 * host in double exactly as the reference's python float division.  idmap int64 [T][Hi][Wi] (:176-209). */
int s2d_point_id_counts(const uint8_t *point_masks, const int64_t *idmap, int T, int H, int W, int Hi, int Wi, int max_id,
                        int *counts, int *total, hipStream_t stream);

/* s2d_tracks_to_masks_u8 + s2d_point_id_counts in one launch without the [T][H][W] point mask: tracks f32 [T][P][2] (x,y px) in a
 * frame of H x W, idmap int64 [T][Hi][Wi] -> the same counts int32 [T][max_id+1] and total int32 [T], bit for bit.
 * One workgroup per frame: each point is rounded half to even and bounds-tested as s2d_tracks_to_masks_u8 does (points
 * with a non-finite coordinate are dropped), the frame's pixel keys are sorted in LDS and each distinct pixel is counted once
 * (two tracks on one pixel count once, as in the scattered mask), through the nearest rule of s2d_point_id_counts.
 * Limits: P <= 32768 (the LDS sort: 4 B per key, padded to a power of two, beside 4 (max_id + 2) B of histogram within the
 * 160 KiB of one CU), max_id <= 8190, H and W < 2^24; anything else returns S2D_ERR_ARG (callers with more points use the
 * two-launch path). */
int s2d_track_point_id_counts(const float *tracks, int T, int P, int H, int W, const int64_t *idmap, int Hi, int Wi, int max_id,
                              int *counts, int *total, hipStream_t stream);

/* get_segmentation_mask (keymask_ident/keymask_utils.py:37-67 == cotracker_matching.py:176-209) for a list of K (frame, object)
 * candidates: out u8 [K][H][W] = (idmap[frames[k]] == objs[k]) * 255, objs[k] == -1 selecting every non-background id.  frames /
 * objs are DEVICE int32 arrays (frame indices are not range-checked here: the caller built them from the same id map).  The
 * masks the cluster / group PNG trees hold (keymask_utils.py:100-126, cotracker_matching.py:402-431). */
int s2d_idmap_select_masks_u8(const int64_t *idmap, int T, int H, int W, const int *frames, const int *objs, int K, uint8_t *out,
                              hipStream_t stream);

/* presence[t][id] = id occurs in frame t (torch.unique at :680); u8 [T][max_id+1]. */
int s2d_idmap_presence_u8(const int64_t *idmap, int T, int Hi, int Wi, int max_id, uint8_t *presence, hipStream_t stream);

/* load_masks (cotracker_matching.py:22-84) after the PNG decode: rgb u8 [T][H][W][3] -> ids int64 [T][H][W], per frame
 * black = 0 and the other distinct colours 1..n in lexicographic (R,G,B) order; n_ids[T] = n.  At most 4096 distinct
 * colours per frame: *overflow is set to 1 otherwise (ids are then invalid).  workspace: s2d_color_ids_workspace_words(T)
 * 32-bit words. */
long s2d_color_ids_workspace_words(int T);
int s2d_color_masks_to_ids(const uint8_t *rgb, int T, int H, int W, unsigned int *workspace, int *n_ids, int64_t *ids,
                           int *overflow, hipStream_t stream);

/* cotracker_occlusions.py:359: curve[t] = mean_n(visibility[t][n] != 0). */
int s2d_visibility_curve_f32(const uint8_t *visibility, int T, int Np, float *curve, hipStream_t stream);

/* K1 (co-tracker is not in the reference tree; self-defined restatement, parity unpinned): local 4-D correlation
 * corr[t][n][i][j] = <bilinear(fmap[t], coords[t][n] + offset_i), support[n][j]> over C channels, offsets on the
 * (2r+1)^2 integer grid, zero padding.  fmap NHWC [T][H][W][C], coords [T][Np][2] in pixels of this level,
 * support [Np][(2r+1)^2][C], corr [T][Np][(2r+1)^2][(2r+1)^2].
 * Contract: C a multiple of 4 (16-B channel vectors), 0 <= r <= 3 (co-tracker's correlation radius is 3; a thread grid of
 * ceil(S/4)^2 <= 256 threads covers the S x S outputs), (S + 1)(C + 4) * 8 bytes of LDS <= 96 KB; anything else returns S2D_ERR_ARG. */
int s2d_local_corr_f32(const float *fmap_nhwc, const float *coords, const float *support, int T, int Np, int H, int W, int C,
                       int r, float *corr, hipStream_t stream);

/* Built-in baseline point tracker of keymask discovery (s2d_amd/keymask/block_tracker.py; self-defined -- the reference tracks with
 * CoTracker, third party): integer block matching on grey frames.  Both calls have exactly one correct output.
 * s2d_video_grey_u8: video f32 [T][3][H][W] (RGB, nominally 0..255) -> grey u8 [T][H][W]; per channel
 * c = (int)rintf(fminf(fmaxf(v, 0), 255)) (half to even; NaN -> 0; +-inf clamp), grey = (77 r + 150 g + 29 b + 128) >> 8. */
int s2d_video_grey_u8(const float *video, int T, int H, int W, uint8_t *grey, hipStream_t stream);

/* points int32 [N][2] = (x, y) inside the frame (DEVICE; a point outside is clamped into it), q the query frame -> tracks f32
 * [T][N][2] (integer-valued x, y), vis u8 [T][N] (0 / 1).  All coordinates clamp to the frame (border replicate).  Template of
 * point p: Tm[j][i] = grey[q][p.y + j][p.x + i], |i|, |j| <= R, never updated.  Frame q: track = p, visible.  Forward: c = p; for
 * t = q+1 .. T-1 the candidates are the (dx, dy), |dx|, |dy| <= S, whose centre c + (dx, dy) lies inside the frame, a candidate's
 * cost is sum |Tm[j][i] - grey[t][c.y + dy + j][c.x + dx + i]|, the best one is the minimum of (cost, dx^2 + dy^2, dy, dx) taken
 * lexicographically, and the point is visible iff cost <= tau (2R+1)^2; visible: c += (dx, dy); not visible: c stays, so a lost
 * point keeps searching round its last good position; tracks[t] = c, vis[t] = visible.  backward != 0: the same from c = p for
 * t = q-1 .. 0; otherwise frames t < q hold p with vis = 0.  It is computed by the search of s2d_block_track_live_u8 with
 * tau_u = -1.  One wave per (point, direction); no input makes the kernel read outside grey.  1 <= R <= 7, 1 <= S <= 24,
 * 0 <= tau <= 255, 0 <= q < T, H and W < 2^15; anything else returns S2D_ERR_ARG. */
int s2d_block_track_u8(const uint8_t *grey, int T, int H, int W, const int *points, int N, int q, int backward, int R, int S,
                       int tau, float *tracks, uint8_t *vis, hipStream_t stream);

/* The same tracker with a wider search and a live template (keymask/block_tracker.py LiveBlockTracker, --tracker block-live).
 * Inputs, outputs, clamping of points and border replicate as in s2d_block_track_u8.  Every (point, direction) -- forward, and
 * backward when backward != 0 -- carries its own template L, |i|, |j| <= R, which starts as the query-frame patch
 * L[j][i] = grey[q][p.y + j][p.x + i]; the two directions never share one.  Frame q: track = p, visible.  Forward: c = p; for
 * t = q+1 .. T-1 the candidates are the (dx, dy), |dx|, |dy| <= S, whose centre c + (dx, dy) lies inside the frame, a candidate's
 * cost is sum |L[j][i] - grey[t][c.y + dy + j][c.x + dx + i]| against the CURRENT L, the best one is the minimum of
 * (cost, dx^2 + dy^2, dy, dx) taken lexicographically, and the point is visible iff cost <= tau (2R+1)^2; visible: c += (dx, dy);
 * not visible: c stays and the point keeps searching round its last good position; tracks[t] = c, vis[t] = visible.  Then, if
 * the point is visible and cost <= tau_u (2R+1)^2, L[j][i] = grey[t][c.y + j][c.x + i] round the new c (border replicate);
 * otherwise L is kept.  tau_u = -1 never refreshes, tau_u = tau refreshes at every visible frame.  backward != 0: the same from
 * c = p and the query-frame patch for t = q-1 .. 0; otherwise frames t < q hold p with vis = 0.  With tau_u = -1 and S <= 24 the
 * output equals s2d_block_track_u8's bit for bit.  One wave per (point, direction); no input makes the kernel read outside grey.
 * 1 <= R <= 7, 1 <= S <= 64, 0 <= tau <= 255, -1 <= tau_u <= tau, 0 <= q < T, H and W < 2^15; anything else returns S2D_ERR_ARG. */
int s2d_block_track_live_u8(const uint8_t *grey, int T, int H, int W, const int *points, int N, int q, int backward, int R, int S,
                            int tau, int tau_u, float *tracks, uint8_t *vis, hipStream_t stream);

/* The live tracker's search under a zero-mean cost, with a texture gate (keymask/block_tracker.py ZeroMeanBlockTracker, --tracker
 * block-zm).  Inputs, tracks, vis, clamping of points, border replicate, candidates (|dx|, |dy| <= S, centre inside the frame),
 * the lexicographic minimum (cost, dx^2 + dy^2, dy, dx), one template per (point, direction), frames t < q without backward
 * tracking and frame q as in s2d_block_track_live_u8.  With P = 2R+1, n = P^2 and, for a patch X of n bytes,
 * mean(X) = (2 sum(X) + n) / (2 n) (integer division: the mean, half rounds up),
 *     zcost(L, X) = sum_i |(L_i - mean(L)) - (X_i - mean(X))|   (< 2^17),      dev(L) = sum_i |L_i - mean(L)|:
 * a candidate's cost is zcost(L, the patch round the candidate) against the current template L; the point is visible iff
 * cost <= tau n and then moves there; L becomes the patch round the new c iff visible and cost <= tau_u n (tau_u = -1: never).
 * Adding one constant to every pixel of a frame adds it to every mean of that frame, so as long as no pixel saturates the
 * output does not change.  Gate: a point is trackable iff dev(its query-frame patch) >= texture n (texture = 0: every point);
 * an untrackable point is not searched: tracks[t] = p at every t, vis = 1 at q only.  trackable u8 [N] receives the flag.
 * One wave per (point, direction); no input makes the kernel read outside grey.  1 <= R <= 7, 1 <= S <= 64, 0 <= tau <= 255,
 * -1 <= tau_u <= tau, 0 <= texture <= 127, 0 <= q < T, H and W < 2^15; anything else returns S2D_ERR_ARG.  N == 0: no launch. */
int s2d_block_track_zm_u8(const uint8_t *grey, int T, int H, int W, const int *points, int N, int q, int backward, int R, int S,
                          int tau, int tau_u, int texture, float *tracks, uint8_t *vis, uint8_t *trackable, hipStream_t stream);

/* ---- timing helpers for the benchmark's per-launch roofline (not on the data path) ------------------------ */

/* HIP events created with hipEventDisableSystemFence (handles are opaque integers, 0 = failure). */
long s2d_prof_event_create(void);
int s2d_prof_event_record(long ev, hipStream_t stream);
int s2d_prof_event_elapsed(long ev_start, long ev_end, double *out_ms_host);
int s2d_prof_event_destroy(long ev);

/* ---- data-side step before the hot path: clip augmentation and video copy-paste on the device ---------- */

/* The dataset mapper's augmentation chain (data_video/dataset_mapper.py:306-404 with augmentation.py:116-168: crop,
 * resize-shortest-edge, flip, brightness, contrast, rotation) as one resampling pass per frame.  frames u8 [T][3][H0][W0] ->
 * out u8 [T][3][H1][W1].  aug_frames_dev: DEVICE array of T records of 16 floats
 *   {a11, a12, a13, a21, a22, a23,  cx, cy, cw, ch,  bright, contrast, cmean, 0, 0, 0}:
 * output pixel centre (x + .5, y + .5) -> source point A . (x + .5, y + .5, 1); read only inside the crop rectangle
 * (outside: 0, the rotation fill; taps clamped to it); bilinear -> round -> brightness (img * w, clip, truncate) ->
 * contrast ((1 - w) * cmean + w * img, clip, truncate), the BlendTransform arithmetic.  cmean < 0: filled in by the call with
 * the crop's mean x bright (what RandomContrast measures).  detectron2 (absent from the reference tree) runs one image pass
 * per transform; the single-pass composition is this library's definition: parity unpinned. */
int s2d_aug_warp_frames_u8(const uint8_t *frames, int T, int H0, int W0, void *aug_frames_dev, int H1, int W1, uint8_t *out,
                           hipStream_t stream);
/* instance masks u8 [N][T][H0][W0] (0 / non-0) -> u8 [N][T][H1][W1] (0 / 1) under the same per-frame maps, nearest source
 * pixel (apply_segmentation). */
int s2d_aug_warp_masks_u8(const uint8_t *masks, int N, int T, int H0, int W0, const void *aug_frames_dev, int H1, int W1, uint8_t *out,
                          hipStream_t stream);
/* s2d_aug_warp_frames_u8 for frames u8 [T][H0][W0][3] (the layout a JPEG decodes to); out stays u8 [T][3][H1][W1] and is
 * bit-identical to s2d_aug_warp_frames_u8 on the planar copy.  The crop mean is summed as integers over many workgroups per
 * frame; the last two words of each record (record floats 14..15) are its scratch: 0 on entry, 0 again on return. */
int s2d_aug_warp_frames_hwc_u8(const uint8_t *frames, int T, int H0, int W0, void *aug_frames_dev, int H1, int W1, uint8_t *out,
                               hipStream_t stream);
/* Annotation masks straight from bit planes bits [P][words_per_plane] (row-major H0 x W0, the s2d_pack_mask_bits_u8 /
 * s2d_rle_decode_bits layout), in the clip's slot order: plane_of DEVICE int32 [T][S] names the plane of slot s at frame t
 * (-1: the mapper's dummy slot, an all-zero plane, nothing read; the host guarantees plane_of < P).  out u8 [T][S][H1][W1]
 * (0 / 1, frame-major), the pixel rule of s2d_aug_warp_masks_u8; area u32 [T][S] = pixels of each output plane (zeroed by the
 * call).  S == 0 is a no-op. */
int s2d_aug_warp_mask_bits(const uint32_t *bits, long words_per_plane, const int *plane_of, int S, int T, int H0, int W0,
                           const void *aug_frames_dev, int H1, int W1, uint8_t *out, unsigned *area, hipStream_t stream);
/* Polygon annotations -> bit planes in the same layout (s2d_amd/data/image_clip.py: COCO image annotations as pseudo-clips).
 * verts f32 [V][2] = (x, y) in source-pixel coordinates, any values; poly_off int32 [NP+1] = vertex range of every polygon;
 * plane_off int32 [P+1] = polygon range of every plane (both DEVICE; the *_host copies are what is validated: offsets that are
 * negative, decreasing or past V / NP are S2D_ERR_ARG).  Plane p goes to row dst_plane[p] of bits [rows][ceil(H*W/32)]
 * (DEVICE int32 [P], distinct rows; NULL: row p, and rows >= P), so that the polygon planes of a record land between its RLE
 * planes; a row outside [0, rows) is not written.  Pixel (x, y) is set iff its centre (x + 0.5, y + 0.5) is inside at least one
 * of the plane's polygons by the even-odd rule: edge (x0, y0)-(x1, y1) counts when (y0 <= cy) != (y1 <= cy) and
 * cx < x0 + (cy - y0) * (x1 - x0) / (y1 - y0) (float32); a polygon closes last vertex -> first; fewer than 3 vertices set
 * nothing; a plane without polygons is all zero.  Every word of the P rows is stored exactly once (tail bits zero): no zero fill,
 * no atomics.  rows * ceil(H*W/32) must stay below 2^31.  The rule is this library's: pycocotools frPoly parity is unpinned at
 * boundary pixels. */
int s2d_polygons_to_bits(const float *verts, int V, const int *poly_off, const int *poly_off_host, int NP, const int *plane_off,
                         const int *plane_off_host, int P, const int *dst_plane, int rows, int H, int W, uint32_t *bits,
                         hipStream_t stream);

/* Sparse-mask densification of the trainer (`propagate_sparse_masks`, mask2former_video/engine/train_loop.py:30-156): all output
 * planes of a clip in one launch.  plan_dev: n_planes records {uint64 address of a source plane (bool / u8 [H, W], device memory),
 * int32 dx, int32 dy} (16 bytes each); out [n_planes][H][W] u8: out[j][y][x] = src_j[y + dy][x + dx] != 0 inside the frame, else 0 --
 * the reference's `_translate` (:58-68) for the instances an id's last sighting fills in, dx = dy = 0 for the instances a frame keeps.
 * A u8 source may hold any non-zero value for "set"; every output byte is 0 or 1, on the aligned 16-byte path as on the byte path.
 * Which planes, and the (dx, dy) draws in the reference's `random.randint` order, are the host's plan (s2d_amd/data/copy_paste.py). */
int s2d_shift_planes_u8(const void *plan_dev, int n_planes, int H, int W, uint8_t *out, hipStream_t stream);

/* One target frame of the trainer's video copy-paste loop exactly as written (engine/train_loop.py:445-570): the K copied masks
 * cur_masks [K][Hc][Wc] -- the source masks at the first frame, the PREVIOUS frame's canvas afterwards (the reference reassigns
 * copied_instances.gt_masks to the pasted canvas every frame, :512-514, so the masks are transformed cumulatively) -- and the source
 * frame [3][Hs][Ws] are resized to (h_new, w_new) with F.interpolate(bilinear, align_corners=False) (masks .bool(), image .byte()),
 * placed at (h_shift, w_shift): canvas u8 [K][H][W]; out_frame = alpha ? pasted source : target; out_tgt [N][H][W] = target masks
 * minus alpha; inter [K][N] / tarea [N] (before alpha: the ioy matrix of :517-527) and alive [N] (target areas after, :543) as
 * int32 counts.  K <= 64.  Used by s2d_amd/data/copy_paste.py, which keeps every decision of the loop on these integers. */
int s2d_copy_paste_frame_u8(const uint8_t *src_frame, int Hs, int Ws, const uint8_t *cur_masks, int K, int Hc, int Wc,
                            const uint8_t *tgt_frame, const uint8_t *tgt_masks, int N, int H, int W, int h_new, int w_new, int h_shift,
                            int w_shift, uint8_t *canvas, uint8_t *out_frame, uint8_t *out_tgt, int *inter, int *tarea, int *alive,
                            hipStream_t stream);

/* Video copy-paste, engine/train_loop.py:441-560: K source masks [K][Hs][Ws] and their frame [3][Hs][Ws] are resized to
 * (h_new, w_new) per target frame with F.interpolate(bilinear, align_corners=False) (image .byte(), masks .bool()), placed at
 * (h_shift, w_shift) and composited over the target clip: out_frames u8 [T][3][H][W]; out_masks u8 [N+K][T][H][W] = the N
 * target masks minus the pasted area, then the K pasted masks (all zero for copies with keep[k] == 0).  paste_frames_dev:
 * DEVICE int32 [T][4] = {h_new, w_new, h_shift, w_shift}; keep_dev: DEVICE u8 [K].
 * s2d_copy_paste_overlap: counts[k][n] = |pasted copy k AND target n| and area[n] = |target n| on frame 0, the integers behind
 * the "intersection over target area < 0.5" rule that decides keep (:515-527). */
int s2d_copy_paste_overlap(const uint8_t *tgt_masks, int N, int T, int H, int W, const uint8_t *src_masks, int K, int Hs, int Ws, int h_new,
                           int w_new, int h_shift, int w_shift, int *counts, int *area, hipStream_t stream);
int s2d_copy_paste_u8(const uint8_t *tgt_frames, const uint8_t *tgt_masks, int N, int T, int H, int W, const uint8_t *src_frame,
                      const uint8_t *src_masks, int K, int Hs, int Ws, const int *paste_frames_dev, const uint8_t *keep_dev,
                      uint8_t *out_frames, uint8_t *out_masks, hipStream_t stream);

/* ---- video demo rendering (s2d_amd/demo.py; model_training/demo_video/demo.py, predictor.py) ------------------------------------- */

/* areas int32 [K][T] = set (non-zero) bytes of every plane of masks u8 [K][T][H][W] (the s2d_infer_masks_u8 layout; zeroed by the
 * call); with order != null, order int32 [T][K] = per frame the instances in descending order of their area there, equal areas in
 * instance order (a stable sort; numpy's argsort(-areas) for K <= 16).  K <= 255, T <= 65535; anything else returns S2D_ERR_ARG. */
int s2d_mask_frame_areas_i32(const uint8_t *masks, int K, int T, int H, int W, int *areas, int *order, hipStream_t stream);

/* The demo's overlay and mask index map in one pass.  frames u8 [T][H][W][3] (RGB) -> overlay u8 [T][H][W][3]: per frame the K
 * instances are drawn in the order order int32 [T][K]; for instance k, every pixel p of its mask becomes
 * (c_k * alpha + p * (256 - alpha) + 128) >> 8 per channel, and a mask pixel with a 4-neighbour outside the frame or outside mask k
 * becomes c_k (colors u8 [K][3]).  index u8 [T][H][W] (skipped when null) = 1 + the highest k whose mask holds the pixel, 0 where
 * none does.  K = 0 copies the frames.  Any alignment and row width; K <= 255, T <= 65535, 0 <= alpha <= 256; otherwise
 * S2D_ERR_ARG. */
int s2d_render_instances_u8(const uint8_t *frames, int T, int H, int W, const uint8_t *masks, int K, const int *order,
                            const uint8_t *colors, int alpha, uint8_t *overlay, uint8_t *index, hipStream_t stream);

/* ---- windowed inference of long videos (s2d_amd/modeling/window_inference.py) ------------------------------ */

/* Cross-window mask counts from two pixel-major fp32 logit blocks A, B [n][ldq] (the frames two consecutive windows share, n =
 * O*hm*wm rows): with a_i = (A[:, i] > 0) and b_j = (B[:, j] > 0) for the Q query columns (so -0.0, 0.0 and NaN are outside the
 * mask), inter [Q][Q] = |a_i & b_j|, area_a [Q] = |a_i|, area_b [Q] = |b_j|, all int64 and zeroed by the call.  The pad columns
 * Q .. ldq-1 may hold anything.  No planes or byte masks are written: the blocks are read once.  Q <= ldq <= 128, ldq a multiple
 * of 4, A and B 16-byte aligned, n < 2^31. */
int s2d_window_pair_counts(const float *A, const float *B, long n, int ldq, int Q, int64_t *inter, int64_t *area_a,
                           int64_t *area_b, hipStream_t stream);

/* dst[row0 + r][p] = src[r][perm[p]] for r < rows and p < Q; the pad columns Q <= p < ldq are copied as they are.  src [rows][ldq],
 * dst [>= row0 + rows][ldq] 16-byte aligned, perm DEVICE int32 [Q] (an entry outside [0, Q) reads column p itself).  A window's
 * owned rows go into the stitched buffer in track order in one pass.  Q <= ldq <= 128, ldq a multiple of 4. */
int s2d_window_scatter_columns(const float *src, long rows, int ldq, int Q, const int *perm, float *dst, long row0,
                               hipStream_t stream);

/* ---- connected components of index maps (s2d_amd/index_components.py) --------------------------------------- */

/* index u8 [N][H][W] is a map as s2d_infer_paint_u8 / s2d_infer_index_u8 write it: 0 = background, any other byte (255 included) an
 * instance id.  A component is a maximal set of pixels of ONE non-zero id connected under conn = 4 or 8; pixels of different ids
 * never join and background is not labelled.  All ids of a frame in one pass, no plane per id.
 * s2d_index_components_tile: the tile (th rows x tw columns) a workgroup labels locally before the tiles are merged.
 * s2d_index_components_workspace_bytes: the scratch both calls below need for [N][H][W] (any address; the calls align it themselves);
 * S2D_ERR_ARG for N, H or W < 1 or H*W >= 2^31 - 1.
 * s2d_index_components_i32: labels i32 [N][H][W] = 0 on background, else 1 + (y*W + x) of the component's first pixel in raster
 * order -- a name that depends on nothing but the map, so a second call is bitwise equal and any host labelling compares by
 * equality.  area i32 [N][H][W] (may be NULL): area[n][p] = pixels of the component whose first pixel is p, 0 everywhere else.
 * Three launches (tile-local union-find in LDS; lock-free merge across tile borders through agent-scope atomics; flatten, with one
 * integer atomic per tile-local component for the areas), none of which waits for another workgroup.
 * s2d_index_filter_components_u8 (labels, area: what the call above wrote for index): a component is kept iff area >= min_area and,
 * with keep_largest != 0, it is the largest component of its (image, id), among equal areas the one with the lowest first pixel.
 * out u8 [N][H][W] = index where the pixel's component is kept, else 0; out may be index.  rgb u8 [N][H][W][3] (may be NULL) is
 * changed in place: the three bytes of every removed pixel become 0 and no other byte is touched.  removed i32 [N] = pixels removed
 * per image (zeroed by the call, like the [N][256] table of largest components in the workspace).
 * Any H, W >= 1 and any alignment of the byte arrays and of the workspace; the i32 arrays are 4-byte aligned.  conn other than 4 or
 * 8, N, H or W < 1, H*W >= 2^31 - 1, min_area < 0, a NULL pointer other than area (components) or rgb (filter) or a misaligned i32
 * array return S2D_ERR_ARG before anything is launched. */
int s2d_index_components_tile(int *th, int *tw);
long s2d_index_components_workspace_bytes(int N, int H, int W);
int s2d_index_components_i32(const uint8_t *index, int N, int H, int W, int conn, int *labels, int *area, void *workspace,
                             hipStream_t stream);
int s2d_index_filter_components_u8(const uint8_t *index, const int *labels, const int *area, int N, int H, int W, int min_area,
                                   int keep_largest, uint8_t *out, uint8_t *rgb, int *removed, void *workspace, hipStream_t stream);

/* s2d_index_fill_holes_u8 fills the holes the filter above (or the model) leaves in such a map.  conn = 4 or 8 is the connectivity
 * of the INSTANCES; the zero pixels of an image are labelled under the complementary connectivity c' (8 -> 4, 4 -> 8), as
 * s2d_plane_clean_ragged does.  A zero component is a hole iff none of its pixels lies in row 0, row H-1, column 0 or column W-1.
 * The owners of a hole are the ids of the non-zero pixels that are c'-neighbours of one of its pixels (every c'-neighbour of a hole
 * outside it is an instance pixel, and exists: a hole never touches the frame border).  A hole is filled iff its area <=
 * max_hole_area (2^31 - 1: all) AND it has exactly ONE owner k: every one of its pixels becomes k in out and, with rgb given,
 * colors[k-1] in rgb.  A hole with two or more owners (the gap between two instances, the ring round an island of another id) stays
 * as it is, and so does, with rgb given, a hole whose owner k > n_colors: map and picture never disagree.  Nothing but zero pixels
 * ever changes; the rule is idempotent, raises the component count of no id and lowers no component's area.
 * out u8 [N][H][W] may be index.  rgb u8 [N][H][W][3] may be NULL; then colors / n_colors are ignored.  colors is a DEVICE u8 array
 * [n_colors][3], 1 <= n_colors <= 255.  filled i32 [N] = pixels set per image (zeroed by the call).
 * s2d_index_fill_holes_workspace_bytes: the scratch the call needs (16 bytes per pixel; any address); S2D_ERR_ARG as above.
 * The zero pixels go through the three labelling launches above (the tile is s2d_index_components_tile); a pass over the zero
 * pixels gives every root the integer min and max of its owners' ids, plus a value above any id from a pixel on the frame border
 * (one owner <=> max == min), aggregated per workgroup in LDS so that a frame-sized hole does not queue on one address; a pass per
 * aligned 4-byte word writes out.  Integer atomics only, no workgroup waits for another: a second call is bitwise equal.  The call
 * only enqueues.  conn other than 4 or 8, N, H or W < 1, H*W >= 2^31 - 1, max_hole_area < 1, a NULL pointer other than rgb (or
 * colors with rgb NULL), n_colors outside 1..255 with rgb given or a misaligned filled return S2D_ERR_ARG before anything is
 * launched.  Any alignment of the byte arrays and of the workspace. */
long s2d_index_fill_holes_workspace_bytes(int N, int H, int W);
int s2d_index_fill_holes_u8(const uint8_t *index, int N, int H, int W, int conn, int max_hole_area, uint8_t *out, uint8_t *rgb,
                            const uint8_t *colors, int n_colors, int *filled, void *workspace, hipStream_t stream);

/* ---- connected components and cleanup of ragged bit planes (s2d_amd/plane_components.py) -------------------- */

/* bits u32 [total_words] and plane DEVICE int64 [P][4] = {word0, H, W, 0} are a chunk as s2d_rle_decode_ragged fills it: plane p is
 * H x W pixels, pixel i = y*W + x in word word0 + i/32, bit i%32; rows are not word-aligned, pixel (y, W-1) and pixel (y+1, 0) are
 * flat neighbours and never join.  The padding bits of a plane's last word are ignored on input and 0 on output.  The planes of a
 * chunk overlap as masks, so every plane is labelled on its own, all of them in one launch: tiles DEVICE int32 [n_tiles][3] =
 * {plane, tile row, tile column} lists every tile of every plane once (built on the host; the grid is 1-D over it).  A table row that
 * names no tile of a plane the buffer holds is skipped, as a plane row that does not fit the buffer is.
 * s2d_plane_components_tile: the tile (th rows x tw columns) a workgroup labels locally before the tiles are merged.
 * s2d_plane_components_workspace_bytes: the scratch either call below needs (any address; the calls align it themselves): 12 bytes
 * per pixel position of the buffer and 8 per plane; S2D_ERR_ARG (-1) for a negative argument.
 * s2d_plane_components_ragged labels the pixels whose bit equals value (0 or 1) under conn = 4 or 8.  labels and area are i32 arrays
 * of 32 * total_words elements, pixel i of plane p at 32 * word0 + i (a 64-bit index); positions of no pixel hold 0.  labels = 0
 * where the bit is not value, else 1 + the flat index i of the component's first pixel in its plane -- a name that depends on
 * nothing but the plane, so a second call is bitwise equal.  area (may be NULL) holds the component's pixel count at its first pixel
 * and 0 elsewhere.  With value = 0 padding bits and everything outside the plane are not pixels: they join nothing, add no area.
 * s2d_plane_clean_ragged writes out = fill(filter(plane)) for every plane; out may be bits.  This rule is the project's own (the
 * reference cleans nothing).  filter (min_area > 0 or keep_largest != 0): a component of set pixels under conn is kept iff area >=
 * min_area and, with keep_largest, it is the largest of its plane, among equal areas the one with the lowest first pixel; every
 * other set pixel becomes 0.  fill (max_hole_area > 0): the ZERO pixels of the filtered plane are labelled under the complementary
 * connectivity (8 -> 4, 4 -> 8); a component none of whose pixels lies in row 0, row H-1, column 0 or column W-1 is a hole, and a
 * hole of at most max_hole_area pixels becomes set.  removed i32 [P] / filled i32 [P] = pixels cleared / set per plane (zeroed by
 * the call).  With all three options off the planes are copied with their padding zeroed.  Words of out that belong to no plane
 * are not written.
 * Tile-local union-find in LDS, lock-free merge across tile borders through agent-scope atomics (a link only ever decreases),
 * flatten; no workgroup waits for another and every atomic is an integer one, so results do not depend on the order of execution.
 * The calls only enqueue.  conn other than 4 or 8, value other than 0 or 1, a negative size or area, a NULL pointer other than area
 * (components) or tiles with n_tiles = 0, or a misaligned array return S2D_ERR_ARG before anything is launched. */
int s2d_plane_components_tile(int *th, int *tw);
long s2d_plane_components_workspace_bytes(long total_words, int P);
int s2d_plane_components_ragged(const uint32_t *bits, const long *plane, int P, long total_words, int value, int conn,
                                const int *tiles, int n_tiles, int *labels, int *area, void *workspace, hipStream_t stream);
int s2d_plane_clean_ragged(const uint32_t *bits, const long *plane, int P, long total_words, int conn, int min_area,
                           int keep_largest, int max_hole_area, const int *tiles, int n_tiles, uint32_t *out, int *removed,
                           int *filled, void *workspace, hipStream_t stream);

/* ---- binary morphology of ragged bit planes (s2d_amd/plane_morph.py) ---------------------------------------- */

/* bits, plane, P and total_words are a chunk as above.  radius DEVICE i32 [P] is the radius of every plane, 0 .. 64 (0: the plane is
 * copied with its padding zeroed; a plane with a radius outside the range is skipped, as one that does not fit the buffer is).  The
 * rule is the project's own, stated once in s2d_amd/plane_morph.py: structuring element B(r, shape) = the disk {dx^2 + dy^2 <= r^2}
 * (shape 0) or the square {|dx|, |dy| <= r} (shape 1); dilate (op 1): a pixel is set iff a set pixel lies in p + B, nothing outside
 * the image is set; erode (op 0): a pixel is set iff every pixel of p + B INSIDE the image is set; open (op 2) = dilate(erode(.));
 * close (op 3) = erode(dilate(.)).  Disks do not compose, so there is no radius over 64 and no chained pass.
 * s2d_plane_morph_tile: the tile a workgroup handles at radius r (0 .. 64): at most `rows` rows of at most `words` row-aligned
 * 32-pixel words; a plane of H rows is cut evenly into ceil(H / rows) tile rows of ceil(H / that) rows.  tiles DEVICE i32
 * [n_tiles][3] = {plane, tile row, tile column} lists every tile of every plane with a radius > 0 once (host-built; the grid is 1-D
 * over it); a row that names no tile of its plane is skipped.  Pure host code.
 * s2d_plane_morph_lds_words: the LDS words the largest tile of an H x W plane at radius r needs (0 at r = 0, at most 10240 = 40 KiB,
 * four workgroups per CU); -1 for a size below 1 or a radius outside 0 .. 64.  Pure host code.  lds_words of the call below is ONE
 * figure per launch, the largest of these over the planes of the chunk: dynamic LDS, so a chunk of small masks at small radii
 * reserves a few KiB per workgroup.  A tile that needs more than lds_words is skipped.
 * s2d_plane_morph_workspace_bytes: the scratch the call needs (any address): 4 bytes per word of the buffer; -1 for a negative size.
 * s2d_plane_morph_ragged writes out = op(plane) for every plane: padding bits 0, words of out that belong to no plane not written.
 * cleared i32 [P] = popcount(in & ~out), set i32 [P] = popcount(out & ~in) over the pixels of each plane (integer sums of one
 * workgroup per plane: deterministic; 0 for a skipped plane).  A tile reads the halo its neighbours own, so out must overlap neither
 * bits nor the workspace, nor the workspace bits: S2D_ERR_ARG, as for an op outside 0 .. 3, a shape other than 0 or 1, a negative
 * size, an lds_words outside 0 .. 10240 (or none with n_tiles > 0), a NULL pointer (tiles with n_tiles = 0 excepted) or a misaligned
 * array, before anything is launched.  open and close are two passes through the workspace.  Plain stores and integer atomicOr
 * only; the call only enqueues.
 * s2d_plane_diff_counts_ragged: the same two counts for any two buffers a, b of the chunk (they may be one): cleared[p] = popcount(a &
 * ~b), set[p] = popcount(b & ~a) over the pixels of plane p, padding bits of either ignored, 0 for a plane that does not fit. */
int s2d_plane_morph_tile(int r, int *rows, int *words);
long s2d_plane_morph_lds_words(int r, int H, int W);
long s2d_plane_morph_workspace_bytes(long total_words, int P);
int s2d_plane_morph_ragged(const uint32_t *bits, const long *plane, int P, long total_words, int op, int shape, const int *radius,
                           const int *tiles, int n_tiles, int lds_words, uint32_t *out, int *cleared, int *set, void *workspace,
                           hipStream_t stream);
int s2d_plane_diff_counts_ragged(const uint32_t *a, const uint32_t *b, const long *plane, int P, long total_words, int *cleared,
                                 int *set, hipStream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* S2D_HIP_H */
