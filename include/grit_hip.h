/*
 * grit_hip.h -- C ABI of libgrit_hip.so, the MI355X (gfx950) kernels behind the GRIT captioning hot path.
 *
 * Every entry point takes plain device pointers + sizes + a hipStream_t (passed as void*), allocates nothing,
 * keeps no state between calls and is re-entrant (forward is called from the Python main thread, backward
 * from the autograd engine thread).  The caller sets the device, owns every buffer and passes the stream the
 * tensors were produced on.  Return value: 0 on success, otherwise one of the GRIT_ERR_* codes below
 * (grit_status_string() gives the text; the Python shim turns it into RuntimeError).
 *
 * Reference interfaces replaced (paths into davidnvq/grit):
 *   grit_msda_fwd_*      <- ms_deform_attn_forward   models/ops/src/ms_deform_attn.h:20-40, vision.cpp:14
 *                           (CUDA body models/ops/src/cuda/ms_deform_attn_cuda.cu:20-80,
 *                            kernel ms_deform_im2col_cuda.cuh:237-299)
 *   grit_msda_bwd_*      <- ms_deform_attn_backward  models/ops/src/ms_deform_attn.h:42-62, vision.cpp:15
 *                           (CUDA body ms_deform_attn_cuda.cu:83-153, kernel ms_deform_im2col_cuda.cuh:406-510)
 *   grit_winattn_*       <- WindowAttention.forward core + roll/partition/reverse around it,
 *                           models/common/swin_model.py:155-186, 244-300, 424-441 (no native ancestor)
 *   grit_attn_*          <- Attention.forward core (QK^T/sqrt(d_k), masked_fill(-inf), softmax, .V),
 *                           models/common/attention.py:51-88 (no native ancestor); also serves
 *                           nn.MultiheadAttention inside models/detection/det_module.py:330-333
 *   grit_layernorm_*, grit_add_layernorm_*
 *                        <- nn.LayerNorm of the Swin blocks (models/common/swin_model.py:229,233,315,495) and the
 *                           "projection -> dropout / drop-path -> residual -> LayerNorm" tails around it
 *                           (swin_model.py:289-298, det_module.py:313-349, attention.py:166-184, pos_embed.py:44-48)
 *   grit_relbias_*       <- relative_position_bias_table[relative_position_index] gather, swin_model.py:168-171
 *   grit_groupnorm_tokens_* <- input_proj's GroupNorm(32, 512) + flatten/cat, models/caption/detector.py:28-33,58,
 *                           models/detection/det_module.py:172-175
 *   grit_colsum, grit_slab_sum <- bias / weight gradient reductions of nn.Linear's backward on the long token maps
 *   grit_adam_flat       <- the two torch.optim.Adam of build_optimizers, engine/caption_engine.py:18-73
 *   grit_adamw_flat_dev, grit_grad_norm_flat
 *                        <- torch.optim.AdamW of build_optimizers_schedulers, train_detector.py:24-89, and
 *                           torch.nn.utils.clip_grad_norm_, engine/det_solver.py:108
 *   grit_resample_taps_bicubic, grit_image_batch_fwd
 *                        <- the image side of the batch contract: PIL resize(BICUBIC) of MaxWHResize / MinMaxResize
 *                           (datasets/caption/transforms/utils.py:4-45), ToTensor + Normalize
 *                           (datasets/caption/transforms/__init__.py:6-32), zero padding + mask of
 *                           nested_tensor_from_tensor_list (engine/utils.py:278-295)
 *   grit_image_batch_aug_fwd <- the same with RandAugment between the resize and ToTensor
 *                           (datasets/caption/transforms/randaug.py:11-104: PIL transform / rotate / ImageOps / ImageEnhance)
 *   grit_resample_taps_bilinear, grit_image_batch_geo_fwd
 *                        <- the detector's input: hflip / resize / crop on PIL images (datasets/detection/transforms.py:107-223,
 *                           torchvision's resize = Image.resize(BILINEAR)), then ToTensor, Normalize, padding and mask
 *   grit_gemm_bf16_nt    <- nn.Linear + nn.GELU of Mlp (models/common/swin_model.py:31-37) and their autograd backward:
 *                           fc1 + bias + exact GELU in one pass; fc2's input gradient x GELU' + fc1's bias gradient in one pass
 *   grit_topk_rows_f32   <- Transformer.select (models/caption/transformer.py:184-188): sort of beam x vocabulary candidates
 *   grit_beam_step       <- the body of Transformer.iter after the word log-probabilities (models/caption/transformer.py:208-240):
 *                           finished-beam masking, candidate scores, selection, beam / word split, score / mask / log-prob gathers
 *     n_maps > 1         <- the same after the averaged word log-probabilities of an ensemble (models/caption/ensemble.py:128-214:
 *                           torch.mean(torch.stack(per_model), 0) followed by the body of `iter`)
 *     its bans           <- nothing in the reference (its search cannot be steered): the same step, of one map or of the mean,
 *                           with a per-beam set of banned words applied while the candidates are scored
 *     its groups         <- nothing in the reference (its beams are near-copies of one sentence): the same step for beam groups
 *                           that are searched in turn, a group paying for every word an earlier group chose at this step
 *     its forced words   <- nothing in the reference (its search cannot be made to mention a word): the same step with sets of
 *                           forced words per image, the beams of a step dealt out over banks by how many sets they have met
 *   grit_sample_step_f32 <- nothing in the reference (it decodes by beam search only): one word per row drawn from the tempered,
 *                           top-k / nucleus truncated word distribution, in integer arithmetic that a host form repeats exactly
 *   grit_decode_step_inputs <- CaptionGenerator.get_seq_inputs in stateful mode + the word / position embedding sum
 *                           (models/caption/cap_generator.py:116-137,148)
 *   grit_kv_append       <- running_keys / running_values of the stateful self-attention (models/common/attention.py:166-181) and
 *                           their per-step re-gather by the surviving beam (models/caption/transformer.py:229)
 *   grit_gate_pack, grit_gate_fuse
 *                        <- the sigmoid-gated merge of the two cross-attentions at inference, ParallelAttentionLayer.forward
 *                           (models/caption/cap_generator.py:44-56): masks, concatenations, sigmoids, products, sum, scale
 *   grit_cider_reward    <- the self-critical reward, engine/caption_engine.py:433-438 (text_field.decode, PTBTokenizer.tokenize,
 *                           cider.compute_score) and datasets/caption/metrics/cider/cider_scorer.py (counts2vec, sim, compute_cider)
 *   grit_caption_scores  <- the evaluation's scores, engine/caption_engine.py:165-190 (decode, itertools.groupby, PTBTokenizer.tokenize,
 *                           compute_scores) and datasets/caption/metrics/{bleu/bleu_scorer.py, rouge/rouge.py, cider/cider_scorer.py}
 *   grit_cider_consensus <- nothing in the reference: consensus (minimum-Bayes-risk) reranking of the candidates of an image under
 *                           CIDEr-D, built from the same steps as grit_cider_reward; the host form is grit_amd/ops/consensus.py
 *   grit_jpeg_probe, grit_jpeg_entropy, grit_jpeg_reconstruct
 *                        <- PIL's Image.open(path).convert('RGB') in the dataset workers (datasets/caption/field.py:65,
 *                           tools/extract_features.py:42): libjpeg-turbo's baseline decode at its defaults
 *   grit_vocab_score_bf16 <- CaptionGenerator.forward's `fc` + F.log_softmax (models/caption/cap_generator.py:157-167) and the gather of
 *                           one target column per row that every caller who scores a GIVEN caption adds (the validation loss,
 *                           engine/caption_engine.py:287-309): log-probability and log-sum-exp per row, no [rows, V] map
 * (none of the last nineteen groups has a native ancestor in the reference: they replace chains of torch / PIL / host ops, and
 *  grit_sample_step_f32 goes one step past it)
 */
#ifndef GRIT_HIP_H
#define GRIT_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GRIT_ABI_VERSION 62

#define GRIT_OK 0
#define GRIT_ERR_BAD_ARG 1      /* null pointer, non-positive dimension, overflow of 32-bit index math      */
#define GRIT_ERR_UNSUPPORTED 2  /* shape outside what the kernels implement (stated per function)           */
#define GRIT_ERR_LAUNCH 3       /* hipGetLastError() != hipSuccess after the launch                         */

/* Library ABI version; bumped whenever a signature below changes. */
int grit_abi_version(void);
const char* grit_status_string(int status);

/* ------------------------------------------------------------------------------------------------------
 * Multi-scale deformable attention.
 *
 *   value           [B, S, M, D]        contiguous; S = sum_l H_l*W_l
 *   spatial_shapes  [L, 2] int64 (H, W) DEVICE memory, as in the reference
 *   level_start     [L]    int64        DEVICE memory
 *   loc             [B, Lq, M, L, P, 2] (x, y) normalised to [0,1]
 *   attn_w          [B, Lq, M, L, P]
 *   out             [B, Lq, M*D]        fully overwritten (need not be zeroed)
 *
 * out[b,q,m,:] = sum_{l,p} attn_w * bilinear(value_l[b,:,m,:], (x*W_l-0.5, y*H_l-0.5)), zero padding,
 * a point contributes only if -1 < h < H_l and -1 < w < W_l  (ms_deform_im2col_cuda.cuh:288).
 * Any D >= 1; D == 64 and D == 32 take the wide-load fast path.  The reference's im2col_step
 * argument has no counterpart here: chunking is internal and B is unrestricted.
 * ------------------------------------------------------------------------------------------------------ */
int grit_msda_fwd_f32(const float* value, const int64_t* spatial_shapes, const int64_t* level_start,
                      const float* loc, const float* attn_w,
                      int B, int S, int M, int D, int L, int Lq, int P,
                      float* out, void* stream);
int grit_msda_fwd_f64(const double* value, const int64_t* spatial_shapes, const int64_t* level_start,
                      const double* loc, const double* attn_w,
                      int B, int S, int M, int D, int L, int Lq, int P,
                      double* out, void* stream);

/*   grad_out    [B, Lq, M*D]
 *   grad_value  like value   -- accumulated with float atomics: the CALLER MUST ZERO IT (reference:
 *                               at::zeros_like, ms_deform_attn_cuda.cu:121)
 *   grad_loc    like loc     -- fully overwritten
 *   grad_attn_w like attn_w  -- fully overwritten
 * Summation order of grad_value is not deterministic (atomics), exactly as in the reference. */
int grit_msda_bwd_f32(const float* value, const int64_t* spatial_shapes, const int64_t* level_start,
                      const float* loc, const float* attn_w, const float* grad_out,
                      int B, int S, int M, int D, int L, int Lq, int P,
                      float* grad_value, float* grad_loc, float* grad_attn_w, void* stream);
int grit_msda_bwd_f64(const double* value, const int64_t* spatial_shapes, const int64_t* level_start,
                      const double* loc, const double* attn_w, const double* grad_out,
                      int B, int S, int M, int D, int L, int Lq, int P,
                      double* grad_value, double* grad_loc, double* grad_attn_w, void* stream);

/* bf16 value maps (D = 64, L*P <= 32): value / out / grad_out are bf16, loc / attn_w and every gradient stay f32.
 * grad_value is f32 [B,S,M,64], zeroed by the caller, accumulated with float atomics.  Other shapes (L*P > 16 for
 * backward): GRIT_ERR_UNSUPPORTED (the caller converts to f32 and uses the entry points above). */
int grit_msda_fwd_bf16(const void* value, const int64_t* spatial_shapes, const int64_t* level_start, const float* loc,
                       const float* attn_w, int B, int S, int M, int D, int L, int Lq, int P, void* out, void* stream);
int grit_msda_bwd_bf16(const void* value, const int64_t* spatial_shapes, const int64_t* level_start, const float* loc,
                       const float* attn_w, const void* grad_out, int B, int S, int M, int D, int L, int Lq, int P,
                       float* grad_value, float* grad_loc, float* grad_attn_w, void* stream);
/* Same backward with grad_value ACCUMULATED IN bf16 by packed atomics (two channels per 32-bit memory-side atomic: twice
 * the rate of the f32 atomics that bound grit_msda_bwd_bf16, no f32 staging map, no cast).  grad_value [B, S, M, D] bf16,
 * zeroed by the caller.  Accumulation order and rounding are those of torch's own bf16 scatter / grid_sample backward;
 * use grit_msda_bwd_bf16 when f32 accumulation of the value gradient is required.  D = 64, L*P <= 16. */
int grit_msda_bwd_bf16acc(const void* value, const int64_t* spatial_shapes, const int64_t* level_start, const float* loc,
                          const float* attn_w, const void* grad_out, int B, int S, int M, int D, int L, int Lq, int P,
                          void* grad_value, float* grad_loc, float* grad_attn_w, void* stream);
/* The same two kernels on a value map whose pixels are `pixel_stride` elements apart (>= M*D, a multiple of 8; image b
 * starts at b * S * pixel_stride): the deformable decoder projects the flat feature map for ALL its layers with one GEMM,
 * value_proj of models/ops/modules/ms_deform_attn.py:93 x 6 layers of models/detection/det_module.py:274-349 -> one
 * [B, S, layers, M, D] tensor, and each layer samples its slice in place.  grad_value has the same layout (one zero-filled
 * buffer that all layers' backward kernels add into), so the projection's input gradient is ONE GEMM over K = layers*M*D. */
int grit_msda_fwd_bf16_strided(const void* value, long pixel_stride, const int64_t* spatial_shapes,
                               const int64_t* level_start, const float* loc, const float* attn_w, int B, int S, int M,
                               int D, int L, int Lq, int P, void* out, void* stream);
int grit_msda_bwd_bf16acc_strided(const void* value, long pixel_stride, const int64_t* spatial_shapes,
                                  const int64_t* level_start, const float* loc, const float* attn_w, const void* grad_out,
                                  int B, int S, int M, int D, int L, int Lq, int P, void* grad_value, float* grad_loc,
                                  float* grad_attn_w, void* stream);
/* bf16 maps, value gradient ACCUMULATED IN f32 (the precision of the reference's atomicAdd on its fp32 grad_value,
 * ms_deform_im2col_cuda.cuh:125-152) and rounded to bf16 once: the default of the training step.  `stage` [B, S, M, 64] f32 and
 * `cell_flags` [B, S, M] u8 are scratch that must ARRIVE ZEROED and is RETURNED ZEROED (the second launch of the call visits the
 * cells the scatter touched -- flagged by the first -- rounds them into grad_value and clears stage and flags), so one
 * allocation serves every layer and every step.  grad_value: bf16 map with `pixel_stride` elements between pixels, zero-filled
 * by the caller (untouched cells are not written).  Same row walk, same-cell merges and grad_loc / grad_attn_w arithmetic as
 * grit_msda_bwd_bf16acc_strided.  D = 64, L*P <= 16. */
int grit_msda_bwd_bf16_staged(const void* value, long pixel_stride, const int64_t* spatial_shapes,
                              const int64_t* level_start, const float* loc, const float* attn_w, const void* grad_out,
                              int B, int S, int M, int D, int L, int Lq, int P, float* stage, unsigned char* cell_flags,
                              void* grad_value, float* grad_loc, float* grad_attn_w, void* stream);

/* bf16 maps, value gradient in GATHER form: the default of the training step.  No atomics on memory -- one workgroup per
 * (image, head) keeps that pair's whole problem in the LDS of its CU: the Lq rows of grad_out, the Lq*L*P*4 corner contributions
 * binned by cell (counting sort: LDS counters, LDS scan, LDS records {query, attention weight x bilinear weight}); every cell then
 * sums its contributions w_i * grad_out[q_i, :] in f32 registers and is rounded to bf16 ONCE.  f32 accumulation like the
 * reference's atomicAdd (ms_deform_im2col_cuda.cuh:125-152) without its rate limit (the memory-side atomic units of gfx950 do
 * ~323 G f32 adds/s: ~460 us per launch at GRIT's shapes; this path: profiles/r03/msda_bwd_methods.txt).
 * grad_value: bf16 map with `pixel_stride` elements between pixels (a multiple of 8, base 16-byte aligned); EVERY cell of the
 * [B, S, M, 64] slice is written (zeros where nothing sampled), so the caller does not zero-fill it.  grad_loc / grad_attn_w: the
 * row walk of grit_msda_bwd_bf16acc_strided with its scatter compiled out.  D = 64, L*P <= 16, Lq*L*P <= 4096 and
 * 4 (S + 1) + 32 Lq L P + 128 Lq + 64 <= 160 KB of LDS (GRIT: 130 KB); grit_msda_bwd_sorted_supported says GRIT_OK /
 * GRIT_ERR_UNSUPPORTED for a shape -- callers fall back to grit_msda_bwd_bf16_staged. */
int grit_msda_bwd_sorted_supported(int B, int S, int M, int L, int Lq, int P);
int grit_msda_bwd_bf16_sorted(const void* value, long pixel_stride, const int64_t* spatial_shapes,
                              const int64_t* level_start, const float* loc, const float* attn_w, const void* grad_out,
                              int B, int S, int M, int D, int L, int Lq, int P, void* grad_value, float* grad_loc,
                              float* grad_attn_w, void* stream);

/* ------------------------------------------------------------------------------------------------------
 * Scaled-dot attention core, fp32 arithmetic, head_dim D = 64 (also the 150-query
 * self-attention of A5).  f32 and bf16 storage variants.
 *
 *   q      [B, Tq, H, 64]   row stride ldq, batch stride bsq (elements) -- a slice of a packed projection is fine
 *   k, v   [B, Nk, H, 64]   row strides ldk / ldv, batch strides bsk / bsv;  Nk <= 256
 *   mask   uint8, nonzero = masked (-inf before softmax), or NULL.  Element (b, q, j) is read at
 *          mask[b*mask_sb + q*mask_sq + j]; pass stride 0 to broadcast over batch and/or query
 *          (reference masks are [B,1,T,T], [B,1,1,Nk]: attention.py:79-80, cap_generator.py:126-136)
 *   out    [B, Tq, H*64] contiguous;   lse [B, H, Tq] row log-sum-exp of the scaled, masked scores
 *   P = softmax(scale * q k^T masked);  dropout_p > 0 drops entries of P with a counter hash of `seed`
 *   (the backward call must pass the same seed);  out = P_drop v.  The effective seed is `seed ^ *seed_dev` when
 *   seed_dev (device uint64, may be NULL) is given: a seed that lives in device memory can be refreshed by a captured
 *   RNG kernel, so a hipGraph replay of the step draws a new mask each time.
 *   A fully masked row yields NaN, as torch.softmax over all -inf does in the reference.
 * Backward overwrites dq [B,Tq,H,64], dk, dv [B,Nk,H,64] (contiguous); no atomics to global memory.
 * ------------------------------------------------------------------------------------------------------ */
int grit_attn_fwd_f32(const void* q, int64_t ldq, int64_t bsq, const void* k, int64_t ldk, int64_t bsk,
                      const void* v, int64_t ldv, int64_t bsv, const uint8_t* mask, int64_t mask_sb, int64_t mask_sq,
                      int B, int H, int Tq, int Nk, int D, float scale, float dropout_p, uint64_t seed,
                      const uint64_t* seed_dev, void* out, float* lse, void* stream);
int grit_attn_fwd_bf16(const void* q, int64_t ldq, int64_t bsq, const void* k, int64_t ldk, int64_t bsk,
                       const void* v, int64_t ldv, int64_t bsv, const uint8_t* mask, int64_t mask_sb, int64_t mask_sq,
                       int B, int H, int Tq, int Nk, int D, float scale, float dropout_p, uint64_t seed,
                       const uint64_t* seed_dev, void* out, float* lse, void* stream);
int grit_attn_bwd_f32(const void* q, int64_t ldq, int64_t bsq, const void* k, int64_t ldk, int64_t bsk,
                      const void* v, int64_t ldv, int64_t bsv, const uint8_t* mask, int64_t mask_sb, int64_t mask_sq,
                      const void* out, const void* dout, const float* lse,
                      int B, int H, int Tq, int Nk, int D, float scale, float dropout_p, uint64_t seed,
                      const uint64_t* seed_dev, void* dq, void* dk, void* dv, void* stream);
int grit_attn_bwd_bf16(const void* q, int64_t ldq, int64_t bsq, const void* k, int64_t ldk, int64_t bsk,
                       const void* v, int64_t ldv, int64_t bsv, const uint8_t* mask, int64_t mask_sb, int64_t mask_sq,
                       const void* out, const void* dout, const float* lse,
                       int B, int H, int Tq, int Nk, int D, float scale, float dropout_p, uint64_t seed,
                       const uint64_t* seed_dev, void* dq, void* dk, void* dv, void* stream);

/* ------------------------------------------------------------------------------------------------------
 * Swin (shifted-)window attention, window 12 (N = 144), head_dim 32, bf16 storage / MFMA, fp32 softmax
 * (SURVEY 8 row A6).  Operates on the map in TOKEN ORDER; pad / roll / partition / reverse / crop of
 * swin_model.py:257-293 and the shift mask of :424-441 are done by address arithmetic inside the kernel.
 *
 *   qkv       bf16 [B, H*W, 3*C]   output of the qkv Linear on the un-partitioned map; channel = which*C + head*32 + d
 *   rel_bias  f32  [nH, 144, 144]  relative_position_bias_table gathered by relative_position_index (:168-171)
 *   pad_qkv   bf16 [3*C]           q/k/v of a window-padding token (= the qkv Linear bias)
 *   mask      f32  [n_mask_windows, 144, 144] additive, or NULL.  NULL + shift > 0 -> the kernel derives the
 *             0 / -100 shift mask from (H, W, shift) itself.  Non-NULL replaces it (WindowAttention.forward(x, mask)
 *             call form); window i uses mask[i % n_mask_windows].
 *   out       bf16 [B, H*W, C]     heads concatenated (channel = head*32 + d), padded positions are not written
 *   lse       f32  [B*nWh*nWw, nH, 144]  per-row log2-sum-exp2 of the logits, consumed by the backward call
 *   scale     q scaling (head_dim^-0.5);  C = num_heads*32;  0 <= shift < 12;  window must be 12.
 * Backward: dqkv bf16 like qkv (fully overwritten); drel_bias f32 like rel_bias and dpad f32 [3*C] are
 * ACCUMULATED with float atomics -- the caller zeroes them.
 * Two kernels behind each entry point, same results: the DMA-staged ones (default; operands of the next window by global_load_lds into
 * double-buffered LDS tiles, 160 KB of dynamic LDS for the backward) and the register-staged ones (environment
 * GRIT_WINATTN_FWD_DMA=0 / GRIT_WINATTN_BWD_DMA=0, read once per process; a non-NULL mask always takes the register-staged forward).
 * ------------------------------------------------------------------------------------------------------ */
int grit_winattn_fwd_bf16(const void* qkv, const float* rel_bias, const void* pad_qkv, const float* mask, int n_mask_windows,
                          int B, int H, int W, int C, int num_heads, int window, int shift, float scale,
                          void* out, float* lse, void* stream);
int grit_winattn_bwd_bf16(const void* qkv, const float* rel_bias, const void* pad_qkv, const float* mask, int n_mask_windows,
                          const void* out, const void* dout, const float* lse,
                          int B, int H, int W, int C, int num_heads, int window, int shift, float scale,
                          void* dqkv, float* drel_bias, float* dpad, void* stream);
/* The forward with the drop-path factors of the branch the attention belongs to (training): the windows of images with
 * row_scale[b] == 0 are not computed, out and lse receive zeros for them -- valid only because the caller multiplies the branch by the
 * factors afterwards and hands the SAME factors to grit_winattn_bwd_bf16_rows.  Applies under the conditions listed there (both
 * DMA-staged kernels in use); otherwise every window is computed. */
int grit_winattn_fwd_bf16_rows(const void* qkv, const float* rel_bias, const void* pad_qkv, const float* mask, int n_mask_windows,
                               int B, int H, int W, int C, int num_heads, int window, int shift, float scale,
                               void* out, float* lse, const float* row_scale, void* stream);
/* The backward with the drop-path factors of the attention branch (reference timm DropPath, models/common/swin_model.py:289-298):
 * row_scale[b] == 0 promises that dout is zero for image b.  Its windows contribute nothing to any output: they are not computed, dqkv
 * receives zeros for its tokens, the workgroups share the windows of the kept images.  row_scale == NULL, an explicit mask, B > 64,
 * a register-staged variant selected (GRIT_WINATTN_FWD_DMA=0 / GRIT_WINATTN_BWD_DMA=0) or GRIT_WINATTN_ROW_SKIP=0: every window is computed
 * (same results). */
int grit_winattn_bwd_bf16_rows(const void* qkv, const float* rel_bias, const void* pad_qkv, const float* mask, int n_mask_windows,
                               const void* out, const void* dout, const float* lse,
                               int B, int H, int W, int C, int num_heads, int window, int shift, float scale,
                               void* dqkv, float* drel_bias, float* dpad, const float* row_scale, void* stream);

/* The same two entry points in fp32 storage and plain fp32 arithmetic (fmaf chains, no matrix cores; lse in natural-log
 * units): the parity path for fp32 weights -- the reference's WindowAttention is fp32 (swin_model.py:155-186).  Not tuned for
 * throughput; a forward of one precision pairs only with the backward of the same precision. */
int grit_winattn_fwd_f32(const float* qkv, const float* rel_bias, const float* pad_qkv, const float* mask, int n_mask_windows,
                         int B, int H, int W, int C, int num_heads, int window, int shift, float scale,
                         float* out, float* lse, void* stream);
int grit_winattn_bwd_f32(const float* qkv, const float* rel_bias, const float* pad_qkv, const float* mask, int n_mask_windows,
                         const float* out, const float* dout, const float* lse, int B, int H, int W, int C, int num_heads,
                         int window, int shift, float scale, float* dqkv, float* drel_bias, float* dpad, void* stream);

/* ------------------------------------------------------------------------------------------------------
 * LayerNorm over the last dimension for the Swin token maps (nn.LayerNorm at swin_model.py:229,233,315,495).
 *   x, y, dy, dx  [rows, C] contiguous, f32 (x_is_bf16 = 0) or bf16 (1);  C in {128, 256, 512, 1024, 2048, 4096}
 *   weight, bias  [C], f32 or bf16 (w_is_bf16); the combination f32 x with bf16 weight is not provided
 *   mean, rstd    [rows] f32, written by forward, read by backward
 *   dweight/dbias [GRIT_LN_BWD_PARTIALS, C] f32 per-workgroup partial sums: rows [0, min(ceil(rows / rows_per_block),
 *                 GRIT_LN_BWD_PARTIALS)) are overwritten and only those may be summed (grit_slab_sum); no zero fill needed
 * Statistics and arithmetic are fp32; eps as in torch.nn.functional.layer_norm.
 * ------------------------------------------------------------------------------------------------------ */
#define GRIT_LN_BWD_PARTIALS 1024
int grit_layernorm_fwd(const void* x, const void* weight, const void* bias, int rows, int C, float eps, int x_is_bf16,
                       int w_is_bf16, void* y, float* mean, float* rstd, void* stream);
int grit_layernorm_bwd(const void* x, const void* weight, const void* dy, const float* mean, const float* rstd, int rows,
                       int C, int x_is_bf16, int w_is_bf16, void* dx, float* dweight, float* dbias, void* stream);

/* ------------------------------------------------------------------------------------------------------
 * Relative-position bias of window attention (WindowAttention.forward, swin_model.py:168-171):
 *   bias[h][p] = (float) table[index[p]][h]          table [n_rows, num_heads] f32 / bf16, index [n_pos] int64
 * and its gradient  dtable[r][h] = sum over the positions p with index[p] == r of dbias[h][p].  The positions are
 * passed sorted by table row: order [n_pos] int32 (a permutation of 0..n_pos-1, stable sort of index) and
 * offsets [n_rows + 1] int32 (row r owns order[offsets[r] .. offsets[r+1])).  dtable is fully overwritten.
 * ------------------------------------------------------------------------------------------------------ */
int grit_relbias_fwd(const void* table, const int64_t* index, int n_rows, int num_heads, int n_pos, int table_is_bf16,
                     float* bias, void* stream);
/* Up to GRIT_RELBIAS_GROUP_MAX forward gathers in ONE launch (the 24 Swin blocks of a step: same arithmetic per job as grit_relbias_fwd). */
#define GRIT_RELBIAS_GROUP_MAX 32
typedef struct grit_relbias_job {
    const void* table;
    const int64_t* index;
    float* bias;
    int n_rows, num_heads, n_pos, table_is_bf16;
} grit_relbias_job;
int grit_relbias_fwd_grouped(const grit_relbias_job* jobs, int n_jobs, void* stream);
/* ... and up to GRIT_RELBIAS_GROUP_MAX table gradients in ONE launch (same arithmetic per job as grit_relbias_bwd). */
typedef struct grit_relbias_bwd_job {
    const float* dbias;
    const int32_t* order;
    const int32_t* offsets;
    void* dtable;
    int n_rows, num_heads, n_pos, table_is_bf16;
} grit_relbias_bwd_job;
int grit_relbias_bwd_grouped(const grit_relbias_bwd_job* jobs, int n_jobs, void* stream);
int grit_relbias_bwd(const float* dbias, const int32_t* order, const int32_t* offsets, int n_rows, int num_heads, int n_pos,
                     int table_is_bf16, void* dtable, void* stream);

/* ------------------------------------------------------------------------------------------------------
 * Residual connection + the LayerNorm that follows it, one pass (SwinTransformerBlock.forward, swin_model.py:289-298:
 * `x = shortcut + self.drop_path(x)` then `self.norm2(x)`; likewise the MLP residual and the next block's norm1):
 *   sum_out = round(shortcut + row_scale[row / rows_per_sample] * branch)     (row_scale NULL: plain add)
 *   y       = LayerNorm(sum_out) with the statistics of the rounded sum, i.e. bit-identical to the unfused pair
 * Backward: dx = dres + dLayerNorm(dy)   (dres = gradient reaching sum_out through the skip path, may be NULL) is the
 * gradient of `shortcut`; with row_scale the gradient of `branch`, dbranch = row_scale[row / rows_per_sample] * dx, is
 * written too (row_scale and dbranch are given together or both NULL: the branch gradient is then dx itself).
 * drop_p > 0 additionally applies element dropout to the branch before the residual add (the nn.Dropout between a
 * projection and `LayerNorm(x + dropout(proj))` in the post-norm decoder layers: det_module.py:313-349, attention.py:
 * 166-184, pos_embed.py:44-48): keep mask = counter hash of (seed read from seed_dev, element index), regenerated in the
 * backward (same drop_p / seed_dev), which then requires dbranch.
 * dbranch_colsum (optional, C <= 1024): [GRIT_LN_BWD_PARTIALS, C] f32 per-workgroup partial column sums of the branch
 * gradient as stored -- the bias gradient of the Linear that produced `branch` (attn.proj / mlp.fc2), for free.
 * Other arguments as in grit_layernorm_{fwd,bwd}.
 * ------------------------------------------------------------------------------------------------------ */
/* Patch embedding of the Swin backbone in one pass (reference models/common/swin_model.py:336-365, PatchEmbed: Conv2d(3, C, kernel 4,
 * stride 4) -> flatten(2).transpose(1, 2) -> LayerNorm(C)): out[b, hh * W/4 + ww, :] = LayerNorm(conv(img)[b, :, hh, ww] + bias),
 * bf16.  img [B, 3, H, W] fp32 (img_is_bf16 = 0: rounded to bf16 on load, as the unfused cast does) or bf16; weight [C, 48] bf16 =
 * the conv weight flattened in its own (c, kh, kw) order; bias, gamma, beta [C] bf16; C in {96, 128, 192}; H % 4 == 0, W % 64 == 0
 * (GRIT_ERR_UNSUPPORTED otherwise: the caller keeps its GEMM path); 16-byte aligned bases.  The conv output is rounded to bf16
 * before the statistics, like the tensor the unfused GEMM stores.  Forward only: PatchEmbed is frozen in GRIT (frozen_stages = 2). */
int grit_patch_embed_ln_fwd(const void* img, int img_is_bf16, int B, int H, int W, int C, const void* weight, const void* bias,
                            const void* gamma, const void* beta, float eps, void* out, void* stream);

/* LayerNorm of the PATCH-MERGED map without the map (reference models/common/swin_model.py:279-288, PatchMerging.forward: 2 x 2
 * neighbourhood concat in the order (0,0), (1,0), (0,1), (1,1) -> LayerNorm(4 Cs)): x is the token map [B, H, W, Cs] (H, W even, Cs a
 * multiple of 8, 4 Cs in the supported widths); row r of the [B * H/2 * W/2, 4 Cs] view is gathered on load.  y, mean, rstd as in
 * grit_layernorm_fwd on that view.  Backward: dy [rows, 4 Cs] contiguous, dx is written straight in the token-map layout
 * [B, H, W, Cs] (every element exactly once).  Replaces the permute + reshape copy and the scatter of its gradient. */
int grit_merge_layernorm_fwd(const void* x, int B, int H, int W, int Cs, const void* weight, const void* bias, float eps,
                             int x_is_bf16, int w_is_bf16, void* y, float* mean, float* rstd, void* stream);
int grit_merge_layernorm_bwd(const void* x, int B, int H, int W, int Cs, const void* weight, const void* dy, const float* mean,
                             const float* rstd, int x_is_bf16, int w_is_bf16, void* dx, float* dweight, float* dbias,
                             void* stream);
int grit_add_layernorm_fwd(const void* shortcut, const void* branch, const float* row_scale, int rows_per_sample,
                           float drop_p, const uint64_t* seed_dev, const void* weight, const void* bias, int rows, int C,
                           float eps, int x_is_bf16, int w_is_bf16, void* sum_out, void* y, float* mean, float* rstd,
                           void* stream);
int grit_add_layernorm_bwd(const void* x, const void* weight, const void* dy, const void* dres, const float* mean,
                           const float* rstd, const float* row_scale, int rows_per_sample, float drop_p,
                           const uint64_t* seed_dev, int rows, int C, int x_is_bf16, int w_is_bf16, void* dx, void* dbranch,
                           float* dweight, float* dbias, float* dbranch_colsum, void* stream);

/* ------------------------------------------------------------------------------------------------------
 * GroupNorm on token-major maps (nn.GroupNorm(32, hidden_dim) after the 1x1 input projection of every feature level,
 * reference models/caption/detector.py:28-33,58; statistics over (H*W, C/G) per image and group, biased variance).
 *   x [B, T, C]: image b at x + b * x_bstride (elements), rows of C channels contiguous; C in {256, 512}, (C/G) % 8 == 0
 *   y            same geometry with its own batch stride: a level can be written straight into its slice of the flat
 *                [B, sum_l T_l, C] map that the deformable-attention decoder consumes
 *   mean, rstd   [B, G] f32, written by forward, read by backward
 *   workspace    f32, forward: B * GRIT_GN_CHUNKS * 2 * G, backward: B * GRIT_GN_CHUNKS * 2 * C elements (fully overwritten)
 * Backward: dx [B, T, C] contiguous; dweight / dbias [C] in the weight dtype.  f32 x with bf16 weight is not provided.
 * ------------------------------------------------------------------------------------------------------ */
#define GRIT_GN_CHUNKS 16
int grit_groupnorm_tokens_fwd(const void* x, long x_bstride, const void* weight, const void* bias, int B, int T, int C, int G,
                              float eps, int x_is_bf16, int w_is_bf16, void* y, long y_bstride, float* mean, float* rstd,
                              float* workspace, void* stream);
int grit_groupnorm_tokens_bwd(const void* x, long x_bstride, const void* dy, long dy_bstride, const void* weight,
                              const float* mean, const float* rstd, int B, int T, int C, int G, int x_is_bf16, int w_is_bf16,
                              void* dx, void* dweight, void* dbias, float* workspace, void* stream);

/* ------------------------------------------------------------------------------------------------------
 * Column sums (bias gradient of nn.Linear: db = sum over rows of dY).  x [M, N] row-major, f32 or bf16, N % 8 == 0.
 * partial [slabs, N] f32 is fully overwritten: row s holds the sums over row slab s; the caller adds the slabs.
 * ------------------------------------------------------------------------------------------------------ */
#define GRIT_COLSUM_MAX_SLABS 256
int grit_colsum(const void* x, int M, int N, int x_is_bf16, int slabs, float* partial, void* stream);

/* ------------------------------------------------------------------------------------------------------
 * Second stage of the slab-wise reductions of the backward pass: out[g][i] = cast(sum_s partial[g][s][i]).
 * Replaces the `partial.sum(0).to(dtype)` pairs that follow grit_colsum, the split-M weight-gradient GEMM
 * (dW of nn.Linear, autograd's mm at the sites of swin_model.py:75-76,139,148) and grit_layernorm_bwd.
 *   partial  f32, group g at partial + g * group_stride, slab s of a group at + s * n      (n % 4 == 0, 16-byte aligned)
 *   out      [groups, n] f32 (out_is_bf16 = 0) or bf16 (1)
 * ------------------------------------------------------------------------------------------------------ */
int grit_slab_sum(const float* partial, int groups, long group_stride, int slabs, long n, void* out, int out_is_bf16,
                  void* stream);

/* Up to GRIT_SLAB_GROUP_MAX slab sums in ONE launch (same arithmetic per job as grit_slab_sum, job table passed by value): the
 * reductions a backward node owes -- split-M weight gradients, bias-gradient column sums, LayerNorm dgamma / dbeta -- done together
 * instead of as dependent launches of a few microseconds each.  bf16 outputs need 8-byte, f32 outputs 16-byte alignment. */
#define GRIT_SLAB_GROUP_MAX 48
typedef struct grit_slab_job {
    const float* partial;   /* group g at partial + g * group_stride, slab s of a group at + s * n */
    long group_stride;
    int groups;
    int slabs;
    long n;
    void* out;              /* [groups, n] */
    int out_is_bf16;
    const float* extra;     /* NULL, or [groups, n] f32 (16-byte aligned): one more term of every sum, added last (ABI 40: the q / k / v
                             * rows of the window-padding tokens are the qkv bias -- grit_winattn_bwd's d(pad) joins the bias gradient's sum) */
} grit_slab_job;
int grit_slab_sum_grouped(const grit_slab_job* jobs, int n_jobs, void* stream);

/* ------------------------------------------------------------------------------------------------------
 * Weight + bias gradient of nn.Linear on SHORT token maps (the decoders and the grid net, M = 640 .. 4 800 rows; autograd of
 * the Linear layers of models/detection/det_module.py:313-349, models/caption/grid_net.py:9-42, models/common/attention.py:51-88,
 * models/common/pos_embed.py:34-48):     dW[n, k] = sum_m dY[m, n] * X[m, k]        db[n] = sum_m dY[m, n]
 * dY [M, N], X [M, K] bf16 row-major with leading dimensions ldy / ldx (elements, multiples of 8; 16-byte aligned bases);
 * N % 64 == 0, K % 64 == 0.  splits = grit_wgrad_small_splits(M, N, K) (0: shape not supported):
 *   splits == 1  (M <= 4 800): dW_out is the finished gradient, bf16 [N, K], db_out bf16 [N] (or NULL: not wanted) -- ONE launch
 *                replaces the library's transposed GEMM (24-47 us for these 2.5 GFLOP problems), the column-sum kernel and the
 *                reduction launch behind it;
 *   splits  > 1  dW_out = f32 partials [splits, N, K], db_out = f32 partials [splits, N] (or NULL), fully overwritten; the
 *                caller sums over the splits (grit_slab_sum / grit_slab_sum_grouped).
 * ------------------------------------------------------------------------------------------------------ */
int grit_wgrad_small_splits(int M, int N, int K);
int grit_wgrad_small(const void* dY, long ldy, const void* X, long ldx, int M, int N, int K, int splits, void* dW_out,
                     void* db_out, void* stream);
/* Up to GRIT_WGRAD_GROUP_MAX such problems in ONE launch (job table by value): the deferred weight / bias gradients of a decoder's
 * short-map Linears (grit_amd/ops/linear.py DeferredWgrads).  Every job writes f32 partials dW_partial [splits, N, K] and, when
 * db_partial != NULL, [splits, N], splits = grit_wgrad_group_splits(M); the caller reduces them (grit_slab_sum_grouped). */
#define GRIT_WGRAD_GROUP_MAX 32
typedef struct grit_wgrad_job {
    const void* dY; long ldy;
    const void* X; long ldx;
    int M, N, K, splits;
    float* dW_partial;
    float* db_partial;
    /* grit_wgrad_tn_grouped only (grit_wgrad_small_grouped ignores them): per-sample factors of the branch whose gradient dY is -- see
     * grit_wgrad_tn_rows.  NULL / 0: every row is processed. */
    const float* row_scale;
    int rows_per_sample;
} grit_wgrad_job;
int grit_wgrad_group_splits(int M);
int grit_wgrad_small_grouped(const grit_wgrad_job* jobs, int n_jobs, void* stream);
/* The same job table through the long-map kernel (grit_wgrad_tn's 256 x 256 tiles, one launch for all jobs): for jobs with
 * N % 256 == 0, K % 256 == 0, M % 32 == 0 (grit_wgrad_tn_group_ok), db_partial [splits, N] (column sums per slice) or NULL,
 * splits = any number of row slices such that every slice owns at least one step (64 rows when M % 64 == 0, else 32; slice s =
 * rows [s * ceil(steps / splits) * step_rows, ...)) -- the caller picks it so that the tiles of all jobs together fill the chip with
 * LONG loops (thirty M = 4 800 problems are 128 tiles x 2 slices of 38 steps).  dW_partial [splits, N, K] fp32 as above.  When every
 * job has M % 64 == 0 the launch runs the four-wave kernel (wgrad_tn4_256_grouped), else the eight-wave one; in both the workgroups
 * of one XCD (block % 8) take a contiguous band of a job's (slice, tile) pairs. */
int grit_wgrad_tn_group_ok(int M, int N, int K);
int grit_wgrad_tn_grouped(const grit_wgrad_job* jobs, int n_jobs, void* stream);
/* Column sums of up to GRIT_COLSUM_GROUP_MAX bf16 matrices x [M, N] (leading dimension ld) in one launch:
 * partial[slabs, N] fp32 per job, slab s = rows [s * ceil(M / slabs), ...); N % 8 == 0, ld % 8 == 0, 16-byte aligned bases. */
#define GRIT_COLSUM_GROUP_MAX 32
typedef struct grit_colsum_job {
    const void* x; long ld;
    int M, N, slabs;
    float* partial;
} grit_colsum_job;
int grit_colsum_grouped(const grit_colsum_job* jobs, int n_jobs, void* stream);

/* Transposed copies dst [cols, rows] of up to GRIT_TRANSPOSE_GROUP_MAX bf16 matrices src [rows, cols] (contiguous) in one launch:
 * the K-contiguous B operands grit_gemm_bf16_nt needs for an input gradient (fc2.weight^T of every Swin Mlp,
 * models/common/swin_model.py:31-37: autograd's Linear backward leaves that transpose to its GEMM) made once per optimizer step
 * instead of once per block inside backward.  rows, cols multiples of 64, 16-byte aligned bases. */
#define GRIT_TRANSPOSE_GROUP_MAX 32
typedef struct grit_transpose_job {
    const void* src; void* dst;
    int rows, cols;
} grit_transpose_job;
int grit_transpose_bf16_grouped(const grit_transpose_job* jobs, int n_jobs, void* stream);

/* Weight gradient of a Linear on a LONG token map (the Swin blocks): partial[s, N, K] (fp32) = dY[rows of slice s]^T . X[rows of
 * slice s] for S = grit_wgrad_tn_splits(M, N, K) row slices (chosen so that tiles x S fills the chip with one 256 x 256-tile
 * workgroup per CU); the caller sums the slices (grit_slab_sum_grouped).  The contraction runs over the slow index of both
 * operands; the transpose happens in the LDS reads (ds_read_b64_tr_b16 on both MFMA operands, grit_amd/csrc/wgrad_tn.hip).
 * Replaces the batched library GEMM over row slices of autograd's Linear backward (models/common/swin_model.py:26-35, 147-149).
 * N, K multiples of 256, M a multiple of 32 (grit_wgrad_tn_splits returns 0 otherwise: use the library), 16-byte aligned bases,
 * leading dimensions multiples of 8.  Slices are whole steps of 64 rows when M % 64 == 0 (the four-wave kernel: 128 x 128 wave
 * tiles, AGPR accumulators; GRIT_WGRAD_TN_W4=0 selects the eight-wave kernel for A/B runs), of 32 rows otherwise (eight waves).
 * db_partial != NULL: [S, N] fp32 column sums of dY per slice (the bias gradient) as a by-product of the workgroups of k-tile 0
 * (four waves: one extra MFMA per dY^T fragment against a block of ones; eight waves: v_dot2 on the fragments + LDS adds). */
int grit_wgrad_tn_splits(int M, int N, int K);
int grit_wgrad_tn(const void* dY, long ldy, const void* X, long ldx, int M, int N, int K, int splits, float* partial,
                  float* db_partial, void* stream);
/* The same with the drop-path factors of the branch whose gradient dY is (reference timm DropPath, models/common/swin_model.py:289-298:
 * per-sample keep w.p. 1 - p): row_scale[b] == 0 promises that rows [b * rows_per_sample, (b + 1) * rows_per_sample) of dY are exact
 * zeros.  Those rows add nothing to dW, so their 64-row steps are never loaded and the S slices share the LIVE steps equally (a slice is
 * a run of live steps instead of a fixed row range: the slice partials differ from grit_wgrad_tn's, their sum only by fp32 summation
 * order).  Applies on the four-wave kernel when rows_per_sample % 64 == 0, M / rows_per_sample is 2..64, at least one sample is
 * dropped and the kept samples hold at least `splits` 64-row steps (every slice needs one); otherwise -- fewer live steps than
 * slices, rows_per_sample % 64 != 0, more than 64 samples, the eight-wave kernel (in a grouped launch: any job with M % 64 == 32),
 * GRIT_WGRAD_ROW_SKIP=0 -- every row is processed, which is equally correct.  Where skipping applies the rows of X in dropped samples
 * are never read and may hold anything; where it does not they ARE read (and multiplied by the zeros of dY), so a caller that cannot
 * tell the two apart keeps X finite everywhere. */
int grit_wgrad_tn_rows(const void* dY, long ldy, const void* X, long ldx, int M, int N, int K, int splits, float* partial,
                       float* db_partial, const float* row_scale, int rows_per_sample, void* stream);

/* ------------------------------------------------------------------------------------------------------
 * Adam step on one flat range of the fp32-master / bf16-compute training state (torch.optim.Adam as configured by the
 * reference's build_optimizers, engine/caption_engine.py:18-73: amsgrad off, weight decay 0).
 *   param, exp_avg, exp_avg_sq  f32 [n], updated in place;  grad [n] bf16 (grad_is_bf16) or f32, multiplied by grad_scale
 *   compute_bf16                bf16 [n] copy of the updated parameters, or NULL
 *   bias_correction1 = 1 - beta1^t,  bias_correction2_sqrt = sqrt(1 - beta2^t)   (t = 1-based step count)
 * n % 4 == 0; f32 pointers 16-byte, bf16 pointers 8-byte aligned.
 * ------------------------------------------------------------------------------------------------------ */
int grit_adam_flat(float* param, const void* grad, int grad_is_bf16, float* exp_avg, float* exp_avg_sq, void* compute_bf16,
                   long n, float lr, float beta1, float beta2, float eps, float bias_correction1,
                   float bias_correction2_sqrt, float grad_scale, void* stream);
/* The same step with its two per-step scalars read from DEVICE memory at run time: hyper[0] = lr / bias_correction1,
 * hyper[1] = 1 / bias_correction2_sqrt (8-byte aligned).  For a training step captured in a HIP graph (grit_amd/engine/graph_step.py):
 * the host rewrites hyper before every replay, so the learning-rate schedule and the step count advance without a re-capture. */
int grit_adam_flat_dev(float* param, const void* grad, int grad_is_bf16, float* exp_avg, float* exp_avg_sq, void* compute_bf16,
                       long n, float beta1, float beta2, float eps, float grad_scale, const float* hyper, void* stream);

/* ------------------------------------------------------------------------------------------------------
 * AdamW and gradient clipping for detector pre-training on the same flat layout (ABI 51; torch.optim.AdamW of the reference's
 * build_optimizers_schedulers, train_detector.py:24-89; torch.nn.utils.clip_grad_norm_ of engine/det_solver.py:108).
 *
 * grit_grad_norm_flat: the global L2 norm of n_ranges flat gradient ranges (a HOST table; all bf16, grad_is_bf16, or all f32) and
 * the clip factor that follows from it, written to DEVICE memory and never read back:
 *     out[0] total_norm = float(grad_scale * sqrt(sum g^2))       squares and sums in float64
 *     out[1] clip_scale = grad_scale * clip_coef                  the factor grit_adamw_flat_dev multiplies every gradient element by
 *     out[2] clip_coef  = min(1, max_norm / (total_norm + 1e-6))  fp32, torch's expression; a NaN gradient gives three NaNs
 * Deterministic: one float64 partial per workgroup, added in index order by the workgroup that takes the last ticket; the entry
 * point zeroes the ticket on the stream in front of the launches, no state outlives a call.  More than GRIT_NORM_MAX_RANGES ranges
 * are taken by a chain of launches, the last of which finalises.
 *   partials  f64 [GRIT_NORM_BLOCK_CAP * ceil(n_ranges / GRIT_NORM_MAX_RANGES)] workspace;  ticket  one unsigned int
 * Every range: n % 4 == 0, bf16 pointers 8-byte, f32 pointers 16-byte aligned (GRIT_ERR_UNSUPPORTED otherwise); null pointers,
 * n <= 0, n_ranges <= 0 or max_norm < 0: GRIT_ERR_BAD_ARG.
 *
 * grit_adamw_flat_dev: grit_adam_flat_dev behind  p <- p * hyper[2]  (decoupled weight decay, torch's order).  hyper is a 16-byte
 * aligned row of four floats {lr / bias_correction1, 1 / bias_correction2_sqrt, 1 - lr * weight_decay, unused}.  clip_scale may be
 * NULL; otherwise the kernel multiplies the gradients by *clip_scale (out + 1 of grit_grad_norm_flat) in place of grad_scale.
 * hyper[2] == 1 and clip_scale == NULL: bit-identical to grit_adam_flat_dev.
 * ------------------------------------------------------------------------------------------------------ */
#define GRIT_NORM_MAX_RANGES 64
#define GRIT_NORM_BLOCK_CAP 2048 /* workgroups (of 256 threads, one 16-byte load each) one pass of the capped grid holds */
typedef struct grit_norm_range {
    const void* grad;
    long n;
} grit_norm_range;
int grit_grad_norm_flat(const grit_norm_range* ranges, int n_ranges, int grad_is_bf16, float grad_scale, float max_norm,
                        double* partials, unsigned int* ticket, float* out, void* stream);
int grit_adamw_flat_dev(float* param, const void* grad, int grad_is_bf16, float* exp_avg, float* exp_avg_sq, void* compute_bf16,
                        long n, float beta1, float beta2, float eps, float grad_scale, const float* hyper, const float* clip_scale,
                        void* stream);

/* ------------------------------------------------------------------------------------------------------
 * Decoded RGB images -> the model's input batch: bicubic resize with Pillow's 8-bit arithmetic
 * (bit-identical to Image.resize(size, Image.BICUBIC) on an RGB image), x/255, (x - mean)/std, zero padding to the
 * batch maximum and the padding mask -- transforms/utils.py:4-45, transforms/__init__.py:6-32, engine/utils.py:278-295.
 *
 * grit_resample_taps_bicubic, grit_resample_taps_bilinear (host code, no GPU work): the tap table of one axis for Pillow's
 * BICUBIC / BILINEAR filter.
 *   bounds [out_size][2] = (first source index, tap count);  taps [out_size][ksize] 22-bit fixed point, zero past the count
 *   returns ksize (> 0); with bounds == taps == NULL only ksize is computed; -GRIT_ERR_BAD_ARG on bad sizes / capacity
 *
 * grit_image_batch_fwd (two launches):
 *   src     uint8 blob holding the images, each [src_h, src_w, 3] contiguous at byte offset src_off; 4-byte aligned and
 *           readable for GRIT_IMAGE_SRC_PAD bytes past the last image (the row pass fetches whole dwords)
 *   desc    [batch][GRIT_IMAGE_DESC_FIELDS] int64 (device): src_off, src_h, src_w, dst_h, dst_w, kx, ky, xb_off, xt_off,
 *           yb_off, yt_off, tmp_off -- k* = ksize of the x / y table, *b_off / *t_off = offsets (in int32 elements) of the
 *           bounds / taps of that axis inside `tables` (even), tmp_off = byte offset (multiple of 4) of this image's slot
 *           in tmp: src_h rows of GRIT_IMAGE_TMP_PITCH(dst_w) bytes
 *   tables  int32 blob (device) of the tap tables;  tmp uint8 scratch, 4-byte aligned, sum of the slots
 *   lut     [3][256] f32: lut[c][v] = (v / 255 - mean[c]) / std[c], computed by the caller
 *   out     [batch, 3, out_h, out_w] f32 and mask [batch, out_h, out_w] uint8 (1 on padding), both fully overwritten
 *   max_src_h = max src_h, max_dst_w = max dst_w (<= out_w), max_kx = max kx over the batch; grid extents <= 65535
 * ------------------------------------------------------------------------------------------------------ */
#define GRIT_IMAGE_DESC_FIELDS 12
#define GRIT_IMAGE_SRC_PAD 64
#define GRIT_IMAGE_TMP_PITCH(dst_w) ((3 * (dst_w) + 3) & ~3)
int grit_resample_taps_bicubic(int in_size, int out_size, int32_t* bounds, int32_t* taps, long taps_capacity);
int grit_resample_taps_bilinear(int in_size, int out_size, int32_t* bounds, int32_t* taps, long taps_capacity);
int grit_image_batch_fwd(const uint8_t* src, const int64_t* desc, const int32_t* tables, uint8_t* tmp, const float* lut,
                         int batch, int max_src_h, int max_dst_w, int max_kx, int out_h, int out_w, float* out,
                         uint8_t* mask, void* stream);

/* ------------------------------------------------------------------------------------------------------
 * The same batch with RandAugment (datasets/caption/transforms/randaug.py:74-104) applied to every resized uint8 image
 * before the lookup table, padding and mask; bit-identical to Pillow's transform(AFFINE) / rotate / ImageOps.autocontrast /
 * ImageEnhance.{Color, Contrast, Brightness, Sharpness} chained on the host.  The random draws stay on the host: the
 * caller passes what to do, per image and stage.
 *
 * grit_image_batch_aug_fwd (3 + n_stages launches: rows, columns -> uint8, one per stage, lookup + padding):
 *   src, desc, tables, tmp, lut, out, mask, max_src_h, max_dst_w, max_kx, out_h, out_w   as for grit_image_batch_fwd
 *   aug     [batch][GRIT_IMAGE_AUG_FIELDS] int32 (device):  [0] buf_off = byte offset (multiple of 4) of the image's slot in
 *           each work buffer: dst_h rows of GRIT_IMAGE_TMP_PITCH(dst_w) bytes;  [1] k = number of operations of this image,
 *           0 .. GRIT_IMAGE_AUG_STAGES: stages >= k leave the image alone and its result is read from work buffer k & 1;
 *           [2], [3] zero;  then GRIT_IMAGE_AUG_STAGES records of 8: (op, p1 .. p7), zero (GRIT_AUG_COPY) from record k on.
 *             GRIT_AUG_COPY          bytes unchanged
 *             GRIT_AUG_AUTOCONTRAST  per channel lut[i] = clamp((int)(i * scale + offset)), scale = 255.0 / (hi - lo),
 *                                    offset = -lo * scale in fp64 with separate roundings; unchanged where hi <= lo
 *             GRIT_AUG_AFFINE_FIXED  p1..p6 = A0..A5, 16.16 fixed point (FIX(t) = floor(t * 65536 + 0.5); A2, A5 include the
 *                                    half-pixel terms): xin = (A2 + A0 x + A1 y) >> 16, yin = (A5 + A3 x + A4 y) >> 16,
 *                                    nearest neighbour, 0 outside.  Rotate and the shears with a non-zero off-diagonal term.
 *             GRIT_AUG_AFFINE_TABLE  p1, p2 = offsets (int32 elements) inside `tables` of xin[dst_w] and yin[dst_h], built on
 *                                    the host by Pillow's walk in doubles; entries outside [0, size) read as 0.  Translations.
 *             GRIT_AUG_COLOR / _CONTRAST / _BRIGHTNESS / _SHARPNESS   p1 = the bits of the fp32 factor alpha;
 *                                    out = blend(degenerate, image, alpha) per byte, t = (float)d + alpha * (float)(i - d) with an
 *                                    fp32 multiply then an fp32 add; truncated for 0 <= alpha <= 1, else clamped to 0 / 255 first.
 *                                    Degenerates: grey L = (R*19595 + G*38470 + B*7471 + 0x8000) >> 16; the constant
 *                                    (2 * sum(L) + count) / (2 * count); zero; the 3 x 3 filter (1,1,1,1,5,1,1,1,1) / 13 in fp32
 *                                    (border rows / columns and images below 3 x 3 unchanged).
 *   n_stages  number of stage launches, 0 .. GRIT_IMAGE_AUG_STAGES: the largest k of the batch
 *   work    uint8 scratch, 4-byte aligned: two buffers of work_bytes (multiple of 4) each, work_bytes >= sum of the slots
 *   stats   uint32 [batch][GRIT_IMAGE_AUG_STAGES][GRIT_IMAGE_AUG_BLOCKS(max_dst_h, max_dst_w)][8] scratch, 16-byte aligned, not
 *           initialised by the caller.  Per stage and block of 1024 pixels the statistics of that stage's INPUT, stored by
 *           the launch that writes it and reduced by the stage that needs them (AutoContrast, Contrast): [0..2] 255 - min
 *           and [3..5] max per channel, [6..7] the 64-bit sum of L.  Integers only, no atomics: deterministic
 *   max_dst_h = max dst_h (<= out_h); dst_h, dst_w <= 32767
 * ------------------------------------------------------------------------------------------------------ */
#define GRIT_IMAGE_AUG_STAGES 4
#define GRIT_IMAGE_AUG_FIELDS 36
#define GRIT_IMAGE_AUG_BLOCKS(max_dst_h, max_dst_w) ((((long)(max_dst_h) * (((max_dst_w) + 3) / 4) + 255) / 256 + 7) / 8 * 8)
#define GRIT_AUG_COPY 0
#define GRIT_AUG_AUTOCONTRAST 1
#define GRIT_AUG_AFFINE_FIXED 2
#define GRIT_AUG_AFFINE_TABLE 3
#define GRIT_AUG_COLOR 4
#define GRIT_AUG_CONTRAST 5
#define GRIT_AUG_BRIGHTNESS 6
#define GRIT_AUG_SHARPNESS 7
int grit_image_batch_aug_fwd(const uint8_t* src, const int64_t* desc, const int32_t* tables, uint8_t* tmp, const float* lut,
                             const int32_t* aug, int n_stages, uint8_t* work, long work_bytes, uint32_t* stats, int batch,
                             int max_src_h, int max_dst_h, int max_dst_w, int max_kx, int out_h, int out_w, float* out,
                             uint8_t* mask, void* stream);

/* ------------------------------------------------------------------------------------------------------
 * The detector's input pipeline (datasets/detection/transforms.py: hflip, resize, crop chained on PIL images, then ToTensor,
 * Normalize and nested_tensor_from_tensor_list): per image one or two resizes, A then B, each over a source window.  The host
 * folds a crop into the window (first byte, height; the width is the in_size of the x table) and a horizontal flip into the x
 * table of the next resize (taps reversed, first' = w - first - count), so the kernels see neither.  Any tap tables may be
 * used; with grit_resample_taps_bilinear the result is bit-identical to the PIL chain.
 *
 * grit_image_batch_geo_fwd (rows B, columns B + lookup + padding + mask; before them rows A, columns A -> uint8 work buffer
 * when a_src_h > 0; images with one resize return at once from the first two):
 *   src     the uint8 blob of grit_image_batch_fwd (4-byte aligned, GRIT_IMAGE_SRC_PAD readable bytes past the last image)
 *   geo     [batch][GRIT_IMAGE_GEO_FIELDS] int64 (device): n = number of resizes (1 or 2), one spare, then two records of 14,
 *           A and B (A all zero when n = 1; B is always the resize that ends in `out`):
 *             buf      0: the window lies in src, 1: in work (B of a two-resize image)
 *             off      byte offset of the window's first pixel in that buffer (>= 0, any alignment)
 *             pitch    bytes between source rows: 3 * width of the stored image, or GRIT_IMAGE_TMP_PITCH(A's dst_w)
 *             src_h    rows of the window;  dst_h, dst_w  the resized size
 *             kx, ky, xb_off, xt_off, yb_off, yt_off   as in grit_image_batch_fwd's descriptor (tables over the window's size)
 *             tmp_off  byte offset (multiple of 4) of this resize's slot in tmp: src_h rows of GRIT_IMAGE_TMP_PITCH(dst_w)
 *             out_off  A: byte offset (multiple of 4) of its result in work, dst_h rows of GRIT_IMAGE_TMP_PITCH(dst_w);  B: zero
 *   tmp     uint8 scratch, 4-byte aligned, holding every slot (A's and B's slots of one image must not overlap)
 *   work    uint8 scratch, 4-byte aligned: every A result plus GRIT_IMAGE_SRC_PAD readable bytes; may be NULL when a_src_h = 0
 *   a_src_h, a_dst_h, a_dst_w, a_kx   maxima of src_h, dst_h, dst_w, kx over the A records; a_src_h = 0: no image has two resizes
 *   b_src_h, b_dst_w, b_kx            the same over the B records;  b_dst_w <= out_w, every B dst_h <= out_h
 *   lut, out, mask, out_h, out_w      as for grit_image_batch_fwd
 * No atomics, nothing to zero; grid extents <= 65535, A's dst_h, dst_w <= 32767.
 * ------------------------------------------------------------------------------------------------------ */
#define GRIT_IMAGE_GEO_FIELDS 30
int grit_image_batch_geo_fwd(const uint8_t* src, const int64_t* geo, const int32_t* tables, uint8_t* tmp, uint8_t* work,
                             const float* lut, int batch, int a_src_h, int a_dst_h, int a_dst_w, int a_kx, int b_src_h,
                             int b_dst_w, int b_kx, int out_h, int out_w, float* out, uint8_t* mask, void* stream);

/* ------------------------------------------------------------------------------------------------------
 * bf16 MFMA GEMM with fused epilogues (Swin Mlp, models/common/swin_model.py:31-37, on the [B*H*W, C] token maps).
 *
 *   C[M, N] = epilogue(A[M, K] . B[N, K]^T)    A, B, C, aux, bias bf16; fp32 accumulation; row-major with leading
 *                                              dimensions lda / ldb / ldc / ldaux in elements (multiples of 8)
 *   GRIT_GEMM_NONE       C = acc
 *   GRIT_GEMM_BIAS       C = acc + bias[n]
 *   GRIT_GEMM_BIAS_GELU  aux = acc + bias[n] (written when aux != NULL: the pre-activation the backward needs);
 *                        C = gelu(acc + bias[n]) in fp32 on the unrounded sum, GELU as x * sigmoid(x * P(x^2)) fitted to the
 *                        erf form (|error| <= 2.6e-5 absolute, below bf16 resolution; tools/micro/fit_gelu.py)
 *   GRIT_GEMM_DGELU      C = acc * gelu'(aux[m, n]) (aux read; the exact derivative of the same expression); colsum[s, n] = sum over rows [128 s, 128 s + 128) of C
 *                        (fp32, before the bf16 rounding of C), s < ceil(M / GRIT_GEMM_COLSUM_ROWS): fully overwritten, to be summed over s
 *                        with grit_slab_sum (the bias gradient of the Linear that produced aux)
 * Needs N % 128 == 0, K % 32 == 0, 16-byte aligned bases; M is free.  variant 0 = tile configuration chosen from the
 * shape; 1..4 = explicit eight-wave configurations, 5 = persistent ping-pong, 7 = persistent FOUR-wave kernel with 128 x 128 wave tiles (gemm_w4.hip: N % 256 == 0,
 * K % 64 == 0, M >= 256, operands below 2 GiB; what the long-map forward / input-gradient GEMMs run where it beats the library).
 * 10..13 = the eight-wave kernel's template on SHORT-map tiles (64 x 128 x 64 three slots, 128 x 128 x 64 two slots, 64 x 64 x 64 three slots (N % 64 == 0
 * suffices), 64 x 128 x 32 four slots; two or three workgroups per CU) for maps of 640 .. 12 800 rows, NONE / BIAS / BIAS_GELU only: measured against
 * the library in profiles/r06/small_gemm.txt (1-2.5 us ahead per call at N, K <= 512; not wired into the decoders: 0.3 ms per step at stake).
 * The NONE / BIAS results are bit-identical across variants (same products, same k order per accumulator).  The GELU epilogues of
 * variant 7 start from the bf16-ROUNDED pre-activation / gradient (what an unfused Linear -> GELU pair computes), those of variants
 * 1..5 from the fp32 values: equal up to that one rounding.  Variant 7 writes its GRIT_GEMM_DGELU column sums as 2 * ceil(M / 256) rows (one per
 * 128-row wave block of its 256-row tiles; every row written).
 * ------------------------------------------------------------------------------------------------------ */
#define GRIT_GEMM_NONE 0
#define GRIT_GEMM_BIAS 1
#define GRIT_GEMM_BIAS_GELU 2
#define GRIT_GEMM_DGELU 3
#define GRIT_GEMM_BIAS_RES 4   /* grit_gemm_bf16_nt_res only */
#define GRIT_GEMM_BIAS_RELU_DROP 5   /* grit_gemm_bf16_nt_relu only */
#define GRIT_GEMM_DRELU 6            /* grit_gemm_bf16_nt_relu only */
#define GRIT_GEMM_COLSUM_ROWS 128
int grit_gemm_bf16_nt(const void* A, long lda, const void* B, long ldb, void* C, long ldc, int M, int N, int K,
                      int epilogue, const void* bias, void* aux, long ldaux, float* colsum, int variant, void* stream);
/* variant 9 = variant 7 with the tile height chosen by shape: 256 rows, or 224 where that needs fewer 16-row block rows per CU
 * (the N = C products of the Swin blocks -- proj, fc2 forward, fc1 / qkv input gradients: 400 / 800 / 200 tiles of 256 rows fill the
 * 256 CUs 1.56 / 3.1 / 0.78 times, 458 / 915 / 232 tiles of 224 rows 1.79 / 3.6 / 0.91 times: 12.5 % less time, same rounds).  Same
 * products in the same k order: results bit-identical to variant 7.  grit_gemm_w4_tile_rows(M, N) = the height variant 9 runs for a
 * shape on the current device; its GRIT_GEMM_DGELU column sums are 2 * ceil(M / height) rows. */
int grit_gemm_w4_tile_rows(int M, int N);
/* The output projection of a Swin branch WITH its residual connection (models/common/swin_model.py:289-298:
 * x = shortcut + drop_path(proj(...)) / x = x + drop_path(mlp(...))):
 *     C[m, n] = residual[m, n] + row_scale[m / rows_per_sample] * bf16(acc[m, n] + bias[n])
 * -- the branch rounded to bf16 as an unfused Linear stores it, product and sum in fp32 (not fused), one rounding: bit for bit what
 * grit_add_layernorm_fwd computes as its `sum_out` from a stored branch.  row_scale NULL = 1 (then rows_per_sample is ignored);
 * otherwise rows_per_sample >= 256.  The branch map is never written or re-read.  N % 256 == 0 and K % 64 == 0: variant 7's kernel and
 * shape limits; other N % 128 == 0, K % 32 == 0 (the 128 output columns of the stage-0 map): the per-tile kernel on 256 x 128 tiles.
 * C must not overlap residual: the four-wave kernel shifts its last row tile back to end at row M and computes and stores the rows it
 * shares with the tile before it twice -- in place the branch would be added twice there. */
int grit_gemm_bf16_nt_res(const void* A, long lda, const void* B, long ldb, void* C, long ldc, int M, int N, int K,
                          const void* bias, const void* residual, long ldres, const float* row_scale, int rows_per_sample,
                          void* stream);
/* The position-wise FFNs of the two decoders and the grid net (models/detection/det_module.py:302-304, models/common/pos_embed.py:44-48:
 * Linear -> ReLU -> dropout -> Linear) on the short-map tiles (variant 12's 64 x 64 x 64; N % 64 == 0, K % 64 == 0), ReLU + dropout in the
 * epilogues instead of a launch each way:
 *   GRIT_GEMM_BIAS_RELU_DROP   C = dropout(relu(bf16(A B^T + bias)), drop_p): the first Linear's forward; keep factors from the hash of
 *                              grit_relu_dropout_fwd over the element index m * N + n (ldc == N), seed read from seed_dev when drop_p > 0;
 *                              bit for bit Linear (bf16 result) followed by grit_relu_dropout_fwd.  aux unused.
 *   GRIT_GEMM_DRELU            C = aux > 0 ? bf16(A B^T) / (1 - drop_p) : 0, aux [M, N] = the forward's C (positive exactly where the unit
 *                              was active and kept): the second Linear's input gradient with the backward of ReLU + dropout applied;
 *                              bit for bit the stored bf16 product followed by grit_relu_dropout_bwd.  bias, seed_dev unused. */
int grit_gemm_bf16_nt_relu(const void* A, long lda, const void* B, long ldb, void* C, long ldc, int M, int N, int K, int epilogue,
                           const void* bias, const void* aux, long ldaux, float drop_p, const uint64_t* seed_dev, void* stream);
/* The fused Mlp GEMMs with the per-sample drop-path factors of the Swin blocks at hand (models/common/swin_model.py:289-298:
 * x = shortcut + drop_path(mlp(norm2(x))); a dropped sample's branch contributes nothing forward and receives an exactly zero
 * gradient): row_scale [ceil(M / rows_per_sample)] f32 on the device; a 256-row tile that lies inside ONE sample with factor 0 is
 * not computed.  GRIT_GEMM_DGELU (backward: the rows of A are already zero): C and its column sums are written as
 * zeros -- the same results as grit_gemm_bf16_nt.  GRIT_GEMM_BIAS_GELU (forward): C and aux are written as zeros instead of the values
 * nobody will use (the caller multiplies the branch by the same factor 0; the saved tensors meet zero gradients).  Eight-wave
 * variants (0..4); row_scale NULL = no skipping. */
int grit_gemm_bf16_nt_rows(const void* A, long lda, const void* B, long ldb, void* C, long ldc, int M, int N, int K, int epilogue,
                           const void* bias, void* aux, long ldaux, float* colsum, const float* row_scale, int rows_per_sample,
                           int variant, void* stream);
/* The Mlp half of a frozen stage-0 Swin block in one launch (grit_amd/csrc/mlp_s0.hip; forward only, no dropout, no drop path):
 *     x_out = x + fc2(gelu(fc1(LayerNorm(x; norm_w, norm_b, eps)) + b1)) + b2        n_out = LayerNorm(x_out; next_w, next_b, next_eps)
 * x, x_out, n_out [rows, C] bf16 contiguous; w1 [hidden, C], w2 [C, hidden], biases and norm parameters bf16.  next_w / next_b / n_out all
 * NULL: no second LayerNorm.  Bit for bit the values of grit_layernorm_fwd -> grit_gemm_bf16_nt / GRIT_GEMM_BIAS_GELU (aux NULL) ->
 * grit_gemm_bf16_nt_res without factors (= GRIT_GEMM_BIAS + a bf16 add) -> grit_layernorm_fwd; the hidden map and the first LayerNorm's
 * output never reach memory.  C == 128 and hidden == 512 only (GRIT_ERR_UNSUPPORTED otherwise); any rows >= 1, rows past the end are
 * neither read nor written; x_out and n_out must not alias x; pointers 16-byte aligned (b1, b2: 8). */
int grit_mlp_s0_fwd_bf16(const void* x, const void* norm_w, const void* norm_b, float eps, const void* w1, const void* b1,
                         const void* w2, const void* b2, const void* next_w, const void* next_b, float next_eps, int rows, int C,
                         int hidden, void* x_out, void* n_out, void* stream);

/* ------------------------------------------------------------------------------------------------------
 * Beam-search candidate selection (reference models/caption/transformer.py:184-188: descending sort of the flattened
 * [beam * vocabulary] candidates, first `beam` kept).  x [rows, n] float32 with row stride ld (elements); the k <= 8 best of
 * every row, best first: idx_out [rows, k] int64 (position in the row), val_out [rows, k].  Equal values: lower index first;
 * NaN ranks above every number (torch's order).  Safe to capture in a HIP graph (no workspace, no host state).
 * ------------------------------------------------------------------------------------------------------ */
int grit_topk_rows_f32(const float* x, long ld, int rows, int n, int k, int64_t* idx_out, float* val_out, void* stream);

/* ------------------------------------------------------------------------------------------------------
 * One beam-search step after the decoder (reference models/caption/transformer.py:208-240, `iter`), for B images with
 * cur_beam live beams each and a vocabulary of V words: grit_beam_step(args, stream), every variant of the step through the one
 * argument struct below.  A zero-initialised struct with the source, beam state, sizes, workspace and outputs filled is the plain
 * step; the bans, the groups and the forced words are switched on by their own fields and described after it.
 *
 * Source, beam state, sizes, outputs.  logp [B * cur_beam, V] float32 word log-probabilities (row stride ld; maps[0] when
 * n_maps == 1), seq_logprob [B * cur_beam] running scores, seq_mask [B * cur_beam] 1 while a beam is alive, prev_words
 * [B * cur_beam] int64 the words chosen at the previous step (both ignored when first_step != 0: every beam alive).
 *     alive      = seq_mask * (prev_words != eos)
 *     candidate  = alive ? seq_logprob + logp : (word == 0 ? seq_logprob : -999)
 *     the k <= 8 best candidates of each image over (beam, word), best first; equal scores by ascending beam * V + word
 * Outputs, all [B, k]: sel_beam / sel_word int64, new_seq_logprob (the candidate score), new_seq_mask (alive of the source beam),
 * picked_logprob = logp[sel_beam][sel_word] * alive.  Bit-identical to the reference's composed arithmetic.
 * workspace: grit_beam_step_workspace(B, cur_beam, k) bytes of device memory, no initialisation needed.  Limits: cur_beam * k <= 64
 * (16 at first_step), B <= 65535.  Two launches; safe to capture in a HIP graph.
 *
 * The mean of n_maps <= 8 maps: the step of an ensemble of captioners (reference models/caption/ensemble.py:128-214), the plain
 * step applied to the average of n_maps word log-probability maps, each [B * cur_beam, V] float32 with the common row stride ld.
 * maps is a HOST array of n_maps device pointers; they travel by value in the kernel arguments (no table to upload, nothing that
 * a captured HIP graph has to keep alive).  The average is formed in registers while the candidates are scored -- it is never
 * written -- and is bit-identical to torch.stack(maps).mean(0) on the device: per element, map m is added to accumulator m % 4
 * (each starting at 0), the four are summed as ((a0 + a1) + a2) + a3 and multiplied by float(N) / float(n_maps * N), N =
 * B * cur_beam * V.  picked_logprob is taken from that average.  Outputs, workspace, limits and the order of ties are those of
 * one map.  n_maps == 1 reads maps[0] directly; the mean of one map, (0 + x) * 1.0f, is the same bits except that it turns a
 * stored -0.0 into +0.0, so only the sign of a picked_logprob (or score) that is exactly zero could ever tell the two apart.
 *
 * Bans: the step under constraints (no ancestor in the reference), on when any of no_repeat_ngram > 0, no_repeat_word, ban_eos,
 * n_suppress > 0 is set, and always on for a step with forced words; with all four off (and no forced words) t and history are
 * not read and t is not checked against its limit.  The candidate score of every banned (beam, word) pair is replaced by -inf.
 * Step t chooses word position t; history [B * cur_beam, t] int64 (row stride history_ld elements; may be NULL when t == 0) holds
 * the words h_0 .. h_{t-1} of every source beam.  A beam is live when first_step != 0 or seq_mask * (prev_words != eos) != 0.
 * The banned set of a LIVE beam is the union of
 *     ban_eos != 0          eos                                    (the caller sets it while t < its minimum length)
 *     suppress[0 .. n_suppress)  always; a HOST array of ids in [0, V), copied into the kernel arguments (nothing to upload,
 *                           nothing that a captured HIP graph has to keep alive)
 *     no_repeat_word != 0   h_{t-1}, when t >= 1
 *     no_repeat_ngram = n >= 1   h_{i+n-1} for every 0 <= i <= t - n with h_i .. h_{i+n-2} == h_{t-n+1} .. h_{t-1}
 *                           (n == 1: every word of the history; nothing while t < n); 0 = off
 * and a finished beam has none (it lives through word 0 alone).  History words outside [0, V) ban nothing and are never used as
 * an index (they still take part in the comparisons).  A banned candidate stays a candidate with its own index: with a small V and
 * many bans -inf candidates are selected, by ascending beam * V + word.  picked_logprob is the word's log-prob as stored, banned or
 * not.  With every constraint off the plain stage 1 runs: a rule that bans nothing leaves every bit as it is.  The host
 * form is grit_amd/ops/beam.py: banned_words_host.  Outputs, workspace, limits and the order of ties are those of the plain step.
 * Further limits (GRIT_ERR_UNSUPPORTED beyond them, the caller uses the host form):
 * 0 <= t <= GRIT_BEAM_MAX_HISTORY, n_suppress <= GRIT_BEAM_MAX_SUPPRESS, and a vocabulary slice (V / 8 at the first step, else
 * V / 2, rounded up to a multiple of 4) of at most GRIT_BEAM_MAX_SLICE words.  A suppress id outside [0, V), eos outside [0, V)
 * with ban_eos, negative t / no_repeat_ngram, or history == NULL with t > 0: GRIT_ERR_BAD_ARG.  No atomics on global memory, no
 * host state.
 *
 * Groups (groups >= 1; 0 is the plain merge): the step of a DIVERSE (group) beam search with a Hamming penalty (Vijayakumar et
 * al. 2016; no ancestor in the reference).  The k beams are `groups` groups of g = k / groups, group i owns the source rows and
 * the output positions [i * g, (i + 1) * g) (at the first step, cur_beam == 1, every group reads row 0), and within the step the
 * groups are resolved in the order 0 .. groups - 1 per image.  counts[w] = how many selections of groups 0 .. i - 1 in THIS step
 * chose word w from a LIVE source row (a finished row that survives through word 0 counts nothing; two beams choosing w count
 * 2).  Group i scores
 *     live row j, word w:   seq_logprob[j] + (logp[j][w] - diversity * float(counts[w]))
 *                           one fp32 multiply, one fp32 subtract, the fp32 add of the plain step; never an fma
 *     finished row j:       seq_logprob[j] at word 0, -999 elsewhere (no penalty)
 *     banned (row, word):   -inf, penalised or not
 * and takes its g best of its g * V candidates, value descending, equal values by ascending row * V + word.  Outputs at position
 * i * g + r: sel_beam (the source row among all cur_beam), sel_word, new_seq_logprob = the PENALISED candidate score, new_seq_mask
 * = the source row's liveness, picked_logprob = the unpenalised logp[sel_beam][sel_word] * liveness.  logp is one map or the
 * mean of n_maps <= 8 maps exactly as above (a penalised score re-forms the mean the same way); the bans are those above.  With
 * counts == 0 the score is the plain step's bit for bit, so groups == 1 gives the outputs of groups == 0 with the same source and
 * bans, whatever the diversity.  The host form is grit_amd/ops/beam.py: beam_step_groups_host.
 *
 * The penalty only lowers candidates, and in one source row at most |P| <= k - g of them (P: the words chosen so far in this
 * step), so a group's g best of a row are among that row's UNPENALISED k best: stage 1 is the first launch of the plain /
 * constrained step with k entries per list, and all the sequential group logic is the second launch, one wave per image over the
 * same <= 128 candidates.  Limits (GRIT_ERR_UNSUPPORTED beyond them, the
 * caller uses the host form): k <= 8, k % groups == 0, cur_beam == 1 or cur_beam == k, V >= k, diversity finite and >= 0,
 * B <= 65535, and with any ban on the limits of the bans.  groups < 0: GRIT_ERR_BAD_ARG.  No atomics on global memory, no host
 * state, nothing uploaded.
 *
 * Forced words (force_words != NULL; NULL is not a forced step): the step with FORCED words (dynamic beam allocation, Post &
 * Vilar 2018; no ancestor in the reference).  It has no groups: force_words with groups > 0 is GRIT_ERR_BAD_ARG.
 * force_words [B, n_sets, n_words] int64, padded with -1, lives on the device: set c of image b is the ids >= 0 of
 * force_words[b][c], a disjunction ("dog" or "dogs"); a set with no ids counts as met from the start.  Every beam carries met, an
 * int32 bitmask of the sets that its words so far have hit; full = all n_sets bits.  met_in [B * cur_beam] may be NULL (the first
 * step): every row of image b then starts from the mask of b's empty sets.  A step for an image with cur_beam source rows and
 * k = beam, liveness of a row exactly that of the bans:
 *   1. Bans.  A live row has the bans above (ban_eos, suppress, no_repeat_word, no_repeat_ngram), and <eos>
 *      is banned in addition while met != full.
 *   2. Candidates A.  Row j contributes its k best candidates under the constrained step's scoring: a live row scores
 *      seq_logprob[j] + logp[j][w] (one fp32 add; -inf where banned), ties to the ascending word -- what stage 1 of that step
 *      leaves in the workspace.  A finished row contributes only its word-0 candidate with the score seq_logprob[j]; its -999
 *      siblings are not candidates here.
 *   3. Candidates F.  A live row j also contributes (j, w) for every w of a set that row j has not met and that is not banned for
 *      that row, scored by the same single add (for n_maps > 1 on the mean re-formed exactly as stage 1 forms
 *      it).  Duplicates of (j, w) are kept once; their scores are identical bits.
 *   4. Banks.  met'(j, w) = met[j] | {c : w in set c} for a live row, met[j] for a finished row; bank = popcount(met'); a
 *      candidate that scores -inf goes to bank -1.
 *   5. Inside a bank the candidates are ordered by score descending, then by j * V + w ascending.
 *   6. Slots.  For round r = 0, 1, 2, ... and within a round for bank = n_sets down to -1: if the bank has more than r candidates
 *      and fewer than k are chosen, choose its r-th.  (There are always at least k candidates: k from row 0 at the first step,
 *      later at least one per row.)
 *   7. Outputs, at the position given by the order of choice: sel_beam, sel_word, new_seq_logprob = the candidate's score,
 *      new_seq_mask = the source row's liveness, picked_logprob = the stored log-prob * liveness as in the other steps, and
 *      new_met [B, k] int32 = met'.
 * By construction the top candidate of the highest non-empty bank gets a slot at every step and banks only grow, so with at least
 * n_sets steps and no forced word under a ban the best hypothesis of the top bank holds a word of every set; that it also reaches
 * <eos> is not promised.  The host form is grit_amd/ops/beam.py: beam_step_forced_host.
 *
 * Stage 1 is the first launch of the step under bans (k entries per list) with the one per-row addition of the <eos> ban;
 * stage 2 is one workgroup per image over at most cur_beam * (k + n_sets * n_words) <= 320 candidates in LDS: it gathers the
 * forced candidates from logp, tests them against the row's ban rules, removes duplicates, banks, ranks and stores.  Limits
 * (GRIT_ERR_UNSUPPORTED beyond them, the caller uses the host form): k <= 8,
 * cur_beam == 1 or cur_beam == k, V >= k, n_sets <= GRIT_BEAM_MAX_FORCED_SETS, n_words <= GRIT_BEAM_MAX_FORCED_WORDS, and the
 * limits of the bans.  n_sets < 1, n_words < 1, or new_met == NULL: GRIT_ERR_BAD_ARG; new_met is required exactly when
 * force_words is set and is not written otherwise.  Forced ids outside [0, V) are skipped.  No atomics on global memory, no host
 * state, nothing uploaded.
 *
 * Every variant: workspace = grit_beam_step_workspace(B, cur_beam, k) bytes, two launches, safe to capture in a HIP graph.  A
 * refusal writes nothing to the outputs.  Statuses are decided in this order: GRIT_ERR_BAD_ARG for a NULL maps, a size or n_maps
 * <= 0, a negative rule, groups or t, a ban without its history, eos or suppress pointer, forced words with groups or without
 * their sizes or new_met; GRIT_ERR_UNSUPPORTED beyond a limit of the source (n_maps), the bans (t, n_suppress), the groups or the
 * forced words; GRIT_ERR_BAD_ARG for a NULL map, state, workspace or output pointer, ld < V or a suppress id outside [0, V);
 * GRIT_ERR_UNSUPPORTED beyond a limit of the plain step or of the bans' slice; GRIT_ERR_BAD_ARG for a workspace that is too small.
 * ------------------------------------------------------------------------------------------------------ */
#define GRIT_BEAM_MAX_HISTORY 64
#define GRIT_BEAM_MAX_SUPPRESS 16
#define GRIT_BEAM_MAX_SLICE 65536
#define GRIT_BEAM_MAX_FORCED_SETS 8
#define GRIT_BEAM_MAX_FORCED_WORDS 4
typedef struct grit_beam_step_args {
    /* source */
    const float* const* maps;  /* HOST array of n_maps device pointers */
    int n_maps;
    long ld;
    /* beam state */
    const float* seq_logprob;
    const float* seq_mask;
    const int64_t* prev_words;
    int eos, first_step;
    /* sizes */
    int B, cur_beam, V, k;
    /* bans */
    const int64_t* history;
    long history_ld;
    int t, no_repeat_ngram, no_repeat_word, ban_eos;
    const int* suppress;  /* HOST array of n_suppress ids */
    int n_suppress;
    /* groups */
    int groups;  /* 0: the plain merge */
    float diversity;
    /* forced words */
    const int64_t* force_words;  /* NULL: not a forced step */
    int n_sets, n_words;
    const int* met_in;
    /* workspace */
    void* workspace;
    long workspace_bytes;
    /* outputs */
    int64_t* sel_beam;
    int64_t* sel_word;
    float* new_seq_logprob;
    float* new_seq_mask;
    float* picked_logprob;
    int* new_met;
} grit_beam_step_args;
long grit_beam_step_workspace(int B, int cur_beam, int k);
int grit_beam_step(const grit_beam_step_args* args, void* stream);

/* ------------------------------------------------------------------------------------------------------
 * One step of sampled decoding after the decoder (no ancestor in the reference, whose only decoder is beam search): one word per
 * output row, drawn from softmax(logp * inv_temperature) restricted to the top_k most probable words and then to the smallest
 * nucleus of mass top_p.  Output row r reads row r / fan of logp [rows / fan, V] float32 (row stride ld elements): at the first
 * step the decoder ran on one row per image and fan = samples per image, afterwards fan = 1.  prev_words [rows] int64 and alive_in
 * [rows] float32 are NULL together: NULL = first step, every row alive.  top_p_q32 = round(top_p * 2^32) in [1, 2^32].  seed_dev
 * points to ONE uint64 in device memory.  Outputs, all [rows]: words int64, picked float32, alive_out float32.
 *
 * The choice is a function of the stored bits of logp, *seed_dev, r and step and of nothing else (no atomics, no workspace, no host
 * state), so a captured HIP graph replays it and a host form (grit_amd/ops/sample.py: sample_step_host) repeats it bit for bit:
 *   0. alive = alive_in[r] * (prev_words[r] != eos).  0: words = fill, picked = +0.0, alive_out = 0, done.  Otherwise alive_out = 1.
 *   1. m = max_i logp_i.
 *   2. t_i = ((logp_i - m) * inv_temperature) * log2e, three rounded fp32 operations (log2e = 0x3FB8AA3B);
 *      k_i = floor(t_i), f_i = t_i - k_i.
 *   3. p_i = P(f_i) ~ 2^f: degree 6, Horner in fp32, every multiply and add rounded, coefficients (constant first) 0x3F800000,
 *      0x3F317216, 0x3E75FEAD, 0x3D634478, 0x3C1E8620, 0x3AA36993, 0x3962A320.  P(0) = 1 and P(1) = 2 exactly, P is monotone on
 *      [0, 1], largest relative error 8.6e-8.
 *   4. w_i = trunc(p_i * 2^(40 + k_i)) as uint64; 0 when 40 + k_i < -1 and for logp_i = -inf.  The largest weight is 2^40.
 *   5. order: i before j iff logp_i > logp_j, or they are equal and i < j.  K = top_k > 0 ? min(top_k, V) : V; S_K = the weight
 *      sum of the first K in that order.
 *   6. need = max(1, (top_p_q32 * S_K) >> 32) (128-bit product); kept = the shortest prefix of the first K whose weight sum is
 *      >= need, at least one word; a boundary inside a group of equal log-probs is resolved by index.  S = the kept sum.
 *   7. c = *seed_dev + 0x9E3779B97F4A7C15 * (r * 4096 + step + 1) mod 2^64, x = splitmix64's finaliser of c
 *      (x ^= x >> 30, x *= 0xBF58476D1CE4E5B9, x ^= x >> 27, x *= 0x94D049BB133111EB, x ^= x >> 31), target = (x * S) >> 64.
 *   8. word = the smallest kept i whose cumulative kept weight, summed in INDEX order, exceeds target.
 *   9. picked = logp[word] as stored: the model's log-prob, not the tempered or truncated one.
 * NaN or +inf log-probs and a live row without a finite entry are outside the contract: the word is then unspecified but in
 * [0, V), and nothing out of bounds is read or written.  Limits: 1 <= V <= GRIT_SAMPLE_MAX_V (UNSUPPORTED above), ld >= V,
 * fan >= 1, rows % fan == 0, 0 <= step < 4096, top_k >= 0, inv_temperature finite and > 0.  One launch, a workgroup per row.
 * ------------------------------------------------------------------------------------------------------ */
#define GRIT_SAMPLE_MAX_V 16384
int grit_sample_step_f32(const float* logp, long ld, int rows, int fan, int V, const int64_t* prev_words, const float* alive_in,
                         int eos, int fill, float inv_temperature, int top_k, unsigned long long top_p_q32,
                         const uint64_t* seed_dev, int step, int64_t* words, float* picked, float* alive_out, void* stream);

/* ------------------------------------------------------------------------------------------------------
 * Gated merge of the grid / region cross-attentions of a caption decoder layer, inference only (reference
 * models/caption/cap_generator.py:44-56).  All tensors [rows, d] row-major of one dtype (is_bf16: bfloat16, else float32),
 * d % 8 == 0, 16-byte aligned; mask_pad [rows] of the same dtype (1 = real token, 0 = padding).
 *   grit_gate_pack: X [2 * rows, 2 * d] with X[r] = (self_att[r], enc1[r] * mask_pad[r]), X[rows + r] = (self_att[r], enc2[r] * mask_pad[r])
 *                   -- the two inputs of fc_alpha1, stacked so that ONE GEMM produces both gate pre-activations.
 *   grit_gate_fuse: gates [2 * rows, d] = fc_alpha1(X);  out[r] = ((enc1*m * sigmoid(gates[r]) + enc2*m * sigmoid(gates[rows + r]))
 *                   * (1 / divisor)) * m, every step rounded to the tensor dtype as the composed torch form rounds it.
 * ------------------------------------------------------------------------------------------------------ */
int grit_gate_pack(const void* self_att, const void* enc1, const void* enc2, const void* mask_pad, int rows, int d, int is_bf16,
                   void* X, void* stream);
int grit_gate_fuse(const void* enc1, const void* enc2, const void* gates, const void* mask_pad, int rows, int d, float divisor,
                   int is_bf16, void* out, void* stream);

/* ------------------------------------------------------------------------------------------------------
 * Element-wise glue of the decoders in the TRAINING step, one launch each instead of a chain of 4-14 torch launches at the ~6 us
 * dependent-launch floor (grit_amd/csrc/glue.hip).  fp32 arithmetic in the reference's operation order, outputs rounded once.
 *
 * grit_msda_geometry_fwd / _bwd -- MSDeformAttn.forward's query-side arithmetic, models/ops/modules/ms_deform_attn.py:97-113:
 *   offsets [rows, M, L, P, 2], logits [rows, M, L*P] (bf16 or f32: the outputs of sampling_offsets / attention_weights; rows =
 *   B * Lq), ref [rows, L, ref_dim] f32 (ref_dim 4: box cx, cy, w, h -> loc = ref_xy + offset / P * wh * 0.5; ref_dim 2: point ->
 *   loc = ref_xy + offset / (W_l, H_l), spatial_shapes [L, 2] int64 (H, W)), L*P <= 64
 *     -> loc [rows, M, L, P, 2] f32, attn_w [rows, M, L*P] f32 = softmax(logits) over the L*P points.
 *   backward: grad_offsets / grad_logits (bf16 or f32) from grad_loc, grad_attn_w, attn_w; ref receives no gradient (the
 *   reference detaches it: det_module.py:52).
 * grit_box_refine -- DetectionModule.bbox_refine, det_module.py:40-53: out [rows, 4] f32 = sigmoid(delta + inverse_sigmoid(ref))
 *   (ref_dim 4) or sigmoid(cat(delta[:2] + inverse_sigmoid(ref), delta[2:])) (ref_dim 2); delta [rows, 4] bf16 / f32.
 * grit_relu_dropout_fwd / _bwd -- dropout(relu(x)) of the position-wise FFNs (det_module.py:302-304, pos_embed.py:44-48), n
 *   elements; the keep mask is a counter hash of (element index, *seed_dev) regenerated in the backward (dx = dy * keep / (1 - p)
 *   where x > 0); p = 0: plain ReLU and its gradient.
 * grit_gate_bwd_a / _b -- backward of the gated merge of models/caption/cap_generator.py:44-56 around the fc_alpha1 GEMMs (forward:
 *   grit_gate_pack, GEMM, grit_gate_fuse): a: d_gates [2 rows, d] from d_out, enc1, enc2, gates, mask_pad; b: d_self, d_enc1,
 *   d_enc2 [rows, d] from d_out, gates, mask_pad and dX [2 rows, 2 d] = d_gates @ W.  One dtype (bf16 / f32) for all tensors.
 * ------------------------------------------------------------------------------------------------------ */
int grit_msda_geometry_fwd(const void* offsets, const void* logits, int in_is_bf16, const float* ref, int ref_dim,
                           const int64_t* spatial_shapes, long rows, int M, int L, int P, float* loc, float* attn_w, void* stream);
int grit_msda_geometry_bwd(const float* grad_loc, const float* grad_attn_w, const float* attn_w, const float* ref, int ref_dim,
                           const int64_t* spatial_shapes, long rows, int M, int L, int P, int out_is_bf16, void* grad_offsets,
                           void* grad_logits, void* stream);
int grit_box_refine(const void* delta, int delta_is_bf16, const float* ref, int ref_dim, long rows, float* out, void* stream);
int grit_relu_dropout_fwd(const void* x, long n, float p, const uint64_t* seed_dev, int is_bf16, void* y, void* stream);
int grit_relu_dropout_bwd(const void* x, const void* dy, long n, float p, const uint64_t* seed_dev, int is_bf16, void* dx, void* stream);
int grit_gate_bwd_a(const void* d_out, const void* enc1, const void* enc2, const void* gates, const void* mask_pad, long rows, int d,
                    float divisor, int is_bf16, void* d_gates, void* stream);
int grit_gate_bwd_b(const void* d_out, const void* gates, const void* mask_pad, const void* dX, long rows, int d, float divisor,
                    int is_bf16, void* d_self, void* d_enc1, void* d_enc2, void* stream);

/* ------------------------------------------------------------------------------------------------------
 * Key / value cache of step-wise decoding under beam search (reference models/common/attention.py:166-181 appends with torch.cat,
 * models/caption/transformer.py:229 re-gathers every state by the surviving beam): for B images with `beam` surviving beams each,
 *     out[(b, j)][0 .. t_old) = old[(b, src_beam[b][j])][0 .. t_old)      (old holds cur_beam histories per image)
 *     out[(b, j)][t_old]      = new[(b, j)]
 * for keys and values in one launch.  old_* [B * cur_beam, t_old, row_bytes] contiguous (ignored when t_old == 0), new_* one row per
 * (b, j) at new_row_stride_bytes (a slice of the fused q/k/v projection), out_* [B * beam, t_old + 1, row_bytes] contiguous.
 * src_beam [B * beam] int64 (index of the source beam within the image) or NULL = identity (then cur_beam must equal beam).
 * Byte copies: any dtype; row_bytes, strides and bases 16-byte aligned.
 * ------------------------------------------------------------------------------------------------------ */
int grit_kv_append(const void* old_k, const void* old_v, const int64_t* src_beam, int B, int cur_beam, int beam, int t_old,
                   int row_bytes, const void* new_k, const void* new_v, long new_row_stride_bytes, void* out_k, void* out_v,
                   void* stream);

/* ------------------------------------------------------------------------------------------------------
 * Inputs of one step of step-wise decoding (reference models/caption/cap_generator.py:116-137 get_seq_inputs in stateful mode and the
 * embedding sum of :148).  tokens [rows] int64; word_emb [vocab, d], pos_emb [n_pos, d] (is_bf16: bfloat16, else float32);
 * running_seq [rows] int64 step counters, advanced in place; old_mask [rows, t_old] bytes (1 = masked key), ignored when t_old == 0.
 *     pos = ++running_seq[r];  x[r] = word_emb[tokens[r]] + pos_emb[pos];  mask_pad[r] = tokens[r] != pad_idx (as 1 / 0 in the table dtype);
 *     new_mask[r] = (old_mask[r], tokens[r] == pad_idx)            [rows, t_old + 1]
 * The caller checks that the step count stays inside pos_emb (the kernel clamps instead of faulting).
 * ------------------------------------------------------------------------------------------------------ */
int grit_decode_step_inputs(const int64_t* tokens, int64_t pad_idx, const void* word_emb, int vocab, const void* pos_emb, int n_pos,
                            int d, int is_bf16, int64_t* running_seq, const uint8_t* old_mask, int t_old, int rows, void* x,
                            void* mask_pad, uint8_t* new_mask, void* stream);

/* ------------------------------------------------------------------------------------------------------
 * CIDEr-D reward of self-critical training (reference engine/caption_engine.py:433-438: decode the beams up to <eos>, PTB-tokenise,
 * score against the image's ground-truth captions; datasets/caption/metrics/cider/cider_scorer.py: tf-idf vectors of the 1..4-grams,
 * clipped cosine similarity, Gaussian length penalty exp(-(len_h - len_r)^2 / (2 sigma^2)), mean over orders and references, x 10).
 * One launch, one workgroup per hypothesis row, float64 arithmetic with every sum in the host's order and no atomics: two launches
 * on the same input are bit-identical.
 *
 * tokens [rows, T] int64, contiguous; rows = images * beam; slots [rows / beam] int32 = the reference slot of each image;
 * out32 [rows] float32; out64 [rows] float64 or NULL.  An empty hypothesis scores 0.  A word id outside [0, vocab) in front of the
 * first <eos>, or a slot outside [0, n_slots), gives NaN for that row (the host path raises there).
 * T * width > GRIT_CIDER_MAX_TOKENS or width > GRIT_CIDER_MAX_EXPANSION: GRIT_ERR_UNSUPPORTED.  Any number of references per image.
 * The tables are built by grit_amd/ops/cider.py (DeviceCider); every pointer is device memory:
 *   expansion [vocab, 2, width] int32   tokens of a word anywhere in the caption ([w][0]) and as its last non-blank word ([w][1])
 *   word_meta [vocab] int32             bits 0-3 count of [w][0], bits 4-7 count of [w][1], GRIT_CIDER_META_BLANK (whitespace-only
 *                                       word), GRIT_CIDER_META_EOS (ends the row)
 *   idf_key / idf_val                   the corpus n-grams as a trie flattened order by order: idf_key[idf_start[k] .. idf_start[k+1])
 *                                       sorted keys (index of the (k)-gram prefix within order k-1, 0 for k = 0) << 32 | token of the
 *                                       (k+1)-grams; idf_val = log(corpus size) - log(max(1, document frequency)) of the same entry.
 *                                       An absent n-gram has idf = log_corpus.
 *   slot_ref_start [n_slots + 1]        references of a slot, CSR
 *   ref_ent_start [4 * n_refs + 1]      entries of (reference, order), CSR; ent_tok [entries] int4 = the n-gram's tokens padded with
 *                                       -1 (16-byte aligned); ent_w [entries] its tf-idf weight; ref_norm [n_refs, 4]; ref_len [n_refs]
 *                                       (length in bigram occurrences)
 * ------------------------------------------------------------------------------------------------------ */
#define GRIT_CIDER_MAX_TOKENS 256
#define GRIT_CIDER_MAX_EXPANSION 8
#define GRIT_CIDER_META_FIN_SHIFT 4
#define GRIT_CIDER_META_BLANK 256
#define GRIT_CIDER_META_EOS 512
typedef struct {
    const int32_t* expansion;
    const int32_t* word_meta;
    int vocab, width;
    const uint64_t* idf_key;
    const double* idf_val;
    long idf_start[5];
    const int32_t* slot_ref_start;
    int n_slots;
    const int32_t* ref_ent_start;
    const void* ent_tok;
    const double* ent_w;
    const double* ref_norm;
    const int32_t* ref_len;
    double sigma, log_corpus;
} grit_cider_tables;
int grit_cider_reward(const int64_t* tokens, int rows, int T, const int32_t* slots, int beam, const grit_cider_tables* tab,
                      float* out32, double* out64, void* stream);

/* ------------------------------------------------------------------------------------------------------
 * Consensus (minimum-Bayes-risk) reranking of the n candidate captions of an image under CIDEr-D (Devlin et al. 2015, "consensus
 * reranking"): the candidate that agrees most with the others is chosen.  The references of a candidate are the OTHER candidates of
 * its image, not ground-truth captions; a candidate as a reference has the vector it has as a hypothesis (tf * idf at each n-gram's
 * first occurrence, norms summed in first-occurrence order, length in bigram occurrences), so nothing is cooked on the host.
 * The host form, and the yardstick of the tests, is grit_amd/ops/consensus.py: consensus_host.
 *
 * tokens [images, n, T] int64, contiguous.  A row's caption is its words in front of the first <eos>, with collapse != 0 after
 * dropping every word equal to its predecessor, tokenised through the per-word tables exactly as grit_cider_reward and
 * grit_caption_scores do.  With v_i the tf-idf vectors of candidate i:
 *     sim[b, i, j]  = the clipped similarity of hypothesis v_i against reference v_j (min(w_h, w_r) * w_r per shared n-gram, over the
 *                     norms, Gaussian length penalty, mean over the orders) for i != j, 0 for i == j: NOT symmetric;
 *     score[b, i]   = (sum over j != i, j ascending, of sim[b, i, j]) / (n - 1) * 10, 0 when n == 1;
 *     best[b]       = the smallest i whose score is maximal.
 * sim64 [images, n, n] float64 or NULL; score64 [images, n] float64; score32 [images, n] float32 or NULL; best [images] int32;
 * bad [images] int32.  An empty caption has similarity 0 in both directions and is still a candidate.  If any row of an image holds
 * a word id outside [0, vocab) in front of its first <eos> (the host form raises), every sim and score of that image is NaN,
 * best = 0 and bad = 1; bad = 0 otherwise.  Other images are unaffected.
 *
 * Two launches (cook every row; score and select per image), float64 arithmetic with every sum in the host's order, no atomics, no
 * synchronisation, no allocation: two calls on the same input are bit-identical.  workspace: grit_cider_consensus_workspace(images,
 * n, T) bytes of device memory, no initialisation needed (0 for arguments that the call itself refuses).
 * Of `tab` only expansion, word_meta, vocab, width, the idf trie, sigma and log_corpus are read: tables without any reference slot
 * (n_slots == 0) are accepted.  Limits: n > GRIT_CONSENSUS_MAX_CANDIDATES, width > GRIT_CIDER_MAX_EXPANSION or
 * T * width > GRIT_CIDER_MAX_TOKENS: GRIT_ERR_UNSUPPORTED.
 * ------------------------------------------------------------------------------------------------------ */
#define GRIT_CONSENSUS_MAX_CANDIDATES 32
long grit_cider_consensus_workspace(int images, int n, int T);
int grit_cider_consensus(const int64_t* tokens, int images, int n, int T, int collapse, const grit_cider_tables* tab, double* sim64,
                         double* score64, float* score32, int32_t* best, int32_t* bad, void* workspace, void* stream);

/* ------------------------------------------------------------------------------------------------------
 * The evaluation's caption scores (reference engine/caption_engine.py:165-190: decode the best beam up to <eos>, collapse repeated
 * words, PTB-tokenise, metrics.compute_scores): per hypothesis row the integers of BLEU-1..4 (bleu_scorer.py cook_test, option
 * 'closest'), ROUGE-L (rouge.py, beta = 1.2) and CIDEr-D (as grit_cider_reward).  METEOR is not computed.  One launch, one workgroup
 * per row, integer and float64 arithmetic in the host's order, no atomics: two launches on the same input are bit-identical.
 *
 * tokens [rows, T] int64, contiguous; slots [rows] int32 = the reference slot of each row; collapse != 0: every word id equal to
 * its predecessor is dropped after the cut at the first <eos> (the evaluation does, the self-critical reward does not; with
 * collapse == 0 the cider output equals grit_cider_reward's out64 bit for bit).
 * comps [rows, GRIT_SCORE_COMPONENTS] int32 = testlen, the reference word count closest to it (a tie goes to the shorter),
 * guess[4] = max(0, testlen - k), correct[4] = sum over the hypothesis' k-grams of min(count, max over references of its count);
 * rouge [rows], cider [rows] float64.  An empty hypothesis is, for ROUGE-L, a sequence of one empty token (it scores 0 against a
 * non-empty reference and 1 against an empty one).  A word id outside [0, vocab) in front of the first <eos>, or a slot outside
 * [0, n_slots): -1 in every component and NaN in rouge and cider of that row.  Limits and `tab` as for grit_cider_reward; `ext` holds
 * what BLEU and ROUGE need per reference, built by grit_amd/ops/caption_scores.py (DeviceCaptionScorer), device memory:
 *   ent_tf [entries] int32          the raw count of the n-gram of tab->ent_tok[e] in its reference
 *   ref_words [n_refs] int32        word count of the tokenised reference
 *   seq_start [n_refs + 1], seq_tok the tokenised reference split at single spaces, CSR (an empty reference is the one token
 *                                   empty_tok)
 *   beta2                           the host's beta ** 2 as a double
 * ------------------------------------------------------------------------------------------------------ */
#define GRIT_SCORE_COMPONENTS 10
typedef struct {
    const int32_t* ent_tf;
    const int32_t* ref_words;
    const int32_t* seq_start;
    const int32_t* seq_tok;
    int empty_tok;
    double beta2;
} grit_score_tables;
int grit_caption_scores(const int64_t* tokens, int rows, int T, const int32_t* slots, int collapse, const grit_cider_tables* tab,
                        const grit_score_tables* ext, int32_t* comps, double* rouge, double* cider, void* stream);

/* ------------------------------------------------------------------------------------------------------
 * Detector set criterion (reference models/detection/od_losses.py: HungarianMatcher :359-431, SetCriterion :68-323): the matching
 * of predictions to targets and the losses of ALL output layers of a step, on the device, with no host round trip.  fp32 tensors
 * (the caller casts the heads' outputs with .float(); there is no bf16 form); duals, path lengths and sums in float64.
 *
 * A "problem" is one (output layer, image) pair, p = layer * B + image, P = L * B.  Targets arrive packed over the batch:
 * tgt_labels [sum T] int64, tgt_boxes [sum T, 4] (cxcywh, normalised), tgt_offsets [B + 1] int32 (device memory, like the rest).
 *
 * grit_det_match_f32: one launch, one wave per problem.  It writes the cost
 *     C[q, t] = w_bbox * |box_q - box_t|_1 + w_class * (pos - neg)(sigmoid(logit[q, label_t])) - w_giou * GIoU(box_q, box_t),
 *     pos = 0.25 (1 - p)^2 (-log(p + 1e-8)),  neg = 0.75 p^2 (-log(1 - p + 1e-8))        (od_losses.py:413-426, box_ops.py:32-69)
 * in fp32, uncontracted, to cost [P, Q, ld] (ld >= Tmax; the caller's workspace, and what a test reads), then solves each problem
 * by shortest augmenting paths over its smaller side (Jonker-Volgenant / Crouse 2016, the algorithm of
 * scipy.optimize.linear_sum_assignment) with float64 duals: the exact optimum of the fp32 matrix as stored, for any T >= 0.  With
 * T > Q, Q pairs are matched and T - Q targets stay unmatched.
 *     match_q [P, Tmax] int32: the query of each target, -1 for an unmatched target and for t >= T
 *     match_t [P, Q]    int32: the target (index within its image) of each query, or -1
 * A label outside [0, K) or a non-finite cost that leaves a row without a finite path leaves the whole problem unmatched (-1).
 * A cost of -inf is outside the contract (scipy refuses it too): what a problem that holds one comes back with is unspecified.
 * BOUND: Q <= GRIT_DET_MAX_SIDE and Tmax <= GRIT_DET_MAX_SIDE (the O(Q + T) solver state of a problem lives in 19 KB of LDS);
 * above it GRIT_ERR_UNSUPPORTED.  An image with more than Tmax targets comes back unmatched.  Tmax >= 1 (pass 1 for an empty batch).
 *
 * grit_lsa_f32: the solver alone on a given cost [P, Q, ld] with counts [P] int32 = T of each problem (device memory); rows [P]
 * int32 = the number of queries of each problem (<= Q; it uses the first rows[p] rows of its slab) or NULL = Q for all; match_t
 * may be NULL.  Same device function, same bound.
 *
 * grit_det_loss_fwd_f32: one launch over logits [L, B, Q, K] and boxes [L, B, Q, 4]; no one-hot target exists anywhere: a row's
 * class is read through match_t and tgt_labels.  out [L, GRIT_DET_LOSS_FIELDS] fp32, per layer:
 *     [0] loss_ce           sum over ALL elements of the sigmoid focal loss (alpha, gamma = 2) / num_boxes
 *                           (= the reference's sigmoid_focal_loss(...) * Q)
 *     [1] loss_bbox         sum of the L1 distance of the matched pairs / num_boxes
 *     [2] loss_giou         sum of 1 - GIoU of the matched pairs / num_boxes
 *     [3] cardinality_error mean over images of | #{q: argmax_k logit != K - 1} - T |
 *     [4] class_error       100 - 100 * (matched rows whose argmax is their label) / (matched rows); 100 with none
 *     [5..]                 0
 * num_boxes: ONE float in device memory, already all-reduced and clamped to >= 1 by the caller.  partials: [L * B * chunks, 8]
 * float64 workspace, chunks = ceil(Q / GRIT_DET_LOSS_ROWS); ticket: one uint32 of workspace that belongs to this call alone, like
 * partials (the entry point zeroes it on `stream` in front of the launch; the workgroup that takes the last ticket finalises).
 *
 * grit_det_loss_bwd_f32: one launch; writes EVERY element of dlogits [L, B, Q, K] and dboxes [L, B, Q, 4] (zero rows for unmatched
 * queries).  coef [L, ldc] fp32 (ldc >= 3): the upstream gradients of out[l][0..2], i.e. the weights of the weighted loss sum;
 * sigmoid is recomputed from the logits, nothing logits-sized is saved by the forward.
 * ------------------------------------------------------------------------------------------------------ */
#define GRIT_DET_MAX_SIDE 512
#define GRIT_DET_LOSS_ROWS 20
#define GRIT_DET_LOSS_FIELDS 8
int grit_det_match_f32(const float* logits, const float* boxes, const int64_t* tgt_labels, const float* tgt_boxes,
                       const int32_t* tgt_offsets, int L, int B, int Q, int K, int Tmax, float w_class, float w_bbox, float w_giou,
                       float* cost, int ld, int32_t* match_q, int32_t* match_t, void* stream);
int grit_lsa_f32(const float* cost, const int32_t* counts, const int32_t* rows, int P, int Q, int ld, int Tmax, int32_t* match_q,
                 int32_t* match_t, void* stream);
int grit_det_loss_fwd_f32(const float* logits, const float* boxes, const int64_t* tgt_labels, const float* tgt_boxes,
                          const int32_t* tgt_offsets, const int32_t* match_t, int L, int B, int Q, int K, float alpha,
                          const float* num_boxes, double* partials, unsigned int* ticket, float* out, void* stream);
int grit_det_loss_bwd_f32(const float* logits, const float* boxes, const int64_t* tgt_labels, const float* tgt_boxes,
                          const int32_t* tgt_offsets, const int32_t* match_t, int L, int B, int Q, int K, float alpha,
                          const float* num_boxes, const float* coef, int ldc, float* dlogits, float* dboxes, void* stream);

/* ------------------------------------------------------------------------------------------------------
 * Detector attribute head (reference models/detection/heads.py AttrHead :33-51, od_losses.py weighted_attr_loss :141-177).
 *
 * grit_attr_embed_cat: the head's front in one launch, one wave per row.  obj_h [rows, d], embed [K, d] and out [rows, 2 d] share
 * one dtype (bf16 != 0: bf16, else fp32); logits [rows, K] are fp32, or bf16 with logits_bf16 != 0 (widened to fp32 first).
 *     labels[r] int32 = the FIRST index of the maximum of 1 / (1 + expf(-logit)) evaluated in fp32 -- the reference's
 *                       argmax(sigmoid(.)), which saturates at 1.0f from a logit of about 16.7: NOT the argmax of the logits
 *     out[r] = [ obj_h[r] | embed[labels[r]] ], copied bit for bit (16 bytes per lane where d * element size and the three base
 *              addresses are multiples of 16, else element by element)
 * NaN logits are outside the contract (the label is then some index in [0, K)).  BOUND: rows * K, rows * 2 d and K * d < 9e15.
 *
 * grit_attr_embed_grad: dweight [K, d] = for every class the sum, in row order, of dcat[r, col0 .. col0 + d) over the rows with
 * labels[r] == k; dcat [rows, ld] (col0 + d <= ld) and dweight share one dtype (bf16 flag as above), the sum is fp32.  One wave
 * per (class, 64 columns); no atomics, two calls give identical bytes; a class nobody chose gets zeros, a label outside [0, K)
 * contributes nowhere.  BOUND: d <= 65535 * 64 (above it GRIT_ERR_UNSUPPORTED), rows * ld and K * d < 9e15.
 *
 * grit_det_attr_fwd_f32: attr_logits [B, Q, A] fp32, attributes [sum T + 1, A] uint8 (0 / 1, rows aligned with tgt_labels),
 * tgt_offsets [B + 1] int32, has_attr [B] uint8, match_t [B, Q] int32 (the LAST layer's slab of grit_det_match_f32).  Over the rows
 * (b, q) with has_attr[b] != 0 and 0 <= t = match_t[b, q] < T_b, x = attr_logits[b, q], y = attributes[offset_b + t]:
 *     bce = max(x, 0) - x y + log1p(exp(-|x|))                                    (fp32 per element, sums in float64)
 *     loss[0] = sum(bce y) / N1 + sum(bce (1 - y)) / N0,  N1 = sum(y), N0 = sum(1 - y) (integers); a term with a zero count is 0
 * totals [2] int64 = (N1, N0), which the backward reads.  partials [B * chunks, 2] float64 and counts [B * chunks, 2] int64 are
 * workspace, chunks = ceil(Q / GRIT_DET_LOSS_ROWS); ticket as for grit_det_loss_fwd_f32.  The counts are this rank's.
 *
 * grit_det_attr_bwd_f32: one launch; writes EVERY element of dlogits [B, Q, A]:
 *     (sigmoid(x) - y) (y / N1 + (1 - y) / N0) upstream[0] on the rows above, 0 elsewhere; upstream: ONE float in device memory.
 * BOUND (both): B * Q * A < 9e15 and B * chunks < 2^31, else GRIT_ERR_BAD_ARG.
 * ------------------------------------------------------------------------------------------------------ */
int grit_attr_embed_cat(const void* obj_h, const void* logits, const void* embed, void* out, int32_t* labels, int rows, int K, int d,
                        int bf16, int logits_bf16, void* stream);
int grit_attr_embed_grad(const void* dcat, const int32_t* labels, void* dweight, int rows, int K, int d, int ld, int col0, int bf16,
                         void* stream);
int grit_det_attr_fwd_f32(const float* attr_logits, const uint8_t* attributes, const int32_t* tgt_offsets, const uint8_t* has_attr,
                          const int32_t* match_t, int B, int Q, int A, double* partials, int64_t* counts, unsigned int* ticket,
                          float* loss, int64_t* totals, void* stream);
int grit_det_attr_bwd_f32(const float* attr_logits, const uint8_t* attributes, const int32_t* tgt_offsets, const uint8_t* has_attr,
                          const int32_t* match_t, int B, int Q, int A, const int64_t* totals, const float* upstream, float* dlogits,
                          void* stream);

/* ------------------------------------------------------------------------------------------------------
 * Detector evaluation (reference models/detection/od_losses.py PostProcess :326-356; datasets/detection/metrics/cocoeval.py
 * computeIoU :172-199 and evaluateImg :252-334 for iouType 'bbox', useCats 1).  The device selects an image's best detections and
 * matches them to its ground truth; packing, accumulation and summary are the host's (grit_amd/ops/det_eval.py,
 * grit_amd/datasets/detection/metrics/coco_eval.py).
 *
 * grit_det_topk_f32: logits [B, Q, K], boxes [B, Q, 4] (cxcywh in [0, 1]), sizes [B, 2] (height, width), all fp32.  With
 * n = Q * K and N = min(GRIT_DET_TOPK, n) it writes, per image, the N largest logits in the order logit descending, then flat index
 * q * K + k ascending -- a function of the data alone:
 *     top_logit [B, N] fp32, top_index [B, N] int32, out_boxes [B, N, 4] fp32 = the query's box as absolute corners,
 *     ((cx - 0.5 w) * width, (cy - 0.5 h) * height, (cx + 0.5 w) * width, (cy + 0.5 h) * height) in fp32, uncontracted.
 * The sigmoid is never evaluated (it is monotonic; the caller applies it to the N selected logits).  Two launches: an image's map is
 * split over chunks = min(GRIT_DET_TOPK_CHUNKS, ceil(n / 8192)) workgroups, chunk c = the flat indices [c * len, (c + 1) * len) with
 * len = ceil(n / chunks); each keeps its chunk's N best (radix select on the order-preserving integer image of the float), one
 * workgroup per image sorts the chunks' candidates.  work: B * GRIT_DET_TOPK_CHUNKS * GRIT_DET_TOPK uint64 of workspace that belongs
 * to this call.  NaN logits are outside the contract (they are ordered by their bit pattern).  n >= 2^31 or B > 65535: GRIT_ERR_BAD_ARG.
 *
 * grit_det_eval_img: one workgroup per image.  scores [B, N] fp32, labels [B, N] int64, boxes [B, N, 4] fp32 absolute corners, an
 * image's rows in score order (the order grit_det_topk_f32 gives); N <= GRIT_DET_TOPK.  slot [B] int32: the image's position in the
 * split's packed ground truth `gt` (an image with a slot outside [0, gt->n_img) is left out):
 *     img_off [n_img + 1] int32; per annotation box [4] float64 (x, y, w, h), area float64, cat int32, crowd uint8; the annotations
 *     of an image sorted by category, in annotation order within a category; cat_valid [n_cat] uint8; max_per_img: the largest
 *     annotation count of an image, > GRIT_DET_MAX_SIDE gives GRIT_ERR_UNSUPPORTED.
 * iou_thr [T] and area_rng [A, 2] float64 are the host's numbers (numpy.linspace), T <= 16, A <= 4.  All arithmetic in float64,
 * uncontracted: a detection is (x1, y1, fp32(x2 - x1), fp32(y2 - y1)) widened, its area w * h, a ground truth's area its `area`
 * field; IoU of D and G: w = min(D2 + D0, G2 + G0) - max(D0, G0), 0 if w <= 0, h likewise, i = w h,
 * u = crowd ? D2 D3 : D2 D3 + G2 G3 - i, iou = i / u.  Per area range a ground truth is ignored if crowd or its area is outside
 * (< and >), ignored ones last, stably; the detections of a category, in order, take the best free ground truth with
 * iou >= min(t, 1 - 1e-10) by the rules of cocoeval.py:296-309; an unmatched detection with its own area outside is ignored.
 * Records at row slot * N + n of buffers over the split (rec_rank filled with -1 by the caller before the first call):
 *     rec_flags [n_img * N, A] uint32   bit t: matched at threshold t; bit 16 + t: ignored at threshold t
 *     rec_rank  [n_img * N] int32       rank among the image's detections of its category; -1: label outside [0, n_cat) or with
 *                                       cat_valid 0 (the detection does not take part)
 *     rec_score [n_img * N] fp32, rec_label [n_img * N] int32, seen [n_img] uint8 = 1
 * No atomics on global memory, no order dependence: two calls give identical bytes.
 *
 * grit_det_voc_img: the per-image matching of the Visual Genome protocol (reference datasets/detection/metrics/vg_eval.py:59-96:
 * PASCAL-VOC matching at ONE overlap threshold, no difficult flags), one workgroup per image, the calling shape of
 * grit_det_eval_img: scores, labels, boxes, slot, B, N <= GRIT_DET_TOPK and `gt` as above (area and crowd are not read and may be
 * null; max_per_img > GRIT_DET_MAX_SIDE gives GRIT_ERR_UNSUPPORTED).  The same launch serves objects and attributes: for attributes
 * the packer has written one row (class = attribute, box) per attribute an object carries.  For a detection with label c, over the
 * image's rows of class c in packed order, all in float64, uncontracted, with the protocol's +1 pixel convention: bb = the fp32
 * corners widened, g = (x, y, x + w, y + h) of the row's box,
 *     iw = max(min(g2, bb2) - max(g0, bb0) + 1, 0), ih likewise, inters = iw ih,
 *     uni = (bb2 - bb0 + 1)(bb3 - bb1 + 1) + (g2 - g0 + 1)(g3 - g1 + 1) - inters, ov = inters / uni;
 * ovmax = the largest ov, jmax = the FIRST row that has it (a row replaces the held one only when its ov is greater, so a NaN
 * overlap is never held); no rows: ovmax = -inf, jmax = -1.  The detection is a true positive iff ovmax > iou_thr (strictly) and no
 * earlier detection of the image with the same label has the same jmax with ovmax > iou_thr; a later one with the same jmax is a
 * duplicate.  That is a first-occurrence test over <= 100 detections: no loop that carries state from detection to detection.
 * Records at row slot * N + n of buffers over the split:
 *     rec_flag  [n_img * N] uint8       0: takes no part (label outside [0, n_cat) or cat_valid 0); 1: true positive;
 *                                       2: false positive, no overlap (ovmax <= iou_thr); 3: false positive, duplicate
 *     rec_gt    [n_img * N] int32       jmax as the row's index within the image, or -1
 *     rec_iou   [n_img * N] float64     ovmax (-inf with rec_gt -1)
 *     rec_score [n_img * N] fp32, rec_label [n_img * N] int32, seen [n_img] uint8 = 1
 * iou_thr must not be NaN (GRIT_ERR_BAD_ARG).  No atomics, plain stores only: two calls give identical bytes.
 * ------------------------------------------------------------------------------------------------------ */
#define GRIT_DET_TOPK 100
#define GRIT_DET_TOPK_CHUNKS 40
typedef struct {
    const int32_t* img_off;
    const double* box;
    const double* area;
    const int32_t* cat;
    const uint8_t* crowd;
    const uint8_t* cat_valid;
    int n_img, n_cat, max_per_img;
} grit_det_gt;
int grit_det_topk_f32(const float* logits, const float* boxes, const float* sizes, int B, int Q, int K, uint64_t* work,
                      float* top_logit, int32_t* top_index, float* out_boxes, void* stream);
int grit_det_eval_img(const float* scores, const int64_t* labels, const float* boxes, const int32_t* slot, int B, int N,
                      const grit_det_gt* gt, const double* iou_thr, int T, const double* area_rng, int A, uint32_t* rec_flags,
                      int32_t* rec_rank, float* rec_score, int32_t* rec_label, uint8_t* seen, void* stream);
int grit_det_voc_img(const float* scores, const int64_t* labels, const float* boxes, const int32_t* slot, int B, int N,
                     const grit_det_gt* gt, double iou_thr, uint8_t* rec_flag, int32_t* rec_gt, double* rec_iou, float* rec_score,
                     int32_t* rec_label, uint8_t* seen, void* stream);

/* ------------------------------------------------------------------------------------------------------
 * JPEG decoding (DESIGN "JPEG decoding"): baseline files -> the [h, w, 3] uint8 RGB pixels of libjpeg-turbo's defaults (JDCT_ISLOW,
 * fancy upsampling; what PIL's Image.open(path).convert('RGB') returns), bit for bit.  The serial entropy stage is host code, the
 * rest two launches for a batch.
 *
 * grit_jpeg_probe (host code, no GPU work): reads the markers up to the scan and fills `info`.  GRIT_ERR_UNSUPPORTED for everything
 * outside the accepted subset -- anything but SOF0 with 8-bit samples, 8-bit quantisation tables and ONE interleaved scan of
 * 1 component (its factors count as 1x1) or of 3 components with luma 1x1, 2x1 or 2x2 over 1x1 chroma that libjpeg takes for YCbCr (JFIF marker; else
 * Adobe transform 1; else component ids other than 'R','G','B'); DNL; any malformed header -- the caller then decodes on the host.
 *   info    width, height, ncomp (1: grey, 3: YCbCr); hs / vs sampling factors per component, hmax / vmax = the luma's;
 *           mcu_cols, mcu_rows; block_cols / block_rows per component = mcu_cols * hs, mcu_rows * vs (padded to whole MCUs);
 *           restart_interval in MCUs (0: none); scan_offset = byte offset of the first entropy-coded byte;
 *           coef_bytes = 128 bytes per block, plane_bytes = 64 bytes per block over all components;
 *           quant [component][64]: the component's quantisation table in natural (row-major) order
 * grit_jpeg_entropy (host code): the Huffman decode of the scan into coef (coef_bytes >= info->coef_bytes): per component one
 *   plane [block_rows][block_cols][64] int16, de-zigzagged, not dequantised, the planes back to back.  info: the probe's record of
 *   the same bytes (GRIT_ERR_BAD_ARG if it is not) or NULL.  GRIT_ERR_UNSUPPORTED -- decode on the host -- for a bad Huffman table,
 *   a code that does not exist, a run past the block, a wrong or missing restart marker, data that ends early or does not end in EOI,
 *   a quantisation entry of 0 or more than GRIT_JPEG_MAX_PIXELS pixels (PIL's MAX_IMAGE_PIXELS: its own guard then decides; probe),
 *   and any coefficient with |coefficient * quant| > GRIT_JPEG_COEF_BOUND (no encoder makes one from 8-bit samples; the bound keeps
 *   the first IDCT pass inside 32 bits).  Both functions are re-entrant, allocate nothing and never read past data + nbytes.
 *
 * grit_jpeg_reconstruct (two launches, no atomics): jobs [n_images] grit_jpeg_job (device memory), every offset relative to the
 * base pointer of its buffer:
 *     coef_off   int16 ELEMENT offset of each component's coefficient plane in coef (a multiple of 8: rows load as 16 bytes)
 *     plane_off  byte offset (a multiple of 8) of each component's sample plane in planes: block_rows * 8 rows of block_cols * 8
 *     out_off    byte offset of the image's [height, width, 3] pixels in out (any; 4-byte aligned offsets store whole dwords)
 *     width, height, ncomp, hmax, vmax, block_cols, block_rows, quant: as in grit_jpeg_info
 *   PRECONDITION: every |coefficient * quant| <= GRIT_JPEG_COEF_BOUND, as grit_jpeg_entropy guarantees; the first IDCT pass works
 *   in int32 and larger products overflow it (undefined values, no fault).  An image with ncomp = 0 (or no pixels) is skipped.
 *   launch 1: dequantise, jidctint.c's jpeg_idct_islow, range limit: every block of every component -> planes
 *   launch 2: per pixel Y, jdsample.c's fancy h2v1 / h2v2 chroma upsampling (replication when the chroma plane is <= 2 wide),
 *             jdcolor.c's YCbCr -> RGB; grey images copy Y to the three channels
 *   coef, planes 16-byte aligned; out 4-byte aligned.  max_blocks = the largest block_cols * block_rows of a component, max_pixels
 *   = the largest width * height; n_images * 3 <= 65535.
 * ------------------------------------------------------------------------------------------------------ */
#define GRIT_JPEG_COEF_BOUND 8191
#define GRIT_JPEG_MAX_PIXELS 89478485
typedef struct {
    int width, height, ncomp, hmax, vmax;
    int hs[3], vs[3];
    int mcu_cols, mcu_rows;
    int block_cols[3], block_rows[3];
    int restart_interval;
    long scan_offset, coef_bytes, plane_bytes;
    int quant[192];
} grit_jpeg_info;
typedef struct {
    long coef_off[3], plane_off[3], out_off;
    int width, height, ncomp, hmax, vmax;
    int block_cols[3], block_rows[3];
    int quant[192];
} grit_jpeg_job;
int grit_jpeg_probe(const uint8_t* data, long nbytes, grit_jpeg_info* info);
int grit_jpeg_entropy(const uint8_t* data, long nbytes, const grit_jpeg_info* info, void* coef, long coef_bytes);
long grit_jpeg_planes_bytes(const grit_jpeg_info* info);
int grit_jpeg_reconstruct(const grit_jpeg_job* jobs, int n_images, int max_blocks, long max_pixels, const void* coef, uint8_t* planes,
                          uint8_t* out, void* stream);

/* ------------------------------------------------------------------------------------------------------
 * Caption likelihood head (DESIGN "Caption likelihood scoring"): the vocabulary projection, log-softmax and the gather of one
 * target column per row, without the [R, V] logit map.
 *   <- CaptionGenerator.forward's `fc` + F.log_softmax, models/caption/cap_generator.py:157-167, followed by the caller's gather.
 *
 * grit_vocab_score_bf16: x [R, D] bf16 (row stride ldx elements), w [V, D] bf16 (row stride ldw), target [R] int64:
 *     logit[v] = sum_k x[r, k] w[v, k]      bf16 products, fp32 accumulation on v_mfma_f32_16x16x32_bf16
 *     lse[r]   = log sum_v exp(logit[v])    fp32, max-subtracted
 *     logp[r]  = logit[target[r]] - lse[r]
 *   logp [R], lse [R] fp32.  target[r] == pad_idx: logp = +0.0 (lse is still written).  target[r] outside [0, V) and not pad_idx:
 *   logp = NaN, nothing is read out of bounds (the host never looks at the targets).  Columns past V take no part.
 *   Two launches, no atomics, nothing passes between the workgroups of a launch: (1) grid (ceil(R / 64), slices): a workgroup keeps
 *   its x tile in LDS, streams its slice of w and writes the row's running (max, sum of exp) to work[slice][row]; the one lane that
 *   holds column target[r] stores that logit; (2) one thread per row merges the pairs in slice order.  The slice width
 *   (grit_vocab_score_slice) is a function of V and D only, so a row's bits do not depend on the other rows of the call:
 *   f(x[idx]) == f(x)[idx], and two calls give identical bytes.
 *   work: grit_vocab_score_workspace(R, V, D) bytes that belong to this call, 4-byte aligned, need no initialisation.
 *   Limits (GRIT_ERR_UNSUPPORTED beyond them: the caller takes the composed form): D % 64 == 0, 64 <= D <= 512; ldx, ldw >= D and
 *   multiples of 8; x and w 16-byte aligned; ceil(V / slice) <= 65535; R <= 2^31 - 65 (row indices are 32-bit; every offset into a
 *   buffer is 64-bit).  Null pointers, R < 1, V < 1, D < 1: GRIT_ERR_BAD_ARG.  fp32 operands: not built.
 * grit_vocab_score_slice: the slice width in columns (a multiple of 128), 0 for a (V, D) outside the limits.
 * grit_vocab_score_workspace: (2 * ceil(V / slice) + 1) * R * 4 bytes, 0 outside the limits.
 * ------------------------------------------------------------------------------------------------------ */
int grit_vocab_score_slice(int V, int D);
long grit_vocab_score_workspace(int R, int V, int D);
int grit_vocab_score_bf16(const void* x, long ldx, const void* w, long ldw, const int64_t* target, long pad_idx, int R, int V, int D,
                          void* work, float* logp, float* lse, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GRIT_HIP_H */
