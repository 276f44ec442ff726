/*
 * hybridgl.h -- C ABI of libhybridgl.so, the MI355X (gfx950) hot path of the
 * HybridGL zero-shot referring-segmentation pipeline.
 *
 * Every entry point replaces a Python call surface of the reference
 * (cited as file:line relative to the reference tree).  Conventions:
 *   - all pointers are DEVICE pointers (HBM) unless the name says host_;
 *   - all tensors are dense row-major fp32 unless stated;
 *   - every call is asynchronous on `stream` (a hipStream_t passed as void*,
 *     NULL = the default stream); no hidden allocation: scratch memory is a
 *     caller-provided workspace whose size comes from *_workspace_bytes();
 *   - return 0 on success, negative HGL_E* otherwise; hgl_last_error() gives
 *     a thread-local human-readable message;
 *   - no torch types, no C++ types, no exceptions cross this boundary.
 *
 * There is NO CPU implementation behind this ABI: without a HIP device every
 * compute entry point returns HGL_ENODEVICE.
 */
#ifndef HYBRIDGL_H
#define HYBRIDGL_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HGL_OK 0
#define HGL_EINVAL (-1)    /* bad argument (shape, alignment, null) */
#define HGL_ENODEVICE (-2) /* no HIP device / device error */
#define HGL_EWORKSPACE (-3)/* workspace too small */
#define HGL_ELAUNCH (-4)   /* kernel launch failed */

/* 2: + hgl_clip_hybrid_forward_segments, hgl_split_overflow_count, hgl_clip_encode_text_ex; hgl_gemm_f16x3_select
 * knows kinds -1, 0, 1 only
 * 5: + hgl_u8_to_chw_lut, hgl_split_overflow_peek_async, hgl_resize_bilinear, hgl_score_ref
 * 6: + hgl_attention_presplit, hgl_attention_presplit_f32, hgl_score_group, hgl_remove_small_regions_boxes
 * 7: + hgl_sam_decode_points_gated */
#define HGL_ABI_VERSION 7

/* activation codes for hgl_gemm_f32 */
#define HGL_ACT_NONE 0
#define HGL_ACT_QUICKGELU 1 /* x*sigmoid(1.702x): clip/model.py:198-200 */
#define HGL_ACT_GELU 2      /* erf GELU: nn.GELU, segment_anything/modeling/image_encoder.py:65 */
#define HGL_ACT_RELU 3      /* transformer.py MLPBlock act=ReLU, mask_decoder.py MLP */

/* fusion modes of CLIPViTFM.forward (model/backbone.py:117-309) */
#define HGL_FUSION_G2L 0      /* model/backbone.py:227-260 */
#define HGL_FUSION_L2G 1      /* model/backbone.py:206-225 */
#define HGL_FUSION_G2L_L2G 2  /* model/backbone.py:262-306 */
#define HGL_FUSION_TOKEN_MASKING 3 /* model/backbone.py:161-184 */
#define HGL_FUSION_ATTN_MASKING 4  /* model/backbone.py:186-204 */
#define HGL_FUSION_CROP 5          /* model/backbone.py:126-128 */

/* attention mask kinds for hgl_attention_f32 */
#define HGL_MASK_NONE 0
#define HGL_MASK_CAUSAL 1  /* clip/model.py:396-402 build_attention_mask */
#define HGL_MASK_CLS_KEEP 2/* model/backbone.py:108-115 make_attn_mask: only the CLS query row is restricted */

int hgl_abi_version(void);
const char* hgl_last_error(void);
/* number of visible HIP devices (0 when none); never initialises a context */
int hgl_device_count(void);

/* Per-kernel-class timing with HIP events on the launch stream (bench.py roofline leg).
 * cls: 0 = fp32 MFMA GEMM, 1 = fused attention, 2 = other, 3 = split-fp16 (f16x3) GEMM, register-staged kernel
 * (gemm_f16x3_kernel), 4 = f16x3 GEMM, LDS-DMA ping-pong kernel (gemm_x3p_kernel), 5 = launches of either f16x3 kernel with
 * fewer than 256 output tiles (latency-bound side-stream work: GEM at 785 rows, text encoder).  hgl_prof_read synchronises,
 * returns and clears the records of one class: launches, summed event ms, and the summed
 * ALGORITHMIC flops / bytes of those launches (2*M*N*K per GEMM; 4*B*H*Sq*Sk*hd per attention). */
int hgl_prof_enable(int on);
int hgl_prof_read(int cls, long long* launches, double* ms, double* flops, double* bytes);

/* GEMM precision mode of the encoders.  HGL_PREC_F32: v_mfma_f32_32x32x2_f32 (exact fp32 products).
 * HGL_PREC_F16X3: every fp32 operand split into fp16 hi+lo, three v_mfma_f32_16x16x32_f16 per
 * step into one fp32 accumulator (a_hi*b_hi + a_hi*b_lo + a_lo*b_hi; ~2^-22 relative error per
 * term, i.e. fp32-class accuracy at 16/3 of the fp32 matrix rate).  It applies to GEMMs whose
 * weight has been registered with hgl_register_split_weight; all others stay on the fp32 path.
 * HGL_PREC_F16 (opt-in): the same GEMMs with fp16 operands -- the activation rounded to fp16, the
 * registered weight's (power-of-two scaled) hi half -- ONE v_mfma_f32_16x16x32_f16 per step, fp32
 * accumulation; no lo plane is written or read.  About 2^-11 relative error per operand: NOT the
 * fp32 parity of the other two modes.  The attention kernels of the encoders and the SAM mask
 * decoder keep their f16x3 arithmetic in this mode; the fp16 range guard below applies unchanged. */
#define HGL_PREC_F32 0
#define HGL_PREC_F16X3 1
#define HGL_PREC_F16 2
int hgl_set_precision(int mode);
int hgl_get_precision(void);
/* Pins the tiling of the f16x3 GEMM: -1 = cost model (default), 0 = register-staged 128x128 (two workgroups per
 * CU), 1 = LDS-DMA 256x256 ping-pong (persistent).  Both tilings give bit-identical results; the switch exists for
 * the parity tests and micro-benchmarks. */
int hgl_gemm_f16x3_select(int kind);
/* f16x3 (and f16) mode splits every fp32 operand into fp16 hi + lo; an activation beyond the fp16 range (|x| > 65504) cannot be
 * split (inf - inf).  The kernels that split GEMM outputs track the largest |x| they meet; *count = GPU threads that met
 * such a value since the last reset (a blocking device read: synchronise the producing streams first).  Non-zero means
 * the results of that run contain inf / NaN: rerun with hgl_set_precision(HGL_PREC_F32). */
int hgl_split_overflow_count(int reset, unsigned long long* count);
/* The same counters copied in STREAM ORDER to host2[0..1] (pinned host memory; GEMM kernels, attention kernels) without
 * waiting and without a reset: the values are what the device had counted when `stream` reached this call.  A caller
 * that reads something back per batch anyway (the evaluator's proposal counts, Hybridgl_main.py:85-87) rides this on the
 * same event and stops at the offending batch instead of voiding the run at its end. */
int hgl_split_overflow_peek_async(unsigned int* host2, void* stream);
/* ALL the counters hgl_split_overflow_count sums, copied in STREAM ORDER to host3[0..2] (pinned host memory; GEMM kernels,
 * attention kernels, the SAM decoder's image -> token preparation) without waiting and without a reset: host3[0] + host3[1] +
 * host3[2] is what hgl_split_overflow_count(0, ..) would have returned had the device stopped when `stream` reached this call.
 * (hgl_split_overflow_peek_async does not see the decoder's counter.)  For a caller that compares totals between two points
 * of a stream and redoes the work in between in HGL_PREC_F32 when they differ (HybridGLPipeline(on_overflow="rescue")).
 * HGL_EINVAL for a null pointer; HGL_ELAUNCH when a copy could not be enqueued. */
int hgl_split_overflow_snapshot_async(unsigned int* host3, void* stream);
/* Splits w_fp32 [N,K] * 2^scale_log2 into caller-owned fp16 arrays hi, lo ([N,K] each) and
 * records them under the fp32 pointer (scale_log2 keeps the lo half in the fp16 normal range;
 * choose max|w| * 2^scale_log2 <= 2^14). */
int hgl_register_split_weight(const float* w_fp32, int N, int K, int scale_log2, void* hi, void* lo, void* stream);
int hgl_unregister_split_weight(const float* w_fp32);
/* 1: every lo half of the registered split is zero -- the weight is fp16-valued, as the tensors of OpenAI's CLIP archives are
 * (clip/model.py:509 is commented out in the reference: they are held as fp32 with fp16 values) -- and the GEMMs on it issue two
 * MFMAs per product step instead of three (the A_hi * W_lo products would add exact zeros: same results bit for bit;
 * HGL_X3_TERMS=3 keeps them).  0: a genuine fp32 weight.  -1: not registered. */
int hgl_split_weight_is_fp16_valued(const float* w_fp32);
/* hgl_gemm_f32 semantics (no batch, dense leading dims) through the split path; A is split into
 * `scratch` (>= M*K*4 bytes) first.  W must be registered.  A scratch LARGER than align256(M*K*4) + 256 bytes selects the
 * row-balanced launch the model code uses for its residual GEMMs (whole rounds of the persistent tiling + a split-K tail over
 * the rows of a mostly empty last round, partial sums in the extra scratch: up to 4 * 256 * ceil(256 CUs / tiles_n) * N * 4
 * bytes are used); rows of the tail then equal the plain launch to fp32 rounding, all others bit for bit. */
int hgl_gemm_f16x3(const float* A, const float* W, const float* bias, const float* R, float* C,
                   int M, int N, int K, int act, void* scratch, size_t scratch_bytes, void* stream);

/* ------------------------------------------------------------------------
 * Primitive operators (building blocks; exported so that parity tests can
 * pin each kernel against the oracle in isolation).
 * --------------------------------------------------------------------- */

/* C[b] = act(A[b] @ W[b]^T + bias) + R[b]      (torch.nn.functional.linear)
 * A:[M,K] lda, W:[N,K] ldw, C:[M,N] ldc, R:[M,N] ldr (may be NULL, may alias C),
 * bias:[N] or NULL.  batch>=1 with element strides sA/sW/sR/sC (0 = shared).
 * K%4==0, lda%4==0, ldw%4==0, pointers 16-byte aligned.  fp32 MFMA
 * (v_mfma_f32_32x32x2_f32), exact fp32 products and accumulation. */
int hgl_gemm_f32(const float* A, const float* W, const float* bias, const float* R, float* C,
                 int M, int N, int K, int lda, int ldw, int ldr, int ldc,
                 int batch, long long sA, long long sW, long long sR, long long sC,
                 int act, void* stream);

/* y = (x-mean)/sqrt(var+eps)*w+b over the last dim D for `rows` rows
 * (clip/model.py:189-195 LayerNorm; eps=1e-5 for CLIP, 1e-6 for SAM). */
int hgl_layernorm_f32(const float* x, const float* w, const float* b, float* y,
                      int rows, int D, float eps, void* stream);

/* Fused softmax(scale*Q K^T + mask + bias) V for B sequences x H heads.
 * q,k,v: row (b*S+s), column (h*hd + d), leading dims ldq/ldk/ldv (so a packed
 * [B*S,3*D] in_proj output works with pointer offsets).  out: [B*Sq, H*hd] ldo.
 * hd in {16,32,64,80}.  mask_kind: HGL_MASK_*; keep: [keep_n,Sk-1] uint8 for
 * HGL_MASK_CLS_KEEP applied to batches b >= keep_b0 (keep row (b-keep_b0)%keep_n;
 * keep_n<=0 means B).
 * rel_h/rel_w (may be NULL): decomposed relative position bias tables
 * [B*H, Sq, kh] and [B*H, Sq, kw] with Sk = kh*kw
 * (segment_anything/modeling/image_encoder.py:325-361). */
int hgl_attention_f32(const float* q, const float* k, const float* v, float* out,
                      int B, int H, int Sq, int Sk, int hd,
                      int ldq, int ldk, int ldv, int ldo,
                      long long sqb, long long skb, long long svb, long long sob,
                      float scale, int mask_kind, const uint8_t* keep, int keep_b0, int keep_n,
                      const float* rel_h, const float* rel_w, int kh, int kw,
                      void* stream);

/* ------------------------------------------------------------------------
 * CLIP hybrid encoder  (model/backbone.py CLIPViTFM, clip/model.py)
 * --------------------------------------------------------------------- */

typedef struct HglResBlockW {          /* clip/model.py:203-257 ResidualAttentionBlock */
  const float *ln1_w, *ln1_b;          /* [D] */
  const float *in_proj_w, *in_proj_b;  /* [3D,D], [3D]  (nn.MultiheadAttention) */
  const float *out_proj_w, *out_proj_b;/* [D,D], [D] */
  const float *ln2_w, *ln2_b;          /* [D] */
  const float *fc_w, *fc_b;            /* mlp.c_fc   [4D,D],[4D] */
  const float *proj_w, *proj_b;        /* mlp.c_proj [D,4D],[D] */
} HglResBlockW;

typedef struct HglClipVisionW {        /* clip/model.py:272-305 VisionTransformer */
  int width, layers, heads, patch, grid, embed; /* ViT-B/16: 768,12,12,16,14,512 */
  const float* conv1_w;                /* [width, 3*patch*patch] (conv weight flattened c,ky,kx) */
  const float* class_embedding;        /* [width] */
  const float* positional_embedding;   /* [grid*grid+1, width] */
  const float *ln_pre_w, *ln_pre_b;
  const HglResBlockW* blocks;          /* host array of `layers` structs (device pointers inside) */
  const float *ln_post_w, *ln_post_b;
  const float* proj_t;                 /* visual.proj transposed: [embed, width] */
} HglClipVisionW;

typedef struct HglClipTextW {          /* clip/model.py:340-431 */
  int width, layers, heads, context, vocab, embed; /* 512,12,8,77,49408,512 */
  const float* token_embedding;        /* [vocab, width] */
  const float* positional_embedding;   /* [context, width] */
  const HglResBlockW* blocks;
  const float *ln_final_w, *ln_final_b;
  const float* text_projection_t;      /* text_projection transposed: [embed, width] */
} HglClipTextW;

/* CLIPViTFM.forward(local_imgs, global_imgs, pred_masks, masking_block, fusion_mode)
 * (model/backbone.py:117).  local,global: [N,3,res,res] NCHW fp32 (res=patch*grid);
 * masks: [N,Hm,Wm] uint8 (0/1, torch.bool storage); out: [N,embed].
 * last_layer is CLIPViTFM.last_layer (10 for ViT-B/16, model/backbone.py:16-21);
 * masking_block<0 means "use last_layer" (model/backbone.py:118-119). */
size_t hgl_clip_hybrid_workspace_bytes(const HglClipVisionW* w, int N, int Hm, int Wm, int fusion_mode);
int hgl_clip_hybrid_forward(const HglClipVisionW* w, const float* local_imgs, const float* global_imgs,
                            const uint8_t* masks, int N, int Hm, int Wm,
                            int fusion_mode, int masking_block, int last_layer,
                            float* out, void* workspace, size_t workspace_bytes, void* stream);
/* The same over the proposals of SEVERAL images in one call (a group of dataset items, Hybridgl_main.py:79-128 taken
 * several at a time): rows of local/global are the masks of image 0, then image 1, ...; run s = seg_n[s] masks of
 * seg_h[s] x seg_w[s] pixels at the device pointer seg_masks[s] (the three arrays and the pointer array are HOST
 * memory); sum(seg_n) == N.  Every row is independent, so out equals the per-image calls stacked.  Workspace: the
 * size query above with the total N. */
int hgl_clip_hybrid_forward_segments(const HglClipVisionW* w, const float* local_imgs, const float* global_imgs,
                                     const uint8_t* const* seg_masks, const int* seg_n, const int* seg_h, const int* seg_w,
                                     int n_seg, int N, int fusion_mode, int masking_block, int last_layer,
                                     float* out, void* workspace, size_t workspace_bytes, void* stream);

/* CLIP.encode_text(text) (clip/model.py:414-431): tokens [B,context] int32
 * -> out [B,embed]; pooled at argmax(token id) (the EOT token). */
size_t hgl_clip_text_workspace_bytes(const HglClipTextW* w, int B);
int hgl_clip_encode_text(const HglClipTextW* w, const int32_t* tokens, int B, float* out,
                         void* workspace, size_t workspace_bytes, void* stream);
/* The same on the first seq_len <= context positions only: exact under the causal mask as long as every EOT token
 * lies inside the prefix (referring expressions use a dozen of the 77 positions); an EOT beyond it yields NaN rows. */
int hgl_clip_encode_text_prefix(const HglClipTextW* w, const int32_t* tokens, int B, int seq_len, float* out,
                                void* workspace, size_t workspace_bytes, void* stream);

/* The two text-tower variants off the Hybridgl_main path (kept for API completeness):
 *  - pool_pos (device int32 [B], nullable): the projected row of string b is position pool_pos[b] instead of its EOT --
 *    CLIP.encode_text(text, target_noun_index) with pool_pos = target_noun_index + 1 (clip/model.py:426-428);
 *  - zero_pos (device int32 [n_zero], nullable) + masking_block: before every block l >= masking_block the positions
 *    zero_pos[*] of EVERY string are set to zero -- CLIPViTFM.text_masking_feature with zero_pos = masking_index + 1
 *    (model/backbone.py:34-56).  Positions >= seq_len are ignored. */
int hgl_clip_encode_text_ex(const HglClipTextW* w, const int32_t* tokens, int B, int seq_len, const int32_t* pool_pos,
                            const int32_t* zero_pos, int n_zero, int masking_block, float* out,
                            void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------
 * Text-conditioned heat-map: the GEM call of Hybridgl_main.py:36-39,200-201
 * (`gem.create_gem_model('ViT-B/16','openai')`, `gem_model(tensor_img, [noun_phrase])`).
 * gem_torch 1.0.1 is an external package (environment.yaml:206): the published
 * algorithm is restated, parity unpinned (oracle/gem_oracle.py).
 * --------------------------------------------------------------------- */

/* GEMViT.forward on ONE image.  w: the CLIP vision tower with grid = res/patch and
 * positional_embedding already interpolated to that grid ([grid*grid+1, width]).
 * img [3,res,res] fp32 (gem.get_gem_img_transform output).  The last gem_blocks
 * blocks are GEM blocks (gem_depth - 1 = 6 by default); ss_attn_iter self-self
 * iterations (1); ss_attn_temp <= 0 selects the adaptive temperature.
 * feat_gem [grid*grid+1, embed] = proj(ln_post(gem stream)), row 0 = CLS;
 * feat_ori (may be NULL) = the same for the original stream (return_ori=True). */
size_t hgl_gem_workspace_bytes(const HglClipVisionW* w);
int hgl_gem_image_features(const HglClipVisionW* w, const float* img, int gem_blocks, int ss_attn_iter,
                           float ss_attn_temp, float* feat_gem, float* feat_ori,
                           void* workspace, size_t workspace_bytes, void* stream);

/* The same for nb images at once ([nb,3,res,res] contiguous; token rows stacked: every GEMM covers all images, one
 * temperature per image); feat_gem / feat_ori [nb, grid*grid+1, embed]. */
size_t hgl_gem_batch_workspace_bytes(const HglClipVisionW* w, int nb);
int hgl_gem_image_features_batch(const HglClipVisionW* w, const float* imgs, int nb, int gem_blocks, int ss_attn_iter,
                                 float ss_attn_temp, float* feat_gem, float* feat_ori,
                                 void* workspace, size_t workspace_bytes, void* stream);

/* GEMWrapper.forward after the encoders: heat[t] = minmax(bilinear_up(100*cos(feat[1:], text[t])))
 * feat [grid*grid+1,E]; text [T,E] (normalised or not); heat [T,res,res]; normalize=0 skips min-max. */
size_t hgl_gem_heatmap_workspace_bytes(int grid, int T, int res);
int hgl_gem_heatmap(const float* feat, int grid, int E, const float* text, int T, int res, int normalize,
                    float* heat, void* workspace, size_t workspace_bytes, void* stream);

/* F.interpolate(bilinear, align_corners=False, antialias=False) of a float tensor [C, h, w] -> [C, H, W] = torchvision
 * 0.15's T.Resize on a TENSOR (Hybridgl_main_PhraseCut.py:69-70: the normalised image back to the annotation's size). */
int hgl_resize_bilinear(const float* in, int C, int h, int w, float* out, int H, int W, void* stream);

/* T.Resize((H,W), antialias=True) on a float tensor (Hybridgl_main.py:201):
 * F.interpolate(bilinear, antialias=True, align_corners=False); in [C,h,w] -> out [C,H,W]. */
int hgl_resize_bilinear_aa(const float* in, int C, int h, int w, float* out, int H, int W, void* stream);

/* TF.resize(pred_masks.float(), (g,g)) bilinear, align_corners=False, no
 * antialias (model/backbone.py:160): masks [N,Hm,Wm] uint8 -> pm [N,g*g] f32. */
int hgl_mask_resize(const uint8_t* masks, int N, int Hm, int Wm, int g, float* pm, void* stream);

/* ------------------------------------------------------------------------
 * Scoring tail  (Hybridgl_main.py:153-230, utils.py:135-161,240-268,365-384)
 * --------------------------------------------------------------------- */

/* CLIPViTFM.calculate_score (model/backbone.py:74-87):
 * logits[n,t] = logit_scale * <I_n/|I_n|, T_t/|T_t|>.  img [N,E], txt [T,E]. */
int hgl_calculate_score(const float* img, const float* txt, int N, int T, int E,
                        float logit_scale, float* logits, void* stream);

/* Spatial-coherence score of every mask against a heat-map
 * (Hybridgl_main.py:201-223): given raw imgattn [H,W] (already resized),
 * applies min-max normalisation, the direction mask of gen_dir_mask
 * (utils.py:135-161; dir: 0 none,1 left,2 right,3 middle), division by the mean,
 * then score[n] = (2-black)*sum(attn*m_n)/sum(m_n) - black*sum(attn*(1-m_n))/sum(1-m_n).
 * masks [N,H,W] uint8; score [N] f32; work: >= hgl_coherence_workspace_bytes(). */
size_t hgl_coherence_workspace_bytes(int N, int H, int W);
int hgl_coherence_scores(const float* imgattn, const uint8_t* masks, int N, int H, int W,
                         int dirflag, float black, float* score,
                         void* workspace, size_t workspace_bytes, void* stream);

/* Compute_IoU (utils.py:365-384): out[0]=|pred&gt|, out[1]=|pred|gt| as int64. */
int hgl_iou(const uint8_t* pred, const uint8_t* gt, long long HW, int64_t* out_IU, void* stream);

/* Whole per-sentence tail in one launch (Hybridgl_main.py:153-196,225-228).
 * hybrid [N,E]; sentence_feat [E], noun_phrase_feat [E] (text_ensemble = r*sentence +
 * (1-r)*noun_phrase, :153); other_noun_feats [n_other,E] = encode_text("a photo of "+noun)
 * rows averaged in order (:157-164; n_other==0 -> the reference scores against zeros and
 * gets NaN logits that it never uses: score_neg is filled with NaN); boxes [N,4] int64
 * XYWH; gem_score [N] (from hgl_coherence_scores); relaword: 0 none,1 left,2 right,3 up,
 * 4 down,5 big,6 small,7 within (utils.py:240-268); has_other_nouns: len(nouns)!=0 (:184).
 * k1,k2 clamp to N (:178-181).  Outputs: idx[0]=argmax(score_clip) ("pure hybridgl"),
 * idx[1]=final index; score_clip [N], score_neg [N] logits before the softmax. */
size_t hgl_score_sentence_workspace_bytes(int N, int E);
int hgl_score_sentence(const float* hybrid, const float* sentence_feat, const float* noun_phrase_feat,
                       const float* other_noun_feats, int n_other, float r,
                       const int64_t* boxes, const float* gem_score,
                       int N, int E, float logit_scale, int k1, int k2, float alpha,
                       int relaword, int has_other_nouns,
                       int32_t* idx, float* score_clip, float* score_neg,
                       void* workspace, size_t workspace_bytes, void* stream);

/* The whole tail of ONE dataset item (Hybridgl_main.py:153-230: every sentence of the ref) in four launches -- SURVEY.md
 * 8b's `score_ref`.  Per sentence: text ensemble r*sentence + (1-r)*noun phrase and the mean of the other-noun features
 * (rows of `text` [T,E]), logits against hybrid [N,E], the two soft-maxes and top-k lists, the relation_boxes sums over boxes
 * [N,4] int64 XYWH, the coherence score of every proposal under the sentence's heat-map imgattn [H,W] (min-max, gen_dir_mask,
 * /mean, `black`: :203-223), the blend and both arg-maxes, Compute_IoU of both winners against the sentence's target [H,W]
 * uint8.  The pooling over masks [N,H,W] uint8 for ALL sentences' heat-maps is one launch.  `sentences`: HOST array of S records
 * holding device pointers.  Outputs: idx [S,2] int32 (pure CLIP winner, winner with spatial guidance), iu [S,4] int64
 * (I, U, I_final, U_final); cum [4] int64 (may be NULL) is INCREMENTED by the column sums of iu on the device
 * (cum_I, cum_U, cum_I_final, cum_U_final of Hybridgl_main.py:52-55); score_clip / score_neg / gem_score [S,N] are optional
 * (NULL) copies of the per-sentence logits and coherence scores.  Results are those of hgl_coherence_scores +
 * hgl_score_sentence + hgl_iou_select per sentence, bit for bit.  The call is hgl_score_group's of a group of this one ref
 * (one host path; the pooling keeps 8 masks per workgroup here, the group's keeps 32: the partial sums are the same).  S is not
 * limited: sixteen sentences make one row of the launch's descriptor table, a ref with more takes ceil(S / 16) rows in the same
 * launches.  Workspace: hgl_score_ref_workspace_bytes holds the descriptor table, the counter of finished blocks and ONE
 * workspace per row (the rows run in the same launches), so query it rather than assume a size. */
typedef struct {
  int sentence_row, noun_phrase_row;  /* rows of text: clip.tokenize(sentence), clip.tokenize(noun_phrase) (:146-152) */
  int other_row0, n_other;            /* n_other consecutive rows from other_row0: 'a photo of ' + other noun (:157-164) */
  int dirflag;                        /* 0 none, 1 left, 2 right, 3 middle (utils.py:135-161) */
  int relaword;                       /* 0 none .. 7 within (utils.py:240-268) */
  int has_other_nouns;                /* len(nouns) != 0 (:184) */
  float black;                        /* :211-216 */
  const float* imgattn;               /* [H,W] fp32, device: gem_model(...) resized to the image (:200-202) */
  const uint8_t* target;              /* [H,W] uint8, device: the sentence's ground truth */
} HglSentence;
size_t hgl_score_ref_workspace_bytes(int S, int N, int E, int H, int W);
int hgl_score_ref(const float* hybrid, const float* text, int T, const int64_t* boxes, const uint8_t* masks, int N, int E,
                  int H, int W, const HglSentence* sentences, int S, float logit_scale, float r, int k1, int k2, float alpha,
                  int32_t* idx, int64_t* iu, int64_t* cum, float* score_clip, float* score_neg, float* gem_score,
                  void* workspace, size_t workspace_bytes, void* stream);

/* The same tail for the R refs of a group in ONE set of launches (the grouped evaluation loop scores a group's refs back to
 * back; four launches of ~31 MB per ref are latency-bound, one launch over the group streams ~0.5 GB).  Shapes may differ from
 * ref to ref.  Per ref: the arguments of hgl_score_ref (any number of sentences; k1 / k2 are this ref's values of the clamp of
 * Hybridgl_main.py:178-181, which the caller carries from ref to ref) and its outputs idx [S,2], iu [S,4] and, optionally,
 * score_clip / score_neg / gem_score [S,N].  cum as for hgl_score_ref (the sums of all refs' sentences are added once).
 * Rows identical to hgl_score_ref's (the same host path and kernels: every ref contributes its rows of at most sixteen
 * sentences to the descriptor table, sixteen rows per set of launches). */
typedef struct HglGroupRef {
  const float* hybrid;                /* [N,E] */
  const float* text;                  /* [T,E] */
  int T;
  const int64_t* boxes;               /* [N,4] XYWH */
  const uint8_t* masks;               /* [N,H*W] */
  int N, H, W;
  const HglSentence* sentences;       /* HOST array [S] */
  int S, k1, k2;
  int32_t* idx;                       /* [S,2] */
  int64_t* iu;                        /* [S,4] */
  float *score_clip, *score_neg, *gem_score;   /* [S,N] each, or NULL */
} HglGroupRef;
size_t hgl_score_group_workspace_bytes(const HglGroupRef* refs, int R, int E);
int hgl_score_group(const HglGroupRef* refs, int R, int E, float logit_scale, float r, float alpha, int64_t* cum, void* workspace,
                    size_t workspace_bytes, void* stream);

/* hgl_score_group under C configurations (r, alpha, k1, k2) in ONE pass: the sweep of the tail's hyper-parameters
 * (Hybridgl_main.py:57-63).  Min / max and pooling run once (they do not depend on the configuration), one pass over the mask
 * planes counts |mask_n & target| of EVERY proposal with every distinct target pointer of a ref (a configuration's I / U is then
 * a look-up), and one workgroup per (sentence, distinct r) builds the soft-maxes and the top-k lists to the largest k of that
 * r -- a list for a smaller k is its prefix -- before one thread per configuration runs the relation sums and the blend.
 * refs: as for hgl_score_group, with the same checks; their k1, k2, idx, iu and score rows are NOT used -- per ref the sweep
 * record stands in: k HOST [C,2] = (k1, k2) of every configuration for THIS ref (the caller carries the clamp of
 * Hybridgl_main.py:178-181 per configuration; clamped to N here as there), idx [C,S,2] int32, iu [C,S,4] int64 and
 * ceiling [S,3] int64 = (n, I, U) of the proposal with the largest I / U against the sentence's target -- the bound no scoring
 * exceeds -- compared exactly (I_a U_b > I_b U_a in 64 bits), lowest index on ties, a pair with U = 0 ranking as ratio 0.
 * configs: HOST [C], 1 <= C <= 256, at most 32 distinct r (by bit pattern); every k in [1, 16] after the clamp: HGL_EINVAL
 * otherwise, before anything is written.  cum [C,4] int64 (may be NULL) is INCREMENTED by the column sums of every ref's iu[c],
 * cum_ceiling [2] int64 (may be NULL) by the sums of the ceilings' I and U, on the device.
 * CONTRACT: row c of idx, iu and cum equals, bit for bit, what hgl_score_group returns for the same refs with r = configs[c].r,
 * alpha = configs[c].alpha and each ref's k1, k2 = k[c] -- NaN logits and NaN coherence scores included (the same device code
 * in the same order).  The workspace depends on the number of distinct r: query it with the call's own configs. */
typedef struct { float r, alpha; } HglSweepConfig;
typedef struct HglSweepRef {
  const int32_t* k;                   /* HOST [C,2] */
  int32_t* idx;                       /* [C,S,2] */
  int64_t* iu;                        /* [C,S,4] */
  int64_t* ceiling;                   /* [S,3] */
} HglSweepRef;
size_t hgl_score_group_sweep_workspace_bytes(const HglGroupRef* refs, int R, int E, const HglSweepConfig* configs, int C);
int hgl_score_group_sweep(const HglGroupRef* refs, const HglSweepRef* sweep, int R, int E, float logit_scale,
                          const HglSweepConfig* configs, int C, int64_t* cum, int64_t* cum_ceiling, void* workspace,
                          size_t workspace_bytes, void* stream);

/* Compute_IoU on a mask selected on the device: pred = masks[idx[which]] ([N,HW] uint8),
 * so the winning index never travels to the host (Hybridgl_main.py:169-171,227-230). */
int hgl_iou_select(const uint8_t* masks, const int32_t* idx, int which, const uint8_t* gt,
                   long long HW, int64_t* out_IU, void* stream);

/* The reference's free helpers, standalone (the fused tail above does not need them):
 * gen_dir_mask (utils.py:135-161): out [H,W] fp32; dirflag 0 none (ones; also "up"/"down", commented out in the
 * reference), 1 left, 2 right, 3 middle; torch.linspace's symmetric single-fma evaluation.
 * relation_boxes (utils.py:240-268) for n independent pairs: boxes XYWH int64 [n,4], scores [n] -> out [n];
 * relaword 0 none .. 7 within (HGL order: none,left,right,up,down,big,small,within). */
int hgl_gen_dir_mask(int dirflag, int H, int W, float* out, void* stream);
int hgl_relation_boxes(const int64_t* boxes_i, const int64_t* boxes_j, const float* score_i, const float* score_j, int n,
                       int relaword, float* out, void* stream);

/* Blurred background of the global views (Hybridgl_main.py:99, cv2.GaussianBlur(img, (15,15), 0)).  cv2's 8-bit
 * fixed-point arithmetic is unpinned (package absent offline): this evaluates the package's own
 * definition -- separable filter with the caller's k odd taps (HOST array of doubles), reflect-101 borders, double
 * accumulation in tap order (rows first), round half up -- bit-identically to hybridgl_amd.synth.box_blur_u8.
 * img/out: [H,W,C] uint8 on the device. */
size_t hgl_gaussian_blur_u8_workspace_bytes(int H, int W, int C);
int hgl_gaussian_blur_u8(const uint8_t* img, int H, int W, int C, const double* taps, int k, uint8_t* out, void* workspace,
                         size_t workspace_bytes, void* stream);

/* cv2.GaussianBlur(img, (k,k), sigma) on uint8 (Hybridgl_main.py:99), OpenCV 4.x bit-exact path restated
 * (opencv-python is external: parity unpinned).  hgl_cv_gaussian_kernel_q8 (HOST) fills the k 8.8 fixed-point
 * taps (sum 256; sigma <= 0 selects OpenCV's 0.15 k + 0.35).  hgl_gaussian_blur_u8_q8 filters rows then columns in
 * integer arithmetic, reflect-101 borders, one rounding (v + 2^15) >> 16.  Workspace: the size query above. */
int hgl_cv_gaussian_kernel_q8(int k, double sigma, uint16_t* taps);
int hgl_gaussian_blur_u8_q8(const uint8_t* img, int H, int W, int C, const uint16_t* taps_x, const uint16_t* taps_y, int k,
                            uint8_t* out, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------
 * Image synthesis (Hybridgl_main.py:93-125): per mask, the blurred-background
 * "global" view and mean-filled "local" view, bilinear (no antialias) to res x res.
 * sam_img [H,W,3] uint8, blurred [H,W,3] uint8 (cv2.GaussianBlur output),
 * image_norm [3,H,W] f32 (ImageNet-normalised), masks [N,H,W] uint8.
 * local,global: [N,3,res,res] f32. */
int hgl_synthesize_views(const uint8_t* sam_img, const uint8_t* blurred, const float* image_norm,
                         const uint8_t* masks, int N, int H, int W, int res,
                         float* local_imgs, float* global_imgs, void* stream);

/* Visual prompts: what the two views show, as one plain struct passed by value to the kernel.  The rules -- box clamping,
 * window, taps, gray, marker bands, ranges -- are csrc/view_prompt.h, integer arithmetic throughout. */
typedef struct HglViewPrompt {
  int window;                 /* 0 frame, 1 the mask's box: what both views look at */
  int pad_permille;           /* 0..4000: margin of the box window, in thousandths of the box's longer side */
  int square;                 /* 0/1: the box window is the square about the box's centre */
  int local_bg;               /* outside the mask in the local view: 0 local_fill, 1 the image */
  float local_fill[3];        /* in the units of image_norm (the CLIP mean by default) */
  int global_bg;              /* outside the mask in the global view: 0 blurred, 1 the image, 2 its gray, 3 global_fill */
  uint8_t global_fill[3];
  uint8_t marker_rgb[3];
  int marker;                 /* drawn on the global view only: 0 none, 1 ellipse, 2 box */
  int thickness;              /* 1..64 source pixels */
  int grow;                   /* 0..4096 source pixels between the box and the band */
} HglViewPrompt;

/* hgl_synthesize_views under a prompt.  boxes_xyxy: [N,4] int32 inclusive XYXY on the device (what hgl_mask_boxes writes),
 * NULL unless window == box or marker != none; blurred: NULL unless global_bg == blur.  H, W <= 8192.  At the default prompt
 * (frame, CLIP-mean fill, blur, no marker) the views are hgl_synthesize_views' bit for bit.  No workspace, no
 * synchronisation. */
int hgl_synthesize_views_prompt(const uint8_t* sam_img, const uint8_t* blurred, const float* image_norm, const uint8_t* masks,
                                const int32_t* boxes_xyxy, int N, int H, int W, int res, const HglViewPrompt* prompt,
                                float* local_imgs, float* global_imgs, void* stream);

/* ------------------------------------------------------------------------
 * SAM ViT-H mask proposals (third_party/segment-anything/segment_anything/,
 * driven by SamAutomaticMaskGenerator at Hybridgl_main.py:66-74,85)
 * --------------------------------------------------------------------- */

typedef struct HglSamBlockW {          /* modeling/image_encoder.py:119-182 Block */
  int window;                          /* 14, or 0 for the global-attention blocks (build_sam.py:19) */
  int rel_len;                         /* rows of rel_pos_h/w = 2*size-1 (27 windowed, 127 global) */
  const float *norm1_w, *norm1_b;
  const float *qkv_w, *qkv_b;          /* [3D,D],[3D] */
  const float *proj_w, *proj_b;        /* [D,D],[D] */
  const float *rel_pos_h, *rel_pos_w;  /* [rel_len, D/heads] */
  const float *norm2_w, *norm2_b;
  const float *lin1_w, *lin1_b;        /* [4D,D],[4D] */
  const float *lin2_w, *lin2_b;        /* [D,4D],[D] */
} HglSamBlockW;

typedef struct HglSamEncoderW {        /* modeling/image_encoder.py:17-116 ImageEncoderViT */
  int embed_dim, depth, heads, img_size, patch, out_chans; /* ViT-H: 1280,32,16,1024,16,256 */
  const float *patch_w, *patch_b;      /* [D, 3*patch*patch], [D] */
  const float* pos_embed;              /* [g*g, D] */
  const HglSamBlockW* blocks;          /* host array of `depth` */
  const float* neck0_w;                /* conv1x1 [C, D] */
  const float *neck1_w, *neck1_b;      /* LayerNorm2d */
  const float* neck2_w;                /* conv3x3 [C, C*9] (weight flattened c,ky,kx) */
  const float *neck3_w, *neck3_b;
} HglSamEncoderW;

typedef struct HglLinearW { const float *w, *b; } HglLinearW;   /* [out,in],[out] */
typedef struct HglNormW { const float *w, *b; } HglNormW;
typedef struct HglSamAttnW { HglLinearW q, k, v, out; int internal; } HglSamAttnW; /* transformer.py:185-240 */

typedef struct HglSamDecoderW {        /* prompt_encoder.py + mask_decoder.py + transformer.py */
  int C, grid, heads, mlp_dim;         /* 256, 64, 8, 2048 */
  const float* pe_gauss;               /* [2, C/2] positional_encoding_gaussian_matrix */
  const float *point_embed_pos, *not_a_point, *no_mask;   /* [C] each */
  const float* dense_pe;               /* [grid*grid, C] = get_dense_pe() (filled by hgl_sam_dense_pe) */
  const float *iou_token, *mask_tokens;/* [C], [4,C] */
  struct { HglSamAttnW self_attn, t2i, i2t; HglNormW n1, n2, n3, n4; HglLinearW lin1, lin2; } layer[2];
  HglSamAttnW final_t2i;
  HglNormW norm_final;
  const float *up0_w, *up0_b;          /* ConvT 256->64 as GEMM: [(pos,oc)=256, 256], bias [(pos,oc)] */
  HglNormW up1;                        /* LayerNorm2d(64) */
  const float *up3_w, *up3_b;          /* ConvT 64->32 as GEMM: [(pos,oc)=128, 64], bias [(pos,oc)] */
  HglLinearW hyper[4][3];              /* output_hypernetworks_mlps */
  HglLinearW iou_head[3];
  /* Optional (NULL = not provided), split-fp16 mode: the image-side projections of one step merged into ONE GEMM over the
   * 256-channel rows, the positional encoding entering as a per-position table instead of a second copy of the rows:
   * (keys + pe) Wk^T = keys Wk^T + (pe Wk^T).  kvq1: layer 1's token->image k, v and image->token q (all read the same
   * rows): weight [3I, C] = rows of layer[1].t2i.k.w, layer[1].t2i.v.w, layer[1].i2t.q.w; bias [3I]; pe table
   * [grid*grid, 3I] = dense_pe @ [Wk; 0; Wq]^T.  kvf: the final token->image k, v: [2I, C], [2I], [grid*grid, 2I]. */
  const float *kvq1_w, *kvq1_b, *kvq1_pe;
  const float *kvf_w, *kvf_b, *kvf_pe;
  /* Optional (NULL = not provided): the other label embeddings of the prompt encoder, [C] each: point_embeddings[0]
   * (background point), [2] / [3] (box corners) -- needed by hgl_sam_decode_prompts only (prompt_encoder.py:40-42). */
  const float *point_embed_neg, *point_embed_box0, *point_embed_box1;
  /* Optional: PromptEncoder.mask_downscaling (prompt_encoder.py:57-66) for hgl_sam_embed_masks: Conv2d(1,4,k2,s2) [4,4] / [4],
   * LayerNorm2d(4), Conv2d(4,16,k2,s2) [16,16 = (c_in,ky,kx)] / [16], LayerNorm2d(16), Conv2d(16,C,k1) [C,16] / [C]. */
  const float *md_c1_w, *md_c1_b, *md_n1_w, *md_n1_b, *md_c2_w, *md_c2_b, *md_n2_w, *md_n2_b, *md_c3_w, *md_c3_b;
} HglSamDecoderW;

/* ResizeLongestSide.apply_image (utils/transforms.py:26-31) = Pillow Image.resize(BILINEAR) on uint8 HWC,
 * bit-exact: horizontal then vertical pass of Pillow's 8-bit resampler with 22-bit fixed-point weights.
 * kx/ky: int32 weights [out, ksize]; bx/by: int32 (first, count) per output index -- computed on the host as
 * Resample.c precompute_coeffs + normalize_coeffs_8bpc do (hybridgl_amd/sam.py:pil_bilinear_coeffs). */
size_t hgl_resize_pil_bilinear_workspace_bytes(int H, int out_w, int C);
int hgl_resize_pil_bilinear(const uint8_t* img, int H, int W, int C, int out_h, int out_w, const int32_t* kx,
                            const int32_t* bx, int ksize_x, const int32_t* ky, const int32_t* by, int ksize_y,
                            uint8_t* out, void* workspace, size_t workspace_bytes, void* stream);

/* The dataset transforms T.ToTensor() + T.Normalize(mean, std) on a uint8 HWC image (data/dataset_refer_bert.py:155-158;
 * gem.get_gem_img_transform, Hybridgl_main.py:39) as a table look-up: out[c, y, x] = lut[c * 256 + img[y, x, c]], out
 * [C, H, W] fp32.  lut [C, 256] is built on the host with the reference's fp32 arithmetic ((v / 255 - mean[c]) / std[c]),
 * which makes the result bit-identical to the host transform.  With hgl_resize_pil_bilinear (any Pillow filter: the
 * weights are the caller's tables, bicubic for the GEM transform) this moves the per-item float work of the reference's
 * DataLoader workers onto the device; the host keeps the JPEG decode. */
int hgl_u8_to_chw_lut(const uint8_t* img, int H, int W, int C, const float* lut, float* out, void* stream);

/* Sam.preprocess + ImageEncoderViT.forward (modeling/sam.py:164-174, image_encoder.py:106-116).
 * resized_img: [in_h,in_w,3] uint8 -- the image after ResizeLongestSide.apply_image (PIL
 * bilinear on the host, utils/transforms.py:26-31).  emb: [g*g, out_chans] NHWC rows
 * (the reference's [1,256,64,64] transposed; it is consumed in this order by the decoder). */
size_t hgl_sam_encode_workspace_bytes(const HglSamEncoderW* w);
int hgl_sam_encode(const HglSamEncoderW* w, const uint8_t* resized_img, int in_h, int in_w, float* emb,
                   void* workspace, size_t workspace_bytes, void* stream);

/* The same for nb images at once (token rows stacked: every launch covers all images, weights read once).
 * resized_imgs / in_h / in_w: HOST arrays of nb device pointers / sizes; emb [nb, g*g, out_chans]. */
size_t hgl_sam_encode_batch_workspace_bytes(const HglSamEncoderW* w, int nb);
int hgl_sam_encode_batch(const HglSamEncoderW* w, const uint8_t* const* resized_imgs, const int* in_h, const int* in_w,
                         int nb, float* emb, void* workspace, size_t workspace_bytes, void* stream);

/* The rel-pos producer of one encoder attention launch, on its own: the decomposed terms of add_decomposed_rel_pos
 * (image_encoder.py:325-361) from the UNSCALED q of B windows (or whole grids) of S = size * size tokens,
 *   rel_h[b*heads + h, q, k] = q_vec . rel_pos_h[q / size - k + size - 1],
 *   rel_w[b*heads + h, q, k] = q_vec . rel_pos_w[q % size - k + size - 1],      both [B*heads, S, size],
 * with q_vec the hd columns of head h in row b*S + q of q.  q comes in one of two forms: fp32 rows of ldq floats (qkv: the
 * packed in-projection output, q in the first heads*hd columns; q_hi = q_lo = NULL), or the fp16 hi / lo planes of the split
 * in-projection (q_hi, q_lo, rows of ldq halfs; qkv = NULL; HGL_PREC_F16X3 only).  rel_pos_h / rel_pos_w: [2*size-1, hd].
 * The kernels are the encoder's own, chosen by the function the encoder calls, from the library precision, hd, size and the
 * form of q: planes -> the matrix-core kernel on planes (hd 64 / 80, size 14 / 64); hd 64 / 80 at an even size <= 64 -> the
 * direct kernels (matrix cores in the split-fp16 modes at size 14 / 64, VALU otherwise); every other (hd, size) with hd in
 * 16 / 32 / 64 / 80 -> two batched GEMMs q . rel_pos^T over all 2*size-1 rows + two gathers, through the workspace.
 * Exported for the per-kernel tests (tests/test_gpu_relpos_tables.py). */
size_t hgl_sam_relpos_tables_workspace_bytes(int B, int heads, int S, int size);
int hgl_sam_relpos_tables(const float* qkv, const void* q_hi, const void* q_lo, int ldq, int B, int heads, int S, int size,
                          int hd, const float* rel_pos_h, const float* rel_pos_w, float* rel_h, float* rel_w,
                          void* workspace, size_t workspace_bytes, void* stream);

/* get_dense_pe() (prompt_encoder.py:194-205): grid_coords01 [grid*grid,2] fp32 = ((x+1)-0.5)/grid,
 * ((y+1)-0.5)/grid; fills dense_pe [grid*grid, C]; call once per model. */
int hgl_sam_dense_pe(const HglSamDecoderW* w, const float* grid_coords01, float* dense_pe, void* stream);

/* PromptEncoder (one positive point per prompt + padding point) + MaskDecoder(multimask)
 * (predictor.py:222-235): points01 [P,2] fp32 = (point+0.5)/img_size computed in float64 by the
 * caller (prompt_encoder.py:79, :207-214) -> low_res [P,3,4*grid,4*grid] logits, iou [P,3]. */
size_t hgl_sam_decode_workspace_bytes(const HglSamDecoderW* w, int P);
int hgl_sam_decode_points(const HglSamDecoderW* w, const float* emb, const float* points01, int P,
                          float* low_res, float* iou_pred, void* workspace, size_t workspace_bytes,
                          void* stream);
/* hgl_sam_decode_points with the IoU gate of the automatic generator: iou_pred depends on the token outputs only
 * (mask_decoder.py:132-149), and SamAutomaticMaskGenerator drops every mask whose prediction does not exceed pred_iou_thresh
 * (automatic_mask_generator.py:287-291) -- so the quality head runs first and a prompt none of whose three predictions
 * exceeds `iou_gate` (NaN fails) skips the output upscaling: its rows of low_res are NOT written (the caller's filter never
 * looks at them; hgl_sam_postprocess with the same threshold zeroes its masks).  iou_pred is complete either way.  The gate
 * acts in the fused upscaling of the split-fp16 mode; elsewhere every prompt is upscaled. */
int hgl_sam_decode_points_gated(const HglSamDecoderW* w, const float* emb, const float* points01, int P, float iou_gate,
                                float* low_res, float* iou_pred, void* workspace, size_t workspace_bytes, void* stream);
/* The prompts of SEVERAL images in one call (a group of images through the automatic generator): emb [n_img, grid*grid, C],
 * points01 [n_img * ppi, 2], prompt p belongs to image p / ppi -> low_res [n_img*ppi,3,4*grid,4*grid], iou [n_img*ppi,3].
 * Every prompt's rows are bit for bit those of hgl_sam_decode_points(_gated) on its image's own ppi prompts: only the first
 * decoder layer knows that prompts share image tokens (it addresses the rows of image p / ppi), and every choice that
 * depends on the batch -- the key-range split of the token -> image attention -- is taken from ppi, never from the
 * launch's total.  With the fused decoder stages (split-fp16 mode, the ViT decoder geometry) the prompts go through one
 * launch sequence per 1024 prompts (whole images: within that bound no kernel choice on the token side depends on the row
 * count); elsewhere the call runs the one-image path image by image.  n_img * ppi <= 65535;
 * workspace >= hgl_sam_decode_multi_workspace_bytes(w, n_img, ppi).  n_img = 1 is hgl_sam_decode_points(_gated). */
size_t hgl_sam_decode_multi_workspace_bytes(const HglSamDecoderW* w, int n_img, int ppi);
int hgl_sam_decode_points_multi(const HglSamDecoderW* w, const float* emb, const float* points01, int n_img, int ppi,
                                float* low_res, float* iou_pred, void* workspace, size_t workspace_bytes, void* stream);
int hgl_sam_decode_points_multi_gated(const HglSamDecoderW* w, const float* emb, const float* points01, int n_img, int ppi,
                                      float iou_gate, float* low_res, float* iou_pred, void* workspace, size_t workspace_bytes,
                                      void* stream);
/* The same for the other prompt kinds of SamPredictor.predict_torch (predictor.py:169-243; PromptEncoder._embed_points /
 * _embed_boxes / _embed_masks, prompt_encoder.py:73-127): n_sparse = 2 .. 11 sparse tokens per prompt, coords01
 * [P,n_sparse,2] ((coordinate + 0.5) / img_size, computed by the caller in the dtype the reference would use), labels
 * [P,n_sparse]: -1 padding point (its coordinate is ignored), 0 background point, 1 foreground point, 2 / 3 the top-left /
 * bottom-right corner of a box.  (point, -1) = one point; (point, ..., point, -1) = several points; (2, 3) = a box;
 * (point, ..., 2, 3) = points and a box.  dense: NULL (no_mask_embed for every prompt) or [P, grid*grid, C] from
 * hgl_sam_embed_masks (mask inputs: the image tokens then differ per prompt from the first layer on, which runs as plain fp32
 * launches).  first_mask = 1: mask tokens 1..3 (multimask_output=True); 0: tokens 0..2 -- column 0 is the single-mask output
 * of multimask_output=False (mask_decoder.py:99-105).  Two sparse tokens take the fused decoder stages; more tokens the
 * general attention kernels (and, beyond three, at most 8191 prompts per call). */
int hgl_sam_decode_prompts(const HglSamDecoderW* w, const float* emb, const float* coords01, const int32_t* labels, int n_sparse,
                           const float* dense, int first_mask, int P, float* low_res, float* iou_pred, void* workspace,
                           size_t workspace_bytes, void* stream);
/* PromptEncoder._embed_masks (prompt_encoder.py:103-106): mask_input [P,1,4*grid,4*grid] fp32 -> dense [P, grid*grid, C] */
int hgl_sam_embed_masks(const HglSamDecoderW* w, const float* mask_input, int P, float* dense, void* stream);

/* Fused stages of the decoder (split-fp16 mode): bit 0 = output upscaling + hyper-network products in one launch; bit 1 =
 * merged image-side projections (kvq1 / kvf of HglSamDecoderW, when provided); bit 2 = image -> token attention +
 * out-projection + residual + norm4 in one launch (needs bit 1); bit 4 = token -> image attention as key chunks of 256 with
 * all heads per workgroup + a combine pass (either precision mode); bit 5 = the token -> image attention of layer 1 and the
 * final one on the RAW image-token planes -- the 7 tokens are projected through W_k / W_v instead of the image tokens, no
 * k | v projection GEMM -- and layer 1's image -> token step with W_q / W_o folded into the 7 tokens the same way, no q
 * projection GEMM (needs bits 1 and 2; one foreground point per prompt; grid * grid a multiple of 128).  Sets the mask (mask >= 0; default all
 * stages) and returns the previous one; mask < 0 only queries.  Fused and unfused stages agree to
 * fp32 rounding: the switch exists for timing and for that test. */
int hgl_sam_decoder_fusion(int mask);

/* Attention on pre-split operands (split-fp16 mode): the in-projection GEMMs of SAM's encoder blocks and of CLIP's residual
 * blocks write q | k | v as fp16 hi / lo planes and the attention kernel stages them by LDS-DMA without converting
 * (csrc/attention_ps.hip).  on >= 0 sets the switch (default on, or HGL_ATTN_PS) and returns the previous value; on < 0 only
 * queries.  Both paths evaluate the same products on the same hi / lo values: the switch exists for timing and for the
 * test that compares them. */
int hgl_attention_presplit(int on);
/* The pre-split kernels on a packed fp32 in-projection output (tests, micro-benchmarks): qkv [B*S, ld] with q | k | v at
 * columns 0, H*hd, 2*H*hd (ld >= 3*H*hd, a multiple of 8) is split into fp16 hi / lo planes in scratch (>= B*S*ld*4 bytes)
 * exactly as the GEMM write-out splits it, then multiplied: out [B*S, ldo] fp32.  hd in {64, 80}; mask_kind
 * HGL_MASK_NONE, or HGL_MASK_CLS_KEEP for S <= 257 (keep as for hgl_attention_f32).  Split-fp16 mode only. */
int hgl_attention_presplit_f32(const float* qkv, int ld, int B, int H, int S, int hd, float* out, int ldo, float scale,
                               int mask_kind, const uint8_t* keep, int keep_b0, int keep_n, void* scratch,
                               size_t scratch_bytes, void* stream);

/* Sam.postprocess_masks + the per-candidate AMG statistics in one pass
 * (modeling/sam.py:133-162, automatic_mask_generator.py:287-308, utils/amg.py:156-176,303-346):
 * low_res [K,hl,wl] -> masks [K,H,W] uint8 (logit > mask_threshold), stability [K]
 * (= |logit>thr+off| / |logit>thr-off|), boxes_xyxy [K,4] int32 inclusive (0 when empty), keep [K]
 * (iou_pred > pred_iou_thresh && stability >= stability_thresh; as in the reference each of the two
 * filters exists only when its threshold is > 0, so an empty mask with its NaN stability survives a zero
 * threshold).  Candidates failing the IoU filter are skipped (zero mask).  full_logits: optional
 * [K,H,W] fp32 (tests), else NULL. */
size_t hgl_sam_postprocess_workspace_bytes(int K);
int hgl_sam_postprocess(const float* low_res, const float* iou_pred, int K, int hl, int wl, int img_size,
                        int in_h, int in_w, int H, int W, float mask_threshold, float stability_offset,
                        float pred_iou_thresh, float stability_thresh, uint8_t* masks, int32_t* boxes_xyxy,
                        float* stability, uint8_t* keep, float* full_logits, void* workspace,
                        size_t workspace_bytes, void* stream);

/* torchvision.ops.batched_nms with one category (automatic_mask_generator.py:251-257): greedy,
 * descending score, suppress IoU > iou_threshold among candidates with keep!=0; K <= 1024.
 * out_idx [K] receives the kept candidate indices in order, *out_n their count (device memory).
 * Exact against torchvision's float32 arithmetic for coordinates in [0, 2896]: there every area and every sum of two areas
 * is an integer below 2^24.  Beyond that the union `wa * ha + wb * hb - inter` rounds, and the kernels evaluate it as
 * fma(wa, ha, wb * hb) - inter, where torchvision rounds both products: with coordinates up to 32768, 5 to 7 of 4800 pairs
 * built to lie within a few float32 steps of the threshold are decided the other way (tools/nms_contraction_probe.py).
 * The same holds for hgl_nms_segments and hgl_nms_large. */
int hgl_nms(const int32_t* boxes_xyxy, const float* scores, const uint8_t* keep, int K, float iou_threshold,
            int32_t* out_idx, int32_t* out_n, void* stream);

/* hgl_nms for n_seg candidate lists in one launch (the images of a group): list s = candidates offsets[s] .. offsets[s+1]
 * (offsets [n_seg + 1] int32, device memory, ascending from 0; a list may be empty), one workgroup per list, each list
 * exactly as hgl_nms treats it alone.  out_idx [offsets[n_seg]] receives, from position offsets[s] on, the kept candidates
 * of list s in order as indices INTO the list; out_n [n_seg] their counts.  max_len: the longest list, <= 1024 (lists of
 * more than 512 candidates add a second launch).  boxes_xyxy 16-byte aligned. */
int hgl_nms_segments(const int32_t* boxes_xyxy, const float* scores, const uint8_t* keep, const int32_t* offsets, int n_seg,
                     int max_len, float iou_threshold, int32_t* out_idx, int32_t* out_n, void* stream);

/* remove_small_regions (utils/amg.py:267-291) for a batch of masks on the device: 8-connected
 * components of the mask (holes=0: "islands") or of its complement (holes=1), components with
 * area < area_thresh are removed / filled; changed[n] tells whether mask n had any.  out may not
 * alias masks.  N*H*W < 2^31. */
size_t hgl_remove_small_regions_workspace_bytes(int N, int H, int W);
int hgl_remove_small_regions(const uint8_t* masks, int N, int H, int W, int area_thresh, int holes,
                             uint8_t* out, uint8_t* changed, void* workspace, size_t workspace_bytes,
                             void* stream);
/* The same pass with the written masks' boxes (batched_mask_to_box, utils/amg.py:303-346: int32 XYXY, inclusive, zeros for an
 * empty mask) out of the pass that writes them, instead of hgl_mask_boxes over `out` afterwards. */
int hgl_remove_small_regions_boxes(const uint8_t* masks, int N, int H, int W, int area_thresh, int holes,
                                   uint8_t* out, uint8_t* changed, int32_t* boxes_xyxy, void* workspace,
                                   size_t workspace_bytes, void* stream);
/* NMS for any K <= 32768 (dense point grids, crop layers and the cross-crop pass of
 * automatic_mask_generator.py:209-220,259-266): identical semantics to hgl_nms (descending score, the original
 * index breaks ties, suppress IoU > threshold), three kernels through a caller-supplied workspace. */
size_t hgl_nms_large_workspace_bytes(int K);
int hgl_nms_large(const int32_t* boxes_xyxy, const float* scores, const uint8_t* keep, int K, float iou_threshold,
                  int32_t* out_idx, int32_t* out_n, void* workspace, size_t workspace_bytes, void* stream);
/* is_box_near_crop_edge (segment_anything/utils/amg.py:78-88) folded into the keep flags: boxes (crop
 * coordinates, XYXY) that come within atol of a crop edge which is not also an image edge get keep = 0.
 * crop_box / orig_box are HOST arrays of 4 ints (XYXY). */
int hgl_box_near_crop_edge(const int32_t* boxes_xyxy, int K, const int32_t* crop_box_xyxy, const int32_t* orig_box_xyxy,
                           float atol, uint8_t* keep, void* stream);
/* batched_mask_to_box (utils/amg.py:303-346): inclusive XYXY, [0,0,0,0] for an empty mask. */
int hgl_mask_boxes(const uint8_t* masks, int N, int H, int W, int32_t* boxes_xyxy, void* stream);

/* out[i] = masks[idx[i]] for i < *n (device-side count), rows of HW bytes (HW % 16 == 0). */
int hgl_gather_masks(const uint8_t* masks, const int32_t* idx, const int32_t* n, int max_n, long long HW,
                     uint8_t* out, void* stream);

/* ---- ground-truth masks of the REFER annotations (host functions, no device work) --------------------
 * refer/refer.py:277-291 getMask over refer/external/maskApi.c (rleFrPoly :161-201, rleDecode :43-47,
 * rleFrString :217-230).  mask: caller-owned [H,W] row-major uint8, set to the per-pixel COUNT of covering
 * polygons (what np.sum(mask.decode(rle), axis=2) returns; the dataset keeps count == 1,
 * data/dataset_refer_bert.py:118-121); area: sum of the polygons' areas (may be NULL).
 * xy: the polygons' x0,y0,x1,y1,... concatenated; n_points[i] = vertices of polygon i. */
int hgl_gt_mask_from_polygons(const double* xy, const int32_t* n_points, int n_polys, int H, int W, uint8_t* mask,
                              int64_t* area);
/* uncompressed RLE counts (column-major runs, zeros first) / the compressed string form */
int hgl_gt_mask_from_rle_counts(const uint32_t* counts, int m, int H, int W, uint8_t* mask, int64_t* area);
int hgl_gt_mask_from_rle_string(const char* s, int H, int W, uint8_t* mask, int64_t* area);
/* The other direction -- the "uncompressed_rle" / "coco_rle" output modes of SamAutomaticMaskGenerator
 * (automatic_mask_generator.py:176-182; utils/amg.py:107-136 mask_to_rle_pytorch, :294-300 coco_encode_rle ->
 * pycocotools frPyObjects -> refer/external/maskApi.c:203-216 rleToString).  HOST memory.
 * hgl_rle_encode_mask: column-major run lengths of mask [H,W] (first count = leading zeros); *m = number of counts
 * (reported even when counts is NULL / cap too small: size query).
 * hgl_rle_to_string: the compressed ASCII string of COCO; out needs at most 7*m+1 bytes; *len = strlen(out). */
int hgl_rle_encode_mask(const uint8_t* mask, int H, int W, uint32_t* counts, long long cap, long long* m);
int hgl_rle_to_string(const uint32_t* counts, long long m, char* out, size_t cap, size_t* len);
/* The same run lengths for masks that live on the DEVICE, selected by a device index tensor (csrc/rle.hip): the mask
 * generator's RLE modes and the evaluator's winning masks without a pixel read-back.  Asynchronous on `stream`; no host
 * synchronisation, allocation or atomics; every entry owns its slot and its table row.
 * masks: device [N,H,W] row-major, nonzero = foreground (N*H*W < 2^31).  sel: device [S] indices into masks, or NULL for
 * masks 0..S-1 (then S <= N).  slots: device [S, slot_words].  table: device [S,4] = (n_counts, form, area, 0); n_counts
 * is always the true number of counts and area the number of foreground pixels.  form says what the slot holds:
 *   0  the n_counts counts (whenever n_counts <= slot_words)
 *   1  the column-major bit plane, bit p % 32 of word p / 32 with p = x*H + y, ceil(H*W/32) words (the counts do not fit
 *      but the plane does: with slot_words = ceil(H*W/32) no mask is ever lost, whatever its run count)
 *   2  neither fits: nothing written
 *   3  sel[s] is outside [0, N): nothing read or written
 * Words of a slot beyond what its form defines are not written.  ws: the size the workspace query returns for (S, H, W). */
size_t hgl_rle_encode_workspace_bytes(int S, int H, int W);
int hgl_rle_encode_device(const uint8_t* masks, int N, int H, int W, const int64_t* sel, int S, uint32_t* slots,
                          long long slot_words, int32_t* table, void* ws, size_t ws_bytes, void* stream);
/* The counts of a compressed COCO RLE string (maskApi.c:217-230 rleFrString without the decode).  HOST memory.  *m = the
 * true number of counts, always; with counts == NULL or cap too small nothing is written beyond cap (size query, as
 * hgl_rle_encode_mask).  A group cut off by the end of the string, or longer than 7 characters, is an error. */
int hgl_rle_from_string(const char* s, uint32_t* counts, long long cap, long long* m);
/* The way back on the DEVICE (csrc/rle.hip): masks out of exactly what hgl_rle_encode_device writes, so that encode ->
 * decode composes with no host in between, and intersection / union of two encoded sets without expanding either.
 * Asynchronous on `stream`; no host synchronisation, allocation or atomics; two calls give the same bytes.
 * slots: device [S, slot_words]; table: device [S,4] = (n_counts, form, ., .), columns 2 and 3 are not read.
 *   form 0  the slot holds n_counts counts (column-major runs, zeros first; zero-length runs anywhere are legal)
 *   form 1  the slot holds the column-major bit plane, bit p % 32 of word p / 32 with p = x*H + y; bits beyond H*W ignored
 * masks: device [S,H,W] row-major uint8, values 0 / 1; every byte of every entry is written (no need to clear), none
 * outside [0, S*H*W).  status: device [S,4] = (code, area, 0, 0), area = foreground pixels written.
 *   code 0  decoded, and (form 0) the counts sum to exactly H*W
 *   code 1  form 0 whose counts do not sum to H*W: decoded as the host codec decodes it (hgl_gt_mask_from_rle_counts):
 *           runs clipped at H*W (positions are summed in 64 bits: [0xFFFFFFFF, 5] does not wrap), pixels past the last
 *           run are 0
 *   code 2  the slot holds no mask: form 2 or 3 or any other form value, n_counts < 0, n_counts > slot_words in form 0,
 *           ceil(H*W/32) > slot_words in form 1; the mask is all zeros
 * hgl_rle_iou_device: iu device [S,2] int64 = (|A & B|, |A | B|) of entry s of A against entry s of B, on bit planes in
 * the workspace; (-1, -1) when either entry would have code 2; code-1 entries count as decoded.
 * Limits: H*W < 2^31 and S*H*W < 2^31.  ws: the size the matching workspace query returns (HGL_EWORKSPACE when smaller). */
size_t hgl_rle_decode_workspace_bytes(int S, int H, int W, long long slot_words);
int hgl_rle_decode_device(const uint32_t* slots, long long slot_words, const int32_t* table, int S, int H, int W,
                          uint8_t* masks, int32_t* status, void* ws, size_t ws_bytes, void* stream);
/* A whole group's stored proposals in one call (csrc/rle.hip): hgl_rle_decode_device for S entries that belong to G <= 64
 * images of their own sizes, with every mask's box -- what loading the per-image record lists of scripts/amg.py:229-232
 * (generate() in coco_rle mode, automatic_mask_generator.py:176-182) needs in place of rle_to_mask (utils/amg.py:138-149)
 * per record and batched_mask_to_box (utils/amg.py:303-346) per image.  Two launches whatever G and the sizes are.
 * Asynchronous on `stream`; no host synchronisation, allocation or atomics; two calls give the same bytes.
 * slots / table: as hgl_rle_decode_device (forms 0 and 1).  images_host: HOST [G,4] int64, row g = (H_g, W_g, first entry
 * e_g, byte offset o_g into masks); image g owns the entries e_g .. e_(g+1)-1 (e_0 = 0, e_G = S, non-decreasing; an image may
 * own none) and entry s of it is written at o_g + (s - e_g)*H_g*W_g.  The extents must lie inside [0, masks_bytes) and must
 * not overlap, n_g*H_g*W_g < 2^31; anything else is HGL_EINVAL and nothing is enqueued.  The array is read before the call
 * returns.  Every byte of every extent is written 0 / 1, none outside; an image whose W is a multiple of 4 and whose base
 * address is 4-byte aligned takes the 4-column store path, any other the byte path.
 * status: device [S,4] = (code, area, 0, 0) as hgl_rle_decode_device, against the entry's own H_g*W_g.
 * boxes_xyxy: device [S,4] int32, the hgl_mask_boxes rule for the mask this call writes (inclusive XYXY, zeros for an empty
 * mask and for code 2), derived from the runs / the plane words, not from the pixels.
 * ws: hgl_rle_decode_group_workspace_bytes(S, slot_words) (HGL_EWORKSPACE when smaller). */
size_t hgl_rle_decode_group_workspace_bytes(int S, long long slot_words);
int hgl_rle_decode_group_device(const uint32_t* slots, long long slot_words, const int32_t* table, int S,
                                const int64_t* images_host, int G, uint8_t* masks, long long masks_bytes,
                                int32_t* boxes_xyxy, int32_t* status, void* ws, size_t ws_bytes, void* stream);
size_t hgl_rle_iou_workspace_bytes(int S, int H, int W, long long slot_words_a, long long slot_words_b);
int hgl_rle_iou_device(const uint32_t* slots_a, long long slot_words_a, const int32_t* table_a,
                       const uint32_t* slots_b, long long slot_words_b, const int32_t* table_b,
                       int S, int H, int W, int64_t* iu, void* ws, size_t ws_bytes, void* stream);
/* Every mask of set A against every mask of set B, image by image (csrc/rle.hip): the m x n form of the reference's
 * rleIou(dt, gt, m, n, iscrowd, o) (refer/external/maskApi.c:77-96, pycocotools' iou) as exact integers, with the best partner
 * of every mask.  Grouped from the start: one image is a group of one.  Asynchronous on `stream`; no host synchronisation,
 * allocation or atomics; two calls give the same bytes; at most six launches, whatever G and the sizes are.
 * Set A = (slots_a, slot_words_a, table_a, Sa), set B likewise: what hgl_rle_encode_device hands out, forms 0 and 1, with the
 * code 0 / 1 / 2 rules of hgl_rle_decode_device.  Sa or Sb may be 0 (the set's pointers are then not read).
 * images_host: HOST [G,5] int64, G <= 64, row g = (H_g, W_g, first A entry, first B entry, element offset of the image's
 * matrix in inter); entries run from 0 to Sa / Sb and do not decrease, an image may own none on either side; H*W < 2^31.
 * The array is read before the call returns.  Image g's matrix is [na_g, nb_g] int32, row-major; the extents must lie inside
 * [0, inter_elems) and must not overlap.  Anything else is HGL_EINVAL and nothing is enqueued.
 * crowd_b: device [Sb] uint8 (nonzero = crowd), or NULL for none.
 * inter: |a & b| of every pair of an image, -1 in the row / column of an entry of code 2; nothing outside the extents is
 * written.  NULL: no matrix is wanted (column 4 of images_host and inter_elems are not read).
 * match_a: device [Sa,4] int32 = (code, area, best, I_best), match_b [Sb,4] likewise.  code and area as the decoder's status;
 * best = the index, within the image's other set, of the partner with the largest I / D, where D(a, b) = area(a) when
 * crowd_b[b] is set and area(a) + area(b) - I otherwise; ratios are compared exactly (I1*D2 > I2*D1 in 64 bits) and the lowest
 * index wins a tie; best = -1 and I_best = 0 when no partner intersects.  An entry of code 2 has area 0 and best = -1 and is
 * nobody's best.
 * Limits: Sa + Sb < 2^31; per side the sum of n_g * W_g * ceil(H_g / 64) < 2^32.
 * ws: hgl_rle_match_workspace_bytes for the same geometry, want_inter = (inter != NULL).  The query returns 0 for a geometry
 * the call refuses and also for a valid call without an entry (Sa = Sb = 0), which needs no workspace and takes ws = NULL.
 * The workspace holds both sets' bit planes and the partial counts: a call of fewer than 1024 tiles of 32 x 64 pairs splits
 * every tile's plane words over up to 32 workgroups, each with a plane of sum(na_g * nb_g) counts of its own. */
size_t hgl_rle_match_workspace_bytes(const int64_t* images_host, int G, int Sa, long long slot_words_a, int Sb,
                                     long long slot_words_b, int want_inter);
int hgl_rle_match_device(const uint32_t* slots_a, long long slot_words_a, const int32_t* table_a, int Sa,
                         const uint32_t* slots_b, long long slot_words_b, const int32_t* table_b, int Sb,
                         const int64_t* images_host, int G, const uint8_t* crowd_b, int32_t* inter, long long inter_elems,
                         int32_t* match_a, int32_t* match_b, void* ws, size_t ws_bytes, void* stream);
/* Ground-truth polygons rasterised on the DEVICE, straight into RLE (csrc/rle_poly.hip): the device form of
 * refer/external/maskApi.c:161-201 rleFrPoly and of the polygon count that refer/refer.py:283-291 takes of its masks --
 * hgl_gt_mask_from_polygons without the pixels.  What it writes is what hgl_rle_encode_device would write for the finished
 * masks, so the targets of an evaluation meet hgl_rle_iou_device / hgl_rle_match_device without ever being an image.
 * Asynchronous on `stream`; no host synchronisation, no allocation; ONE launch whatever G, S, P and the sizes are (none for
 * S = 0); two calls give the same bytes.  This is the one entry of the RLE family that uses an atomic: every crossing of the
 * boundary walk XORs one bit, and an integer XOR does not depend on the order.
 * xy: device doubles, the polygons' x0,y0,x1,y1,... concatenated.  point_offsets: device [P+1], polygon i owns the vertices
 * point_offsets[i] .. point_offsets[i+1]-1.  entry_polys: device [S+1], entry s owns the polygons entry_polys[s] ..
 * entry_polys[s+1]-1; an entry may own none and is then the empty mask (one count, H*W).
 * images_host: HOST [G,3] int64, G <= 64, row g = (H_g, W_g, first entry) with the rules of hgl_rle_decode_group_device: entries
 * run from 0 to S and do not decrease, an image may own none, H*W < 2^31; read before the call returns.  A bad geometry,
 * slot_words < 1 or a rule other than 0 / 1 is HGL_EINVAL and nothing is enqueued.
 * rule 0: the pixels covered by exactly one polygon (the REFER target, data/dataset_refer_bert.py:118-121); rule 1: the pixels
 * covered by at least one (mask.merge / annToMask of a multi-polygon object).
 * slots / table: hgl_rle_encode_device's contract against the entry's own H_g x W_g -- form 0 (the counts) whenever
 * n_counts <= slot_words, form 1 (the column-major bit plane) when ceil(H*W/32) <= slot_words, form 2 otherwise;
 * table = (true n_counts, form, area of the final mask, 0); words beyond what the form defines are not written.
 * status: device [S,4] = (code, sum of the areas of the entry's polygons each on its own -- what hgl_gt_mask_from_polygons
 * returns as area -- saturated at 2^31-1, 0, 0).  code 0: rasterised.  code 2: the entry is refused -- a polygon without a
 * vertex, a coordinate that is NaN or outside (-1e5, 1e5) (the host codec's guard), polygon indices outside [0, P], or a walk
 * of 2^31 steps or more; its table row is (0, 3, 0, 0), its area sum 0 and its slot untouched.
 * ws: hgl_rle_from_polygons_workspace_bytes for the same geometry (HGL_EWORKSPACE when smaller): two bit planes per entry, a
 * third for an entry whose plane of H*W + 1 bits does not fit into 40 KB of LDS.  The query returns 0 for a geometry the call
 * refuses and for S = 0, which needs no workspace and takes ws = NULL. */
size_t hgl_rle_from_polygons_workspace_bytes(const int64_t* images_host, int G, int S, int P);
int hgl_rle_from_polygons_device(const double* xy, const int32_t* point_offsets, int P,
                                 const int32_t* entry_polys, int S,
                                 const int64_t* images_host, int G, int rule,
                                 uint32_t* slots, long long slot_words, int32_t* table, int32_t* status,
                                 void* ws, size_t ws_bytes, void* stream);
/* New masks out of masks that are already encoded (csrc/rle.hip): the device form of rleMerge(R, M, n, intersect)
 * (refer/external/maskApi.c:49-70, mask.merge of refer/external/mask.py) generalised to a vote -- every output entry is a rule
 * over the per-pixel count of its members.  No mask becomes pixels.  Asynchronous on `stream`; no host synchronisation,
 * allocation or atomics; two calls give the same bytes; at most three launches whatever G, S, M and the sizes are, none for S = 0.
 * Source set = (slots_src, slot_words_src, table_src, Ssrc): what hgl_rle_encode_device hands out, forms 0 and 1, with the
 * code 0 / 1 / 2 rules of hgl_rle_decode_device.  Ssrc may be 0 (the set's pointers are then not read).
 * images_host: HOST [G,4] int64, G <= 64, row g = (H_g, W_g, first source entry, first output entry); both entry columns run
 * from 0 to Ssrc / S and do not decrease, an image may own none on either side; H*W < 2^31.  The array is read before the call
 * returns.  Anything else is HGL_EINVAL and nothing is enqueued.
 * members: device [M] int32, absolute source indices (not read when M = 0).  member_offsets: device [S+1] int32; output entry s
 * merges the source entries members[member_offsets[s] .. member_offsets[s+1]-1], k_s of them; a source listed twice counts
 * twice (integer weights).  bounds: device [S,2] int32 = (lo_s, hi_s): a pixel of output s is set iff
 * lo_s <= (number of its members that cover the pixel) <= hi_s.
 *   union         (1, k)          rleMerge(.., 0)
 *   intersection  (k, k)          rleMerge(.., 1)
 *   majority      (k/2 + 1, k)
 *   exactly one   (1, 1)          the REFER target rule of hgl_rle_from_polygons_device
 * (0, 0) gives the complement of the union; k = 0 follows from the formula: all pixels when lo = 0, none otherwise.
 * slots [S, slot_words] / table [S,4]: what hgl_rle_encode_device would write for the merged mask against the entry's own
 * H_g x W_g -- form 0 (the counts) whenever n_counts <= slot_words, form 1 (the column-major bit plane) when they do not fit but
 * ceil(H*W/32) words do, form 2 otherwise; table = (true n_counts, form, area, 0); words beyond what the form defines are
 * not written.
 * status: device [S,4] int32 = (code, k_s, 0, 0).  code 0: merged.  code 1: merged, and at least one member had the decoder's
 * code 1; such a member is used as the decoder decodes it.  code 2: refused -- a member index outside the source entries of the
 * entry's own image, a member of code 2, offsets that step back or leave [0, M] (k_s is then reported as 0), lo < 0 or lo > hi,
 * k_s > 65535; the table row is (0, 3, 0, 0) and the slot is untouched.
 * Limits: M, S, Ssrc < 2^31; the source plane words, sum of n_g * W_g * ceil(H_g / 64), < 2^32, and the merged plane words
 * likewise; fewer than 2^31 blocks.  The outputs must not alias the sources.
 * ws: hgl_rle_merge_workspace_bytes for the same geometry (HGL_EWORKSPACE when smaller): the source set's run starts, status
 * and bit planes, and one bit plane per output entry (the merged plane is written once and read by both sweeps of the run
 * writer).  The query returns 0 for a geometry the call refuses and for S = 0, which needs no workspace and takes ws = NULL. */
size_t hgl_rle_merge_workspace_bytes(const int64_t* images_host, int G, int Ssrc, long long slot_words_src, int S, int M);
int hgl_rle_merge_device(const uint32_t* slots_src, long long slot_words_src, const int32_t* table_src, int Ssrc,
                         const int64_t* images_host, int G, const int32_t* members, int M,
                         const int32_t* member_offsets, const int32_t* bounds,
                         uint32_t* slots, long long slot_words, int32_t* table, int S, int32_t* status,
                         void* ws, size_t ws_bytes, void* stream);
/* Greedy suppression by MASK overlap inside one encoded set, image by image (csrc/rle.hip): the device form of
 * rleNms(dt, n, keep, thr) (refer/external/maskApi.c:98-107, mask.nms of pycocotools) with the exact intersection of every pair
 * in place of rleIou's box pre-filter, a second metric, and the order of the box NMS.  No mask becomes pixels.  Asynchronous on
 * `stream`; no host synchronisation, allocation or atomics; two calls give the same bytes; SIX launches whatever G and the
 * sizes are, none for S = 0 (out_n is then not written).
 * Set = (slots, slot_words, table, S): what hgl_rle_encode_device hands out, forms 0 and 1, with the code 0 / 1 / 2 rules of
 * hgl_rle_decode_device; an entry of code 1 counts as decoded.
 * images_host: HOST [G,3] int64, G <= 64, row g = (H_g, W_g, first entry e_g) with the rules of hgl_rle_from_polygons_device:
 * entries run from 0 to S and do not decrease, an image may own none, H*W < 2^31; read before the call returns.
 * HGL_EINVAL, and nothing is enqueued: a bad geometry; an image that owns more than 4096 entries (its pair counts are n^2 int32
 * per split in the workspace); a NaN thr; a metric other than 0 / 1.
 * Order of the walk within an image.  scores == NULL: the given order, rleNms's.  Otherwise device [S] float and the order of
 * hgl_nms: descending score, the original index breaks ties, a NaN ranks above every number.
 * Ratio of a pair with I common pixels: 0 when I = 0; metric 0 (IoU): (double)I / (double)(area_i + area_j - I); metric 1
 * (containment): (double)I / (double)min(area_i, area_j), which drops a part nested in a whole, or the whole, whichever ranks
 * later.  An entry is kept iff no kept entry before it in the order has ratio > thr with it, compared in double as
 * maskApi.c:104.  An empty mask never suppresses and is never suppressed.
 * out_idx: device [S] int32; from position e_g on, the kept entries of image g in walk order, as indices into the image's list;
 * the positions behind the out_n[g] kept ones are not written.  out_n: device [G] int32, the kept entries per image -- the shape
 * hgl_nms_segments returns.
 * result: device [S,4] int32 = (code, area, rank, by).  code and area as the decoder's status; rank = the entry's position in
 * the walk; by = the index within the image of the kept entry of lowest rank that suppressed it, -1 for a kept entry.  An entry
 * of code 2 has rank -1 and by -1, is not listed in out_idx and suppresses nobody.
 * Limits: the plane words, sum of n_g * W_g * ceil(H_g / 64), < 2^32.
 * ws: hgl_rle_nms_workspace_bytes for the same geometry (HGL_EWORKSPACE when smaller): the set's run starts, status, boxes and
 * bit planes (built once, both sides of the pair count), the partial counts as in hgl_rle_match_device (only the tiles that hold
 * a pair i < j are counted), the walk order and n_g * ceil(n_g / 64) 64-bit suppression words per image.  The query returns 0
 * for a geometry the call refuses and for S = 0, which needs no workspace and takes ws = NULL. */
size_t hgl_rle_nms_workspace_bytes(const int64_t* images_host, int G, int S, long long slot_words);
int hgl_rle_nms_device(const uint32_t* slots, long long slot_words, const int32_t* table, int S,
                       const int64_t* images_host, int G, const float* scores, double thr, int metric,
                       int32_t* out_idx, int32_t* out_n, int32_t* result,
                       void* ws, size_t ws_bytes, void* stream);
/* The kept entries of an encoded set, compacted image by image into a second, dense set (csrc/rle.hip): what stands between a
 * stage that decides which entries survive (hgl_rle_nms_device, or any caller's flags) and a stage that takes a dense set (the
 * decoders).  Stable: survivors keep their stored order.  Nothing is decoded; an entry moves as the words its table row defines.
 * Asynchronous on `stream`; no host synchronisation, allocation, workspace or atomics; two calls give the same bytes; TWO
 * launches whatever G and the sizes are, none for S = 0 (out_n is then not written).
 * Set = (slots, slot_words, table, S): as everywhere in the family, forms 0 and 1, with the code 0 / 1 / 2 rules of
 * hgl_rle_decode_device.
 * images_host: HOST [G,4] int64, G <= 64, row g = (H_g, W_g, first entry e_g, max_keep_g); the first three columns with the
 * rules (and the limits) of hgl_rle_nms_device, at most 4096 entries per image; max_keep_g < 0: no limit, otherwise only the
 * first max_keep_g kept entries of the image, in stored order, survive.  Read before the call returns.
 * Exactly one of keep and nms_result is non-NULL.  keep: device [S] bytes, nonzero = kept.  nms_result: the result [S,4] rows of
 * hgl_rle_nms_device; an entry is kept iff its code is 0 or 1 and by == -1.
 * cols: device [C,S] 4-byte words, 0 <= C <= 8 (NULL for C = 0): side columns that travel with the entries, moved as bits.
 * HGL_EINVAL, and nothing is enqueued: a bad geometry; slot_words < 0 or >= 2^31, or 0 with S > 0 (a placeholder is one word); C
 * outside 0 .. 8; both or neither of keep / nms_result; out_slots overlapping slots or out_table overlapping table (the other
 * outputs must not overlap an input either; that is the caller's to keep).
 * Outputs, with k_g survivors in image g.  Position e_g + p, p < k_g, holds the p-th survivor in stored order: out_table row =
 * its row, whole; out_slots = exactly the words its form defines (n_counts in form 0, ceil(H*W/32) in form 1), nothing beyond
 * them; a kept entry whose row describes no mask (code 2; reachable through keep only) has its row copied and no slot word
 * written; out_src = its index within the image's list; out_cols[c] = cols[c] of it.  Positions p >= k_g of the image's range
 * receive a PLACEHOLDER: row (1, 0, 0, 0), slot word 0 = H_g*W_g (nothing behind it), out_src = -1, columns 0 -- a legal, empty,
 * code-0 mask for every consumer in the family, so a decode can run over the original layout with no count known on the host.
 * out_n: device [G] int32 = k_g.  out_slots [S, slot_words], out_table [S,4], out_cols [C,S], out_src [S].
 * The slots move 16 bytes a lane when slot_words % 4 == 0 and both slot buffers are 16-byte aligned, 4 bytes otherwise. */
int hgl_rle_select_device(const uint32_t* slots, long long slot_words, const int32_t* table, int S,
                          const int64_t* images_host, int G,
                          const uint8_t* keep, const int32_t* nms_result,
                          const uint32_t* cols, int C,
                          uint32_t* out_slots, int32_t* out_table, uint32_t* out_cols,
                          int32_t* out_src, int32_t* out_n, void* stream);
/* remove_small_regions (utils/amg.py:267-291) on an encoded set (csrc/rle_clean.hip): small holes filled, small islands dropped,
 * every entry encoded again with its box -- the step of postprocess_small_regions that hgl_remove_small_regions /
 * hgl_remove_small_regions_boxes take on byte masks, without the bytes.  No [S,H,W] byte array and no per-pixel label exists
 * anywhere: the components are found on column segments (maximal vertical stretches of equal pixels inside one column).
 * Asynchronous on `stream`; no host synchronisation or allocation; two calls give the same bytes; THREE launches whatever G, S and
 * the sizes are, none for S = 0.  Integer atomics only where the order cannot show: atomicMin on the union-find's parent links
 * (link by minimum), atomicAdd on a component's area, atomicMin on its raster key.
 * Set = (slots, slot_words, table, S): as everywhere in the family, forms 0 and 1, with the code 0 / 1 / 2 rules of
 * hgl_rle_decode_device; an entry of code 1 counts as decoded (clipped as the decoder clips).
 * images_host: HOST [G,3] int64, G <= 64, row g = (H_g, W_g, first entry e_g) with the rules (and the limits) of
 * hgl_rle_nms_device; read before the call returns.
 * modes: bit 0 = holes, bit 1 = islands; both: holes first, then islands ON THE RESULT of the hole filling (SAM's order: a filled
 * hole can join two islands, and the island pass sees the joined one).
 * HGL_EINVAL, and nothing is enqueued: a bad geometry; slot_words or out_slot_words outside 0 .. 2^31 - 1; area_thresh < 0; modes
 * outside 1 .. 3; seg_cap outside 1 .. 2^31 - 1.
 * Rule: 8-connected components of the foreground are islands, 8-connected components of the complement are holes, the ones
 * that touch the border included; a component of area < area_thresh is removed / filled; in islands mode, when every component
 * is small, the largest survives, the first in raster (row-major) order of its first pixel among equals.  Padding bits beyond
 * H in a column word are neither foreground nor background.
 * out_slots [S, out_slot_words] / out_table [S,4]: what hgl_rle_encode_device writes for the cleaned mask at H_g x W_g: form 0
 * whenever the counts fit out_slot_words, form 1 when they do not but the plane does, else form 2; words beyond what the form
 * defines are not written.  With nothing to remove this is the canonical re-encoding of the input (zero-length runs gone).
 * boxes_xyxy: device [S,4] int32, the hgl_mask_boxes rule for the cleaned mask.
 * result: device [S,4] int32 = (code, area after, changed, area before); changed bit 0: the holes pass found a small component,
 * bit 1: the islands pass did (also when it was the one island that stays) -- the `changed` flags of the pixel entries.
 * Code 2 (the slot holds no mask): table row (0, 3, 0, 0), slot untouched, box zeros, result (2, 0, 0, 0).
 * seg_cap: the column segments per entry and colour the workspace is sized for.  A form-0 entry of n counts has at most
 * (n + 1) / 2 + W of either colour, any entry at most W * ceil(H / 2).  An entry that needs more, in a pass that runs, is refused
 * with code 3 and the outputs of code 2 -- never truncated.
 * ws: hgl_rle_clean_workspace_bytes for the same geometry (HGL_EWORKSPACE when smaller): the set's run starts, status and bit
 * planes, one 32-bit word per 64-bit plane word, and 5 * min(seg_cap, the largest W * ceil(H / 2)) 32-bit words per entry.  The
 * query returns 0 for a geometry the call refuses and for S = 0, which needs no workspace and takes ws = NULL.
 * The outputs must not overlap the inputs. */
size_t hgl_rle_clean_workspace_bytes(const int64_t* images_host, int G, int S, long long slot_words, long long seg_cap);
int hgl_rle_clean_device(const uint32_t* slots, long long slot_words, const int32_t* table, int S,
                         const int64_t* images_host, int G, int area_thresh, int modes, long long seg_cap,
                         uint32_t* out_slots, long long out_slot_words, int32_t* out_table,
                         int32_t* boxes_xyxy, int32_t* result, void* ws, size_t ws_bytes, void* stream);
/* COCO's compressed RLE strings written and read on the DEVICE (csrc/rle_string.hip; the arithmetic of a count and of a
 * character group once, in csrc/rle_string.h): the two ends of an encoded set's life, in place of hgl_rle_to_string per
 * record (refer/external/maskApi.c:203-216 rleToString, what coco_encode_rle of utils/amg.py:294-300 ends in) and of
 * hgl_rle_from_string per record (maskApi.c:217-230 rleFrString).  Asynchronous on `stream`; no host synchronisation,
 * allocation or atomics; two calls give the same bytes; no workspace.
 * hgl_rle_to_strings_device: THREE launches whatever S is (lengths, one scan over the S lengths, write); one for S = 0.
 * Set = (slots, slot_words, table, S) as hgl_rle_encode_device writes it.  offsets: device int64 [S+1]; offsets[s] is where
 * entry s's string begins in a buffer without limit -- the strings are packed in entry order with no separator and no
 * terminator -- and offsets[S] the true total, BOTH ALSO WHEN cap IS SMALLER (the size-query convention of hgl_rle_to_string).
 * status: device int32 [S]; the codes other than 0 contribute length 0:
 *   0  the string was written: form 0 and 0 <= n_counts <= slot_words (n_counts == 0 gives the empty string); its bytes equal
 *      hgl_rle_to_string of the slot's counts
 *   1  the entry is in form 1: the slot holds the bit plane, its counts are not in memory; nothing is written, the caller
 *      finishes such an entry on the host
 *   2  no mask: form 2 or 3 or any other form value, n_counts < 0, n_counts > slot_words
 *   3  the string is good (it has its length in offsets) but offsets[s+1] > cap: no byte of it is written
 * bytes: device uint8 [cap] (may be NULL when cap is 0).  No byte outside the code-0 extents is written, the bytes between
 * offsets[S] and cap included.  Neighbouring strings meet at any byte alignment: the kernel stores bytes, never words.
 * hgl_rle_from_strings_device: ONE launch whatever S is, none for S = 0.  bytes: device uint8 [total_bytes], total_bytes
 * < 2^31; offsets: device int64 [S+1], entry s's string is bytes[offsets[s] .. offsets[s+1]).  A byte b is read as
 * c = (uint8)(b - 48), of which only c & 31 and c & 32 count (bytes >= 112 are accepted, as the host accepts them); the host
 * parser stops at a NUL byte, the device does not: a string with one is outside the equality with the host.
 * slots [S, slot_words] / table [S,4] receive what hgl_rle_encode_device would have written in form 0; status: device int32
 * [S,4] = (code, n_counts, 0, 0):
 *   0  the slot holds the n_counts counts, the table row is (n_counts, 0, 0, 0); words beyond n_counts are not written; the
 *      empty string is code 0 with n_counts 0
 *   1  n_counts > slot_words: the status carries the true n_counts, the row is (n_counts, 2, 0, 0), the slot is untouched
 *   2  truncated: the string ends inside a group of at most seven characters
 *   3  long: a group has an eighth character in the string (the first offending group in string order decides: a long group
 *      lies before the end, so it wins over a truncated end)
 *   4  offsets[s] > offsets[s+1], or the extent is not inside [0, total_bytes]
 * Codes 2 to 4: row (0, 2, 0, 0), slot untouched, n_counts 0 in the status -- the decoders see "no mask". */
int hgl_rle_to_strings_device(const uint32_t* slots, long long slot_words, const int32_t* table, int S, uint8_t* bytes,
                              long long cap, int64_t* offsets, int32_t* status, void* stream);
int hgl_rle_from_strings_device(const uint8_t* bytes, long long total_bytes, const int64_t* offsets, int S, uint32_t* slots,
                                long long slot_words, int32_t* table, int32_t* status, void* stream);
/* Encoded masks painted onto RGB canvases on the DEVICE (csrc/rle_paint.hip): any ordered selection of an encoded set composited
 * over the images it belongs to, for a whole group of images of different sizes -- the paint-side sibling of
 * hgl_rle_decode_group_device.  It works from the runs: no byte mask exists and nothing is read back.  Asynchronous on `stream`; no
 * host synchronisation, allocation or atomics; two calls give the same bytes; FOUR launches whatever G, K and the sizes are
 * (starts and planes of the listed entries, edge counts, paint), ONE for K = 0, which still copies the bases.
 * Set = (slots, slot_words, table, S): what hgl_rle_encode_device hands out, forms 0 and 1, with the code 0 / 1 / 2 rules of
 * hgl_rle_decode_device.  S may be 0 (the set's pointers are then not read).
 * images_host: HOST [G,5] int64, G <= 64, row g = (H_g, W_g, first entry e_g, first list position k_g, pixel offset p_g).  Entries
 * with the rules of hgl_rle_decode_group_device: from 0 to S without a step back, an image may own none, H*W < 2^31.  List
 * positions from 0 to K without a step back; an image may own none and is then a plain copy of its base.  Image g's canvas is
 * H_g*W_g RGB pixels, row-major HWC: it sits at byte 3*p_g of base and of out and at element p_g of labels; the extents
 * [p_g, p_g + H_g*W_g) must lie inside [0, canvas_pixels) and must not overlap; out must not overlap base.  slot_words outside
 * 0 .. 2^31 - 1, a negative S or K and anything else above is HGL_EINVAL with the reason in hgl_last_error() and nothing is enqueued.
 * The array is read before the call returns.
 * order: device [K] int32.  Position t of image g paints entry e_g + order[t] when 0 <= order[t] < n_g; the same entry may be
 * listed several times.  Only listed entries are staged as planes: one winner out of 64 proposals touches one entry.
 * style: device [K,4] uint32, one row per position.  Word 0: the fill colour 0x00RRGGBB, bit 24 = fill, bit 25 = outline; words 1
 * and 2: the bit patterns of the fp32 weights a and b; word 3: the outline colour 0x00RRGGBB.
 * Pixel rule.  The positions of an image are applied in list order, each on the result of the one before.  M = the mask the
 * decoder would write for the entry; edge = M & ~(up & down & left & right), a neighbour outside the image counting as clear.
 * Fill: every channel c of every pixel of M becomes sat_u8(rint(f32(c)*a + f32(colour_c)*b)) -- both products and the sum each
 * rounded to fp32, no fused multiply-add, rint to nearest even, the clamp to [0, 255], a NaN (inf - inf) to 0.  Outline:
 * afterwards every pixel of edge becomes the outline colour.  A position with neither flag paints nothing.
 * base: device, 3*canvas_pixels bytes, or NULL for black canvases.  out: device, 3*canvas_pixels bytes.  labels: device
 * [canvas_pixels] int32 or NULL: the image-local list position (t - k_g) of the last position that changed the pixel (fill on M,
 * outline on edge), -1 for none.  Every byte of every extent of out and, when given, every element of every extent of labels is
 * written; nothing outside the extents is.
 * status: device [K,4] int32 = (code, area, edge pixels, 0): area and edge pixels are those of M, whatever the flags.
 *   0 / 1 / 2   as the decoder's status; a code-2 position paints nothing: (2, 0, 0, 0)
 *   3           order[t] is outside the image's entries: (3, 0, 0, 0)
 *   4           a or b is not finite; the position paints nothing: (4, area, 0, 0)
 * ws: hgl_rle_paint_workspace_bytes for the same geometry (HGL_EWORKSPACE when smaller): one row of run starts and one set of
 * bit planes per list position.  The query returns 0 for a geometry the call refuses and for K = 0, which takes ws = NULL. */
size_t hgl_rle_paint_workspace_bytes(const int64_t* images_host, int G, int S, long long slot_words, int K, long long canvas_pixels);
int hgl_rle_paint_device(const uint32_t* slots, long long slot_words, const int32_t* table, int S, const int32_t* order,
                         const uint32_t* style, int K, const int64_t* images_host, int G, const uint8_t* base, uint8_t* out,
                         long long canvas_pixels, int32_t* labels, int32_t* status, void* ws, size_t ws_bytes, void* stream);
/* Heat-maps painted onto RGB canvases on the DEVICE (csrc/rle_paint.hip): the guided map of the scoring tail -- min-max
 * normalised, times the direction weight of gen_dir_mask -- turned into colours with a weight per pixel, for a whole group of maps
 * of different sizes, with nothing read back.  Asynchronous on `stream`; no host synchronisation, allocation or atomics; two
 * calls give the same bytes; THREE launches whatever M and the sizes are (min/max partials; peak partials; paint).
 * maps_host: HOST [M,6] int64, 1 <= M <= 64, row m = (H_m, W_m, dirflag, h_m, b_m, p_m); H, W >= 1, H*W < 2^31; dirflag 0 none,
 * 1 left, 2 right, 3 middle, as for hgl_coherence_scores.  Map m is H*W fp32 values, row-major, at element h_m of heat
 * [heat_elems]; its base image is H*W RGB pixels, row-major HWC, at byte 3*b_m of base; its canvas sits at byte 3*p_m of out and
 * at element p_m of levels.  Heat extents and base extents are only read: they may coincide or overlap (several sentences over
 * one image, one map under two directions).  The extents [p_m, p_m + H*W) must lie inside [0, canvas_pixels) and must not
 * overlap; out must not overlap the bytes of base that the maps name.  Anything else is HGL_EINVAL with the reason in
 * hgl_last_error() and nothing is enqueued.  The array is read before the call returns.
 * ramp: device [256,3] uint32, row L = (colour 0x00RRGGBB, the fp32 bits of a_L, the fp32 bits of b_L).
 * base: device, or NULL for black.  out: device, 3*canvas_pixels bytes.  levels: device uint8 [canvas_pixels], or NULL.
 * Pixel rule, every operation rounded to fp32 on its own (no fused multiply-add).  mn, mx = the map's minimum and maximum;
 * n = (x - mn) / (mx - mn), IEEE division; g = n * w(col), w the column weight of gen_dir_mask(dirflag, H, W) -- the very bits
 * the coherence pooling multiplies with; peak = max g; t = g / peak; L = (int)rint(t * 255), to nearest even; every channel c of
 * the pixel becomes sat_u8(rint(f32(base_c)*a_L + f32(colour_c(L))*b_L)), the fill rule of hgl_rle_paint_device (both products and
 * the sum rounded, the clamp, a NaN to 0); levels gets L.  The scorer's division by the mean scales g by a constant and cancels
 * in g / peak.  Minimum and maximum do not depend on the order they are taken in: every byte is defined by this rule alone.
 * status: device [M,4] int32 = (code, bits of mn, bits of mx, bits of peak):
 *   0   painted
 *   1   mx == mn: a flat map
 *   2   a value is NaN or +-inf, or mx - mn is not finite
 *   3   peak == 0: all of the map's weight lies where the direction weight is 0 (W = 1 under `right`)
 * A map with a code other than 0 is a plain copy of its base with levels 0 and status (code, 0, 0, 0).  Every byte of every extent
 * of out and, when given, of levels is written; nothing outside the extents is.
 * ws: hgl_heat_paint_workspace_bytes for the same geometry (HGL_EWORKSPACE when smaller): a (min, max) pair and a peak per
 * workgroup -- a map of n pixels takes ceil(n / 4096) of them, at most 256 -- and four words per map.  The query returns 0 for a
 * geometry the call refuses. */
size_t hgl_heat_paint_workspace_bytes(const int64_t* maps_host, int M, long long heat_elems, long long canvas_pixels);
int hgl_heat_paint_device(const float* heat, long long heat_elems, const int64_t* maps_host, int M, const uint32_t* ramp,
                          const uint8_t* base, uint8_t* out, long long canvas_pixels, uint8_t* levels, int32_t* status,
                          void* ws, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HYBRIDGL_H */
