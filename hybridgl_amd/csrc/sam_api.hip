// Host orchestration of the SAM image encoder and prompt/mask decoder behind the C ABI.
//   hgl_sam_encode(_batch)  == Sam.preprocess + ImageEncoderViT.forward
//                              (modeling/sam.py:164-174, modeling/image_encoder.py:106-116)
//   hgl_sam_decode_*        == PromptEncoder(points / labelled points and boxes / mask inputs) + MaskDecoder
//                              (predictor.py:222-235, modeling/mask_decoder.py:71-149), for the prompts of one or several images
// This file decides and launches.  In the split-fp16 modes the contractions are the GEMMs of gemm_f16x3.hip, the attention of
// attention_ps.hip / attention.hip and the fused decoder stages of sam_decoder_fused.hip / sam_decoder_t2i.hip; in f32 mode, and
// wherever a weight has no registered split halves, the fp32 MFMA GEMM / attention of gemm.hip / attention.hip.  Which of them a
// call takes is decided ONCE, before anything is enqueued: per encoder block by enc_block_route, per decoder call by dec_route
// (DecRoute); the code below those two reads their fields and re-derives nothing.
// Tokens stay NHWC ([g*g, C] rows) end to end; the reference's NCHW permutes disappear.
#include "hgl_common.h"
#include <stdlib.h>
#include <math.h>

namespace {

struct EncPlan {
  float *img, *cols, *X, *H, *Hw, *QKV, *O, *P, *F, *Th, *Tw, *relh, *relw, *neckA, *neckB, *cols3;
  int *pad_of, *tok_of, *pad_list, *pad_count;   // row maps of the padded window partition (win_maps_kernel)
  int n_pad_max;
  int nb;                                         // images stacked along the token rows
};

bool carve_enc(HglArena& ar, const HglSamEncoderW* w, int nb, EncPlan& p) {
  const int D = w->embed_dim, S = w->img_size, g = S / w->patch, C = w->out_chans;
  const size_t T = (size_t)nb * g * g;
  // windowed blocks pad the grid up to a multiple of the window size
  size_t Tw_max = T;
  int rl_max = 0, size_max = 0;   // longest rel-pos table; largest attention grid side (a window may be larger than the grid)
  for (int i = 0; i < w->depth; ++i) {
    const int ws = w->blocks[i].window;
    if (ws > 0) {
      const size_t nw = (g + ws - 1) / ws;
      Tw_max = Tw_max > nb * nw * nw * ws * ws ? Tw_max : nb * nw * nw * ws * ws;
    }
    rl_max = rl_max > w->blocks[i].rel_len ? rl_max : w->blocks[i].rel_len;
    size_max = size_max > (ws > 0 ? ws : g) ? size_max : (ws > 0 ? ws : g);
  }
  p.nb = nb;
  p.img = ar.take<float>((size_t)nb * 3 * S * S);
  p.cols = ar.take<float>(T * 3 * w->patch * w->patch);
  p.X = ar.take<float>(T * D);
  p.H = ar.take<float>(T * D);
  p.Hw = ar.take<float>(Tw_max * D);
  p.QKV = ar.take<float>(Tw_max * 3 * D);
  p.O = ar.take<float>(Tw_max * D);
  p.P = ar.take<float>(Tw_max * D);
  p.F = ar.take<float>(T * 4 * D);
  p.Th = ar.take<float>((size_t)w->heads * Tw_max * rl_max);
  p.Tw = ar.take<float>((size_t)w->heads * Tw_max * rl_max);
  p.relh = ar.take<float>((size_t)w->heads * Tw_max * size_max);
  p.relw = ar.take<float>((size_t)w->heads * Tw_max * size_max);
  p.neckA = ar.take<float>(T * C);
  p.neckB = ar.take<float>(T * C);
  p.cols3 = ar.take<float>(T * C * 9);
  p.pad_of = ar.take<int>(T);
  p.tok_of = ar.take<int>(T);
  p.n_pad_max = (int)(Tw_max - T);
  p.pad_list = ar.take<int>(Tw_max - T + 1);
  p.pad_count = ar.take<int>(1);
  return ar.ok();
}

bool valid_enc(const HglSamEncoderW* w) {
  return w && w->embed_dim > 0 && w->depth > 0 && w->heads > 0 && w->img_size > 0 && w->patch > 0 &&
         w->out_chans > 0 && w->img_size % w->patch == 0 && w->embed_dim % w->heads == 0 &&
         (w->embed_dim & 3) == 0 && w->patch_w && w->patch_b && w->pos_embed && w->blocks && w->neck0_w &&
         w->neck1_w && w->neck1_b && w->neck2_w && w->neck3_w && w->neck3_b;
}

// ---- one encoder block: Block.forward (modeling/image_encoder.py:166-182) ----
enum EncAttn {
  ENC_ATTN_PS_WIN,      // q | k | v as fp16 hi / lo planes, 14 x 14 windows: the kernel takes the rel-pos terms from the registered tables
  ENC_ATTN_PS_GLOBAL,   // the same planes, the whole 64 x 64 grid: the rel-pos terms as tensors, from the split q
  ENC_ATTN_WIN14,       // fp32 qkv, 14 x 14 windows at head dim 80: the kernel computes the decomposed rel-pos terms itself
  ENC_ATTN_TABLES       // fp32 qkv, decomposed rel-pos tables first, then the generic attention
};

// The geometry of a block and everything that is decided about its launches
struct EncBlockRoute {
  int D, g, heads, hd;
  int T1, T;            // tokens of one image; token rows of the batch (images stacked along the rows)
  int ws, size, nw;     // window (0: global attention), attention grid side, windows per grid side
  int B1, B;            // windows of one image (1 for global attention), of the batch
  int S, M1, M;         // tokens per window; padded rows of one image, of the batch
  int L;                // rel-pos table length
  bool x3;              // the split-fp16 path: every GEMM operand activation exists only as fp16 hi | lo planes
  EncAttn attn;
  bool gather;          // the windowed GEMMs read and write the real tokens only (the window does not divide the grid)
  bool planes;          // the in-projection writes q | k | v as fp16 hi / lo planes (same bytes as the fp32 tensor)
  int ks;               // split-K factor of mlp.lin2 (0: whole rounds + a tail where that pays)
};

// q | k | v of the block's B windows, as fp32 or as the fp16 hi | lo planes aliasing the same buffer
HglAct enc_qkv(const EncPlan& p, const EncBlockRoute& r, bool planes) { return hgl_act(p.QKV, (size_t)r.M * 3 * r.D, planes); }
// the window buffer as an operand: the in-projection's input in window order and, on the split path, the attention's output
HglAct enc_win(const EncPlan& p, const EncBlockRoute& r, bool planes) { return hgl_act(p.Hw, (size_t)r.M * r.D, planes); }

// the attention of the B windows (or whole grids) as `kind` runs it: on p.QKV as planes or as fp32 -> the planes of the window
// buffer (x3) or p.O (fp32); the rel-pos terms from the block's tables or as the tensors p.relh / p.relw that enc_attention
// computes first
HglAttn enc_attn(const HglSamBlockW& b, const EncPlan& p, const EncBlockRoute& r, EncAttn kind) {
  const bool planes = kind == ENC_ATTN_PS_WIN || kind == ENC_ATTN_PS_GLOBAL;
  const HglAct Q = enc_qkv(p, r, planes), Ow = enc_win(p, r, true);
  HglAttn d = planes ? hgl_attn_packed_planes(Q.hi, Q.lo, r.B, r.heads, r.S, r.hd) : hgl_attn_packed(p.QKV, r.B, r.heads, r.S, r.hd);
  d.out = r.x3 ? nullptr : p.O, d.out_hi = Ow.hi, d.out_lo = Ow.lo;   // (the pair is named in both forms; read when out is null)
  if (kind == ENC_ATTN_PS_WIN || kind == ENC_ATTN_WIN14) d.tab_h = b.rel_pos_h, d.tab_w = b.rel_pos_w;
  else d.rel_h = p.relh, d.rel_w = p.relw, d.kh = d.kw = r.size;
  return d;
}

int enc_block_route(const HglSamEncoderW* w, const HglSamBlockW& b, const EncPlan& p, EncBlockRoute& r) {
  const int nb = p.nb;
  r.D = w->embed_dim, r.g = w->img_size / w->patch, r.heads = w->heads, r.hd = r.D / r.heads;
  r.T1 = r.g * r.g, r.T = nb * r.T1;
  r.ws = b.window, r.size = r.ws > 0 ? r.ws : r.g, r.nw = r.ws > 0 ? (r.g + r.ws - 1) / r.ws : 1;
  r.B1 = r.nw * r.nw, r.B = nb * r.B1;
  r.S = r.size * r.size, r.M1 = r.B1 * r.S, r.M = r.B * r.S;
  r.L = b.rel_len;
  HGL_REQUIRE(r.L == 2 * r.size - 1, "sam_encode: rel_pos length %d does not match attention size %d", r.L, r.size);
  const int D = r.D;
  r.x3 = hgl_use_x3(b.qkv_w, D) && hgl_use_x3(b.proj_w, D) && hgl_use_x3(b.lin1_w, D) && hgl_use_x3(b.lin2_w, 4 * D) &&
         (D % 256) == 0;
  static const int padskip = HGL_DIAG_SWITCH("HGL_SAM_PADSKIP", 1);   // 0: the windowed GEMMs run over the padded rows as well (A/B timing)
  // only the real tokens go through the windowed GEMMs (16 % fewer rows at 64x64 / 14x14)
  r.gather = r.x3 && r.ws > 0 && r.M > r.T && padskip;
  static const int ps_glob_on = HGL_DIAG_SWITCH("HGL_ATTN_PS_GLOBAL", 1);   // 0: the global blocks keep the fp32-input kernels (A/B timing)
  // each candidate is hgl_attention_route's answer for the descriptor the block would launch with (plane distance + one item's
  // rows within 32 bits, shapes, registered tables, switches), taken here because the in-projection writes planes OR fp32
  const auto serves = [&](EncAttn kind, HglAttnRoute family) { return hgl_attention_route(enc_attn(b, p, r, kind)) == family; };
  r.attn = ENC_ATTN_TABLES;
  if (r.x3 && r.ws == 14 && serves(ENC_ATTN_PS_WIN, HGL_ATTN_PS_WIN)) r.attn = ENC_ATTN_PS_WIN;
  else if (r.x3 && r.ws == 0 && r.size == 64 && ps_glob_on && serves(ENC_ATTN_PS_GLOBAL, HGL_ATTN_PS_RELT)) r.attn = ENC_ATTN_PS_GLOBAL;
  else if (r.x3 && r.ws == 14 && serves(ENC_ATTN_WIN14, HGL_ATTN_WIN14)) r.attn = ENC_ATTN_WIN14;
  r.planes = r.attn == ENC_ATTN_PS_WIN || r.attn == ENC_ATTN_PS_GLOBAL;
  // mlp.lin2: few output tiles, K = 4D -> split-K over the idle CUs; the partial sums borrow the qkv buffer
  static const int splitk_on = HGL_DIAG_SWITCH("HGL_SAM_SPLITK", 1);   // 0 disables (A/B timing)
  const int ks = r.x3 && splitk_on ? hgl_gemm_f16x3_splitk_factor(r.T, D, 4 * D) : 1;
  r.ks = ks > 1 && (size_t)ks * r.T * D <= (size_t)r.M * 3 * D ? ks : 0;   // its slices fit the qkv buffer
  return HGL_OK;
}

// The rel-pos producer: the decomposed terms rel_h / rel_w [B*heads, S, size] from the UNSCALED q (image_encoder.py:351-354) of
// B windows (or whole grids) of S = size * size tokens.  q as the fp16 hi | lo planes of the split in-projection (q_hi / q_lo,
// ldq in halfs; qkv null) or as fp32 rows (qkv, ldq in floats).  The ONE place that picks the producer -- enc_attention and the
// exported hgl_sam_relpos_tables both call it; which kernel a launcher below runs (matrix cores or VALU) is that launcher's.
// Th / Tw: [heads][B*S][2*size-1] floats each, the products of the generic path.
int enc_relpos_tables(const float* qkv, const void* q_hi, const void* q_lo, int ldq, int B, int heads, int S, int size, int hd,
                      const float* Rh, const float* Rw, float* rel_h, float* rel_w, float* Th, float* Tw, hipStream_t st) {
  if (q_hi || q_lo) return hgl_launch_relpos_split(q_hi, q_lo, ldq, B, heads, S, size, hd, Rh, Rw, rel_h, rel_w, st);
  // the direct kernels hold a query's head in registers (head dim 64 / 80) and store its terms in pairs (even sizes) from a
  // table of at most 127 rows in LDS
  if ((hd == 80 || hd == 64) && (size & 1) == 0 && size <= 64)
    return hgl_launch_relpos_direct(qkv, ldq, B, heads, S, size, hd, Rh, Rw, rel_h, rel_w, st);
  // every other head dim and size: q . rel_pos[r] for every r as a batched GEMM, then gathered per (q, k)
  const int M = B * S, L = 2 * size - 1;
  HglGemm rel = hgl_gemm_linear(qkv, Rh, nullptr, Th, M, L, hd);    // one batch per head: q's columns of that head
  rel.lda = ldq, rel.batch = heads, rel.sA = hd, rel.sC = (long long)M * L;
  HGL_TRY(hgl_launch_gemm(rel, st));
  rel.W = Rw, rel.C = Tw;
  HGL_TRY(hgl_launch_gemm(rel, st));
  HGL_TRY(hgl_launch_relpos_gather(Th, B, heads, S, size, L, 0, rel_h, st));
  return hgl_launch_relpos_gather(Tw, B, heads, S, size, L, 1, rel_w, st);
}

// attention of the B windows (or whole grids): the rel-pos producer where r.attn takes the terms as tensors, then the kernel the
// route named
int enc_attention(const HglSamBlockW& b, const EncPlan& p, const EncBlockRoute& r, hipStream_t st) {
  if (r.attn == ENC_ATTN_PS_GLOBAL || r.attn == ENC_ATTN_TABLES) {
    const HglAct Q = enc_qkv(p, r, r.attn == ENC_ATTN_PS_GLOBAL);
    HGL_TRY(enc_relpos_tables(Q.f32, Q.hi, Q.lo, 3 * r.D, r.B, r.heads, r.S, r.size, r.hd, b.rel_pos_h, b.rel_pos_w, p.relh, p.relw, p.Th,
                              p.Tw, st));
  }
  // f16x3: the attention writes its output as the fp16 hi+lo pair the projection reads
  return hgl_launch_attention(enc_attn(b, p, r, r.attn), st);
}

// The block, once: the GEMM operand activations are fp32 rows of the plan's buffers or -- r.x3 -- fp16 hi | lo planes aliasing
// the same buffers; what else differs between the routes is a condition on r where it differs
int enc_block(const HglSamEncoderW* w, const HglSamBlockW& b, const EncPlan& p, hipStream_t st) {
  EncBlockRoute r;
  HGL_TRY(enc_block_route(w, b, p, r));
  const int D = r.D, T = r.T, M = r.M, ws = r.ws;
  const HglAct Hw = enc_win(p, r, r.x3), H = hgl_act(p.H, (size_t)T * D, r.x3), F = hgl_act(p.F, (size_t)T * 4 * D, r.x3);
  // norm1 -> the in-projection's input: in window order (the split path writes there for global attention as well)
  const HglAct& in = r.x3 || ws > 0 ? Hw : H;
  if (r.gather) {
    // the real tokens written straight to their rows of the padded window layout (the pad rows are never read: the GEMMs
    // below gather the real tokens only)
    HGL_TRY(hgl_launch_layernorm_split_maps(p.X, b.norm1_w, b.norm1_b, Hw.hi, Hw.lo, T, D, 1e-6f, p.tok_of, p.pad_of, st));
  } else if (ws > 0) {
    HGL_TRY(hgl_launch_layernorm(p.X, b.norm1_w, b.norm1_b, p.H, T, D, 1e-6f, st));
    for (int i = 0; i < p.nb; ++i) {
      const float* h = p.H + (size_t)i * r.T1 * D;
      const size_t o = (size_t)i * r.M1 * D;
      HGL_TRY(r.x3 ? hgl_launch_win_partition_split(h, r.g, ws, r.nw, D, Hw.hi + o, Hw.lo + o, st)
                   : hgl_launch_win_partition(h, r.g, ws, r.nw, D, Hw.f32 + o, st));
    }
  } else {
    HGL_TRY(hgl_launch_layernorm_act(p.X, b.norm1_w, b.norm1_b, in, T, D, 1e-6f, st));
  }
  // in-projection, (fp32 qkv | planes) x (every row | the real tokens gathered: a padded row of qkv is the bias).  Planes:
  // q | k | v as fp16 hi / lo planes (the write-out splits; same bytes as the fp32 tensor) for the attention kernel that stages
  // them by LDS-DMA without converting (attention_ps.hip)
  const HglAct Q = enc_qkv(p, r, r.planes);
  HglGemm qkv = hgl_gemm_act(in, b.qkv_w, b.qkv_b, Q, M, 3 * D, D);
  if (r.gather) {
    HGL_TRY(r.planes ? hgl_launch_fill_rows_split(Q.hi, Q.lo, 3 * D, p.pad_list, p.pad_count, p.n_pad_max, b.qkv_b, 3 * D, st)
                     : hgl_launch_fill_rows(Q.f32, 3 * D, p.pad_list, p.pad_count, p.n_pad_max, b.qkv_b, 3 * D, st));
    qkv.M = T, qkv.amap = qkv.cmap = p.pad_of;
  }
  HGL_TRY(hgl_launch_gemm(qkv, st));
  HGL_TRY(enc_attention(b, p, r, st));
  const HglAct att = r.x3 ? Hw : hgl_act(p.O, (size_t)M * D, false);   // where enc_attn put the output
  const size_t qkv_bytes = (size_t)M * 3 * D * sizeof(float);         // q, k, v are dead after the attention
  if (ws > 0 && !r.gather) {
    HGL_TRY(hgl_launch_gemm(hgl_gemm_act(att, b.proj_w, b.proj_b, p.P, M, D, D), st));
    for (int i = 0; i < p.nb; ++i)
      HGL_TRY(hgl_launch_win_unpartition_add(p.X + (size_t)i * r.T1 * D, r.g, ws, r.nw, D, p.P + (size_t)i * r.M1 * D, st));
  } else {
    // windows: the projection of the real tokens only, written straight back to token order with the residual added
    // (window_unpartition + shortcut, image_encoder.py:178-180); global: every row where it is
    HglGemm proj = hgl_gemm_act(att, b.proj_w, b.proj_b, p.X, T, D, D, HGL_ACT_NONE, p.X);
    if (r.gather) proj.amap = p.pad_of, proj.cmap = p.tok_of;
    proj.part = p.QKV, proj.part_bytes = qkv_bytes;
    HGL_TRY(hgl_launch_gemm(proj, st));
  }
  const HglMlp mlp{b.norm2_w, b.norm2_b, b.lin1_w, b.lin1_b, b.lin2_w, b.lin2_b, 1e-6f, HGL_ACT_GELU};
  return hgl_mlp_half(mlp, p.X, H, F, T, D, p.QKV, qkv_bytes, r.ks, st);
}

// ------------------------------------------------------------------------------ decoder
struct DecPlan {
  float *sparse, *tokens, *queries, *qpe, *q1, *k1, *v1, *att, *keys0, *kpe0, *keys, *kpe, *kp, *vp,
      *qi, *atti, *mlp, *u1, *u2, *hy_a, *hy_b, *hyper, *iou_a, *iou_b, *keysS;
  uint8_t* skip;      // IoU gate: prompts whose upscaling is skipped
};

// the two buffers that also serve as scratch (layouts below): their sizes, for carve_dec and for the route's capacity conditions
// kp: k / v / q projections of the image tokens: three [P*HW, C/2] matrices, or -- merged projections -- ONE [P*HW, 3C/2]
inline size_t dec_kp_floats(const HglSamDecoderW* w, size_t P) { return 3 * (P * ((size_t)w->grid * w->grid) * w->C / 2); }
// atti: the image -> token attention's output [P*HW, C/2]
inline size_t dec_atti_floats(const HglSamDecoderW* w, size_t P) { return P * ((size_t)w->grid * w->grid) * w->C / 2; }

// n_img > 1: the P prompts belong to n_img images (P / n_img each): one set of shared layer-0 image tokens per image
bool carve_dec(HglArena& ar, const HglSamDecoderW* w, int P, DecPlan& p, int n_img = 1) {
  const size_t C = w->C, HW = (size_t)w->grid * w->grid, T = 16;   // 5 output tokens + up to 11 sparse prompt tokens
  p.sparse = ar.take<float>((size_t)P * (T - 5) * C);
  p.tokens = ar.take<float>(P * T * C);
  p.queries = ar.take<float>(P * T * C);
  p.qpe = ar.take<float>(P * T * C);
  p.q1 = ar.take<float>(P * T * C);
  p.k1 = ar.take<float>(P * T * C);
  p.v1 = ar.take<float>(P * T * C);
  p.att = ar.take<float>(P * T * C);
  p.keys0 = ar.take<float>(n_img * HW * C);
  p.kpe0 = ar.take<float>(n_img * HW * C);
  p.keys = ar.take<float>(P * HW * C);
  p.kpe = ar.take<float>(P * HW * C);
  p.kp = ar.take<float>(dec_kp_floats(w, P));
  p.vp = p.kp ? p.kp + P * HW * C / 2 : nullptr;
  p.qi = p.kp ? p.kp + 2 * (P * HW * C / 2) : nullptr;
  p.atti = ar.take<float>(dec_atti_floats(w, P));
  p.mlp = ar.take<float>(P * T * w->mlp_dim);
  p.u1 = ar.take<float>(P * HW * C);           // [P*HW*4, C/4]
  p.u2 = ar.take<float>(P * HW * 16 * (C / 8)); // [P*HW*16, C/8]
  p.hy_a = ar.take<float>((size_t)P * C);
  p.hy_b = ar.take<float>((size_t)P * C);
  p.hyper = ar.take<float>((size_t)P * 4 * (C / 8));
  p.keysS = ar.take<float>(P * HW * C);        // f16x3 mode: the normalised image tokens as fp16 hi | lo planes
  p.iou_a = ar.take<float>((size_t)P * C);
  p.iou_b = ar.take<float>((size_t)P * C);
  p.skip = ar.take<uint8_t>((size_t)P);
  return ar.ok();
}

bool valid_lin(const HglLinearW& l) { return l.w && l.b; }
bool valid_attn(const HglSamAttnW& a) {
  return valid_lin(a.q) && valid_lin(a.k) && valid_lin(a.v) && valid_lin(a.out) && a.internal > 0;
}
bool valid_dec(const HglSamDecoderW* w) {
  if (!w || w->C <= 0 || w->grid <= 0 || w->heads <= 0 || w->mlp_dim <= 0 || (w->C & 31)) return false;
  if (!w->pe_gauss || !w->point_embed_pos || !w->not_a_point || !w->no_mask || !w->iou_token || !w->mask_tokens) return false;
  for (int i = 0; i < 2; ++i) {
    const auto& l = w->layer[i];
    if (!valid_attn(l.self_attn) || !valid_attn(l.t2i) || !valid_attn(l.i2t) || !valid_lin(l.lin1) || !valid_lin(l.lin2) ||
        !l.n1.w || !l.n2.w || !l.n3.w || !l.n4.w) return false;
  }
  if (!valid_attn(w->final_t2i) || !w->norm_final.w || !w->up0_w || !w->up0_b || !w->up1.w || !w->up3_w || !w->up3_b) return false;
  for (int i = 0; i < 4; ++i) for (int j = 0; j < 3; ++j) if (!valid_lin(w->hyper[i][j])) return false;
  for (int j = 0; j < 3; ++j) if (!valid_lin(w->iou_head[j])) return false;
  return true;
}

inline HglGemm lin_desc(const float* A, int lda, const HglLinearW& l, const float* R, int ldr, float* Cc, int ldc, int M,
                        int N, int K, int act) {
  HglGemm d = hgl_gemm_linear(A, l.w, l.b, Cc, M, N, K, act, R);
  d.lda = lda, d.ldr = ldr, d.ldc = ldc;
  // the token side of a large prompt batch (512 prompts: 3584 rows) and the image-side projections shared by all prompts
  // (4096 rows) are still small-tile work: 8 x 116 workgroups of 32 x 32 instead of the fp32 kernel (35 -> 12 us each,
  // 23 launches per decoder call)
  d.skinny_max_m = 8192;
  return d;
}
inline int lin(const float* A, int lda, const HglLinearW& l, const float* R, int ldr, float* Cc, int ldc, int M,
               int N, int K, int act, hipStream_t st) {
  return hgl_launch_gemm(lin_desc(A, lda, l, R, ldr, Cc, ldc, M, N, K, act), st);
}

// lin() over the rows of n sets of M rows each (the shared image tokens of n images), every row as lin() over ONE set gives
// it: the kernel lin() picks for M rows is a small-tile one whose rows do not depend on the row count -> one launch over
// n * M rows; any other choice (fp32 tiles, whose dispatch looks at M) -> set by set.
inline int lin_sets(const float* A, int lda, const HglLinearW& l, float* Cc, int ldc, int M, int n, int N, int K, hipStream_t st) {
  HglGemm d = lin_desc(A, lda, l, nullptr, 0, Cc, ldc, M, N, K, HGL_ACT_NONE);
  if (n == 1) return hgl_launch_gemm(d, st);
  if (hgl_gemm_route(d) == HGL_GEMM_SKINNY) {
    d.M = d.skinny_max_m = n * M;   // the row bound held for ONE set
    return hgl_launch_gemm(d, st);
  }
  for (int i = 0; i < n; ++i)
    HGL_TRY(lin(A + (size_t)i * M * lda, lda, l, nullptr, 0, Cc + (size_t)i * M * ldc, ldc, M, N, K, HGL_ACT_NONE, st));
  return HGL_OK;
}

// which fused decoder stages are in use (bit 0: upscaling + hyper-network products, bit 1: merged image-side projections,
// bit 2: image -> token attention + out-projection + norm4, bit 3: unused, bit 4: chunked token -> image attention,
// bit 5: token -> image attention on the raw image-token planes); default: all stages fused
int g_dec_fusion = -1;
int dec_fusion_mask() {
  if (g_dec_fusion < 0) g_dec_fusion = HGL_DIAG_SWITCH("HGL_SAM_DEC_FUSED", 0x7fffffff);   // product: hgl_sam_decoder_fusion()
  return g_dec_fusion;
}

// ---- scratch layouts: DecPlan::atti, idle whenever tokens attend to the image, serves three other purposes and DecPlan::kp
// one; each layout gives its pointers and its byte count side by side, and dec_route's capacity conditions call bytes() ----
// (1) the partials of the chunked few-query attention: hgl_attention_fewq_part_bytes(B, Nk), see dec_fewq
// (2) the raw token -> image attention: the folded queries Q' [P*56, C] as fp16 hi | lo planes, then [P*56, C] floats that hold Q' in fp32 first and
// the attended rows afterwards, then the key-range partial rows (counted for one key range as well, where nothing is written
// there: the attended rows leave the kernel directly)
struct RawT2iScratch {
  uint16_t *Qh, *Ql;
  float *A, *part;
  RawT2iScratch(float* atti, int P, int C)
      : Qh((uint16_t*)atti), Ql(Qh + (size_t)P * 56 * C), A((float*)(Ql + (size_t)P * 56 * C)), part(A + (size_t)P * 56 * C) {}
  static size_t bytes(int P, int n_img, int ppi, int HW, int C) { return (size_t)P * (56 * C * 8) + n_img * hgl_t2i_part_bytes(ppi, HW); }
};
// (3) the folded image -> token step: K' [P*56, C] hi | lo, the U fragments [P, 16, 2, 64, 8] hi | lo, cb [P*56] floats (256
// bytes a prompt)
struct I2tFoldScratch {
  uint16_t *Kh, *Kl, *Uh, *Ul;
  float* cb;
  I2tFoldScratch(float* atti, int P, int C)
      : Kh((uint16_t*)atti), Kl(Kh + (size_t)P * 56 * C), Uh(Kl + (size_t)P * 56 * C), Ul(Uh + (size_t)P * 16384),
        cb((float*)(Ul + (size_t)P * 16384)) {}
  static size_t bytes(int P, int C) { return (size_t)P * (56 * C * 4 + 16384 * 4 + 256); }
};
// kp as the positional bias [P*56, HW] of (2) and (3): the folded rows against dense_pe
inline size_t dec_bias_bytes(int P, int HW) { return (size_t)P * 56 * HW * sizeof(float); }

// token -> image attention (7 queries, thousands of keys): the chunked kernel where the route says it serves (DecRoute::chunked:
// part != null), with the partials in `part` (the image -> token buffer, idle at that point)
int dec_fewq(const float* q, const float* k, const float* v, float* att, int B, int heads, int Nq, int Nk, int hd, int ldq,
             int ldk, int ldv, int ldo, long long sqb, long long skb, long long svb, long long sob, float* part,
             size_t part_bytes, hipStream_t st, int kv_group = 1) {
  HglAttn d;
  d.B = B, d.H = heads, d.Sq = Nq, d.Sk = Nk, d.hd = hd, d.scale = 1.0f / sqrtf((float)hd);
  d.q = q, d.k = k, d.v = v, d.out = att;
  d.ldq = ldq, d.ldk = ldk, d.ldv = ldv, d.ldo = ldo;
  d.sqb = sqb, d.skb = skb, d.svb = svb, d.sob = sob;
  if (part) {
    d.part = part, d.part_bytes = part_bytes, d.kv_group = kv_group;
    // the chunked kernel holds up to 7 queries: longer prompts (more sparse tokens) go through it 7 queries at a time
    for (int q0 = 0; q0 < Nq; q0 += 7) {
      d.q = q + (long long)q0 * ldq, d.out = att + (long long)q0 * ldo, d.Sq = Nq - q0 < 7 ? Nq - q0 : 7;
      HGL_TRY(hgl_launch_attention(d, st));
    }
    return HGL_OK;
  }
  HGL_REQUIRE(kv_group == 1, "sam_decode: keys shared by groups of %d prompts need the chunked attention", kv_group);
  return hgl_launch_attention(d, st);
}

// Attention.forward (modeling/transformer.py:218-240).  q: [Bq? , Nq, C] rows; when q_shared the same
// Nq rows serve every batch (batch stride 0).  out: [B, Nq, C] (+ residual R, may alias out).
int dec_attn(const HglSamDecoderW* w, const HglSamAttnW& a, const float* q, bool q_shared, int Nq, const float* k,
             const float* v, bool kv_shared, int Nk, int B, float* qp, float* kp, float* vp, float* att,
             const float* R, long long sR, float* out, hipStream_t st, float* part = nullptr, size_t part_bytes = 0,
             int kv_sets = 1) {
  const int C = w->C, I = a.internal, heads = w->heads, hd = I / heads;
  const int Bq = q_shared ? 1 : B, Bk = kv_shared ? 1 : B;
  HGL_TRY(lin(q, C, a.q, nullptr, 0, qp, I, Bq * Nq, I, C, HGL_ACT_NONE, st));
  if (kv_shared && kv_sets > 1) {
    // the prompts of kv_sets images in one launch: prompt b attends to the keys / values of image b / (B / kv_sets)
    HGL_TRY(lin_sets(k, C, a.k, kp, I, Nk, kv_sets, I, C, st));
    HGL_TRY(lin_sets(v, C, a.v, vp, I, Nk, kv_sets, I, C, st));
    HGL_TRY(dec_fewq(qp, kp, vp, att, B, heads, Nq, Nk, hd, I, I, I, I, (long long)Nq * I, (long long)Nk * I, (long long)Nk * I,
                     (long long)Nq * I, part, part_bytes, st, B / kv_sets));
  } else {
    HGL_TRY(lin(k, C, a.k, nullptr, 0, kp, I, Bk * Nk, I, C, HGL_ACT_NONE, st));
    HGL_TRY(lin(v, C, a.v, nullptr, 0, vp, I, Bk * Nk, I, C, HGL_ACT_NONE, st));
    HGL_TRY(dec_fewq(qp, kp, vp, att, B, heads, Nq, Nk, hd, I, I, I, I, q_shared ? 0 : (long long)Nq * I,
                     kv_shared ? 0 : (long long)Nk * I, kv_shared ? 0 : (long long)Nk * I, (long long)Nq * I, part, part_bytes, st));
  }
  // out_proj (+ residual): one GEMM over all B*Nq rows when the residual is laid out like the output (small row
  // counts then take the small-tile kernel); batched when a shared residual (stride 0) has to be broadcast
  if (!R || sR == (long long)Nq * C)
    return lin(att, I, a.out, R, C, out, C, B * Nq, C, I, HGL_ACT_NONE, st);
  HglGemm d = hgl_gemm_linear(att, a.out.w, a.out.b, out, Nq, C, I, HGL_ACT_NONE, R);
  d.batch = B, d.sA = (long long)Nq * I, d.sR = sR, d.sC = (long long)Nq * C;
  return hgl_launch_gemm(d, st);
}

// ---- f16x3 path of the decoder's image-token side (M = P*HW rows) -------------------------------------------
// The normalised image tokens exist as fp16 hi|lo planes (keysS) and, with the positional encoding added, as a
// second pair (kpeS): ln256_pe_split emits both, the few-key attention emits its output split, so every large
// GEMM below reads split operands and nothing is converted in a separate pass.

bool dec_x3_ready(const HglSamDecoderW* w) {
  if (!hgl_split_layout() || w->C != 256) return false;   // (f16 mode: the entry points pin three terms)
  const float* need[] = {w->layer[0].i2t.out.w, w->layer[1].i2t.out.w, w->layer[1].i2t.q.w, w->layer[1].t2i.k.w,
                         w->layer[1].t2i.v.w, w->final_t2i.k.w, w->final_t2i.v.w, w->up0_w, w->up3_w};
  for (const float* x : need) if (!hgl_has_split_weight(x)) return false;
  return true;
}

// merged image-side projections (HglSamDecoderW.kvq1 / kvf): present and registered
bool dec_merged_ready(const HglSamDecoderW* w) {
  return w->kvq1_w && w->kvq1_b && w->kvq1_pe && w->kvf_w && w->kvf_b && w->kvf_pe && hgl_has_split_weight(w->kvq1_w) &&
         hgl_has_split_weight(w->kvf_w);
}

// ---- the route of one decoder call: every decision about its launches, taken by dec_route() from the weights, the shape of
// the call and the fusion mask before anything is enqueued.  decode_impl and its helpers read these fields. ----
struct DecRoute {
  int P, n_img, ppi;     // prompts; images they belong to; prompts per image (prompt p belongs to image p / ppi)
  int T, HW;             // tokens per prompt, image tokens
  size_t atti_bytes;     // capacity of DecPlan::atti
  bool x3;               // the image-token side on split planes
  bool merged;           // merged image-side projections (fusion bit 1)
  bool raw_t2i;          // token -> image attention of layer 1 and the final one on the raw planes (fusion bit 5)
  bool shared[2];        // per layer: the image tokens are identical for every prompt of an image (layer 0 without dense prompts)
  bool plain[2];         // per layer: per-prompt image tokens in layer 0 -> the plain fp32 launches
  bool fuse_i2t[2];      // per layer: attention over the 7 tokens + out-projection + residual + norm4 in one launch (fusion bit 2)
  bool chunked[3];       // token -> image attention of layer 0, layer 1, the final one: the chunked few-query kernel serves (fusion bit 4)
  bool fused_tail;       // upscaling + hyper-network products in one launch (fusion bit 0)
  int ns;                // key ranges per prompt of the raw attention
  bool multi;            // the prompts of several images can share this launch sequence
};

DecRoute dec_route(const HglSamDecoderW* w, int P, int n_img, int n_sparse, bool dense, int fusion) {
  DecRoute r;
  const int C = w->C, g = w->grid, HW = g * g, T = 5 + n_sparse, heads = w->heads, I1 = w->layer[1].t2i.internal, ppi = P / n_img;
  r.P = P, r.n_img = n_img, r.ppi = ppi, r.T = T, r.HW = HW;
  r.atti_bytes = dec_atti_floats(w, P) * sizeof(float);
  r.x3 = dec_x3_ready(w);
  r.merged = r.x3 && (fusion & 2) && dec_merged_ready(w) && w->layer[1].t2i.internal == w->layer[1].i2t.internal &&
             w->layer[1].t2i.internal == w->final_t2i.internal && 2 * w->final_t2i.internal == C;
  // fusion bit 5: the token -> image attention of layer 1 and the final one on the raw image-token planes (the 7 tokens go
  // through W_k / W_v instead of the HW image tokens: no k | v projection GEMM; layer 1 projects q alone for its step 4).
  // Capacity: both reuses of atti, and kp as the bias of either
  r.raw_t2i = r.merged && (fusion & 32) && (fusion & 4) && T == 7 && I1 == 128 && heads == 8 && C == 256 && HW % 128 == 0 &&
              P <= 65535 && !dense && hgl_has_split_weight(w->dense_pe) &&
              RawT2iScratch::bytes(P, n_img, ppi, HW, C) <= r.atti_bytes && I2tFoldScratch::bytes(P, C) <= r.atti_bytes &&
              dec_bias_bytes(P, HW) <= dec_kp_floats(w, P) * sizeof(float);
  // (prompt batches of <= 128: eight key ranges per prompt, see the kernel.  The batch that decides is the image's own, ppi,
  // not the launch's total: a prompt's sums keep their order whether its image is decoded alone or with others)
  r.ns = hgl_t2i_key_ranges(ppi, HW);
  for (int li = 0; li < 2; ++li) {
    r.shared[li] = li == 0 && !dense;   // keys identical for every prompt in layer 0
    // layer 0 on per-prompt image tokens: the plain fp32 launches (the split planes / merged weights belong to layer 1's input)
    r.plain[li] = li == 0 && dense;
    r.fuse_i2t[li] = r.merged && (fusion & 4) && w->layer[li].i2t.internal == I1 && I1 == 128 && heads == 8 && HW % 64 == 0 &&
                     P <= 65535 && T == 7 && !r.plain[li];
  }
  const HglSamAttnW* t2i[3] = {&w->layer[0].t2i, &w->layer[1].t2i, &w->final_t2i};
  // the chunked kernel: 8 heads of 16, at least one chunk of keys, its partials in atti
  for (int s = 0; s < 3; ++s)
    r.chunked[s] = (fusion & 16) && heads == 8 && t2i[s]->internal / heads == 16 && HW >= 256 && P <= 65535 &&
                   r.atti_bytes >= hgl_attention_fewq_part_bytes(P, HW);
  // fused upscaling + hyper-network products (one launch, the 256-channel rows read once)
  r.fused_tail = r.x3 && (fusion & 1) && (HW % 64) == 0 && (g % 64 == 0 || 64 % g == 0) && P <= 65535;
  // Several images in ONE launch sequence: only layer 0 knows that prompts share image tokens; its two shared steps then need
  // the kernels that address "the rows of image p / ppi": the chunked token -> image attention and the fused image -> token step
  r.multi = r.shared[0] && r.fuse_i2t[0] && r.chunked[0];
  return r;
}

// steps (2) of a layer (step 0 / 1) and the final attention (step 2): the tokens attend to the image (transformer.py:126-131,
// :98-104), queries += out_proj(attn): plain, or -- layer 1 and the final attention of the split path -- raw, merged or split
int dec_t2i(const DecRoute& r, const HglSamDecoderW* w, const HglSamAttnW& a, int step, const DecPlan& p, const HglAct& keysS,
            const HglAct& kpeS, hipStream_t st) {
  const int P = r.P, HW = r.HW, T = r.T, C = w->C, I = a.internal, heads = w->heads, hd = I / heads;
  float* const part = r.chunked[step] ? p.atti : nullptr;   // the chunked attention's partials
  const long long sq = (long long)T * I, sk = (long long)HW * I;   // batch strides of the projected tokens / image tokens
  if (step == 0 || !r.x3) {   // fp32 projections of the image tokens; the only form for layer 0
    const bool shared = step < 2 && r.shared[step];
    return dec_attn(w, a, p.qpe, false, T, shared ? p.kpe0 : p.kpe, shared ? p.keys0 : p.keys, shared, HW, P, p.q1, p.kp, p.vp, p.att,
                    p.queries, (long long)T * C, p.queries, st, part, r.atti_bytes, shared ? r.n_img : 1);
  }
  const bool merged = r.merged && !r.raw_t2i, fin = step == 2;
  const int N = fin ? 2 * I : 3 * I;
  if (merged) {
    // k, v of this step and (layer 1) q of step (4) read the same rows: one GEMM, the positional encoding as a per-position
    // table.  kvq [P*HW, N] = keys W^T + b + pe_table[row % HW]; N = 3I: k | v | q of layer 1 (kvq1), N = 2I: k | v of the final
    // attention (kvf)
    HglGemm kvq = hgl_gemm_planes(keysS.hi, keysS.lo, fin ? w->kvf_w : w->kvq1_w, fin ? w->kvf_b : w->kvq1_b, p.kp, P * HW, N, C,
                                  HGL_ACT_NONE, fin ? w->kvf_pe : w->kvq1_pe);
    kvq.rmod = HW;
    HGL_TRY(hgl_launch_gemm(kvq, st));
  }
  HGL_TRY(lin(p.qpe, C, a.q, nullptr, 0, p.q1, I, P * T, I, C, HGL_ACT_NONE, st));
  if (r.raw_t2i) {
    // no projection of the image tokens at all (sam_decoder_t2i.hip): the 7 tokens are projected through W_k / W_v instead of
    // the HW image tokens, the attention reads the raw planes, its positional term in p.kp
    const RawT2iScratch s(p.atti, P, C);
    HGL_TRY(hgl_launch_t2i_fold_q(p.q1, a.k.w, 1.0f / sqrtf((float)hd), s.A, P, st));
    HGL_TRY(hgl_launch_split_f16(s.A, 1.0f, s.Qh, s.Ql, (long long)P * 56 * C, st));
    // bias[p*56 + r, key] = Qk[p*56 + r, :] . pe[key, :]: pe is the "weight" [HW, C] of a split-fp16 GEMM
    HGL_TRY(hgl_launch_gemm(hgl_gemm_planes(s.Qh, s.Ql, w->dense_pe, nullptr, p.kp, P * 56, HW, C), st));
    // several key ranges: their partial rows behind the folded queries; one: the attended rows over the folded queries
    float* const rows = r.ns > 1 ? s.part : s.A;
    HGL_TRY(hgl_launch_t2i_raw_attn(s.Qh, s.Ql, p.kp, keysS.hi, keysS.lo, P, HW, rows, r.ns, st));
    HGL_TRY(hgl_launch_t2i_unfold_v(rows, r.ns, a.v.w, a.v.b, p.att, P, st));
  } else if (merged) {   // k = kvq[:, 0:I], v = kvq[:, I:2I], row stride N
    HGL_TRY(dec_fewq(p.q1, p.kp, p.kp + I, p.att, P, heads, T, HW, hd, I, N, N, I, sq, (long long)HW * N, (long long)HW * N, sq, part,
                     r.atti_bytes, st));
  } else {
    // per-prompt image tokens (transformer.py:126-131): the K / V projections read the split planes
    HGL_TRY(hgl_launch_gemm(hgl_gemm_planes(kpeS.hi, kpeS.lo, a.k.w, a.k.b, p.kp, P * HW, I, C), st));
    HGL_TRY(hgl_launch_gemm(hgl_gemm_planes(keysS.hi, keysS.lo, a.v.w, a.v.b, p.vp, P * HW, I, C), st));
    HGL_TRY(dec_fewq(p.q1, p.kp, p.vp, p.att, P, heads, T, HW, hd, I, I, I, I, sq, sk, sk, sq, part, r.atti_bytes, st));
  }
  return lin(p.att, I, a.out, p.queries, C, p.queries, C, P * T, C, I, HGL_ACT_NONE, st);
}

// step (4) of layer li: the image attends to the tokens: q = keys+pe, k = queries+pe, v = queries ; keys += out, then norm4
// (transformer.py:139-150); the image tokens leave it in the form the next step of the route reads
int dec_i2t(const DecRoute& r, const HglSamDecoderW* w, int li, const DecPlan& p, const HglAct& keysS, const HglAct& kpeS,
            hipStream_t st) {
  const auto& L = w->layer[li];
  const auto& a = L.i2t;
  const int P = r.P, HW = r.HW, T = r.T, C = w->C, I = a.internal, heads = w->heads, hd = I / heads;
  const long long sK = (long long)HW * C;
  const bool shared = r.shared[li];
  const float* keys = shared ? p.keys0 : p.keys;
  const float* kpe = shared ? p.kpe0 : p.kpe;
  if (r.fuse_i2t[li]) {
    HGL_TRY(lin(p.qpe, C, a.k, nullptr, 0, p.k1, I, P * T, I, C, HGL_ACT_NONE, st));
    HGL_TRY(lin(p.queries, C, a.v, nullptr, 0, p.v1, I, P * T, I, C, HGL_ACT_NONE, st));
    if (r.raw_t2i && !shared) {
      // layer 1 on per-prompt image tokens: scores = (keys + pe) . (W_q^T k_tok) and update = P (W_o v_tok) by MFMA against
      // per-prompt 56 x 256 matrices (sam_decoder_t2i.hip: dec_i2t_fold_kernel); the planes are updated in place
      const I2tFoldScratch s(p.atti, P, C);
      HGL_TRY(hgl_launch_i2t_prep(p.k1, p.v1, a.q.w, a.q.b, a.out.w, 1.0f / sqrtf((float)hd), s.Kh, s.Kl, s.cb, s.Uh, s.Ul, P, st));
      HGL_TRY(hgl_launch_gemm(hgl_gemm_planes(s.Kh, s.Kl, w->dense_pe, nullptr, p.kp, P * 56, HW, C), st));
      return hgl_launch_dec_i2t_fold(keysS.hi, keysS.lo, s.Kh, s.Kl, p.kp, s.cb, s.Uh, s.Ul, a.out.b, L.n4.w, L.n4.b, 1e-5f, P, HW,
                                     keysS.hi, keysS.lo, st);
    }
    // attention over the 7 tokens, out-projection, residual and norm4 in one launch: the image tokens leave it as the
    // split planes the next projections read (and, in layer 0, as the fp32 rows layer 1 adds its update to)
    if (shared) HGL_TRY(lin_sets(p.kpe0, C, a.q, p.qi, I, HW, r.n_img, I, C, st));
    // (shared rows: stride 0 for one image; n_img images: the rows of image p / ppi, one image's rows apart)
    const bool sets = shared && r.n_img > 1;
    return hgl_launch_dec_i2t(shared ? p.qi : p.kp + 2 * I, shared ? I : 3 * I, sets ? (long long)HW * I : shared ? 0 : (long long)HW * 3 * I,
                              p.k1, p.v1, a.out.w, a.out.b, keys, sets ? sK : shared ? 0 : sK, L.n4.w, L.n4.b, 1e-5f,
                              1.0f / sqrtf((float)hd), P, HW, (li == 0 && !r.raw_t2i) ? p.keys : nullptr, keysS.hi, keysS.lo, st,
                              sets ? r.ppi : 1);
  }
  if (!r.x3 || r.plain[li]) {   // the plain fp32 launches
    HGL_TRY(dec_attn(w, a, kpe, shared, HW, p.qpe, p.queries, false, T, P, p.qi, p.k1, p.v1, p.atti, keys, shared ? 0 : sK, p.keys, st));
    if (!r.x3) {
      HGL_TRY(hgl_launch_layernorm(p.keys, L.n4.w, L.n4.b, p.keys, P * HW, C, 1e-5f, st));
      return hgl_launch_add_rows_bcast(p.keys, sK, w->dense_pe, sK, P, p.kpe, st);
    }
  } else {
    // q = (keys + pe) Wq: of the shared rows, from the merged projection of step (2) (kvq[:, 2I:3I]), or from the split planes;
    // 7 token keys / values (the few-key kernel for up to 8 tokens, the general one beyond), its output split;
    // keys' = keys + out_proj(attn)
    const bool from_kvq = r.merged && !shared;
    const int ldq = from_kvq ? 3 * I : I;
    if (shared) {
      HGL_TRY(lin(p.kpe0, C, a.q, nullptr, 0, p.qi, I, HW, I, C, HGL_ACT_NONE, st));
    } else if (!from_kvq) {
      HGL_TRY(hgl_launch_gemm(hgl_gemm_planes(kpeS.hi, kpeS.lo, a.q.w, a.q.b, p.qi, P * HW, I, C), st));
    }
    HGL_TRY(lin(p.qpe, C, a.k, nullptr, 0, p.k1, I, P * T, I, C, HGL_ACT_NONE, st));
    HGL_TRY(lin(p.queries, C, a.v, nullptr, 0, p.v1, I, P * T, I, C, HGL_ACT_NONE, st));
    const HglAct at = hgl_act(p.atti, (size_t)P * HW * I, true);
    HglAttn d;
    d.B = P, d.H = heads, d.Sq = HW, d.Sk = T, d.hd = hd, d.scale = 1.0f / sqrtf((float)hd);
    d.q = from_kvq ? p.kp + 2 * I : p.qi, d.k = p.k1, d.v = p.v1;
    d.ldq = ldq, d.ldk = d.ldv = I, d.sqb = shared ? 0 : (long long)HW * ldq, d.skb = d.svb = (long long)T * I;
    d.out_hi = at.hi, d.out_lo = at.lo, d.ldo = I, d.sob = (long long)HW * I;
    HGL_TRY(hgl_launch_attention(d, st));
    HglGemm out = hgl_gemm_planes(at.hi, at.lo, a.out.w, a.out.b, p.keys, P * HW, C, I, HGL_ACT_NONE, keys);
    out.rmod = shared ? HW : 0;
    HGL_TRY(hgl_launch_gemm(out, st));
  }
  // norm4, then keys (and, unmerged, keys + dense_pe) as split planes; the fp32 rows are kept only while a later layer
  // needs them as a residual
  return hgl_launch_ln256_pe_split(p.keys, L.n4.w, L.n4.b, w->dense_pe, HW, (long long)P * HW, 1e-5f, li == 0 ? 1 : 0, keysS.hi,
                                   keysS.lo, r.merged ? nullptr : kpeS.hi, r.merged ? nullptr : kpeS.lo, st);
}

}  // namespace

extern "C" {

size_t hgl_sam_encode_batch_workspace_bytes(const HglSamEncoderW* w, int nb) {
  if (!valid_enc(w) || nb < 1) return 0;
  HglArena ar(nullptr, 0);
  EncPlan p;
  carve_enc(ar, w, nb, p);
  return ar.off;
}

size_t hgl_sam_encode_workspace_bytes(const HglSamEncoderW* w) { return hgl_sam_encode_batch_workspace_bytes(w, 1); }

// nb images through the encoder at once: the token rows of the images are stacked, so every GEMM / LayerNorm / window
// attention launch covers all of them (weights read once, M = nb * 4096: the tilings fill the chip better and mlp.lin2
// needs no split-K).  Each image's result is what the single-image call gives up to the summation order of split-K.
int hgl_sam_encode_batch(const HglSamEncoderW* w, const uint8_t* const* resized_imgs, const int* in_h, const int* in_w, int nb,
                         float* emb, void* workspace, size_t workspace_bytes, void* stream) {
  HGL_TRY(hgl_require_device());
  HGL_REQUIRE(valid_enc(w), "sam_encode: invalid weight struct");
  HGL_REQUIRE(resized_imgs && in_h && in_w && emb && nb >= 1 && nb <= 64, "sam_encode: bad arguments (nb %d)", nb);
  for (int i = 0; i < nb; ++i)
    HGL_REQUIRE(resized_imgs[i] && in_h[i] > 0 && in_w[i] > 0 && in_h[i] <= w->img_size && in_w[i] <= w->img_size,
                "sam_encode: bad image %d (%dx%d for img_size %d)", i, in_h[i], in_w[i], w->img_size);
  HglArena ar(workspace, workspace_bytes);
  EncPlan p;
  if (!workspace || !carve_enc(ar, w, nb, p)) {
    hgl_set_error("sam_encode: workspace too small (%zu bytes given)", workspace_bytes);
    return HGL_EWORKSPACE;
  }
  hipStream_t st = (hipStream_t)stream;
  const int D = w->embed_dim, S = w->img_size, g = S / w->patch, C = w->out_chans, T1 = g * g, T = nb * T1;
  const int kd = 3 * w->patch * w->patch;
  for (int i = 0; i < nb; ++i)
    HGL_TRY(hgl_launch_sam_preprocess(resized_imgs[i], in_h[i], in_w[i], S, p.img + (size_t)i * 3 * S * S, st));
  // patch embedding + bias + absolute position embedding (image_encoder.py:107-109); the position rows repeat per image
  // (split: the im2col matrix written as fp16 hi | lo planes, same bytes as fp32)
  const bool embed_x3 = (w->patch & 3) == 0 && hgl_use_x3(w->patch_w, kd);
  HglGemm embed = hgl_gemm_linear(p.cols, w->patch_w, w->patch_b, p.X, embed_x3 ? T : T1, D, kd, HGL_ACT_NONE, w->pos_embed);
  if (embed_x3) embed.rmod = nb > 1 ? T1 : 0;
  else embed.batch = nb, embed.sA = (long long)T1 * kd, embed.sC = (long long)T1 * D;    // one batch per image, the table shared
  HGL_TRY(hgl_linear_split_or_not(embed, embed_x3, p.cols, (size_t)T * kd,
                                  [&](const HglAct& a) { return hgl_launch_im2col_patch_act(p.img, nb, S, w->patch, a, st); }, st));
  for (int i = 0; i < w->depth; ++i) {
    const int ws = w->blocks[i].window;
    if (ws > 0) {   // every windowed block shares one window size (build_sam.py:55-101)
      HGL_TRY(hgl_launch_win_maps(g, ws, (g + ws - 1) / ws, nb, p.pad_of, p.tok_of, p.pad_list, p.pad_count, st));
      break;
    }
  }
  for (int i = 0; i < w->depth; ++i) HGL_TRY(enc_block(w, w->blocks[i], p, st));
  // neck: conv1x1 -> LayerNorm2d -> conv3x3(pad 1) -> LayerNorm2d, all on NHWC rows
  const bool neck_x3 = hgl_use_x3(w->neck0_w, D) && hgl_use_x3(w->neck2_w, C * 9);
  // (neck_x3: operands split into the (dead) MLP buffers: H holds T*D, F holds T*4D floats)
  HGL_TRY(hgl_linear_split_or_not(hgl_gemm_linear(p.X, w->neck0_w, nullptr, p.neckA, T, C, D), neck_x3, p.H, (size_t)T * D, st));
  HGL_TRY(hgl_launch_layernorm(p.neckA, w->neck1_w, w->neck1_b, p.neckB, T, C, 1e-6f, st));
  for (int i = 0; i < nb; ++i)
    HGL_TRY(hgl_launch_im2col3x3(p.neckB + (size_t)i * T1 * C, g, C, p.cols3 + (size_t)i * T1 * C * 9, st));
  HGL_TRY(hgl_linear_split_or_not(hgl_gemm_linear(p.cols3, w->neck2_w, nullptr, p.neckA, T, C, C * 9),
                                  neck_x3 && (size_t)C * 9 <= (size_t)4 * D, p.F, (size_t)T * C * 9, st));
  HGL_TRY(hgl_launch_layernorm(p.neckA, w->neck3_w, w->neck3_b, emb, T, C, 1e-6f, st));
  return HGL_OK;
}

int hgl_sam_encode(const HglSamEncoderW* w, const uint8_t* resized_img, int in_h, int in_w, float* emb,
                   void* workspace, size_t workspace_bytes, void* stream) {
  return hgl_sam_encode_batch(w, &resized_img, &in_h, &in_w, 1, emb, workspace, workspace_bytes, stream);
}

// the generic path's products Th | Tw, [heads][B*S][2*size-1] floats each
size_t hgl_sam_relpos_tables_workspace_bytes(int B, int heads, int S, int size) {
  if (B < 1 || heads < 1 || S < 1 || size < 1) return 0;
  HglArena ar(nullptr, 0);
  ar.take<float>((size_t)heads * B * S * (2 * size - 1));
  ar.take<float>((size_t)heads * B * S * (2 * size - 1));
  return ar.off;
}

int hgl_sam_relpos_tables(const float* qkv, const void* q_hi, const void* q_lo, int ldq, int B, int heads, int S, int size, int hd,
                          const float* rel_pos_h, const float* rel_pos_w, float* rel_h, float* rel_w, void* workspace,
                          size_t workspace_bytes, void* stream) {
  HGL_TRY(hgl_require_device());
  const bool planes = q_hi || q_lo;
  HGL_REQUIRE(rel_pos_h && rel_pos_w && rel_h && rel_w && (planes ? (q_hi && q_lo && !qkv) : qkv != nullptr),
              "sam_relpos_tables: null argument (q as fp32 rows OR as both planes)");
  HGL_REQUIRE(B > 0 && heads > 0 && size > 0 && S == size * size && (long long)B * heads <= 65535 && (long long)B * S < (1ll << 31),
              "sam_relpos_tables: bad shape (B %d, heads %d, S %d, size %d)", B, heads, S, size);
  HGL_REQUIRE(hd == 16 || hd == 32 || hd == 64 || hd == 80, "sam_relpos_tables: unsupported head dim %d (16,32,64,80)", hd);
  HGL_REQUIRE(ldq >= heads * hd && (ldq & (planes ? 7 : 3)) == 0, "sam_relpos_tables: bad leading dim %d", ldq);
  HGL_REQUIRE((((uintptr_t)qkv | (uintptr_t)q_hi | (uintptr_t)q_lo | (uintptr_t)rel_pos_h | (uintptr_t)rel_pos_w | (uintptr_t)rel_h |
                (uintptr_t)rel_w) & 15) == 0, "sam_relpos_tables: operands must be 16-byte aligned");
  // (the in-projection writes planes in f16x3 mode only: f16 mode keeps no lo plane, f32 mode no planes at all)
  HGL_REQUIRE(!planes || (hgl_split_layout() && hgl_split_terms() == 3), "sam_relpos_tables: q as planes exists in f16x3 mode only");
  HglArena ar(workspace, workspace_bytes);
  float* Th = ar.take<float>((size_t)heads * B * S * (2 * size - 1));
  float* Tw = ar.take<float>((size_t)heads * B * S * (2 * size - 1));
  if (!workspace || !ar.ok()) {
    hgl_set_error("sam_relpos_tables: workspace too small (%zu bytes given)", workspace_bytes);
    return HGL_EWORKSPACE;
  }
  return enc_relpos_tables(qkv, q_hi, q_lo, ldq, B, heads, S, size, hd, rel_pos_h, rel_pos_w, rel_h, rel_w, Th, Tw, (hipStream_t)stream);
}

int hgl_sam_dense_pe(const HglSamDecoderW* w, const float* grid_coords01, float* dense_pe, void* stream) {
  HGL_TRY(hgl_require_device());
  HGL_REQUIRE(w && w->pe_gauss && grid_coords01 && dense_pe && w->grid > 0 && w->C > 0, "sam_dense_pe: bad arguments");
  return hgl_launch_pe(grid_coords01, w->pe_gauss, w->grid * w->grid, w->C / 2, 0, nullptr, nullptr, dense_pe,
                       (hipStream_t)stream);
}

size_t hgl_sam_decode_workspace_bytes(const HglSamDecoderW* w, int P) {
  if (!valid_dec(w) || P <= 0) return 0;
  HglArena ar(nullptr, 0);
  DecPlan p;
  carve_dec(ar, w, P, p);
  return ar.off;
}

int hgl_sam_decoder_fusion(int mask) {
  const int old = dec_fusion_mask();
  if (mask >= 0) g_dec_fusion = mask;
  return old;
}

// MaskDecoder.predict_masks.  points01 != null: one foreground point + the padding point per prompt (what
// SamAutomaticMaskGenerator issues); else coords01 [P,n_sparse,2] / labels [P,n_sparse] with n_sparse = 2 .. 11 and, optionally,
// dense [P,HW,C]: per-prompt dense embeddings (mask inputs) instead of no_mask_embed.  first_mask = 1: the three multimask
// outputs (mask tokens 1..3); 0: tokens 0..2 (token 0 is the single-mask output, mask_decoder.py:99-105).
// IoU gate (hgl_sam_decode_points_gated): skip[p] = none of prompt p's three quality predictions exceeds `gate` (NaN counts as
// failing, as `iou_preds > thresh` does in automatic_mask_generator.py:287-288)
__global__ void iou_gate_kernel(const float* __restrict__ iou, int P, float gate, uint8_t* __restrict__ skip) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= P) return;
  skip[p] = (iou[3 * p] > gate || iou[3 * p + 1] > gate || iou[3 * p + 2] > gate) ? 0 : 1;
}

static int decode_impl(const HglSamDecoderW* w, const float* emb, const float* points01, const float* coords01,
                       const int32_t* labels, int n_sparse, const float* dense, int first_mask, int P, float* low_res,
                       float* iou_pred, void* workspace, size_t workspace_bytes, void* stream, bool gated = false,
                       float iou_gate = 0.f, int n_img = 1) {
  // the decoder keeps the f16x3 arithmetic in f16 mode: its split producers write both planes, its GEMMs issue three terms
  const HglSplitTermsScope three_terms(3);
  HGL_TRY(hgl_require_device());
  HGL_REQUIRE(valid_dec(w) && w->dense_pe, "sam_decode: invalid weight struct (dense_pe missing?)");
  HGL_REQUIRE(emb && (points01 || (coords01 && labels)) && low_res && iou_pred && P > 0, "sam_decode: null input");
  HGL_REQUIRE(first_mask == 0 || first_mask == 1, "sam_decode: first_mask must be 0 or 1");
  HGL_REQUIRE(n_sparse >= 2 && n_sparse <= 11, "sam_decode: %d sparse tokens per prompt (2 .. 11 supported)", n_sparse);
  HGL_REQUIRE(n_sparse <= 3 || (long long)P * w->heads <= 65535, "sam_decode: %d prompts of more than 3 sparse tokens in one call", P);
  HGL_REQUIRE(n_img >= 1 && P % n_img == 0 && (n_img == 1 || (points01 && !dense)), "sam_decode: %d prompts for %d images", P, n_img);
  // emb holds n_img embeddings, prompt p belongs to image p / (P / n_img)
  const DecRoute r = dec_route(w, P, n_img, n_sparse, dense != nullptr, dec_fusion_mask());
  HGL_REQUIRE(n_img == 1 || r.multi, "sam_decode: %d images in one launch sequence need the fused image -> token step and the "
              "chunked token -> image attention", n_img);
  HglArena ar(workspace, workspace_bytes);
  DecPlan p;
  if (!workspace || !carve_dec(ar, w, P, p, n_img)) {
    hgl_set_error("sam_decode: workspace too small (%zu bytes given)", workspace_bytes);
    return HGL_EWORKSPACE;
  }
  hipStream_t st = (hipStream_t)stream;
  const int C = w->C, g = w->grid, HW = g * g, T = 5 + n_sparse;
  const long long sQ = (long long)T * C, sK = (long long)HW * C;

  // ---- prompt encoder + token assembly ----
  if (points01) {
    HGL_TRY(hgl_launch_pe(points01, w->pe_gauss, 2 * P, C / 2, 1, w->point_embed_pos, w->not_a_point, p.sparse, st));
  } else {
    const float* pe4[4] = {w->point_embed_neg, w->point_embed_pos, w->point_embed_box0, w->point_embed_box1};
    HGL_REQUIRE(pe4[0] && pe4[2] && pe4[3], "sam_decode_prompts: the weight struct lacks point_embeddings 0 / 2 / 3");
    HGL_TRY(hgl_launch_pe_labeled(coords01, labels, w->pe_gauss, n_sparse * P, C / 2, w->not_a_point, pe4, p.sparse, st));
  }
  HGL_TRY(hgl_launch_build_tokens(w->iou_token, w->mask_tokens, p.sparse, P, C, T, p.tokens, st));
  if (dense) {   // the image tokens differ from prompt to prompt already in layer 0
    // src[p] = image_embedding + dense[p] (mask_decoder.py:121-123 with dense_prompt_embeddings from mask inputs)
    HGL_TRY(hgl_launch_add_rows_bcast(dense, sK, emb, sK, P, p.keys, st));
    HGL_TRY(hgl_launch_add_rows_bcast(p.keys, sK, w->dense_pe, sK, P, p.kpe, st));
  } else {
    // src = image_embedding + no_mask_embed (dense prompt) ; shared by all prompts until the first update
    // (n_img images: one such set per image, sK apart)
    HGL_TRY(hgl_launch_add_rows_bcast(emb, C, w->no_mask, C, n_img * HW, p.keys0, st));   // rows of C, "pe" = no_mask [C]
    HGL_TRY(hgl_launch_add_rows_bcast(p.keys0, n_img > 1 ? sK : 0, w->dense_pe, (long long)HW * C, n_img, p.kpe0, st));
  }
  HGL_TRY(hgl_copy_d2d(p.queries, p.tokens, sizeof(float) * P * sQ, "sam_decode: copying the tokens", st));

  const HglAct keysS = hgl_act(p.keysS, (size_t)P * HW * C, true), kpeS = hgl_act(p.kpe, (size_t)P * HW * C, true);
  // TwoWayAttentionBlock (transformer.py:109-150) x 2
  for (int li = 0; li < 2; ++li) {
    const auto& L = w->layer[li];
    // (1) self attention of the tokens
    if (li == 0) {  // skip_first_layer_pe: queries = self_attn(q,q,q), no residual
      HGL_TRY(dec_attn(w, L.self_attn, p.queries, false, T, p.queries, p.queries, false, T, P, p.q1, p.k1, p.v1, p.att,
                       nullptr, 0, p.qpe, st));
      HGL_TRY(hgl_copy_d2d(p.queries, p.qpe, sizeof(float) * P * sQ, "sam_decode: copying the tokens", st));
    } else {
      HGL_TRY(hgl_launch_add_rows_bcast(p.queries, P * sQ, p.tokens, P * sQ, 1, p.qpe, st));
      HGL_TRY(dec_attn(w, L.self_attn, p.qpe, false, T, p.qpe, p.queries, false, T, P, p.q1, p.k1, p.v1, p.att,
                       p.queries, sQ, p.queries, st));
    }
    HGL_TRY(hgl_launch_layernorm(p.queries, L.n1.w, L.n1.b, p.queries, P * T, C, 1e-5f, st));
    // (2) tokens attend to the image
    HGL_TRY(hgl_launch_add_rows_bcast(p.queries, P * sQ, p.tokens, P * sQ, 1, p.qpe, st));
    HGL_TRY(dec_t2i(r, w, L.t2i, li, p, keysS, kpeS, st));
    HGL_TRY(hgl_launch_layernorm(p.queries, L.n2.w, L.n2.b, p.queries, P * T, C, 1e-5f, st));
    // (3) MLP on the tokens
    HGL_TRY(lin(p.queries, C, L.lin1, nullptr, 0, p.mlp, w->mlp_dim, P * T, w->mlp_dim, C, HGL_ACT_RELU, st));
    HGL_TRY(lin(p.mlp, w->mlp_dim, L.lin2, p.queries, C, p.queries, C, P * T, C, w->mlp_dim, HGL_ACT_NONE, st));
    HGL_TRY(hgl_launch_layernorm(p.queries, L.n3.w, L.n3.b, p.queries, P * T, C, 1e-5f, st));
    // (4) image attends to the tokens
    HGL_TRY(hgl_launch_add_rows_bcast(p.queries, P * sQ, p.tokens, P * sQ, 1, p.qpe, st));
    HGL_TRY(dec_i2t(r, w, li, p, keysS, kpeS, st));
  }
  // final token -> image attention
  HGL_TRY(hgl_launch_add_rows_bcast(p.queries, P * sQ, p.tokens, P * sQ, 1, p.qpe, st));
  HGL_TRY(dec_t2i(r, w, w->final_t2i, 2, p, keysS, kpeS, st));
  HGL_TRY(hgl_launch_layernorm(p.queries, w->norm_final.w, w->norm_final.b, p.queries, P * T, C, 1e-5f, st));

  // ---- IoU head on the iou token (row 0); multimask output = columns 1..3.  BEFORE the upscaling: the predictions depend on
  // the token outputs only (mask_decoder.py:132-149), and the automatic generator drops every mask whose prediction does not
  // exceed pred_iou_thresh (automatic_mask_generator.py:287-291) -- a prompt whose three predictions all fail needs no
  // upscaling at all (the gate of hgl_sam_decode_points_gated) ----
  HGL_TRY(lin(p.queries, T * C, w->iou_head[0], nullptr, 0, p.iou_a, C, P, C, C, HGL_ACT_RELU, st));
  HGL_TRY(lin(p.iou_a, C, w->iou_head[1], nullptr, 0, p.iou_b, C, P, C, C, HGL_ACT_RELU, st));
  HGL_TRY(lin(p.iou_b, C, w->iou_head[2], nullptr, 0, p.iou_a, 4, P, 4, C, HGL_ACT_NONE, st));
  HGL_TRY(hgl_launch_gather_rows(p.iou_a + first_mask, 4, P, 3, iou_pred, st));
  const uint8_t* skip = nullptr;
  if (gated) {
    hipLaunchKernelGGL(iou_gate_kernel, dim3((P + 255) / 256), dim3(256), 0, st, (const float*)iou_pred, P, iou_gate, p.skip);
    HGL_TRY(hgl_check_launch("iou_gate"));
    skip = p.skip;
  }

  // ---- output upscaling: two ConvTranspose2d(k=2,s=2) as GEMMs, columns ordered (pos, out_channel) ----
  const int C4 = C / 4, C8 = C / 8;
  HGL_REQUIRE(C4 == 64, "sam_decode: LayerNorm2d width %d unsupported (64 expected)", C4);
  HGL_REQUIRE(C8 == 32, "sam_decode: hyper-network width %d unsupported (32 expected)", C8);
  // ---- hyper-networks on the mask tokens (rows 1..4 of each prompt's 7 tokens) ----
  for (int i = 0; i < 4; ++i) {
    HGL_TRY(lin(p.queries + (1 + i) * C, T * C, w->hyper[i][0], nullptr, 0, p.hy_a, C, P, C, C, HGL_ACT_RELU, st));
    HGL_TRY(lin(p.hy_a, C, w->hyper[i][1], nullptr, 0, p.hy_b, C, P, C, C, HGL_ACT_RELU, st));
    HGL_TRY(lin(p.hy_b, C, w->hyper[i][2], nullptr, 0, p.hyper + i * C8, 4 * C8, P, C8, C, HGL_ACT_NONE, st));
  }
  // fused upscaling + hyper-network products; hgl_sam_decoder_fusion(0) / HGL_SAM_DEC_FUSED=0 keep the four launches below
  // (same products, sums associated differently: tests compare the two)
  if (r.fused_tail) {
    HGL_TRY(hgl_launch_dec_tail(keysS.hi, keysS.lo, w->up0_w, w->up0_b, w->up1.w, w->up1.b, w->up3_w, w->up3_b, p.hyper, first_mask,
                                P, g, 1e-6f, low_res, skip, st));
  } else {
    if (r.x3) {
      HGL_TRY(hgl_launch_gemm(hgl_gemm_planes(keysS.hi, keysS.lo, w->up0_w, w->up0_b, p.u1, P * HW, 4 * C4, C), st));
      const HglAct u1S = hgl_act(p.kpe, (size_t)P * HW * 4 * C4, true);   // kpeS is dead from here on
      HGL_TRY(hgl_launch_ln_gelu64(p.u1, w->up1.w, w->up1.b, (long long)P * HW * 4, 1e-6f, u1S.hi, u1S.lo, st));
      HGL_TRY(hgl_launch_gemm(hgl_gemm_planes(u1S.hi, u1S.lo, w->up3_w, w->up3_b, p.u2, P * HW * 4, 4 * C8, C4, HGL_ACT_GELU), st));
    } else {
      HGL_TRY(hgl_launch_gemm(hgl_gemm_linear(p.keys, w->up0_w, w->up0_b, p.u1, P * HW, 4 * C4, C), st));
      HGL_TRY(hgl_launch_ln_gelu64(p.u1, w->up1.w, w->up1.b, (long long)P * HW * 4, 1e-6f, nullptr, nullptr, st));
      HGL_TRY(hgl_launch_gemm(hgl_gemm_linear(p.u1, w->up3_w, w->up3_b, p.u2, P * HW * 4, 4 * C8, C4, HGL_ACT_GELU), st));
    }
    // masks[p, t, pix] = hyper[p, t, :] . upscaled[p, pix, :] for the three multimask tokens, un-shuffled into
    // [P,3,4g,4g] by the same kernel
    HGL_TRY(hgl_launch_hyper_logits(p.u2, p.hyper, P, g, first_mask, low_res, st));
  }
  return HGL_OK;
}

int hgl_sam_decode_points(const HglSamDecoderW* w, const float* emb, const float* points01, int P, float* low_res,
                          float* iou_pred, void* workspace, size_t workspace_bytes, void* stream) {
  HGL_REQUIRE(points01, "sam_decode: null input");
  return decode_impl(w, emb, points01, nullptr, nullptr, 2, nullptr, 1, P, low_res, iou_pred, workspace, workspace_bytes, stream);
}

int hgl_sam_decode_points_gated(const HglSamDecoderW* w, const float* emb, const float* points01, int P, float iou_gate,
                                float* low_res, float* iou_pred, void* workspace, size_t workspace_bytes, void* stream) {
  HGL_REQUIRE(points01, "sam_decode: null input");
  return decode_impl(w, emb, points01, nullptr, nullptr, 2, nullptr, 1, P, low_res, iou_pred, workspace, workspace_bytes, stream, true,
                     iou_gate);
}

// Images per launch sequence: whole images, at most 1024 prompts.  The token-side GEMMs of up to 8192 rows (1170 prompts of 7
// tokens) run on the small-tile kernel whatever their row count (lin()), larger ones on fp32 tiles with other sums: within
// the bound a prompt's rows do not depend on how many images share the launch.
// Where the route of such a launch sequence does not serve several images (DecRoute::multi): 1.
static int dec_multi_images(const HglSamDecoderW* w, int n_img, int ppi) {
  const int most = ppi >= 1024 ? 1 : 1024 / ppi, per = most < n_img ? most : n_img;
  return per > 1 && dec_route(w, per * ppi, per, 2, false, dec_fusion_mask()).multi ? per : 1;
}

// n_img images x ppi prompts.  One image: exactly hgl_sam_decode_points(_gated).  Several: launch sequences over
// dec_multi_images() images each (1: image by image through the one-image path); either way every prompt's rows are those of
// its image's own call.
static int decode_multi(const HglSamDecoderW* w, const float* emb, const float* points01, int n_img, int ppi, float* low_res,
                        float* iou_pred, void* workspace, size_t workspace_bytes, void* stream, bool gated, float iou_gate) {
  HGL_REQUIRE(points01, "sam_decode: null input");
  HGL_REQUIRE(valid_dec(w) && w->dense_pe, "sam_decode: invalid weight struct (dense_pe missing?)");
  HGL_REQUIRE(n_img >= 1 && ppi >= 1 && (long long)n_img * ppi <= 65535, "sam_decode_multi: %d images x %d prompts", n_img, ppi);
  if (n_img == 1)
    return decode_impl(w, emb, points01, nullptr, nullptr, 2, nullptr, 1, ppi, low_res, iou_pred, workspace, workspace_bytes, stream,
                       gated, iou_gate);
  const int per = dec_multi_images(w, n_img, ppi);
  const size_t HW = (size_t)w->grid * w->grid, lowsz = (size_t)3 * 16 * HW;
  for (int i = 0; i < n_img; i += per) {
    const int k = n_img - i < per ? n_img - i : per;
    HGL_TRY(decode_impl(w, emb + i * HW * w->C, points01 + (size_t)i * ppi * 2, nullptr, nullptr, 2, nullptr, 1, k * ppi,
                        low_res + (size_t)i * ppi * lowsz, iou_pred + (size_t)i * ppi * 3, workspace, workspace_bytes, stream, gated,
                        iou_gate, k));
  }
  return HGL_OK;
}

size_t hgl_sam_decode_multi_workspace_bytes(const HglSamDecoderW* w, int n_img, int ppi) {
  if (!valid_dec(w) || n_img <= 0 || ppi <= 0 || (long long)n_img * ppi > 65535) return 0;
  const int per = dec_multi_images(w, n_img, ppi);
  HglArena ar(nullptr, 0);
  DecPlan p;
  carve_dec(ar, w, per * ppi, p, per);
  return ar.off;
}

int hgl_sam_decode_points_multi(const HglSamDecoderW* w, const float* emb, const float* points01, int n_img, int ppi,
                                float* low_res, float* iou_pred, void* workspace, size_t workspace_bytes, void* stream) {
  return decode_multi(w, emb, points01, n_img, ppi, low_res, iou_pred, workspace, workspace_bytes, stream, false, 0.f);
}

int hgl_sam_decode_points_multi_gated(const HglSamDecoderW* w, const float* emb, const float* points01, int n_img, int ppi,
                                      float iou_gate, float* low_res, float* iou_pred, void* workspace, size_t workspace_bytes,
                                      void* stream) {
  return decode_multi(w, emb, points01, n_img, ppi, low_res, iou_pred, workspace, workspace_bytes, stream, true, iou_gate);
}

int hgl_sam_decode_prompts(const HglSamDecoderW* w, const float* emb, const float* coords01, const int32_t* labels, int n_sparse,
                           const float* dense, int first_mask, int P, float* low_res, float* iou_pred, void* workspace,
                           size_t workspace_bytes, void* stream) {
  HGL_REQUIRE(coords01 && labels, "sam_decode_prompts: null input");
  return decode_impl(w, emb, nullptr, coords01, labels, n_sparse, dense, first_mask, P, low_res, iou_pred, workspace,
                     workspace_bytes, stream);
}

int hgl_sam_embed_masks(const HglSamDecoderW* w, const float* mask_input, int P, float* dense, void* stream) {
  HGL_TRY(hgl_require_device());
  HGL_REQUIRE(w && mask_input && dense && P > 0 && P <= 65535, "sam_embed_masks: bad arguments");
  HGL_REQUIRE(w->md_c1_w && w->md_c1_b && w->md_n1_w && w->md_n1_b && w->md_c2_w && w->md_c2_b && w->md_n2_w && w->md_n2_b &&
              w->md_c3_w && w->md_c3_b, "sam_embed_masks: the weight struct lacks mask_downscaling");
  HGL_REQUIRE(w->C == 256, "sam_embed_masks: embedding width %d unsupported", w->C);
  return hgl_launch_mask_downscaling(mask_input, P, w->grid, w->md_c1_w, w->md_c1_b, w->md_n1_w, w->md_n1_b, w->md_c2_w, w->md_c2_b,
                                     w->md_n2_w, w->md_n2_b, w->md_c3_w, w->md_c3_b, dense, (hipStream_t)stream);
}

}  // extern "C"
