"""Drop-in for the segment-anything surface Hybridgl_main.py uses (Hybridgl_main.py:66-74,85):
`sam_model_registry[...]`, `SamAutomaticMaskGenerator(model, ...).generate(image)`.

The ViT-H image encoder, the prompt encoder, the two-way mask decoder and the fused mask
post-processing (upsampling, thresholds, stability score, boxes, NMS, connected-component clean-up)
and the Pillow-exact ResizeLongestSide resize run in libhybridgl.so (hand-written HIP).  Host work
kept here: the point grid, the two proposal counts read back, and the list-of-dict packaging.
"""
import ctypes as C
import os

import numpy as np
import torch

from . import _lib, ops, weights
from ._lib import check


from ._lib import (HglLinearW, HglNormW, HglSamAttnW, HglSamBlockW, HglSamDecoderW,  # noqa: E402
                   HglSamEncoderW)


def _dev(a, device):
    if isinstance(a, torch.Tensor):
        t = a.detach().to(torch.float32)
    else:
        t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
    return t.contiguous().to(device)


def _image_on(image, device):
    """an image [H,W,3] uint8, numpy or tensor, as a tensor on the device"""
    return image if isinstance(image, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(image)).to(device)


def _xywh(boxes_xyxy):
    """box_xyxy_to_xywh (utils/amg.py:255-259) as int64"""
    b = boxes_xyxy.long()
    return torch.stack([b[:, 0], b[:, 1], b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]], 1)


def load_sam_state_dict(path):
    """`torch.load` of the released checkpoint (build_sam.py:103-106)."""
    sd = torch.load(path, map_location="cpu")
    return {k: v.float().numpy() for k, v in sd.items()}


class Sam:
    """Weights of segment_anything.modeling.Sam on the device + the C weight structs."""

    mask_threshold = 0.0  # modeling/sam.py:19
    image_format = "RGB"

    def __init__(self, state_dict, cfg, device="cuda", precision=None):
        _lib.load()
        import weakref
        precision = precision or ops.default_precision()
        ops.use_precision(precision)
        self.precision = precision
        _before = set(ops._split_cache)
        self.cfg = dict(cfg)
        self.device = torch.device(device)
        self._t = []  # keep every device tensor alive
        sd = state_dict
        D, L, H = cfg["embed_dim"], cfg["depth"], cfg["num_heads"]
        S, ps, Cc = cfg["img_size"], cfg["patch_size"], cfg["out_chans"]
        g = S // ps
        self.img_size, self.grid = S, g

        def t(a):
            x = _dev(a, self.device)
            self._t.append(x)
            return x.data_ptr()

        e = "image_encoder"
        self._blocks = (HglSamBlockW * L)()
        for i in range(L):
            b, p = self._blocks[i], f"{e}.blocks.{i}"
            b.window = 0 if i in cfg["global_attn_indexes"] else cfg["window_size"]
            b.rel_len = sd[f"{p}.attn.rel_pos_h"].shape[0]
            for f, k in [("norm1_w", "norm1.weight"), ("norm1_b", "norm1.bias"), ("qkv_w", "attn.qkv.weight"),
                         ("qkv_b", "attn.qkv.bias"), ("proj_w", "attn.proj.weight"), ("proj_b", "attn.proj.bias"),
                         ("rel_pos_h", "attn.rel_pos_h"), ("rel_pos_w", "attn.rel_pos_w"),
                         ("norm2_w", "norm2.weight"), ("norm2_b", "norm2.bias"), ("lin1_w", "mlp.lin1.weight"),
                         ("lin1_b", "mlp.lin1.bias"), ("lin2_w", "mlp.lin2.weight"), ("lin2_b", "mlp.lin2.bias")]:
                setattr(b, f, t(sd[f"{p}.{k}"]))
                if ops.split_mode(precision) and f in ("qkv_w", "proj_w", "lin1_w", "lin2_w"):
                    ops.register_split_weight(self._t[-1])
                if ops.split_mode(precision) and f in ("rel_pos_h", "rel_pos_w") and b.window == 14 and self._t[-1].shape == (27, 80):
                    # the windowed attention multiplies with these tables on the matrix cores: split once here (unscaled)
                    # instead of per wave and item in the kernel
                    ops.register_split_weight(self._t[-1], scale_log2=0)
        enc = HglSamEncoderW()
        enc.embed_dim, enc.depth, enc.heads, enc.img_size, enc.patch, enc.out_chans = D, L, H, S, ps, Cc
        enc.patch_w = t(np.asarray(sd[f"{e}.patch_embed.proj.weight"]).reshape(D, -1))
        enc.patch_b = t(sd[f"{e}.patch_embed.proj.bias"])
        enc.pos_embed = t(np.asarray(sd[f"{e}.pos_embed"]).reshape(g * g, D))
        enc.blocks = C.cast(self._blocks, C.POINTER(HglSamBlockW))
        enc.neck0_w = t(np.asarray(sd[f"{e}.neck.0.weight"]).reshape(Cc, D))
        enc.neck1_w, enc.neck1_b = t(sd[f"{e}.neck.1.weight"]), t(sd[f"{e}.neck.1.bias"])
        enc.neck2_w = t(np.asarray(sd[f"{e}.neck.2.weight"]).reshape(Cc, Cc * 9))
        enc.neck3_w, enc.neck3_b = t(sd[f"{e}.neck.3.weight"]), t(sd[f"{e}.neck.3.bias"])
        if ops.split_mode(precision):     # patch embedding and neck convolutions as split-fp16 GEMMs (K % 64 == 0 permitting)
            for x in self._t:
                if x.data_ptr() in (enc.patch_w, enc.neck0_w, enc.neck2_w) and x.shape[1] % 64 == 0:
                    ops.register_split_weight(x)
        self.enc_w = enc

        m, pe = "mask_decoder", "prompt_encoder"
        dec = HglSamDecoderW()
        dec.C, dec.grid, dec.heads, dec.mlp_dim = Cc, g, 8, sd[f"{m}.transformer.layers.0.mlp.lin1.weight"].shape[0]
        dec.pe_gauss = t(sd[f"{pe}.pe_layer.positional_encoding_gaussian_matrix"])
        dec.point_embed_pos = t(np.asarray(sd[f"{pe}.point_embeddings.1.weight"]).reshape(-1))
        dec.not_a_point = t(np.asarray(sd[f"{pe}.not_a_point_embed.weight"]).reshape(-1))
        dec.point_embed_neg = t(np.asarray(sd[f"{pe}.point_embeddings.0.weight"]).reshape(-1))
        dec.point_embed_box0 = t(np.asarray(sd[f"{pe}.point_embeddings.2.weight"]).reshape(-1))
        dec.point_embed_box1 = t(np.asarray(sd[f"{pe}.point_embeddings.3.weight"]).reshape(-1))
        if f"{pe}.mask_downscaling.0.weight" in sd and tuple(np.asarray(sd[f"{pe}.mask_downscaling.3.weight"]).shape) == (16, 4, 2, 2):
            md = f"{pe}.mask_downscaling"                      # prompt_encoder.py:57-66 (mask_in_chans = 16)
            for dst, key, shape in (("md_c1_w", "0.weight", (4, 4)), ("md_c1_b", "0.bias", (4,)), ("md_n1_w", "1.weight", (4,)),
                                    ("md_n1_b", "1.bias", (4,)), ("md_c2_w", "3.weight", (16, 16)), ("md_c2_b", "3.bias", (16,)),
                                    ("md_n2_w", "4.weight", (16,)), ("md_n2_b", "4.bias", (16,)),
                                    ("md_c3_w", "6.weight", (Cc, 16)), ("md_c3_b", "6.bias", (Cc,))):
                setattr(dec, dst, t(np.asarray(sd[f"{md}.{key}"]).reshape(shape)))
        dec.no_mask = t(np.asarray(sd[f"{pe}.no_mask_embed.weight"]).reshape(-1))
        dec.iou_token = t(np.asarray(sd[f"{m}.iou_token.weight"]).reshape(-1))
        dec.mask_tokens = t(sd[f"{m}.mask_tokens.weight"])

        def lin(dst, key):
            dst.w, dst.b = t(sd[f"{key}.weight"]), t(sd[f"{key}.bias"])
            wshape = np.asarray(sd[f"{key}.weight"]).shape
            if ops.split_mode(precision) and len(wshape) == 2 and wshape[1] % 16 == 0:
                ops.register_split_weight(self._t[-2])     # small-M GEMMs of the decoder (token MLPs, hyper-nets, IoU head)

        def attn(dst, key):
            for nm in ("q", "k", "v", "out"):
                lin(getattr(dst, nm), f"{key}.{nm}_proj")
            dst.internal = sd[f"{key}.q_proj.weight"].shape[0]

        for i in range(2):
            l, lay = f"{m}.transformer.layers.{i}", dec.layer[i]
            attn(lay.self_attn, f"{l}.self_attn")
            attn(lay.t2i, f"{l}.cross_attn_token_to_image")
            attn(lay.i2t, f"{l}.cross_attn_image_to_token")
            for j, nm in enumerate(("n1", "n2", "n3", "n4")):
                lin(getattr(lay, nm), f"{l}.norm{j + 1}")
            lin(lay.lin1, f"{l}.mlp.lin1")
            lin(lay.lin2, f"{l}.mlp.lin2")
        attn(dec.final_t2i, f"{m}.transformer.final_attn_token_to_image")
        lin(dec.norm_final, f"{m}.transformer.norm_final_attn")
        # ConvTranspose2d(k=2,s=2) weights [Cin,Cout,2,2] -> GEMM rows ordered (ky,kx,cout)
        w0 = np.asarray(sd[f"{m}.output_upscaling.0.weight"])
        dec.up0_w = t(np.transpose(w0, (2, 3, 1, 0)).reshape(-1, w0.shape[0]))
        if ops.split_mode(precision):
            ops.register_split_weight(self._t[-1])
        dec.up0_b = t(np.tile(np.asarray(sd[f"{m}.output_upscaling.0.bias"]), 4))
        lin(dec.up1, f"{m}.output_upscaling.1")
        w3 = np.asarray(sd[f"{m}.output_upscaling.3.weight"])
        dec.up3_w = t(np.transpose(w3, (2, 3, 1, 0)).reshape(-1, w3.shape[0]))
        if ops.split_mode(precision):
            ops.register_split_weight(self._t[-1])
        dec.up3_b = t(np.tile(np.asarray(sd[f"{m}.output_upscaling.3.bias"]), 4))
        for i in range(4):
            for j in range(3):
                lin(dec.hyper[i][j], f"{m}.output_hypernetworks_mlps.{i}.layers.{j}")
        for j in range(3):
            lin(dec.iou_head[j], f"{m}.iou_prediction_head.layers.{j}")
        # dense positional encoding of the embedding grid, once (prompt_encoder.py:194-205)
        ax = ((np.arange(g, dtype=np.float32) + np.float32(1)) - np.float32(0.5)) / np.float32(g)
        coords = np.stack(np.broadcast_arrays(ax[None, :], ax[:, None]), axis=-1).reshape(-1, 2)
        self.dense_pe = torch.empty((g * g, Cc), dtype=torch.float32, device=self.device)
        dec.dense_pe = self.dense_pe.data_ptr()
        cd = _dev(coords, self.device)
        check(_lib.load().hgl_sam_dense_pe(C.byref(dec), cd.data_ptr(), self.dense_pe.data_ptr(), ops._stream()),
              "hgl_sam_dense_pe")
        torch.cuda.current_stream().synchronize()
        if ops.split_mode(precision) and Cc == 256:
            # merged image-side projections of the decoder (HglSamDecoderW.kvq1 / kvf): concatenated weights, and the
            # positional-encoding part of k and q as per-position tables: (keys + pe) W^T = keys W^T + pe W^T
            def cat_w(keys):
                w = torch.cat([_dev(sd[f"{k}.weight"], self.device) for k in keys], 0).contiguous()
                b = torch.cat([_dev(sd[f"{k}.bias"], self.device) for k in keys], 0).contiguous()
                self._t += [w, b]
                ops.register_split_weight(w)
                return w, b

            def pe_table(keys, with_pe):
                cols = []
                for k, use in zip(keys, with_pe):
                    wk = _dev(sd[f"{k}.weight"], self.device)
                    cols.append(ops.gemm(self.dense_pe, wk) if use else
                                torch.zeros((self.dense_pe.shape[0], wk.shape[0]), dtype=torch.float32, device=self.device))
                tab = torch.cat(cols, 1).contiguous()
                self._t.append(tab)
                return tab
            l1 = f"{m}.transformer.layers.1"
            k1 = [f"{l1}.cross_attn_token_to_image.k_proj", f"{l1}.cross_attn_token_to_image.v_proj",
                  f"{l1}.cross_attn_image_to_token.q_proj"]
            kf = [f"{m}.transformer.final_attn_token_to_image.k_proj", f"{m}.transformer.final_attn_token_to_image.v_proj"]
            w1, b1 = cat_w(k1)
            wf, bf = cat_w(kf)
            dec.kvq1_w, dec.kvq1_b, dec.kvq1_pe = w1.data_ptr(), b1.data_ptr(), pe_table(k1, (True, False, True)).data_ptr()
            dec.kvf_w, dec.kvf_b, dec.kvf_pe = wf.data_ptr(), bf.data_ptr(), pe_table(kf, (True, False)).data_ptr()
            # the token -> image attention on the raw image tokens (csrc/sam_decoder_t2i.hip) multiplies its folded queries with
            # the positional encoding as a GEMM "weight" [HW, C]
            ops.register_split_weight(self.dense_pe)
            torch.cuda.current_stream().synchronize()
        self.dec_w = dec
        # the fp16 splits registered above die with this model (library registry + hi/lo tensors)
        self._split_keys = ops.split_weight_keys_since(_before)
        weakref.finalize(self, ops.release_split_weights, list(self._split_keys))

    def to(self, device):
        if torch.device(device).type != "cuda":
            raise _lib.HybridGLError("Sam runs on the GPU only (no CPU path exists)")
        return self

    def eval(self):
        return self

    # ---- the three device stages -------------------------------------------------------
    def encode(self, resized_u8):
        """resized_u8: [h,w,3] uint8 device tensor (long side == img_size) -> emb [g*g, C]."""
        lib = _lib.load()
        ops.use_precision(self.precision)
        h, w = resized_u8.shape[:2]
        need = lib.hgl_sam_encode_workspace_bytes(C.byref(self.enc_w))
        ws = ops.workspace(need, self.device, "sam_encode")
        emb = torch.empty((self.grid * self.grid, self.cfg["out_chans"]), dtype=torch.float32, device=self.device)
        check(lib.hgl_sam_encode(C.byref(self.enc_w), ops._dev(resized_u8, torch.uint8, "resized_img"), h, w,
                                 emb.data_ptr(), ws.data_ptr(), ws.numel(), ops._stream()), "hgl_sam_encode")
        return emb

    def encode_batch(self, resized_list):
        """several images through the encoder at once (token rows stacked: weights read once, better-filled GEMMs).
        resized_list: [h_i,w_i,3] uint8 device tensors -> emb [nb, g*g, C]; each slice equals encode() of that image
        up to the summation order of split-K."""
        lib = _lib.load()
        ops.use_precision(self.precision)
        nb = len(resized_list)
        imgs = [r.contiguous() for r in resized_list]
        ptrs = (C.c_void_p * nb)(*[ops._dev(r, torch.uint8, "resized_img") for r in imgs])
        hs = (C.c_int * nb)(*[int(r.shape[0]) for r in imgs])
        wsz = (C.c_int * nb)(*[int(r.shape[1]) for r in imgs])
        need = lib.hgl_sam_encode_batch_workspace_bytes(C.byref(self.enc_w), nb)
        ws = ops.workspace(need, self.device, "sam_encode")
        emb = torch.empty((nb, self.grid * self.grid, self.cfg["out_chans"]), dtype=torch.float32, device=self.device)
        check(lib.hgl_sam_encode_batch(C.byref(self.enc_w), ptrs, hs, wsz, nb, emb.data_ptr(), ws.data_ptr(), ws.numel(),
                                       ops._stream()), "hgl_sam_encode_batch")
        return emb

    def _decode(self, entry, P, ws_query, ws_args, *args):
        """The outputs and the workspace of P prompts, and the call of one decoder entry point, all of which end in
        (..., low_res, iou, workspace, workspace_bytes, stream) behind their own arguments args; ws_query(dec_w, *ws_args):
        the entry point's workspace size -> (low_res [P,3,4g,4g], iou [P,3])."""
        lib = _lib.load()
        ops.use_precision(self.precision)
        ws = ops.workspace(getattr(lib, ws_query)(C.byref(self.dec_w), *ws_args), self.device, "sam_decode")
        g4 = 4 * self.grid
        low = torch.empty((P, 3, g4, g4), dtype=torch.float32, device=self.device)
        iou = torch.empty((P, 3), dtype=torch.float32, device=self.device)
        check(getattr(lib, entry)(C.byref(self.dec_w), *args, low.data_ptr(), iou.data_ptr(), ws.data_ptr(), ws.numel(),
                                  ops._stream()), entry)
        return low, iou

    def decode_points(self, emb, points01, iou_gate=None):
        """points01: [P,2] fp32 device ((point+0.5)/img_size) -> (low_res [P,3,4g,4g], iou [P,3]).
        iou_gate: a pred_iou_thresh the caller will filter with (automatic_mask_generator.py:287-291): prompts none of whose
        three predictions exceeds it skip the output upscaling -- their rows of low_res are unwritten memory, which the caller's
        filter never reads (hgl_sam_decode_points_gated)."""
        P = int(points01.shape[0])
        gated = iou_gate is not None
        return self._decode("hgl_sam_decode_points_gated" if gated else "hgl_sam_decode_points", P,
                            "hgl_sam_decode_workspace_bytes", (P,), ops._dev(emb, torch.float32, "emb"),
                            ops._dev(points01, torch.float32, "points01"), P, *((float(iou_gate),) if gated else ()))

    def decode_points_multi(self, emb, points01, n_img, iou_gate=None):
        """decode_points for the prompts of SEVERAL images in one call: emb [n_img, g*g, C], points01 [n_img * ppi, 2], prompt p
        belongs to image p // ppi -> (low_res [n_img*ppi,3,4g,4g], iou [n_img*ppi,3]); every prompt's rows are bit for bit
        those of decode_points on its image's own ppi prompts (hgl_sam_decode_points_multi)."""
        P = int(points01.shape[0])
        n_img = int(n_img)
        if n_img < 1 or P % n_img or tuple(emb.shape[:1]) != (n_img,):
            raise ValueError(f"{P} prompts / embeddings {tuple(emb.shape)} for {n_img} images")
        ppi = P // n_img
        gated = iou_gate is not None
        return self._decode("hgl_sam_decode_points_multi_gated" if gated else "hgl_sam_decode_points_multi", P,
                            "hgl_sam_decode_multi_workspace_bytes", (n_img, ppi), ops._dev(emb, torch.float32, "emb"),
                            ops._dev(points01, torch.float32, "points01"), n_img, ppi, *((float(iou_gate),) if gated else ()))

    def decode_prompts(self, emb, coords01, labels, first_mask=1, dense=None):
        """prompts of two or three sparse tokens (prompt_encoder.py:73-101): coords01 [P,n,2] fp32 device
        ((coordinate + 0.5) / img_size), labels [P,n] int32 (-1 padding, 0 / 1 background / foreground point, 2 / 3 box
        corners); dense: None or [P, g*g, C] from embed_masks; first_mask 1 -> mask tokens 1..3 (multimask), 0 -> tokens 0..2
        (column 0 = the single-mask output) -> (low_res [P,3,4g,4g], iou [P,3])."""
        P, n = int(coords01.shape[0]), int(coords01.shape[1])
        return self._decode("hgl_sam_decode_prompts", P, "hgl_sam_decode_workspace_bytes", (P,),
                            ops._dev(emb, torch.float32, "emb"), ops._dev(coords01, torch.float32, "coords01"),
                            ops._dev(labels, torch.int32, "labels"), n,
                            None if dense is None else ops._dev(dense, torch.float32, "dense"), int(first_mask), P)

    def embed_masks(self, mask_input):
        """PromptEncoder._embed_masks (prompt_encoder.py:103-106): [P,1,4g,4g] fp32 device -> dense rows [P, g*g, C]"""
        lib = _lib.load()
        P = int(mask_input.shape[0])
        g4 = 4 * self.grid
        if tuple(mask_input.shape) != (P, 1, g4, g4):
            raise ValueError(f"mask_input must be [P,1,{g4},{g4}], got {tuple(mask_input.shape)}")
        dense = torch.empty((P, self.grid * self.grid, self.dec_w.C), dtype=torch.float32, device=self.device)
        check(lib.hgl_sam_embed_masks(C.byref(self.dec_w), ops._dev(mask_input, torch.float32, "mask_input"), P, dense.data_ptr(),
                                      ops._stream()), "hgl_sam_embed_masks")
        return dense

    def postprocess(self, low_res, iou_pred, input_size, original_size, pred_iou_thresh=-1e30,
                    stability_thresh=0.0, stability_offset=1.0, return_logits=False):
        """low_res [K,hl,wl], iou_pred [K] -> masks [K,H,W] u8, boxes XYXY [K,4] i32, stability [K], keep [K]."""
        lib = _lib.load()
        K, hl, wl = low_res.shape
        H, W = original_size
        dev = self.device
        masks = torch.empty((K, H, W), dtype=torch.uint8, device=dev)
        boxes = torch.empty((K, 4), dtype=torch.int32, device=dev)
        stab = torch.empty((K,), dtype=torch.float32, device=dev)
        keep = torch.empty((K,), dtype=torch.uint8, device=dev)
        full = torch.empty((K, H, W), dtype=torch.float32, device=dev) if return_logits else None
        need = lib.hgl_sam_postprocess_workspace_bytes(K)
        ws = ops.workspace(need, dev, "sam_post")
        check(lib.hgl_sam_postprocess(ops._dev(low_res, torch.float32, "low_res"),
                                      ops._dev(iou_pred, torch.float32, "iou_pred"), K, hl, wl, self.img_size,
                                      int(input_size[0]), int(input_size[1]), H, W, float(self.mask_threshold),
                                      float(stability_offset), float(pred_iou_thresh), float(stability_thresh),
                                      masks.data_ptr(), boxes.data_ptr(), stab.data_ptr(), keep.data_ptr(),
                                      full.data_ptr() if full is not None else None, ws.data_ptr(), ws.numel(),
                                      ops._stream()), "hgl_sam_postprocess")
        return masks, boxes, stab, keep, full


def nms(boxes_xyxy, scores, keep, iou_threshold):
    """Device NMS -> (idx [K] int32, n [1] int32), both on the device.  K <= 1024: one workgroup; larger K
    (dense grids, crop layers): the three-pass bit-matrix kernels (nms_large), same semantics."""
    lib = _lib.load()
    K = boxes_xyxy.shape[0]
    if K > 1024:
        return nms_large(boxes_xyxy, scores, keep, iou_threshold)
    idx = torch.empty((K,), dtype=torch.int32, device=boxes_xyxy.device)
    n = torch.empty((1,), dtype=torch.int32, device=boxes_xyxy.device)
    check(lib.hgl_nms(ops._dev(boxes_xyxy, torch.int32, "boxes"), ops._dev(scores, torch.float32, "scores"),
                      ops._dev(keep, torch.uint8, "keep"), K, float(iou_threshold), idx.data_ptr(), n.data_ptr(),
                      ops._stream()), "hgl_nms")
    return idx, n


def nms_segments(boxes_xyxy, scores, keep, offsets, max_len, iou_threshold):
    """nms() for several candidate lists in one launch (hgl_nms_segments): list s = candidates offsets[s] .. offsets[s+1]
    (offsets: int32 device tensor [n_seg + 1], ascending from 0; max_len: the longest list, <= 1024) -> (idx [K] int32: from
    position offsets[s] on, the kept candidates of list s as indices INTO the list; n [n_seg] int32)."""
    lib = _lib.load()
    K, n_seg = boxes_xyxy.shape[0], offsets.shape[0] - 1
    idx = torch.empty((K,), dtype=torch.int32, device=boxes_xyxy.device)
    n = torch.empty((n_seg,), dtype=torch.int32, device=boxes_xyxy.device)
    check(lib.hgl_nms_segments(ops._dev(boxes_xyxy, torch.int32, "boxes"), ops._dev(scores, torch.float32, "scores"),
                               ops._dev(keep, torch.uint8, "keep"), ops._dev(offsets, torch.int32, "offsets"), n_seg, int(max_len),
                               float(iou_threshold), idx.data_ptr(), n.data_ptr(), ops._stream()), "hgl_nms_segments")
    return idx, n


def nms_large(boxes_xyxy, scores, keep, iou_threshold):
    """hgl_nms_large regardless of K: nms() above 1024 candidates (and the tests below that)."""
    lib = _lib.load()
    K = boxes_xyxy.shape[0]
    idx = torch.empty((K,), dtype=torch.int32, device=boxes_xyxy.device)
    n = torch.empty((1,), dtype=torch.int32, device=boxes_xyxy.device)
    ws = ops.workspace(lib.hgl_nms_large_workspace_bytes(K), boxes_xyxy.device, "nms_large")
    check(lib.hgl_nms_large(ops._dev(boxes_xyxy, torch.int32, "boxes"), ops._dev(scores, torch.float32, "scores"),
                            ops._dev(keep, torch.uint8, "keep"), K, float(iou_threshold), idx.data_ptr(), n.data_ptr(),
                            ws.data_ptr(), ws.numel(), ops._stream()), "hgl_nms_large")
    return idx, n


def box_near_crop_edge(boxes_xyxy, keep, crop_box, orig_box, atol=20.0):
    """keep[i] = 0 where box i (crop coordinates) touches a crop edge that is not an image edge (amg.py:78-88)."""
    import ctypes as C
    lib = _lib.load()
    cb = (C.c_int32 * 4)(*[int(v) for v in crop_box])
    ob = (C.c_int32 * 4)(*[int(v) for v in orig_box])
    check(lib.hgl_box_near_crop_edge(ops._dev(boxes_xyxy, torch.int32, "boxes"), boxes_xyxy.shape[0], cb, ob, float(atol),
                                     ops._dev(keep, torch.uint8, "keep"), ops._stream()), "hgl_box_near_crop_edge")
    return keep


def _build(cfg_name, checkpoint=None, state_dict=None, seed=0, device="cuda", precision=None):
    checkpoint = checkpoint or os.environ.get("HYBRIDGL_SAM_CHECKPOINT")
    if state_dict is None and checkpoint:
        state_dict = load_sam_state_dict(checkpoint)
    if state_dict is None:
        state_dict = weights.sam_state_dict(cfg_name, seed)
    return Sam(state_dict, weights.SAM_CONFIGS[cfg_name], device, precision)


def build_sam_vit_h(checkpoint=None, **kw):
    """build_sam.py:14-21."""
    return _build("vit_h", checkpoint, **kw)


# build_sam.py:47-52 (Hybridgl_main.py:66 uses 'default' = vit_h)
sam_model_registry = {"default": build_sam_vit_h, "vit_h": build_sam_vit_h,
                      "vit_l": lambda checkpoint=None, **kw: _build("vit_l", checkpoint, **kw),
                      "vit_b": lambda checkpoint=None, **kw: _build("vit_b", checkpoint, **kw),
                      "tiny": lambda checkpoint=None, **kw: _build("tiny", checkpoint, **kw)}


_PIL_PB = 22
_coeff_cache = {}


def pil_bilinear_coeffs(in_size, out_size):
    """Pillow's precompute_coeffs + normalize_coeffs_8bpc for the bilinear filter (host, double precision):
    int32 weights [out, ksize] and (first, count) bounds."""
    import math
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = 1.0 * fs
    ksize = int(math.ceil(support)) * 2 + 1
    kk = np.zeros((out_size, ksize), dtype=np.int32)
    bounds = np.zeros((out_size, 2), dtype=np.int32)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        cnt = min(int(center + support + 0.5), in_size) - xmin
        w = [max(0.0, 1.0 - abs((x + xmin - center + 0.5) / fs)) for x in range(cnt)]
        ww = sum(w)
        for x in range(cnt):
            kk[xx, x] = int(0.5 + (w[x] / ww if ww != 0.0 else w[x]) * (1 << _PIL_PB))
        bounds[xx] = (xmin, cnt)
    return kk, bounds


def resize_longest_side(img_u8, long_side):
    """ResizeLongestSide.apply_image on the device, bit-exact with Pillow: img_u8 [H,W,3] uint8 device tensor."""
    lib = _lib.load()
    H, W, Cc = img_u8.shape
    nh, nw = get_preprocess_shape(H, W, long_side)
    key = (H, W, nh, nw, str(img_u8.device))
    tabs = _coeff_cache.get(key)
    if tabs is None:
        kx, bx = pil_bilinear_coeffs(W, nw)
        ky, by = pil_bilinear_coeffs(H, nh)
        tabs = tuple(torch.from_numpy(a).to(img_u8.device) for a in (kx, bx, ky, by))
        _coeff_cache[key] = tabs
    kx, bx, ky, by = tabs
    out = torch.empty((nh, nw, Cc), dtype=torch.uint8, device=img_u8.device)
    need = lib.hgl_resize_pil_bilinear_workspace_bytes(H, nw, Cc)
    ws = ops.workspace(need, img_u8.device, "pil_resize")
    check(lib.hgl_resize_pil_bilinear(ops._dev(img_u8, torch.uint8, "img"), H, W, Cc, nh, nw, kx.data_ptr(), bx.data_ptr(),
                                      kx.shape[1], ky.data_ptr(), by.data_ptr(), ky.shape[1], out.data_ptr(),
                                      ws.data_ptr(), ws.numel(), ops._stream()), "hgl_resize_pil_bilinear")
    return out


def build_point_grid(n):
    """utils/amg.py:179-186."""
    off = 1 / (2 * n)
    p = np.linspace(off, 1 - off, n)
    return np.stack([np.tile(p[None, :], (n, 1)), np.tile(p[:, None], (1, n))], axis=-1).reshape(-1, 2)


def build_all_layer_point_grids(n_per_side, n_layers, scale_per_layer):
    """utils/amg.py:189-198."""
    return [build_point_grid(int(n_per_side / (scale_per_layer ** i))) for i in range(n_layers + 1)]


def generate_crop_boxes(im_size, n_layers, overlap_ratio):
    """Crop windows of the crop-layer generator (what utils/amg.py:201-238 produces; pinned by the known answers in
    tests/golden/sam_crops.npz) -> (XYXY boxes, layer index of each).  Layer 0 is the whole image; layer L tiles the
    image with a 2^L x 2^L grid of equal windows that overlap by int(overlap_ratio * short_side * 2 / 2^L) pixels,
    window size = ceil((overlap * (n - 1) + side) / n), origins = int((size - overlap) * k), enumerated x-major,
    clipped to the image."""
    import math
    height, width = im_size
    boxes, layers = [[0, 0, width, height]], [0]
    for layer in range(1, n_layers + 1):
        n = 1 << layer
        overlap = int(overlap_ratio * min(height, width) * (2 / n))
        win_w = int(math.ceil((overlap * (n - 1) + width) / n))
        win_h = int(math.ceil((overlap * (n - 1) + height) / n))
        for kx in range(n):
            x0 = int((win_w - overlap) * kx)
            for ky in range(n):
                y0 = int((win_h - overlap) * ky)
                boxes.append([x0, y0, min(x0 + win_w, width), min(y0 + win_h, height)])
                layers.append(layer)
    return boxes, layers


def get_preprocess_shape(oldh, oldw, long_side):
    """utils/transforms.py:93-102."""
    scale = long_side * 1.0 / max(oldh, oldw)
    return int(oldh * scale + 0.5), int(oldw * scale + 0.5)


class ResizeLongestSide:
    """utils/transforms.py:16-102 (the pieces the predictor uses)."""

    def __init__(self, target_length):
        self.target_length = target_length

    def apply_image(self, image):
        return resize_longest_side(_image_on(image, "cuda").contiguous(), self.target_length)

    def apply_coords(self, coords, original_size):
        """utils/transforms.py:33-45 (float64, as numpy)."""
        old_h, old_w = original_size
        new_h, new_w = get_preprocess_shape(old_h, old_w, self.target_length)
        c = np.array(coords, dtype=np.float64, copy=True)
        c[..., 0] = c[..., 0] * (new_w / old_w)
        c[..., 1] = c[..., 1] * (new_h / old_h)
        return c

    def apply_boxes(self, boxes, original_size):
        """utils/transforms.py:47-53: [B,4] XYXY -> the resized frame"""
        return self.apply_coords(np.asarray(boxes, dtype=np.float64).reshape(-1, 2, 2), original_size).reshape(-1, 4)


class SamPredictor:
    """predictor.py:17-269: set_image, predict_torch, predict.  Points (foreground / background; the padding point follows
    them), a box (its two corners), or points and a box -- up to eleven sparse tokens per prompt --, optionally a mask
    input per prompt (per-prompt dense embeddings); multimask_output True or False.  One point per prompt (what
    automatic_mask_generator.py:269-285 issues) takes the fused decoder stages."""

    def __init__(self, sam_model):
        self.model = sam_model
        self.transform = ResizeLongestSide(sam_model.img_size)
        self.reset_image()

    @property
    def device(self):
        return self.model.device

    def reset_image(self):
        self.is_image_set = False
        self.features = None
        self.original_size = self.input_size = None

    def set_image(self, image, image_format="RGB"):
        assert image_format in ("RGB", "BGR"), f"image_format must be in ['RGB', 'BGR'], is {image_format}."
        img = _image_on(image, self.device)
        if image_format != self.model.image_format:
            img = img.flip(-1)
        self.reset_image()
        self.original_size = tuple(int(v) for v in img.shape[:2])
        resized = resize_longest_side(img.contiguous(), self.model.img_size)
        self.input_size = tuple(int(v) for v in resized.shape[:2])
        self.features = self.model.encode(resized)
        self.is_image_set = True

    def _coords01(self, xy):
        """(coordinate + 0.5) / img_size in the dtype the caller handed over (prompt_encoder.py:79,95,207-214: float64 from
        the automatic generator, float32 from predict()), then float32"""
        xy = torch.as_tensor(xy, device=self.device)
        xy = xy if xy.dtype == torch.float64 else xy.to(torch.float32)
        return ((xy + 0.5) / float(self.model.img_size)).to(torch.float32)

    def predict_torch(self, point_coords, point_labels, boxes=None, mask_input=None, multimask_output=True,
                      return_logits=False):
        """predictor.py:169-243.  point_coords [P,N,2] in the resized frame (transform.apply_coords) with point_labels [P,N]
        in {0, 1}, and / or boxes [P,4] XYXY in the resized frame (transform.apply_boxes), and / or mask_input [P,1,4g,4g]
        (low-resolution logits of an earlier call).  Up to eleven sparse tokens per prompt: points (the padding point
        follows them when there is no box), a box, or points and a box.  Returns (masks [P,C,H,W] bool or logits,
        iou_predictions [P,C], low_res_masks [P,C,4g,4g]) with C = 3 (multimask_output) or 1."""
        if not self.is_image_set:
            raise RuntimeError("An image must be set with .set_image(...) before mask prediction.")   # predictor.py:214
        toks, labs = [], []
        P = None
        if point_coords is not None:
            pc = torch.as_tensor(point_coords, device=self.device)
            pl = torch.as_tensor(point_labels, device=self.device)
            if pc.dim() != 3 or pc.shape[2] != 2 or pl.shape != pc.shape[:2]:
                raise ValueError(f"point_coords must be [P,N,2] with point_labels [P,N], got {tuple(pc.shape)} / {tuple(pl.shape)}")
            if not bool(((pl == 0) | (pl == 1) | (pl == -1)).all()):
                raise ValueError("point_labels must be 1 (foreground), 0 (background) or -1 (padding)")
            P = int(pc.shape[0])
            toks.append(self._coords01(pc))
            labs.append(pl.to(torch.int32))
            if boxes is None:                                                            # prompt_encoder.py:80-84: padding point
                toks.append(torch.zeros((P, 1, 2), dtype=torch.float32, device=self.device))
                labs.append(torch.full((P, 1), -1, dtype=torch.int32, device=self.device))
        if boxes is not None:
            b = torch.as_tensor(boxes, device=self.device)
            if b.dim() != 2 or b.shape[1] != 4 or (P is not None and b.shape[0] != P):
                raise ValueError(f"boxes must be [P,4] (XYXY), got {tuple(b.shape)}")
            P = int(b.shape[0])
            toks.append(self._coords01(b.reshape(-1, 2, 2)))                              # prompt_encoder.py:93-101
            labs.append(torch.tensor([2, 3], dtype=torch.int32, device=self.device).repeat(P, 1))
        if P is None:
            raise NotImplementedError("a prompt needs points and / or a box (a mask input alone has no sparse tokens)")
        c01, labels = torch.cat(toks, dim=1).contiguous(), torch.cat(labs, dim=1).contiguous()
        if c01.shape[1] > 11:
            raise NotImplementedError(f"{c01.shape[1]} sparse tokens per prompt: up to eleven are supported (ten points, or nine "
                                      "points and a box)")
        dense = None
        if mask_input is not None:
            mi = torch.as_tensor(mask_input, device=self.device).to(torch.float32)
            if mi.shape[0] != P:
                raise ValueError(f"mask_input must have one mask per prompt ({P}), got {tuple(mi.shape)}")
            dense = self.model.embed_masks(mi.contiguous())
        fast = (dense is None and boxes is None and multimask_output and c01.shape[1] == 2 and bool((labels[:, 0] == 1).all()))
        if fast:                                                                          # the automatic generator's prompts
            low, iou = self.model.decode_points(self.features, c01[:, 0, :].contiguous())
        else:
            low, iou = self.model.decode_prompts(self.features, c01, labels, first_mask=1 if multimask_output else 0, dense=dense)
            if not multimask_output:
                low, iou = low[:, :1].contiguous(), iou[:, :1].contiguous()
        Cm = low.shape[1]
        H, W = self.original_size
        _, _, _, _, full = self.model.postprocess(low.flatten(0, 1), iou.flatten(), self.input_size, (H, W), -1e30, 0.0, 1.0,
                                                  return_logits=True)
        full = full.reshape(P, Cm, H, W)
        masks = full if return_logits else full > self.model.mask_threshold
        return masks, iou, low

    def predict(self, point_coords=None, point_labels=None, box=None, mask_input=None, multimask_output=True,
                return_logits=False):
        """predictor.py:90-167 for one prompt: points [N,2] with labels [N], a box [4] (XYXY), both in the original frame,
        mask_input [1,4g,4g]: numpy in, numpy out ([C,H,W], [C], [C,4g,4g])."""
        pc = pl = bx = mi = None
        if point_coords is not None:
            assert point_labels is not None, "point_labels must be supplied if point_coords is supplied."
            pts = self.transform.apply_coords(np.asarray(point_coords, dtype=np.float64), self.original_size)
            pc = torch.as_tensor(pts, dtype=torch.float32)[None, :, :]                   # predictor.py:141-143: float32
            pl = torch.as_tensor(np.asarray(point_labels), dtype=torch.int32)[None, :]
        if box is not None:
            bx = torch.as_tensor(self.transform.apply_boxes(np.asarray(box, dtype=np.float64), self.original_size),
                                 dtype=torch.float32).reshape(1, 4)
        if mask_input is not None:
            mi = torch.as_tensor(np.asarray(mask_input), dtype=torch.float32)[None, :, :, :]
        m, iou, low = self.predict_torch(pc, pl, bx, mi, multimask_output=multimask_output, return_logits=return_logits)
        return m[0].cpu().numpy(), iou[0].cpu().numpy(), low[0].cpu().numpy()


class _GroupState:
    """a group of images on its way through SamAutomaticMaskGenerator.group_begin / group_cleanup / group_finish"""
    __slots__ = ("sizes", "crops", "cap", "cand", "n1", "ev1", "ovf", "overflow", "n1_list", "stage", "n2", "ev2")


class SamAutomaticMaskGenerator:
    """automatic_mask_generator.py:35-372.  Proposals go from the decoder's candidates to the final records through ONE tail,
    that of a group of images (group_begin / group_cleanup / group_finish); an image with crop layers is a group of one,
    generate_device the same steps with its two counts read where they are needed.  The Hybridgl_main.py:67-73
    configuration (one crop, 8x8 points) reads two counts per GROUP back (one without the small-region clean-up), crop
    layers / dense grids (Hybridgl_main_PhraseCut.py) three."""

    def __init__(self, model, points_per_side=32, points_per_batch=64, pred_iou_thresh=0.88,
                 stability_score_thresh=0.95, stability_score_offset=1.0, box_nms_thresh=0.7, crop_n_layers=0,
                 crop_nms_thresh=0.7, crop_overlap_ratio=512 / 1500, crop_n_points_downscale_factor=1,
                 point_grids=None, min_mask_region_area=0, output_mode="binary_mask"):
        assert (points_per_side is None) != (point_grids is None), \
            "Exactly one of points_per_side or point_grid must be provided."
        assert output_mode in ["binary_mask", "uncompressed_rle", "coco_rle"], f"Unknown output_mode {output_mode}."
        self.output_mode = output_mode      # automatic_mask_generator.py:103-112 (coco_rle needs no pycocotools here: native codec)
        self.model = model
        self.predictor = SamPredictor(model)
        if point_grids is None:
            self.point_grids = build_all_layer_point_grids(points_per_side, crop_n_layers, crop_n_points_downscale_factor)
        else:
            self.point_grids = point_grids
        assert len(self.point_grids) >= crop_n_layers + 1, "one point grid per crop layer"
        self.crop_n_layers = crop_n_layers
        self.crop_overlap_ratio = crop_overlap_ratio
        # The prompts of ONE image that go through the decoder together.  A group of images decodes many such batches in one
        # launch (_propose_classes), but every batch-dependent choice of the decoder -- the key-range split of its token ->
        # image attention (eight partial sums per prompt for batches of up to 128) -- follows this per-image batch, never the
        # launch's total: a candidate does not depend on how many images share its launch.
        self.points_per_batch = points_per_batch
        self.pred_iou_thresh = pred_iou_thresh
        self.stability_score_thresh = stability_score_thresh
        self.stability_score_offset = stability_score_offset
        self.box_nms_thresh = box_nms_thresh
        self.crop_nms_thresh = crop_nms_thresh
        self.min_mask_region_area = min_mask_region_area
        # the fifth tensor of a finished image names every survivor's origin: crop * source_stride + candidate of that crop
        self.source_stride = 3 * max(len(g) for g in self.point_grids)
        # HybridGLPipeline.run(on_overflow="rescue") sets this for the length of a run: the range guard that rides on a
        # group's count read-back is then ops.split_overflow_snapshot (all three counters) instead of the two-word peek
        self.overflow_snapshot = False

    # ---- small pieces every path shares ---------------------------------------------------------
    def _points(self, H, W, layer_idx=0):
        """the prompt point of every candidate of a crop of H x W, in crop coordinates: [3 * points, 2] float64 (host)"""
        return np.repeat(self.point_grids[layer_idx] * np.array([[W, H]], dtype=np.float64), 3, axis=0)

    def _gate(self):
        """The post-processing drops every candidate whose prediction does not exceed pred_iou_thresh (when that is > 0:
        automatic_mask_generator.py:287-291): prompts that fail with all three masks skip the decoder's upscaling."""
        return float(self.pred_iou_thresh) if self.pred_iou_thresh > 0 and getattr(self, "iou_gate", True) else None

    def _empty(self, H, W):
        """the tensors of an image without a survivor"""
        dev, e = self.model.device, torch.empty
        return (e((0, H, W), dtype=torch.uint8, device=dev), e((0, 4), dtype=torch.int64, device=dev),
                e((0,), device=dev), e((0,), device=dev), e((0,), dtype=torch.int64, device=dev))

    def _read_back(self, counts, overflow=False):
        """A device tensor of counts on its way to the host, nothing waited for: (pinned copy, the event behind it, None).
        overflow: the fp16 range guard of the f16x3 mode rides on the same read-back -- the third element is the pinned pair
        of counters, what the device had counted (any stream) when this stream got here: the caller stops at this group
        instead of finding out at the end of the dataset.  With self.overflow_snapshot it is the pinned triple of
        ops.split_overflow_snapshot, the SAM decoder's counter included."""
        host = torch.empty(counts.shape[0], dtype=torch.int32).pin_memory()
        host.copy_(counts, non_blocking=True)
        ovf = None
        if overflow and self.overflow_snapshot:
            ovf = torch.zeros(3, dtype=torch.int32).pin_memory()
            ops.split_overflow_snapshot(ovf)
        elif overflow:
            ovf = torch.zeros(2, dtype=torch.int32).pin_memory()
            ops.split_overflow_peek(ovf)     # (the counters are process-wide: the CLIP / GEM models of the loop may be f16x3 when this one is not)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(self.model.device))
        return host, ev, ovf

    def _cleanup(self, m, counts, offs=None):
        """postprocess_small_regions (automatic_mask_generator.py:324-372) on the device, without its read-back: m [total,H,W]
        uint8, the masks of one or several images packed image by image, counts their number per image.  Holes, then islands
        with the boxes of what remains, one image per call into slices of the outputs (by measurement, see group_cleanup);
        untouched masks score 1 in the NMS at max(box_nms_thresh, crop_nms_thresh) that follows.  offs (int32 device tensor
        [len(counts) + 1], the packed offsets): ONE segmented launch, a list per image of at most 1024; None: the masks are ONE
        list of any length.  -> (masks, boxes XYXY i32, order [total] i32, n [len(counts)] i32)"""
        area, total, dev = self.min_mask_region_area, m.shape[0], m.device
        m1, c1 = torch.empty_like(m), torch.empty((total,), dtype=torch.uint8, device=dev)
        m2, c2 = torch.empty_like(m), torch.empty((total,), dtype=torch.uint8, device=dev)
        nb = torch.empty((total, 4), dtype=torch.int32, device=dev)
        o = 0
        for c in counts:
            if c > 0:
                sl = slice(o, o + c)
                remove_small_regions(m[sl], area, "holes", out=(m1[sl], c1[sl]))
                remove_small_regions_boxes(m1[sl], area, "islands", out=(m2[sl], c2[sl], nb[sl]))
            o += c
        unchanged = ((c1 | c2) == 0).to(torch.float32)           # score 1 for untouched masks
        keep = torch.ones(total, dtype=torch.uint8, device=dev)
        thresh = max(self.box_nms_thresh, self.crop_nms_thresh)
        if offs is not None and max(counts) <= 1024:
            order, n = nms_segments(nb, unchanged, keep, offs, max(counts), thresh)
        else:
            assert len(counts) == 1, "more than 1024 survivors of one image: the segmented NMS does not take them"
            order, n = nms(nb, unchanged, keep, thresh)
        return m2, nb, order, n

    def cleanup_fixed(self, m):
        """postprocess_small_regions kernels on a fixed batch of masks [n,H,W] uint8 without reading any
        count back: holes, islands, boxes, second NMS (its order is left on the device)."""
        if self.min_mask_region_area <= 0:
            return m, mask_boxes(m)
        return self._cleanup(m, [m.shape[0]])[:2]

    # ---- device part: everything up to and including the first NMS, no host sync -----------
    def propose(self, image, resized=None, layer_idx=0, crop_box=None, orig_size=None):
        """image: uint8 [H,W,3] numpy or device tensor: the crop (automatic_mask_generator.py:222-267; the whole
        image in the reference's own configuration).  crop_box / orig_size (H, W) of the full image enable the
        crop-edge filter (:305-307).
        Returns device tensors (masks [K,H,W] u8, boxes_xyxy [K,4] i32, iou [K], stab [K], order [K] i32,
        n [1] i32, points [K,2] float64 numpy): candidates order[:n] survive the filters + NMS; boxes, masks and
        points are in crop coordinates."""
        m = self.model
        H, W = image.shape[:2]
        nh, nw = get_preprocess_shape(H, W, m.img_size)
        if resized is None:
            # ResizeLongestSide.apply_image (utils/transforms.py:26-31): Pillow's bilinear resampler, bit-exact, on the device
            resized = resize_longest_side(_image_on(image, m.device).contiguous(), m.img_size)
        emb = m.encode(resized)
        return self._propose_from_embedding(emb, H, W, nh, nw, layer_idx, crop_box, orig_size)

    def propose_batch(self, images, encoded_event=None):
        """propose() for several whole images with ONE encoder pass over all of them (Sam.encode_batch) and, per class of
        images of one size, ONE decoder call, ONE post-processing call and ONE NMS launch (_propose_classes).  Returns the
        list of propose() tuples, bit for bit what propose() gives for each image alone up to the encoder's batching.
        encoded_event: a torch.cuda.Event that is recorded behind the encoder pass (the boundary between the GEMM-bound
        and the latency-bound part of the stage)."""
        out = [None] * len(images)
        for idxs, (masks, boxes, iou, stab, order, cnt), k3, (H, W) in self._propose_classes(images, encoded_event):
            pts = self._points(H, W)
            for j, i in enumerate(idxs):
                sl = slice(j * k3, (j + 1) * k3)
                out[i] = (masks[sl], boxes[sl], iou[sl], stab[sl], order[sl], cnt[j:j + 1], pts)
        return out

    def _propose_classes(self, images, encoded_event=None):
        """The proposal stage of a group up to the first NMS, by size class: the images are partitioned into classes of equal
        (H, W) -- whose resized shape, prompt grid and post-processing geometry agree --, and a class goes through ONE decoder
        call over all its prompts (Sam.decode_points_multi: whole images, at most 1024 prompts per launch sequence), ONE
        post-processing call over its candidates and ONE segmented NMS launch (one workgroup per image).
        points_per_batch keeps its meaning per IMAGE: it is the prompt batch the decoder's batch-dependent choices see (the
        key-range split of the token -> image attention is taken from the prompts per image, never from the launch's
        total), so every candidate is bit for bit what the image's own decoder call gives; an image whose grid needs
        several such batches goes through the decoder alone, as in propose().
        Returns [(image indices, (masks [n*k3,H,W] u8, boxes [n*k3,4] i32, iou [n*k3], stab [n*k3], order [n*k3] i32 -- per
        image, indices into the image's k3 candidates --, counts [n] i32), k3, (H, W))]."""
        m = self.model
        sizes, resized = [], []
        for image in images:
            H, W = image.shape[:2]
            sizes.append((int(H), int(W)) + get_preprocess_shape(H, W, m.img_size))
            resized.append(resize_longest_side(_image_on(image, m.device).contiguous(), m.img_size))
        emb = m.encode_batch(resized)
        if encoded_event is not None:
            encoded_event.record(torch.cuda.current_stream(m.device))
        npts = len(self.point_grids[0])
        k3 = 3 * npts
        classes = {}
        for i, sz in enumerate(sizes):
            classes.setdefault(sz, []).append(i)
        out = []
        for (H, W, nh, nw), idxs in classes.items():
            # (the clean-up's and the post-processing's 32-bit pixel offsets bound the candidates of one call)
            n_max = min(max(1, (2 ** 31 - 1) // (k3 * H * W)), 65535 // k3) if k3 <= 1024 and npts <= self.points_per_batch else 1
            for c0 in range(0, len(idxs), n_max):
                part = idxs[c0:c0 + n_max]
                if len(part) == 1:
                    c = self._propose_from_embedding(emb[part[0]], H, W, nh, nw, 0, None, None)
                    out.append((part, c[:6], k3, (H, W)))
                else:
                    out.append((part, self._propose_class(emb, part, H, W, nh, nw), k3, (H, W)))
        return out

    def _dev_const(self, key, make):
        """small device tensors that depend on a group's shape only (index lists, offsets, tiled prompt grids): uploaded once"""
        cache = self.__dict__.setdefault("_const_cache", {})
        t = cache.get(key)
        if t is None:
            if len(cache) >= 256:
                cache.clear()
            t = cache[key] = make()
        return t

    def _prompt_grid(self, H, W, nh, nw, layer_idx):
        """the point grid of a crop of H x W in crop coordinates (float64, host) and as the decoder's [npts, 2] fp32 device
        tensor ((point in the resized frame + 0.5) / img_size)"""
        m = self.model
        pts = self.point_grids[layer_idx] * np.array([[W, H]], dtype=np.float64)   # automatic_mask_generator.py:240-241
        tp = pts.copy()
        tp[:, 0] *= nw / W                                                       # apply_coords, utils/transforms.py:33-45
        tp[:, 1] *= nh / H
        key = (H, W, layer_idx)
        cache = self.__dict__.setdefault("_p01_cache", {})
        p01 = cache.get(key)
        if p01 is None:      # the prompt grid depends on the crop size only: upload it once (a crop layer alternates between sizes)
            if len(cache) >= 64:
                cache.clear()
            p01 = cache[key] = torch.from_numpy(((tp + 0.5) / float(m.img_size)).astype(np.float32)).to(m.device)
        return pts, p01

    def _propose_class(self, emb, idxs, H, W, nh, nw):
        """decoder, post-processing and first NMS of the images idxs (rows of emb), all of size H x W, in one call each"""
        m = self.model
        dev = m.device
        n = len(idxs)
        pts, p01 = self._prompt_grid(H, W, nh, nw, 0)
        npts = len(pts)
        k3 = 3 * npts
        if idxs == list(range(idxs[0], idxs[0] + n)):
            e = emb[idxs[0]:idxs[0] + n]
        else:
            e = emb.index_select(0, self._dev_const(("rows",) + tuple(idxs), lambda: torch.tensor(idxs, dtype=torch.int64, device=dev)))
        # (the call itself goes through whole images, at most 1024 prompts per launch sequence)
        pk = self._dev_const(("p01", H, W, n), lambda: p01.repeat(n, 1).contiguous())
        low, iou = m.decode_points_multi(e, pk, n, iou_gate=self._gate())
        low, iou = low.flatten(0, 1), iou.flatten()
        masks, boxes, stab, keep, _ = m.postprocess(low, iou, (nh, nw), (H, W), self.pred_iou_thresh,
                                                    self.stability_score_thresh, self.stability_score_offset)
        offs = self._dev_const(("offs", n, k3), lambda: torch.arange(0, (n + 1) * k3, k3, dtype=torch.int32, device=dev))
        order, cnt = nms_segments(boxes, iou, keep, offs, k3, self.box_nms_thresh)
        return masks, boxes, iou, stab, order, cnt

    def _propose_from_embedding(self, emb, H, W, nh, nw, layer_idx, crop_box, orig_size):
        m = self.model
        pts, p01 = self._prompt_grid(H, W, nh, nw, layer_idx)
        lows, ious = [], []
        gate = self._gate()
        for s in range(0, len(pts), self.points_per_batch):
            low, iou = m.decode_points(emb, p01[s:s + self.points_per_batch].contiguous(), iou_gate=gate)
            lows.append(low.flatten(0, 1))
            ious.append(iou.flatten())
        low = lows[0] if len(lows) == 1 else torch.cat(lows)
        iou = ious[0] if len(ious) == 1 else torch.cat(ious)
        masks, boxes, stab, keep, _ = m.postprocess(low, iou, (nh, nw), (H, W), self.pred_iou_thresh,
                                                    self.stability_score_thresh, self.stability_score_offset)
        if crop_box is not None and orig_size is not None and list(crop_box) != [0, 0, orig_size[1], orig_size[0]]:
            box_near_crop_edge(boxes, keep, crop_box, [0, 0, orig_size[1], orig_size[0]])
        order, n = nms(boxes, iou, keep, self.box_nms_thresh)
        return masks, boxes, iou, stab, order, n, self._points(H, W, layer_idx)

    # ---- the tail: a GROUP of images from the candidates to the final tensors --------------------------------------
    def group_begin(self, images, cap=None, encoded_event=None):
        """Stage A of generate() for several images on the current stream: Pillow-exact resize, the encoder, then decoder +
        fused post-processing + first NMS.  Without crop layers ONE encoder pass takes all images and every size class one
        decoder call (_propose_classes); with crop layers the crops of all images go through the encoder in batches of up to
        16, then decoder, crop-edge filter and NMS crop by crop (_crops_begin).
        The survivor counts of the whole group leave in ONE device->host copy (pinned), marked by an event, with the fp16
        range counters: nothing is waited for here, so the caller can enqueue other work (the CLIP stage of the previous
        group) before group_cleanup().
        cap: keep at most this many proposals per image (not in the reference -- synthetic benchmark: 'AMG forced to keep a
        fixed 64').  Without crop layers it bounds the survivors of the first NMS, before the clean-up; with crop layers it
        truncates the finished lists."""
        return self._begin(images, cap, encoded_event, 16)

    def _begin(self, images, cap, encoded_event, encoder_chunk):
        st = _GroupState()
        st.cap, st.overflow = cap, 0
        st.sizes = [tuple(int(v) for v in im.shape[:2]) for im in images]
        if self.crop_n_layers > 0:
            counts = self._crops_begin(st, images, encoded_event, encoder_chunk)
        else:
            st.cand = self._propose_classes(images, encoded_event)
            # (counts in image order: a class holds its images' counts side by side)
            cnts = [c[1][5] for c in st.cand]
            counts = cnts[0] if len(cnts) == 1 else torch.cat(cnts)
            perm = [i for c in st.cand for i in c[0]]
            if perm != list(range(len(images))):
                inv = [0] * len(perm)
                for pos, i in enumerate(perm):
                    inv[i] = pos
                counts = counts.index_select(0, self._dev_const(("rows",) + tuple(inv), lambda: torch.tensor(
                    inv, dtype=torch.int64, device=self.model.device)))
        st.n1, st.ev1, st.ovf = self._read_back(counts, overflow=True)
        return st

    def group_cleanup(self, st):
        """Stage B: waits for the counts of group_begin (the first host sync) and enqueues what they decide.  Without crop
        layers: the survivors' gather and the small-region clean-up with its NMS (_classes_cleanup); with crop layers:
        every crop's survivors in its image's frame and the cross-crop NMS (_crops_merge).  The next counts leave in one
        copy again (none without crop layers and without clean-up).  st.overflow: the fp16 range counters of group_begin."""
        st.ev1.synchronize()
        st.overflow = sum(int(v) for v in st.ovf.tolist())      # (two words, or three with self.overflow_snapshot)
        n1 = [int(v) for v in st.n1.tolist()]
        counts = self._crops_merge(st, n1) if self.crop_n_layers > 0 else self._classes_cleanup(st, n1)
        st.n2 = st.ev2 = None
        if counts is not None:
            st.n2, st.ev2, _ = self._read_back(counts)
        return st

    def group_finish(self, st):
        """Stage C: the second host sync (none without crop layers and without clean-up) and the final gathers; with crop
        layers the clean-up and a third sync lie between them (_crops_finish).  Returns per image (masks [n,H,W] uint8,
        boxes_xywh [n,4] int64, iou [n], stability [n], source [n] int64), in the reference's output order; n may be 0.
        source: crop index * source_stride + index into that crop's 3 * points candidates (no crop layers: the candidate)."""
        n2 = None
        if st.n2 is not None:
            st.ev2.synchronize()
            n2 = [int(v) for v in st.n2.tolist()]
        out = self._crops_finish(st, n2) if self.crop_n_layers > 0 else self._classes_finish(st, n2)
        st.stage = None
        return out

    def generate_group(self, images, cap=None):
        """generate_device() for several images with one encoder pass and two host syncs in all (one without clean-up)."""
        return self.group_finish(self.group_cleanup(self.group_begin(images, cap)))

    def generate_crops_group(self, images):
        """generate_device_crops (masks, boxes, iou, stability) for several images with three host syncs in all"""
        return [p[:4] for p in self.group_finish(self.group_cleanup(self.group_begin(images)))]

    def generate_device(self, image, resized=None, fixed_n=None):
        """Whole `generate` on the device.  Returns (masks [n,H,W] uint8, boxes_xywh [n,4] int64,
        iou [n], stability [n], cand [n] int64 indices into the 3*points candidates), all device
        tensors, in the reference's output order.  Two host syncs (the two proposal counts), read where they are needed: by
        measurement one image is faster this way than as a group of one, whose pinned read-backs cost it 0.3 ms.
        fixed_n (benchmark only): take the first fixed_n survivors of the first NMS without reading
        the count back (the caller guarantees that many survive), run the clean-up kernels on them
        and skip the final gather -- no host sync at all."""
        masks, boxes, iou, stab, order, n, points = self.propose(image, resized)
        if fixed_n is not None:
            idx = order[:fixed_n].long()
            m, nb = self.cleanup_fixed(masks.index_select(0, idx).contiguous())
            return m, nb, iou.index_select(0, idx), stab.index_select(0, idx), idx
        n = int(n.item())                       # host sync: number of survivors of the first NMS
        idx = order[:n].long()
        m = masks.index_select(0, idx).contiguous()
        bx = boxes.index_select(0, idx).contiguous()
        if self.min_mask_region_area > 0 and n > 0:
            m, bx, order2, n2 = self._cleanup(m, [n])
            k = order2[: int(n2.item())].long()     # host sync: survivors of the second NMS
            m, bx, idx = m.index_select(0, k), bx.index_select(0, k), idx.index_select(0, k)
        return m, _xywh(bx), iou.index_select(0, idx), stab.index_select(0, idx), idx

    def generate_device_crops(self, image):
        """_generate_masks with crop layers (automatic_mask_generator.py:197-220) + postprocess_small_regions: the crop group
        of one (its encoder batches hold up to 8 crops).  Returns device tensors (masks [n,H,W] u8, boxes_xywh [n,4] i64,
        iou [n], stability [n]) and host arrays (points [n,2] f64, crop_boxes [n,4] i64), in the reference's output order.
        Four host syncs: the group's three and the read-back of the survivors' sources."""
        (m, xywh, iou, stab, src), size = self.crops_of_one(image)
        return (m, xywh, iou, stab) + self._sources(src, *size)

    def crops_of_one(self, image):
        """the crop group of one image through the 8-crop encoder chunk: (group_finish's tuple of the image, its (H, W))"""
        st = self._begin([image], None, None, 8)
        return self.group_finish(self.group_cleanup(st))[0], st.sizes[0]

    def _sources(self, src, H, W):
        """the source indices of an image's survivors on the host: (prompt points [n,2] f64 in image coordinates, crop boxes
        XYXY [n,4] i64)"""
        crop_boxes, layer_idxs = generate_crop_boxes((H, W), self.crop_n_layers, self.crop_overlap_ratio)
        crop, cand = np.divmod(src.cpu().numpy(), self.source_stride)
        pts = np.zeros((len(crop), 2))
        for c in np.unique(crop):
            x0, y0, x1, y1 = crop_boxes[c]
            sel = crop == c
            pts[sel] = self._points(y1 - y0, x1 - x0, layer_idxs[c])[cand[sel]] + np.array([[x0, y0]], dtype=np.float64)   # uncrop_points
        return pts, np.asarray(crop_boxes, dtype=np.int64)[crop]

    # ---- the tail without crop layers: by size class ------------------------------------------------------------
    def _segment_index(self, counts, stride):
        """Device index lists for "the first counts[j] entries of segment j" of a flat array whose segments lie `stride`
        apart, from ONE pinned upload: (positions [total] i64, segment starts of every entry [total] i64, offsets of the
        packed result [n + 1] i32)."""
        total, n = int(sum(counts)), len(counts)
        host = torch.empty(2 * total + n + 1, dtype=torch.int64, pin_memory=True)
        h = host.numpy()
        o = 0
        h[2 * total] = 0
        for j, c in enumerate(counts):
            h[o:o + c] = np.arange(j * stride, j * stride + c)
            h[total + o:total + o + c] = j * stride
            o += c
            h[2 * total + j + 1] = o
        d = host.to(self.model.device, non_blocking=True)
        return d[:total], d[total:2 * total], d[2 * total:].to(torch.int32)

    def _packed_index(self, counts, seg_lens):
        """_segment_index for segments packed back to back (segment j starts at sum(seg_lens[:j])): the first counts[j]
        entries of each -> (positions [total] i64, segment starts [total] i64, None)"""
        total = int(sum(counts))
        host = torch.empty(2 * total, dtype=torch.int64, pin_memory=True)
        h = host.numpy()
        o = s0 = 0
        for c, ln in zip(counts, seg_lens):
            h[o:o + c] = np.arange(s0, s0 + c)
            h[total + o:total + o + c] = s0
            o += c
            s0 += ln
        d = host.to(self.model.device, non_blocking=True)
        return d[:total], d[total:], None

    def _classes_cleanup(self, st, n1):
        """group_cleanup without crop layers: per size class ONE gather of the survivors of all its images and _cleanup on
        them (its passes image by image, its NMS one segmented launch) -> the second NMS counts in class order, or None.
        The clean-up passes stay one image per call, by measurement (profiles/group_tail_ab.json): alone on the device the two
        passes over a group's 16 x 64 masks of 640 x 640 take 13.12 ms at one image per call, 11.44 at 2, 10.95 at 4 and
        10.16 at 16, but beside the CLIP stream the step is SLOWER with the whole class per call (0.980 of the parent's time
        against 0.975): its launches then hold the whole chip for milliseconds while the persistent GEMMs of the other stream
        wait, and its union-find planes (8 bytes per pixel: 3.4 GB against one image's 210 MB) leave the last-level cache."""
        dev = self.model.device
        if st.cap is not None:
            n1 = [min(v, st.cap) for v in n1]
        st.n1_list = n1
        st.stage = []
        n2_dev = []
        area = self.min_mask_region_area
        for idxs, (masks, boxes, iou, stab, order, _cnt), k3, _hw in st.cand:
            counts = [n1[i] for i in idxs]
            if sum(counts) == 0:
                st.stage.append(None)
                if area > 0:
                    n2_dev.append(torch.zeros(len(idxs), dtype=torch.int32, device=dev))
                continue
            pos, base, offs = self._segment_index(counts, k3)
            idx = order.index_select(0, pos).long()          # per image: indices into its k3 candidates, first NMS order
            gidx = idx + base                                # the same as rows of the class's tensors
            m = masks.index_select(0, gidx)
            bx = boxes.index_select(0, gidx)
            order2 = None
            if area > 0:
                m, bx, order2, n2 = self._cleanup(m, counts, offs)
                n2_dev.append(n2)
            st.stage.append((m, bx, idx, gidx, order2, iou, stab, counts))
        # (class order; _classes_finish reads them the same way)
        counts = (n2_dev[0] if len(n2_dev) == 1 else torch.cat(n2_dev)) if area > 0 else None
        st.cand = [c[0] for c in st.cand]     # the candidate tensors (192 full-size masks per image) can go back to the allocator
        return counts

    def _classes_finish(self, st, n2_all):
        """group_finish without crop layers: the final gathers, one per size class"""
        out = [None] * len(st.sizes)
        k0 = 0
        for idxs, stg in zip(st.cand, st.stage):
            n2 = n2_all[k0:k0 + len(idxs)] if n2_all is not None else [st.n1_list[i] for i in idxs]
            k0 += len(idxs)
            if stg is not None and sum(n2) > 0:
                m, bx, idx, gidx, order2, iou, stab, counts = stg
                if order2 is not None:
                    pos, base, _ = self._packed_index(n2, counts)
                    k = order2.index_select(0, pos).long() + base
                    m, bx, idx, gidx = m.index_select(0, k), bx.index_select(0, k), idx.index_select(0, k), gidx.index_select(0, k)
                xywh = _xywh(bx)
                iou, stab = iou.index_select(0, gidx), stab.index_select(0, gidx)
            o = 0
            for i, n in zip(idxs, n2):
                if stg is None or n == 0:
                    out[i] = self._empty(*st.sizes[i])
                    continue
                sl = slice(o, o + n)
                out[i] = (m[sl], xywh[sl], iou[sl], stab[sl], idx[sl])
                o += n
        return out

    # ---- the tail with crop layers: image by image, crop by crop --------------------------------------------------
    def _encode_crops(self, resized, chunk):
        """the embeddings of a list of resized crops, through the encoder in batches of up to `chunk` (better-filled GEMMs,
        weights read once: 13.5 -> 11 ms per crop at ViT-H in batches of 8)"""
        embs = []
        for c0 in range(0, len(resized), chunk):
            e = self.model.encode_batch(resized[c0:c0 + chunk])
            embs.extend(e[i] for i in range(e.shape[0]))
        return embs

    def _crops_begin(self, st, images, encoded_event, chunk):
        """group_begin with crop layers -> the first NMS counts of ALL crops, image by image.  The crops are known from the
        image sizes alone, so the encoder takes them across images; decoder / filters / NMS crop by crop as in the reference."""
        m = self.model
        st.crops, res = [], []
        for image, hw in zip(images, st.sizes):
            dev_img = _image_on(image, m.device)
            crop_boxes, layer_idxs = generate_crop_boxes(hw, self.crop_n_layers, self.crop_overlap_ratio)
            st.crops.append((crop_boxes, layer_idxs))
            res += [resize_longest_side(dev_img[y0:y1, x0:x1, :].contiguous(), m.img_size) for x0, y0, x1, y1 in crop_boxes]
        embs = self._encode_crops(res, chunk)
        if encoded_event is not None:
            encoded_event.record(torch.cuda.current_stream(m.device))
        st.cand, counts, k = [], [], 0
        for hw, (crop_boxes, layer_idxs) in zip(st.sizes, st.crops):
            per = []
            for crop_box, layer_idx in zip(crop_boxes, layer_idxs):
                x0, y0, x1, y1 = crop_box
                ch, cw = y1 - y0, x1 - x0
                c = self._propose_from_embedding(embs[k], ch, cw, *get_preprocess_shape(ch, cw, m.img_size), layer_idx, crop_box, hw)
                k += 1
                per.append(c[:5])
                counts.append(c[5])
            st.cand.append(per)
        return torch.cat(counts)

    def _uncrop(self, cand, n, crop_box, H, W):
        """the n survivors of one crop in the image's frame (uncrop_masks / uncrop_boxes_xyxy, amg.py:225-252) -> (masks
        [n,H,W], boxes XYXY, iou, stability, their indices into the crop's candidates [n] i64)"""
        masks, boxes, iou, stab, order = cand
        x0, y0, x1, y1 = crop_box
        dev = masks.device
        idx = order[:n].long()
        if (x0, y0, x1, y1) == (0, 0, W, H):
            full = masks.index_select(0, idx)
        else:
            full = torch.zeros((n, H, W), dtype=torch.uint8, device=dev)
            full[:, y0:y1, x0:x1] = masks.index_select(0, idx)
        off = torch.tensor([x0, y0, x0, y0], dtype=torch.int32, device=dev)
        return full, boxes.index_select(0, idx) + off, iou.index_select(0, idx), stab.index_select(0, idx), idx

    def _cross_crop_nms(self, boxes, areas):
        """duplicates between crops: prefer masks from smaller crops (automatic_mask_generator.py:209-220); areas: the crop
        area of every box (host, int64) -> nms() order and count"""
        scores = torch.from_numpy((1.0 / torch.from_numpy(areas)).to(torch.float32).numpy()).to(boxes.device)
        return nms(boxes, scores, torch.ones(len(boxes), dtype=torch.uint8, device=boxes.device), self.crop_nms_thresh)

    def _crops_merge(self, st, n1):
        """group_cleanup with crop layers: every crop's survivors uncropped, the crops of an image concatenated in the
        reference's order, the cross-crop NMS -> its counts, one per image"""
        dev = self.model.device
        k = 0
        st.stage, n_dev = [], []
        for (H, W), (crop_boxes, _layers), per in zip(st.sizes, st.crops, st.cand):
            parts, areas = [], []
            for ci, (crop_box, cand) in enumerate(zip(crop_boxes, per)):
                n = n1[k]
                k += 1
                if n == 0:
                    continue
                part = self._uncrop(cand, n, crop_box, H, W)
                parts.append(part[:4] + (part[4] + ci * self.source_stride,))
                areas.append(np.full(n, (crop_box[2] - crop_box[0]) * (crop_box[3] - crop_box[1]), dtype=np.int64))
            if not parts:
                st.stage.append(None)
                n_dev.append(torch.zeros(1, dtype=torch.int32, device=dev))
                continue
            mk, bx, iou, stab, src = (torch.cat(t) for t in zip(*parts))
            bx = bx.contiguous()
            order, n = None, torch.full((1,), len(bx), dtype=torch.int32, device=dev)
            if len(crop_boxes) > 1:
                order, n = self._cross_crop_nms(bx, np.concatenate(areas))
            st.stage.append((mk, bx, iou, stab, src, order))
            n_dev.append(n.reshape(1))
        st.cand = None
        return torch.cat(n_dev)

    def _crops_finish(self, st, n2):
        """group_finish with crop layers: the survivors of the cross-crop NMS through _cleanup, image by image (a crop
        configuration can leave more than 1024 of them), its counts in one copy (host sync 3 of 3), the final gathers"""
        dev = self.model.device
        stage, n_dev = [], []
        for stg, n in zip(st.stage, n2):
            if stg is None or n == 0:
                stage.append(None)
                n_dev.append(torch.zeros(1, dtype=torch.int32, device=dev))
                continue
            mk, bx, iou, stab, src, order = stg
            if order is not None:
                k = order[:n].long()
                mk, bx, iou, stab, src = mk.index_select(0, k), bx.index_select(0, k).contiguous(), iou[k], stab[k], src[k]
            order2, nn = None, torch.full((1,), n, dtype=torch.int32, device=dev)
            if self.min_mask_region_area > 0:
                mk, bx, order2, nn = self._cleanup(mk.contiguous(), [n])
            stage.append((mk, bx, iou, stab, src, order2))
            n_dev.append(nn.reshape(1))
        n3, ev3, _ = self._read_back(torch.cat(n_dev))
        ev3.synchronize()
        out = []
        for stg, n, hw in zip(stage, n3.tolist(), st.sizes):
            if stg is None or n == 0:
                out.append(self._empty(*hw))
                continue
            mk, bx, iou, stab, src, order2 = stg
            if order2 is not None:
                k = order2[:n].long()
                mk, bx, iou, stab, src = mk.index_select(0, k), bx.index_select(0, k), iou[k], stab[k], src[k]
            out.append(tuple(t[:st.cap] for t in (mk, _xywh(bx), iou, stab, src)))
        return out

    # ---- host records ---------------------------------------------------------------------------------------------
    def _segmentation(self, mask):
        """automatic_mask_generator.py:176-182: the record's `segmentation` in the configured output mode (binary mask,
        uncompressed RLE dict, COCO RLE dict with the compressed counts string)."""
        if self.output_mode == "binary_mask":
            return mask
        rle = mask_to_rle(mask)
        return coco_encode_rle(rle) if self.output_mode == "coco_rle" else rle

    def generate(self, image):
        """automatic_mask_generator.py:137-195 -> list of records."""
        H, W = image.shape[:2]
        m, xywh, iou, stab, src = self.crops_of_one(image)[0] if self.crop_n_layers > 0 else self.generate_device(image)
        pts, cbs = self._sources(src, H, W)
        if self.output_mode == "binary_mask":
            segs = m.bool().cpu().numpy()
            areas = [int(k.sum()) for k in segs]
        else:
            # the RLE modes: runs encoded on the device, only runs cross to the host (no [n,H,W] byte copy, no host codec)
            segs, areas = _masks_to_rle(m)
            if self.output_mode == "coco_rle":
                segs = [coco_encode_rle(r) for r in segs]
        return build_records(H, W, None, areas, xywh.cpu().numpy(), iou.cpu().numpy(), stab.cpu().numpy(), pts, cbs, segmentations=segs)


def mask_to_rle(mask):
    """utils/amg.py:107-136 mask_to_rle_pytorch for one host mask [H,W]: {"size": [h, w], "counts": [...]} (column-major
    runs, the first one counts zeros) through the native codec."""
    lib = _lib.load()
    mk = np.ascontiguousarray(np.asarray(mask).astype(np.uint8))
    H, W = mk.shape
    m = C.c_longlong(0)
    check(lib.hgl_rle_encode_mask(mk.ctypes.data, H, W, None, 0, C.byref(m)), "hgl_rle_encode_mask")
    counts = np.empty(m.value, dtype=np.uint32)
    check(lib.hgl_rle_encode_mask(mk.ctypes.data, H, W, counts.ctypes.data, m.value, C.byref(m)), "hgl_rle_encode_mask")
    return {"size": [H, W], "counts": [int(v) for v in counts]}


def rle_from_slot(slot, n_counts, form, H, W):
    """The counts of one entry of ops.rle_encode from its slot on the HOST (`slot`: the entry's words as a numpy array, at
    least as many as its form defines).  Form 0: the slot holds the n_counts counts.  Form 1 (more runs than the slot
    holds): the slot is the column-major bit plane, bit p % 32 of word p / 32 with p = x*H + y; it is unpacked and the
    host codec finishes the job.  Forms 2 / 3 carry no mask."""
    slot = np.ascontiguousarray(np.asarray(slot)).view(np.uint32).reshape(-1)
    if form == 0:
        return [int(v) for v in slot[:n_counts]]
    if form != 1:
        raise ValueError("rle_from_slot: " + ("the entry's index was out of range" if form == 3 else
                                              f"neither the {n_counts} counts nor the bit plane fit the slot"))
    words = (H * W + 31) // 32
    bits = np.unpackbits(slot[:words].astype("<u4").view(np.uint8), bitorder="little")[:H * W]
    counts = mask_to_rle(bits.reshape(W, H).T)["counts"]
    assert len(counts) == n_counts, (len(counts), n_counts)
    return counts


def counts_from_set(slots, table, H, W):
    """rle_from_slot for every entry of an encoded set on the HOST (ops.rle_split of the copied buffer): a list of uint32
    arrays, each a copy -- the buffer behind `slots` may be reused"""
    out = []
    for slot, (nc, form) in zip(slots, table[:, :2].tolist()):
        out.append(slot[:nc].astype(np.uint32) if form == 0 else np.asarray(rle_from_slot(slot, nc, form, H, W), dtype=np.uint32))
    return out


def build_records(H, W, counts, areas, xywh, iou, stab, points, crop_boxes, strings=None, segmentations=None):
    """The record list of one image from its survivors' host arrays (automatic_mask_generator.py:176-192); the `segmentation`
    of a record, in this order: segmentations[i] as it is (a binary mask, an uncompressed RLE dict), the COCO string strings[i]
    (bytes, where the device wrote it), the COCO encoding of counts[i]."""
    out = []
    for i in range(len(areas)):
        cb = crop_boxes[i]
        seg = (segmentations[i] if segmentations is not None else
               {"size": [int(H), int(W)], "counts": strings[i].decode("ascii")} if strings is not None else
               coco_encode_rle({"size": [int(H), int(W)], "counts": counts[i]}))
        out.append({"segmentation": seg, "area": int(areas[i]),
                    "bbox": [int(v) for v in xywh[i]], "predicted_iou": float(iou[i]), "point_coords": [points[i].tolist()],
                    "stability_score": float(stab[i]),
                    "crop_box": [int(cb[0]), int(cb[1]), int(cb[2] - cb[0]), int(cb[3] - cb[1])]})   # XYWH
    return out


def _masks_to_rle(masks, sel=None):
    """masks_to_rle plus the areas of the table: (list of RLE dicts, list of int)"""
    n, H, W = masks.shape
    S = n if sel is None else int(sel.numel())
    if S == 0:
        return [], []
    if not masks.is_contiguous():
        masks = masks.contiguous()
    sw = ops.rle_slot_words(H, W)
    flat = torch.empty(ops.rle_block_words("set", S, sw), dtype=torch.int32, device=masks.device)
    ops.rle_encode(masks, sel, sw, out=flat)
    slots, table = ops.rle_split(flat.cpu().numpy(), S, sw)      # the one device -> host copy
    return [{"size": [H, W], "counts": c.tolist()} for c in counts_from_set(slots, table, H, W)], [int(a) for a in table[:, 2]]


def masks_to_rle(masks, sel=None):
    """mask_to_rle for device masks [n,H,W] (bool / uint8), all of them or masks[sel] (sel: integer device tensor): the runs
    are formed on the device (ops.rle_encode) and one device -> host copy brings table and slots over -- runs, not pixels.
    Returns a list of {"size": [H, W], "counts": [...]}, identical to mask_to_rle of every mask."""
    return _masks_to_rle(masks, sel)[0]


def rle_to_mask(rle):
    """utils/amg.py:139-151."""
    lib = _lib.load()
    h, w = rle["size"]
    counts = np.ascontiguousarray(np.asarray(rle["counts"], dtype=np.uint32))
    out = np.empty((h, w), dtype=np.uint8)
    check(lib.hgl_gt_mask_from_rle_counts(counts.ctypes.data, len(counts), h, w, out.ctypes.data, None), "hgl_gt_mask_from_rle_counts")
    return out.astype(bool)


def rle_counts_from_string(s):
    """The counts of a COCO compressed RLE string (str / bytes) as a uint32 array: the native restatement of
    maskApi.c:217-230 rleFrString without the decode (hgl_rle_from_string).  Raises on a malformed string."""
    lib = _lib.load()
    b = s.encode("ascii") if isinstance(s, str) else bytes(s)
    counts = np.empty(max(len(b), 1), dtype=np.uint32)      # every count takes at least one character
    m = C.c_longlong(0)
    check(lib.hgl_rle_from_string(C.c_char_p(b), counts.ctypes.data, len(counts), C.byref(m)), "hgl_rle_from_string")
    return counts[:m.value]


def rle_counts(rle):
    """the counts of an RLE dict as a uint32 array, whichever form it carries them in (list / array, or COCO string / bytes)"""
    c = rle["counts"]
    if isinstance(c, (str, bytes, bytearray)):
        return rle_counts_from_string(c)
    return np.ascontiguousarray(np.asarray(c, dtype=np.uint32)).reshape(-1)


def rles_to_masks(rles, device=None):
    """rle_to_mask for a list of RLE dicts {"size": [h, w], "counts": list | COCO string / bytes} of ONE size, decoded on the
    device: the runs cross the bus (ops.rle_pack: one copy), the pixels are formed there (ops.rle_decode).  Returns a bool
    [n,H,W] device tensor.  Raises ValueError naming the first entry whose counts do not sum to H*W (one read-back of the
    status table)."""
    if len(rles) == 0:
        raise ValueError("rles_to_masks: no entries (the size of the result is the entries')")
    h, w = (int(v) for v in rles[0]["size"])
    for i, r in enumerate(rles):
        if [int(v) for v in r["size"]] != [h, w]:
            raise ValueError(f"rles_to_masks: entry {i} has size {list(r['size'])}, entry 0 has {[h, w]}")
    slots, table = ops.rle_pack([rle_counts(r) for r in rles], h, w, device=device)
    masks, status = ops.rle_decode(slots, table, h, w)
    code = status[:, 0].cpu().numpy()
    bad = np.flatnonzero(code != 0)
    if len(bad):
        raise ValueError(f"rles_to_masks: entry {int(bad[0])} does not decode to a {h} x {w} mask (status {int(code[bad[0]])}: "
                         "its counts do not sum to H*W)")
    return masks.view(torch.bool)


def area_from_rle(rle):
    """utils/amg.py:154-155."""
    return sum(rle["counts"][1::2])


def coco_encode_rle(uncompressed_rle):
    """utils/amg.py:294-300: pycocotools' frPyObjects(uncompressed_rle) with the counts as a str -- the compressed string
    comes from the native restatement of maskApi.c:203-216 rleToString."""
    lib = _lib.load()
    h, w = uncompressed_rle["size"]
    counts = np.ascontiguousarray(np.asarray(uncompressed_rle["counts"], dtype=np.uint32))
    buf = C.create_string_buffer(7 * len(counts) + 1)
    n = C.c_size_t(0)
    check(lib.hgl_rle_to_string(counts.ctypes.data, len(counts), buf, len(buf), C.byref(n)), "hgl_rle_to_string")
    return {"size": [h, w], "counts": buf.raw[:n.value].decode("utf-8")}


def strings_from_device(slots, table, H, W, cap=None):
    """The COCO strings (bytes) of an encoded set that lives on the device: ops.rle_to_strings, one read of offsets and status,
    one copy of exactly offsets[S] bytes.  A second call at the true size when `cap` (default: ops.rle_to_strings's) was too
    small; an entry in form 1 (a bit plane) is finished by the host codec from its slot; an entry without a mask raises
    ValueError, as rle_from_slot does."""
    S = int(slots.shape[0])
    if S == 0:
        return []
    cap = ops.RLE_STRING_CAP_PER_ENTRY * S if cap is None else int(cap)
    flat = torch.empty(ops.rle_strings_bytes(S, cap), dtype=torch.uint8, device=slots.device)
    data, _, _ = ops.rle_to_strings(slots, table, cap, out=flat)
    head = flat[:ops.rle_strings_bytes(S, 0)].cpu().numpy()      # the one read of offsets and status
    _, offsets, status = ops.rle_strings_split(head, S, 0)
    total = int(offsets[S])
    if total > cap:      # the offsets are true under any cap: once more, at the size they give
        data, _, st = ops.rle_to_strings(slots, table, total)
        status = st.cpu().numpy()
    raw = data[:total].cpu().numpy().tobytes()      # the one copy of exactly offsets[S] bytes
    return strings_from_bytes(raw, offsets, status, slots, table, H, W)


def strings_from_bytes(raw, offsets, status, slots, table, H, W):
    """the strings of strings_from_device out of the bytes, offsets and status on the host; slots / table (device or host)
    are read only for an entry that the device did not finish"""
    out = []
    for s in range(len(status)):
        code = int(status[s])
        if code == 0:
            out.append(raw[int(offsets[s]):int(offsets[s + 1])])
            continue
        if code == 3:
            raise ValueError(f"strings_from_bytes: entry {s} was not written (the buffer was too small)")
        row = [int(v) for v in (table[s].cpu().numpy() if isinstance(table, torch.Tensor) else table[s])]
        slot = slots[s].cpu().numpy() if isinstance(slots, torch.Tensor) else slots[s]
        counts = rle_from_slot(slot, row[0], row[1] if code == 1 else max(row[1], 2), H, W)      # code 2: raises
        out.append(coco_encode_rle({"size": [H, W], "counts": counts})["counts"].encode("ascii"))
    return out


def masks_to_coco_rle(masks, sel=None):
    """[coco_encode_rle(r) for r in masks_to_rle(masks, sel)] with the strings written on the device (ops.rle_encode ->
    ops.rle_to_strings): what crosses the bus is the strings, about 1.3 bytes per run, and no Python loop touches a count.
    Returns a list of {"size": [H, W], "counts": str}, identical to the host path's."""
    n, H, W = masks.shape
    S = n if sel is None else int(sel.numel())
    if S == 0:
        return []
    if not masks.is_contiguous():
        masks = masks.contiguous()
    slots, table = ops.rle_encode(masks, sel, ops.rle_slot_words(H, W))
    return [{"size": [H, W], "counts": b.decode("ascii")} for b in strings_from_device(slots, table, H, W)]


def coco_rles_to_masks(rles, device=None):
    """rles_to_masks for RLE dicts that carry their counts as COCO strings / bytes, with the strings read on the device: the
    strings cross the bus as they are (ops.rle_strings_pack: one copy), ops.rle_from_strings makes them counts and
    ops.rle_decode pixels.  Returns a bool [n,H,W] device tensor.  Raises ValueError naming the entry and the code for a
    string that is truncated (2) or has a group of more than 7 characters (3), and rles_to_masks's ValueError for counts that
    do not sum to H*W (one read-back of the two status tables)."""
    if len(rles) == 0:
        raise ValueError("coco_rles_to_masks: no entries (the size of the result is the entries')")
    h, w = (int(v) for v in rles[0]["size"])
    for i, r in enumerate(rles):
        if [int(v) for v in r["size"]] != [h, w]:
            raise ValueError(f"coco_rles_to_masks: entry {i} has size {list(r['size'])}, entry 0 has {[h, w]}")
        if not isinstance(r["counts"], (str, bytes, bytearray)):
            raise ValueError(f"coco_rles_to_masks: entry {i} carries its counts as {type(r['counts']).__name__}, not as a string")
    S = len(rles)
    buf, _, n_counts = ops.rle_strings_pack([r["counts"] for r in rles])
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    dev = buf.to(device, non_blocking=True)      # the one upload
    slots, table, st = ops.rle_from_strings(dev[8 * (S + 1):], dev[:8 * (S + 1)].view(torch.int64), S, max(int(n_counts.max()), 1))
    masks, status = ops.rle_decode(slots, table, h, w)
    both = torch.stack([st[:, 0], status[:, 0]]).cpu().numpy()
    bad = np.flatnonzero(both[0] != 0)
    if len(bad):
        k, code = int(bad[0]), int(both[0, bad[0]])
        raise ValueError(f"coco_rles_to_masks: entry {k} is no compressed RLE string (code {code}: " +
                         {2: "it ends inside a count", 3: "a count of more than 7 characters"}.get(code, "not read") + ")")
    bad = np.flatnonzero(both[1] != 0)
    if len(bad):
        raise ValueError(f"coco_rles_to_masks: entry {int(bad[0])} does not decode to a {h} x {w} mask (status {int(both[1, bad[0]])}: "
                         "its counts do not sum to H*W)")
    return masks.view(torch.bool)


def merge_rles(rles, intersect=False, device=None):
    """mask.merge of refer/external/mask.py (maskApi.c:49-70 rleMerge) for a list of RLE dicts of ONE size, on the device: the
    runs cross the bus (ops.rle_pack), the union -- or, with intersect, the intersection -- is formed on bit planes
    (ops.rle_merge) and comes back as runs; no mask becomes pixels.  The dicts carry their counts as lists / arrays or as COCO
    strings; the result is an RLE dict in the form of the first.  Raises ValueError on an empty list, on sizes that differ and
    on an entry that does not decode."""
    if len(rles) == 0:
        raise ValueError("merge_rles: no entries (the size of the result is the entries')")
    h, w = (int(v) for v in rles[0]["size"])
    for i, r in enumerate(rles):
        if [int(v) for v in r["size"]] != [h, w]:
            raise ValueError(f"merge_rles: entry {i} has size {list(r['size'])}, entry 0 has {[h, w]}")
    n = len(rles)
    slots, table = ops.rle_pack([rle_counts(r) for r in rles], h, w, device=device)
    out = ops.rle_merge(slots, table, [(h, w)], [n], [list(range(n))], None, [ops.rle_merge_rule("intersect" if intersect else "union", n)],
                        [1])
    s, t, st = (x.cpu().numpy() for x in out)
    if st[0, 0] == 2:
        raise ValueError("merge_rles: an entry holds no mask")
    counts = rle_from_slot(s[0], int(t[0, 0]), int(t[0, 1]), h, w)
    merged = {"size": [h, w], "counts": counts}
    return coco_encode_rle(merged) if isinstance(rles[0]["counts"], (str, bytes, bytearray)) else merged


def nms_rles(rles, scores=None, thr=0.7, metric="iou", device=None):
    """mask.nms of pycocotools (maskApi.c:98-107 rleNms) for a list of RLE dicts of ONE image, on the device: the runs cross the
    bus (ops.rle_pack), the pairs are counted on bit planes and the walk runs there (ops.rle_nms); no mask becomes pixels.
    Returns the kept indices in walk order: the given order without scores (rleNms's), else descending score with the index
    breaking ties, a NaN first.  metric "iou", or "containment" (I / the smaller area).  The ratio is the exact one on every
    pair; rleNms's differs only where rleIou's box pre-filter is not tight.  Raises ValueError on sizes that differ and on an
    entry that does not decode."""
    import numpy as np
    if len(rles) == 0:
        return []
    h, w = (int(v) for v in rles[0]["size"])
    for i, r in enumerate(rles):
        if [int(v) for v in r["size"]] != [h, w]:
            raise ValueError(f"nms_rles: entry {i} has size {list(r['size'])}, entry 0 has {[h, w]}")
    n = len(rles)
    if scores is not None and len(scores) != n:
        raise ValueError(f"nms_rles: {len(scores)} scores for {n} entries")
    slots, table = ops.rle_pack([rle_counts(r) for r in rles], h, w, device=device)
    sc = None if scores is None else torch.as_tensor(np.asarray(scores, dtype=np.float32)).to(slots.device)
    out_idx, out_n, result = (x.cpu().numpy() for x in ops.rle_nms(slots, table, [(h, w)], [n], sc, thr, metric))
    bad = np.flatnonzero(result[:, 0] == 2)
    if len(bad):
        raise ValueError(f"nms_rles: entry {int(bad[0])} holds no mask")
    return [int(i) for i in out_idx[:int(out_n[0])]]


def remove_small_regions_rles(rles, area_thresh, mode):
    """utils/amg.py:267-291 for a list of RLE dicts of ONE size, on the device: the runs cross the bus (ops.rle_pack), the
    components are found on column segments (ops.rle_remove_small_regions) and the cleaned masks come back as runs; no mask
    becomes pixels.  mode "holes" or "islands" as the reference's, or "both" (holes, then islands on the result).  Returns
    (rles, changed): every dict in the form of its input (counts as a list, or as a COCO string), changed[i] True where a small
    region was found -- the reference's flag.  Raises ValueError on sizes that differ and on an entry that does not decode."""
    if len(rles) == 0:
        return [], []
    h, w = (int(v) for v in rles[0]["size"])
    for i, r in enumerate(rles):
        if [int(v) for v in r["size"]] != [h, w]:
            raise ValueError(f"remove_small_regions_rles: entry {i} has size {list(r['size'])}, entry 0 has {[h, w]}")
    n = len(rles)
    counts = [rle_counts(r) for r in rles]
    slots, table = ops.rle_pack(counts, h, w)
    sw, osw = int(slots.shape[1]), ops.rle_slot_words(h, w)
    flat = torch.empty(ops.rle_block_words("clean", n, osw), dtype=torch.int32, device=slots.device)
    ops.rle_remove_small_regions(slots, table, [(h, w)], [n], area_thresh, mode, seg_cap=sw // 2 + w + 1, slot_words=osw, out=flat)
    t, s, _, result = ops.rle_block("clean", flat.cpu().numpy(), n, osw)      # the one device -> host copy
    bad = np.flatnonzero(result[:, 0] != 0)
    if len(bad):
        raise ValueError(f"remove_small_regions_rles: entry {int(bad[0])} does not decode to a {h} x {w} mask (status {int(result[bad[0], 0])})")
    out = []
    for i, r in enumerate(rles):
        new = {"size": [h, w], "counts": rle_from_slot(s[i], int(t[i, 0]), int(t[i, 1]), h, w)}
        out.append(coco_encode_rle(new) if isinstance(r["counts"], (str, bytes, bytearray)) else new)
    return out, [bool(c) for c in result[:, 2]]


def remove_small_regions(masks, area_thresh, mode, out=None):
    """utils/amg.py:267-291 for a batch [n,H,W] uint8 on the device -> (new masks, changed [n] uint8).
    out: (masks, changed) to write into (contiguous slices of a group's tensors) instead of fresh ones."""
    lib = _lib.load()
    n, H, W = masks.shape
    if out is not None:
        out, changed = out
        ops._dev(out, torch.uint8, "out"), ops._dev(changed, torch.uint8, "changed")
    else:
        out = torch.empty_like(masks)
        changed = torch.empty((n,), dtype=torch.uint8, device=masks.device)
    need = lib.hgl_remove_small_regions_workspace_bytes(n, H, W)
    ws = ops.workspace(need, masks.device, "sam_ccl")
    check(lib.hgl_remove_small_regions(ops._dev(masks, torch.uint8, "masks"), n, H, W, int(area_thresh),
                                       1 if mode == "holes" else 0, out.data_ptr(), changed.data_ptr(),
                                       ws.data_ptr(), ws.numel(), ops._stream()), "hgl_remove_small_regions")
    return out, changed


def remove_small_regions_boxes(masks, area_thresh, mode, out=None):
    """remove_small_regions with the boxes of the masks it writes (batched_mask_to_box, utils/amg.py:303-346) out of the
    same pass -> (new masks, changed [n] uint8, int32 XYXY [n,4]).  out: (masks, changed, boxes) to write into."""
    lib = _lib.load()
    n, H, W = masks.shape
    if out is not None:
        out, changed, boxes = out
        ops._dev(out, torch.uint8, "out"), ops._dev(changed, torch.uint8, "changed"), ops._dev(boxes, torch.int32, "boxes")
    else:
        out = torch.empty_like(masks)
        changed = torch.empty((n,), dtype=torch.uint8, device=masks.device)
        boxes = torch.empty((n, 4), dtype=torch.int32, device=masks.device)
    need = lib.hgl_remove_small_regions_workspace_bytes(n, H, W)
    ws = ops.workspace(need, masks.device, "sam_ccl")
    check(lib.hgl_remove_small_regions_boxes(ops._dev(masks, torch.uint8, "masks"), n, H, W, int(area_thresh),
                                             1 if mode == "holes" else 0, out.data_ptr(), changed.data_ptr(), boxes.data_ptr(),
                                             ws.data_ptr(), ws.numel(), ops._stream()), "hgl_remove_small_regions_boxes")
    return out, changed, boxes


def mask_boxes(masks):
    """batched_mask_to_box (utils/amg.py:303-346) -> int32 XYXY [n,4]."""
    lib = _lib.load()
    n, H, W = masks.shape
    boxes = torch.empty((n, 4), dtype=torch.int32, device=masks.device)
    check(lib.hgl_mask_boxes(ops._dev(masks, torch.uint8, "masks"), n, H, W, boxes.data_ptr(), ops._stream()),
          "hgl_mask_boxes")
    return boxes
