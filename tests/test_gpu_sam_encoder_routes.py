"""GPU: whole SAM image encoders on geometries chosen for the ROUTE they take through csrc/sam_api.hip (enc_block_route,
enc_relpos_tables, the padded-window gather, the window partition launches), not for their size.

The encoder tests of tests/test_gpu_sam.py all have window 14 and head dim 64 or 80.  The geometries here -- each one windowed
block + one global block + the neck unless noted, weights drawn by weights.sam_state_dict from the config dict beside the case --
reach what those leave out:

  hd32_f32       D 64, 2 heads of 32, grid 16, window 14, f32 mode: the generic rel-pos producer (two GEMMs + two gathers) in the
                 fp32 block, 2 x 2 padded windows
  hd32_split     D 256, 8 heads of 32, grid 16, window 14: the split-fp16 block that gathers the real tokens of the padded windows
                 (LayerNorm through the row maps, fill_rows for the pad rows of qkv) with the generic rel-pos producer
  window7        D 128, 2 heads of 64, grid 16, window 7: an ODD window (3 x 3 windows padded to 21) at head dim 64 -- the direct
                 rel-pos kernels store pairs, the generic producer serves it; this geometry failed to encode ("relpos_direct:
                 window size 7 unsupported") before enc_relpos_tables picked the producer by size as well
  window8        D 256, 4 heads of 64, grid 16, window 8: a window that divides the grid, other than 14 -- win_partition_split /
                 win_unpartition_add, the VALU rel-pos kernel under the split layout (sizes 8 and 16)
  window_gt_grid D 160, 2 heads of 80, grid 8, window 14: ONE padded window larger than the grid, more pad rows than tokens; the
                 rel-pos terms of that block are [heads * 196, 14], more than the grid-sized buffers the plan used to carve
  grid66         D 128, 2 heads of 64, patch 8, image 528, ONE global block: a 66 x 66 attention grid at head dim 64 (the direct
                 kernels hold at most 127 table rows) -- the generic producer; S = 4356 is no multiple of any query-block size;
                 failed to encode before, as window7 did

Each case: the embedding of a non-square image (zero padding in the preprocess) against oracle/sam_oracle.py:image_encoder at
atol 2e-4, the bar of the two-block encoders of tests/test_gpu_sam.py; a second call gives equal bits; the rel-pos / window /
LayerNorm kernels launched are exactly the set the route should produce.  The worst |error| is printed before the assertion.

Worst |error| measured on an MI355X (oracle embeddings: max |x| 4.1 .. 4.9, std 1.0): hd32_f32 8.1e-6, hd32_split 4.2e-6,
window7 4.9e-6, window8 4.9e-6, window_gt_grid 3.5e-6, grid66 1.0e-5.  Batch of three against single images: window7 2.7e-6,
grid66 0 (equal bits).
"""
import numpy as np
import pytest
import torch

import abi_ref
import relpos_cases as R
from hybridgl_amd import ops
from hybridgl_amd import sam as hsam
from hybridgl_amd import weights
from hybridgl_amd.synth import synth_image
from oracle import sam_oracle as S

pytestmark = pytest.mark.gpu


def _cfg(D, heads, img, patch, window, depth=2, global_at=(1,)):
    return dict(embed_dim=D, depth=depth, num_heads=heads, global_attn_indexes=global_at, img_size=img, patch_size=patch,
                window_size=window, out_chans=256)


LN_NECK = "layernorm_vec_kernel<1>"          # the neck's two LayerNorms over 256 channels
# name -> (config, precision (None: the default), (h, w) of the image, the glue kernels of the route)
GEOMS = {
    "hd32_f32": (_cfg(64, 2, 256, 16, 14), "f32", (192, 256),
                 {"win_maps_kernel", "layernorm_any_kernel", "win_partition_kernel", "win_unpartition_add_kernel",
                  "relpos_gather_kernel", LN_NECK}),
    "hd32_split": (_cfg(256, 8, 256, 16, 14), None, (192, 256),
                   {"win_maps_kernel", "layernorm_split_kernel<1>", "fill_rows_kernel", "relpos_gather_kernel", LN_NECK}),
    "window7": (_cfg(128, 2, 256, 16, 7), None, (192, 256),
                {"win_maps_kernel", "layernorm_any_kernel", "win_partition_kernel", "win_unpartition_add_kernel",
                 "relpos_gather_kernel", "relpos_direct_kernel<64>", LN_NECK}),
    "window8": (_cfg(256, 4, 256, 16, 8), None, (192, 256),
                {"win_maps_kernel", LN_NECK, "win_partition_split_kernel", "win_unpartition_add_kernel",
                 "relpos_direct_kernel<64>", "layernorm_split_kernel<1>"}),
    "window_gt_grid": (_cfg(160, 2, 128, 16, 14), None, (96, 128),
                       {"win_maps_kernel", "layernorm_any_kernel", "win_partition_kernel", "win_unpartition_add_kernel",
                        "relpos_mfma_kernel<80,1,0>", "relpos_direct_kernel<80>", LN_NECK}),
    "grid66": (_cfg(128, 2, 528, 8, 0, depth=1, global_at=(0,)), None, (396, 528),
               {"layernorm_any_kernel", "relpos_gather_kernel", LN_NECK}),
}
GLUE = ("relpos_", "win_", "fill_rows", "layernorm_")


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _model(name, dev):
    cfg, precision, hw, kernels = GEOMS[name]
    sd = weights.sam_state_dict(cfg, 0)
    return cfg, sd, hsam.Sam(sd, cfg, dev, precision=precision), hw, kernels


@pytest.mark.parametrize("name", list(GEOMS))
def test_encoder_route_vs_oracle(cuda, name):
    try:
        cfg, sd, m, (h, w), kernels = _model(name, cuda)
        g = cfg["img_size"] // cfg["patch_size"]
        img = synth_image(h, w, 31)
        x = T(img, cuda)
        out = {}
        names = R.kernel_ids(abi_ref.launched_kernels(lambda: out.setdefault("emb", m.encode(x))))
        emb = out["emb"].cpu().numpy().reshape(g, g, 256)
        glue = {n for n in names if n.startswith(GLUE)}
        ref = S.image_encoder(sd, S.preprocess(img, cfg["img_size"]), cfg)
        print(f"encoder route {name} ({m.precision}): max |error| {np.abs(emb - ref).max():.3e} (max |ref| {np.abs(ref).max():.2f}); "
              f"glue kernels {sorted(glue)}")
        assert glue == kernels, (sorted(glue), sorted(kernels))
        np.testing.assert_allclose(emb, ref, rtol=0, atol=2e-4)
        assert np.array_equal(emb, m.encode(x).cpu().numpy().reshape(g, g, 256))      # run-to-run bit reproducible
    finally:
        ops.set_precision(ops.default_precision())


@pytest.mark.parametrize("name", ["window7", "grid66"])
def test_encoder_route_batch_of_three_equals_single_images(cuda, name):
    """the two geometries that did not encode before: hgl_sam_encode_batch of three images (an odd count, mixed heights) == the
    single-image passes, at the tolerance test_encoder_batch_of_two_equals_single_images has for the same arithmetic (fp32
    blocks, split-fp16 patch embedding and neck: 1e-5, the `tiny` row there); a batch of one equals encode() bit for bit"""
    try:
        cfg, _, m, (h, w), _ = _model(name, cuda)
        imgs = [T(synth_image(h, w, 41), cuda), T(synth_image(w, w, 42), cuda), T(synth_image(w // 2, w, 43), cuda)]
        single = [m.encode(x).cpu().numpy() for x in imgs]
        both = m.encode_batch(imgs).cpu().numpy()
        assert both.shape == (3,) + single[0].shape
        for i in range(3):
            print(f"encoder route {name}: batch image {i} max |difference| {np.abs(both[i] - single[i]).max():.3e}")
        for i in range(3):
            np.testing.assert_allclose(both[i], single[i], rtol=0, atol=1e-5)
        assert np.array_equal(m.encode_batch([imgs[2]])[0].cpu().numpy(), single[2])
    finally:
        ops.set_precision(ops.default_precision())
