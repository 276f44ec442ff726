"""GPU: the ordered kernel launches of the three encoders' host code (csrc/clip_api.hip, gem_api.hip, sam_api.hip) equal the
lists of tests/golden/block_launches.json.

Every transformer block of that host code is written once over an activation operand (fp32 rows or the fp16 hi | lo planes
that alias them, HglAct in csrc/hgl_common.h); the route of a block says what differs.  The lists were recorded from the
build of the commit before the blocks were unified, with this case table (`python tests/test_gpu_block_launches.py --record`):
a change of the host code that adds, drops, reorders or re-instantiates a launch of any case shows here as a list difference.
Entries are what abi_ref.launched_kernels gives: template arguments included, memcpy / memset filtered.

The cases are the smallest shapes at which the paths differ:
  CLIP ViT-B/16, G2L, masking_block 9   3 proposals (6 x 197 = 1182 rows > 512: the split block) in f16x3, f32 and f16;
                                        1 proposal (394 rows: fp32-row blocks under the split layout) in f16x3
  text encoder ViT-B/16, f16x3          9 strings (693 rows: split block), 2 strings (154 rows: fp32 rows)
  GEM ViT-B/16, one 448 x 448 image     image_features as the wrapper calls it, and with feat_ori; f16x3 and f32
  SAM encoder                           the six geometries of test_gpu_sam_encoder_routes.GEOMS in their own precisions, tiny28
                                        and vit_b_d2 (the production route: planes, padded 14 x 14 windows with the gather, the
                                        global block, the neck on planes) in f16x3; encode of one image, encode_batch of two
                                        for hd32_split and vit_b_d2
"""
import json
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:   # (run as a script: --record)
    sys.path.insert(0, ROOT)

import abi_ref  # noqa: E402
from hybridgl_amd import gem as G  # noqa: E402
from hybridgl_amd import ops, weights  # noqa: E402
from hybridgl_amd import sam as hsam  # noqa: E402
from hybridgl_amd.backbone import CLIPViTFM  # noqa: E402
from hybridgl_amd.synth import synth_image, synth_tokens  # noqa: E402
from oracle.cases import views_for_case  # noqa: E402
from test_gpu_sam_encoder_routes import GEOMS  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(ROOT, "tests", "golden", "block_launches.json")

SAM_GEOMS = {name: (cfg, precision or "f16x3", hw) for name, (cfg, precision, hw, _) in GEOMS.items()}
SAM_GEOMS["tiny28"] = (weights.SAM_CONFIGS["tiny28"], "f16x3", (336, 448))
SAM_GEOMS["vit_b_d2"] = (weights.SAM_CONFIGS["vit_b_d2"], "f16x3", (768, 1024))

# case name -> (model key, what to call on it)
CASES = {}
for _p in ("f16x3", "f32", "f16"):
    CASES[f"clip_n3_{_p}"] = (("clip", _p), ("hybrid", 3))
CASES["clip_n1_f16x3"] = (("clip", "f16x3"), ("hybrid", 1))
CASES["text_9_f16x3"] = (("clip", "f16x3"), ("text", 9))
CASES["text_2_f16x3"] = (("clip", "f16x3"), ("text", 2))
for _p in ("f16x3", "f32"):
    CASES[f"gem_{_p}"] = (("clip", _p), ("gem", False))
    CASES[f"gem_ori_{_p}"] = (("clip", _p), ("gem", True))
for _n in SAM_GEOMS:
    CASES[f"sam_{_n}"] = (("sam", _n), ("encode", 1))
for _n in ("hd32_split", "vit_b_d2"):
    CASES[f"sam_{_n}_batch2"] = (("sam", _n), ("encode", 2))

_models = {}


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def model(key, dev):
    """one model per key for the whole module (the synthetic ViT-B/16 weights are drawn once per precision)"""
    if key not in _models:
        kind, which = key
        if kind == "clip":
            _models[key] = CLIPViTFM("ViT-B/16", state_dict=weights.clip_state_dict("ViT-B/16", 0), device=dev, precision=which)
        else:
            cfg, precision, _ = SAM_GEOMS[which]
            _models[key] = hsam.Sam(weights.sam_state_dict(cfg, 0), cfg, dev, precision=precision)
    return _models[key]


def make_call(name, dev):
    """the call of a case: () -> its output tensor"""
    key, (what, n) = CASES[name]
    m = model(key, dev)
    if what == "hybrid":
        loc, glo, masks = (T(a, dev) for a in views_for_case(n, 224, 97, 130))
        return lambda: m(loc, glo, masks, masking_block=9, fusion_mode="G2L")
    if what == "text":
        tok = T(synth_tokens(n, 77, 49408, 21), dev)
        return lambda: m.model.encode_text(tok)
    if what == "gem":
        gm = G.create_gem_model("ViT-B/16", clip=m)
        img = T(np.random.default_rng(11).standard_normal((3, 448, 448)).astype(np.float32), dev)
        return lambda: gm.image_features(img, return_ori=n)
    h, w = SAM_GEOMS[key[1]][2]
    imgs = [T(synth_image(h, w, 31), dev), T(synth_image(w, w, 42), dev)]
    return (lambda: m.encode(imgs[0])) if n == 1 else (lambda: m.encode_batch(imgs))


def launches(name, dev):
    """the kernels of one call of the case, made once before so that nothing is allocated under the profiler"""
    try:
        call = make_call(name, dev)
        call()
        return abi_ref.launched_kernels(call)
    finally:
        ops.set_precision(ops.default_precision())


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        yield json.load(f)
    _models.clear()   # the models (and their registered splits) leave with the module


def test_golden_holds_exactly_the_cases(golden):
    assert sorted(golden) == sorted(CASES)


@pytest.mark.parametrize("name", list(CASES))
def test_launch_sequence_is_the_recorded_one(cuda, golden, name):
    got = launches(name, cuda)
    want = golden[name]
    first = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
    assert got == want, f"{name}: {len(got)} launches against {len(want)} recorded; first difference at launch {first}: " \
                        f"{got[first:first + 3]} against {want[first:first + 3]}"


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: test_gpu_block_launches.py --record   (writes tests/golden/block_launches.json from the loaded build)")
    assert torch.cuda.is_available(), "recording needs a GPU"
    device = torch.device("cuda:0")
    rec = {}
    for case in CASES:
        rec[case] = launches(case, device)
        print(f"{case}: {len(rec[case])} launches", flush=True)
    with open(GOLDEN, "w") as f:
        json.dump(rec, f, indent=0)
        f.write("\n")
