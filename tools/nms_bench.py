#!/usr/bin/env python3
"""The box NMS (csrc/sam_nms.hip) timed on every route; prints one JSON object of us per call.

Input: the `clusters` family of tests/nms_cases.py at threshold 0.7 -- lists that suppress most of their candidates, so the walk
over the row blocks does real work.  Each route is warmed with its own shape, then timed with device events around --calls
back-to-back calls (the median of --reps such series, us per call):

  hgl_nms            K = 192 (an 8 x 8 point grid), 512, 768 (a 16 x 16 crop-layer grid: the serial body) and 1024
  hgl_nms_segments   16 lists of 192, 16 lists of 64 (the second NMS of a group), [192] * 8 + [768] * 8 with max_len 768
  hgl_nms_large      K = 3072 (a 32 x 32 grid) and 16390

HGL_LIB_NAME=<file beside libhybridgl.so> binds another build of the library (tools/_diag.py): a parent commit's, for an A/B.

    python tools/nms_bench.py [--calls 200] [--reps 5]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

from _diag import use_lib_from_env

LIB = use_lib_from_env()
import nms_cases as N
from hybridgl_amd import sam as hsam

THR = 0.7


def device_us(fn, calls, reps, warm=20):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / calls)
    return round(statistics.median(out), 2)


def lists(lens, dev):
    """the clusters lists of the given lengths, packed -> (boxes, scores, keep, offsets) on the device and the kept counts the
    reference gives"""
    cs = [N.clusters(L, THR, seed=i) for i, L in enumerate(lens)]
    up = lambda f: torch.from_numpy(np.concatenate([getattr(c, f) for c in cs])).to(dev)
    offs = torch.from_numpy(np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)).to(dev)
    return up("boxes"), up("scores"), up("keep"), offs, [len(N.run(c)) for c in cs]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "nms_bench.py needs a GPU"
    dev = torch.device("cuda:0")
    us, kept = {}, {}
    for name, fn, Ks in (("hgl_nms", hsam.nms, (192, 512, 768, 1024)), ("hgl_nms_large", hsam.nms_large, (3072, 16390))):
        for K in Ks:
            b, s, k, _, want = lists([K], dev)
            idx, n = fn(b, s, k, THR)
            assert int(n.item()) == want[0], (name, K, int(n.item()), want)
            key = f"{name} K={K}"
            kept[key] = want[0]
            us[key] = device_us(lambda: fn(b, s, k, THR), args.calls, args.reps)
    for key, lens in (("hgl_nms_segments 16x192", [192] * 16), ("hgl_nms_segments 16x64", [64] * 16),
                      ("hgl_nms_segments 8x192+8x768", [192] * 8 + [768] * 8)):
        b, s, k, offs, want = lists(lens, dev)
        idx, n = hsam.nms_segments(b, s, k, offs, max(lens), THR)
        assert n.cpu().tolist() == want, (key, n.cpu().tolist(), want)
        kept[key] = sum(want)
        us[key] = device_us(lambda: hsam.nms_segments(b, s, k, offs, max(lens), THR), args.calls, args.reps)
    print(json.dumps({"lib": os.path.basename(LIB), "device": torch.cuda.get_device_name(0), "calls": args.calls, "reps": args.reps,
                      "threshold": THR, "kept": kept, "us_per_call": us}))


if __name__ == "__main__":
    main()
