"""Does the contraction of the NMS's union into a fused multiply-add decide anything outside the exact domain?

Inside coordinates [0, 2896] every area and sum of two areas is an integer below 2^24, exact in float32 (tests/nms_cases.py).
Beyond it `wa * ha + wb * hb - inter` rounds, and the library's -ffp-contract=on lets the compiler fuse one product into the
sum, which torchvision's CPU kernel (the reference's NMS) does not do.  This builds box pairs with coordinates up to 32768
whose IoU lies within a few float32 steps of the threshold, predicts on the host the decision of the stepwise float32
expression and of both possible fusions, and runs the pairs on the device: lists of two through hgl_nms_segments
(the LDS body, nms_bits_body) and a sample through hgl_nms with an unaligned pointer (the serial body, nms_serial_body): two
inlinings of the one IoU expression, nms_overlap of csrc/sam_nms.hip.

    python tools/nms_contraction_probe.py [--out FILE.json]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
F32 = np.float32
MAXC = 32768


def near_threshold_pairs(thr, n_base, rng, span=40, per_base=12):
    """-> int64 [n, 8] (box a, box b): random overlapping pairs, b's right and bottom edges searched over +-span for the
    exact IoUs closest to thr"""
    out = []
    while len(out) < n_base * per_base:
        wa, ha = rng.integers(3000, 24000, size=2)
        ax0, ay0 = rng.integers(0, MAXC - wa), rng.integers(0, MAXC - ha)
        a = np.array([ax0, ay0, ax0 + wa, ay0 + ha])
        bx0, by0 = ax0 + rng.integers(0, wa // 3), ay0 + rng.integers(0, ha // 3)
        bx1 = min(bx0 + rng.integers(wa // 2, 2 * wa), MAXC - span)
        # solve for by1 in double, then search the neighbourhood in exact integers
        iw = min(a[2], bx1) - bx0
        best = None
        for by1 in range(by0 + 100, MAXC - span, 64):
            ih = min(a[3], by1) - by0
            inter = iw * ih
            iou = inter / (wa * ha + (bx1 - bx0) * (by1 - by0) - inter)
            if best is None or abs(iou - thr) < best[0]:
                best = (abs(iou - thr), by1)
        if best[0] > 0.01:
            continue
        dx, dy = np.meshgrid(np.arange(-span, span + 1), np.arange(-span, span + 1))
        x1, y1 = bx1 + dx.ravel(), best[1] + dy.ravel()
        iw = np.minimum(a[2], x1) - bx0
        ih = np.minimum(a[3], y1) - by0
        inter = iw * ih
        iou = inter / (wa * ha + (x1 - bx0) * (y1 - by0) - inter).astype(np.float64)
        for j in np.argsort(np.abs(iou - thr))[:per_base]:
            out.append([*a, bx0, by0, x1[j], y1[j]])
    return np.array(out, dtype=np.int64)


def decisions(p, thr):
    """host predictions -> dict of bool [n]: stepwise float32, the two fusions, exact"""
    f = p.astype(F32)
    wa, ha, wb, hb = f[:, 2] - f[:, 0], f[:, 3] - f[:, 1], f[:, 6] - f[:, 4], f[:, 7] - f[:, 5]
    iw = np.maximum(np.minimum(f[:, 2], f[:, 6]) - np.maximum(f[:, 0], f[:, 4]), F32(0))
    ih = np.maximum(np.minimum(f[:, 3], f[:, 7]) - np.maximum(f[:, 1], f[:, 5]), F32(0))
    inter = iw * ih
    pa, pb = wa * ha, wb * hb                                              # rounded products
    ea, eb = wa.astype(np.float64) * ha.astype(np.float64), wb.astype(np.float64) * hb.astype(np.float64)     # exact
    t = F32(thr)
    step = inter / ((pa + pb) - inter) > t
    fuse_a = inter / ((ea + pb.astype(np.float64)).astype(F32) - inter) > t                    # fma(wa, ha, wb * hb)
    fuse_b = inter / ((pa.astype(np.float64) + eb).astype(F32) - inter) > t                    # fma(wb, hb, wa * ha)
    q = p.astype(object)
    ei = np.array([max(min(r[2], r[6]) - max(r[0], r[4]), 0) * max(min(r[3], r[7]) - max(r[1], r[5]), 0) for r in q], dtype=object)
    eu = np.array([(r[2] - r[0]) * (r[3] - r[1]) + (r[6] - r[4]) * (r[7] - r[5]) for r in q], dtype=object) - ei
    num, den = float(F32(thr)).as_integer_ratio()
    exact = np.array([i * den > num * u for i, u in zip(ei, eu)])
    return dict(stepwise=step, fuse_a=fuse_a, fuse_b=fuse_b, exact=exact)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--bases", type=int, default=400)
    args = ap.parse_args()
    import torch
    from hybridgl_amd import sam as hsam
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(5)
    report = {}
    for thr in (0.5, 0.7, 0.75):
        p = near_threshold_pairs(thr, args.bases, rng)
        d = decisions(p, thr)
        n = len(p)
        boxes = torch.from_numpy(p.reshape(2 * n, 4).astype(np.int32)).to(dev)
        scores = torch.tensor([1.0, 0.0], device=dev).repeat(n)
        keep = torch.ones(2 * n, dtype=torch.uint8, device=dev)
        offs = torch.arange(0, 2 * n + 1, 2, dtype=torch.int32, device=dev)
        _, cnt = hsam.nms_segments(boxes, scores, keep, offs, 2, thr)
        bits = cnt.cpu().numpy() == 1                                       # the second box of the pair was suppressed
        # the serial kernel: the pairs on which the predictions part first, then the rest, 300 launches
        first = np.argsort(~(d["stepwise"] != d["fuse_a"]) & ~(d["stepwise"] != d["fuse_b"]), kind="stable")[:300]
        serial = np.zeros(len(first), bool)
        for j, i in enumerate(first):
            flat = torch.zeros(9, dtype=torch.int32, device=dev)
            flat[1:] = boxes[2 * i:2 * i + 2].reshape(-1)
            _, c = hsam.nms(flat[1:].view(2, 4), scores[:2], keep[:2], thr)
            serial[j] = int(c.item()) == 1
        r = dict(pairs=n, max_coord=int(p.max()),
                 stepwise_vs_fuse_a=int((d["stepwise"] != d["fuse_a"]).sum()), stepwise_vs_fuse_b=int((d["stepwise"] != d["fuse_b"]).sum()),
                 stepwise_vs_exact=int((d["stepwise"] != d["exact"]).sum()),
                 bits_vs_stepwise=int((bits != d["stepwise"]).sum()), bits_vs_fuse_a=int((bits != d["fuse_a"]).sum()),
                 bits_vs_fuse_b=int((bits != d["fuse_b"]).sum()), bits_vs_exact=int((bits != d["exact"]).sum()),
                 serial_sampled=len(first), serial_vs_stepwise=int((serial != d["stepwise"][first]).sum()),
                 serial_vs_fuse_a=int((serial != d["fuse_a"][first]).sum()), serial_vs_fuse_b=int((serial != d["fuse_b"][first]).sum()))
        diff = np.nonzero(bits != d["stepwise"])[0]
        r["bits_differing_pairs"] = p[diff[:5]].tolist()
        report[str(thr)] = r
        print(thr, json.dumps(r))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(report, f, indent=1)


if __name__ == "__main__":
    main()
