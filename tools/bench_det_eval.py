#!/usr/bin/env python
"""One append of detection records at the flagship shape (n = 2, k = 20 organs, 27 queries per organ; bf16 and fp32 outputs):
the single launch of csrc/det_eval.hip, hipEvents around N appends issued back to back from Python after a warm-up (so the figure
is the rate at which the host enqueues them, an upper bound of the kernel's own time), next to the host route of the reference's
validation loop restated on the same tensors (transoar/inference.py + the evaluator's IoU: the outputs and targets copied to the
host, a Python loop over images and classes, numpy IoU per class), timed with the host clock around whole batches because it
synchronises by construction.  Also the largest score / IoU difference between the two.

    python tools/bench_det_eval.py [--warmup 50] [--reps 2000] [--host-reps 50] [--out profiles/det_eval_bench.jsonl]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from tests._eval_inputs import random_inputs  # noqa: E402
from transoar_amd.evaluation import DetectionRecords  # noqa: E402

N, K, QPO = 2, 20, 27


def _iou_np(a, b):
    """(6,) cx cy cz w h d boxes -> IoU, numpy fp32"""
    a1, a2, b1, b2 = a[:3] - 0.5 * a[3:], a[:3] + 0.5 * a[3:], b[:3] - 0.5 * b[3:], b[:3] + 0.5 * b[3:]
    inter = np.prod(np.clip(np.minimum(a2, b2) - np.maximum(a1, b1), 0, None))
    return inter / (np.prod(a2 - a1) + np.prod(b2 - b1) - inter)


def host_route(logits, boxes, gt, present):
    """What the reference does per batch before its evaluator's threshold loop: -> (scores, ious) per image"""
    bs = logits.shape[0]
    probs = logits.sigmoid().squeeze().reshape(bs, K, QPO).cpu()
    pred = boxes.reshape(bs, K, QPO, -1).cpu()
    ids = probs.argmax(dim=-1)
    gt_np, present_np = gt.detach().cpu().numpy(), present.detach().cpu().numpy()
    scores, ious = [], []
    for s in range(bs):
        row_scores, row_ious = [], []
        for c in range(K):
            box = pred[s, c, ids[s, c]].detach().float().numpy()
            row_scores.append(probs[s, c, ids[s, c]].detach().float().numpy())
            row_ious.append(_iou_np(box, gt_np[s, c]) if present_np[s, c] else -1.0)
        scores.append(np.array(row_scores))
        ious.append(np.array(row_ious, dtype=np.float32))
    return np.stack(scores), np.stack(ious)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--reps", type=int, default=2000)
    ap.add_argument("--host-reps", type=int, default=50)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    rows = []
    for dtype in (torch.bfloat16, torch.float32):
        logits, boxes, gt, present = (t.cuda() for t in random_inputs(N, K, QPO, seed=7, dtype=dtype))
        losses = torch.rand(13, device="cuda")
        buf = DetectionRecords(N, K, 13, "cuda")
        assert buf.usable(logits, boxes, gt, present, losses)

        def launch():
            buf.state.zero_()                       # keep the cursor inside the buffer: one memset node per launch, timed too
            buf.append(logits, boxes, gt, present, losses)
        for _ in range(args.warmup):
            launch()
        torch.cuda.synchronize()
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(args.reps):
            launch()
        end.record()
        torch.cuda.synchronize()
        hip_us = start.elapsed_time(end) * 1e3 / args.reps
        host = buf.to_host()
        for _ in range(3):
            scores, ious = host_route(logits, boxes, gt, present)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.host_reps):
            scores, ious = host_route(logits, boxes, gt, present)
        host_us = (time.perf_counter() - t0) * 1e6 / args.host_reps
        row = {"shape": {"n": N, "k": K, "qpo": QPO}, "dtype": str(dtype)[6:], "reps": args.reps, "host_reps": args.host_reps,
               "hip_append_us": round(hip_us, 2), "host_route_us": round(host_us, 1), "ratio": round(host_us / hip_us, 1),
               "max_score_err": float(np.abs(host["score"] - scores.astype(np.float32)).max()),
               "max_iou_err": float(np.abs(host["iou"] - ious).max()), "cpu_threads": torch.get_num_threads()}
        rows.append(row)
        print(json.dumps(row), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(json.dumps(r) for r in rows) + "\n")


if __name__ == "__main__":
    main()
